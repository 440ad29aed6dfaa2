"""The post-solve pass and the dogleg step in every device form against the long-double reference of
tests/helpers/step_reference.py, through the inspection hook svin_ba_debug_trust_region_step (one trust-region iteration with the
launches optimize() issues), on windows from tests/helpers/obs_patterns.py that cross each size-dependent edge of k_post_solve /
k_step_retract / the deferred landmark step: device landmark counts 1 / 15 / 16 / 17, constant blocks and chunks without rows,
the extrinsics instantiation, tracks of 15 .. 34 observations (sixteen lanes per landmark, the first observation in registers),
launches of 256 / 257 and 512 / 513 blocks (second round of the tail reduction, the _wide variant), 2048 / 2049 / more than
16384 landmarks (landmark rounds of the fused tail, the grid-stride loop), 96 / 98 parameter blocks (staged items; the block
count of these rigs is even), 63 / 66 pose + extrinsics blocks (the two-wave split), 128 / 129 poses (staged block maps),
d > 1024 (staged solution vectors), a window whose landmarks the device re-sorts.

Per case and damping: the records of gpu_records() and the block table of linearize() give the reference; per form the window
can take (1 fused, landmarks moved by the post-solve tail; 2 post-solve + k_step_retract; 3 fused, landmarks moved by the
candidate evaluation -- what optimize() runs) and per radius (2 |gn|, alpha |g| / 2, three in between, the device's own
sqrt(gnHatSq)) every Stage A and Stage B quantity must lie inside its a-priori bound, the form that ran must be the one asked
for, the hook's y_C must agree with debug_reduced_solve(fused) to the bound of tests/test_gpu_reduced_solve.py, the candidates of
the forms must agree bit for bit wherever they started from the same bits, and all three dogleg branches must have run.  With
commit the getters return the candidate bit for bit and the hook's candidate cost lies inside the cost bound of
schur_reference.assemble at the committed state.  The printed `error / tol` ratios are a record, not the criterion.
test_step_with_moved_prior runs the same on windows whose marginalisation prior lies away from its linearisation point (the last block
of k_post_solve with M3 != I and grad = b0 + H dchi, tests/helpers/prior_reference.py), and holds a second linearize() at the
committed state to assemble() there.

The batched kernels are held bit for bit to these forms by tests/test_gpu_batch*.py.  Not covered: the sharded path, the batched
Schur form."""
import os
import sys
import time

import numpy as np
import pytest

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "helpers"))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import obs_patterns as op          # noqa: E402
import schur_reference as sr       # noqa: E402
import step_reference as st        # noqa: E402
from test_gpu_schur_edges import DIM, KIND, gpu_records   # noqa: E402

from svin_amd import synthetic as syn   # noqa: E402

pytestmark = pytest.mark.gpu

FUSED, SEPARATE, DEFERRED = 1, 2, 3


def post_blocks(L, N, F):
    """blocks of the post-solve launch (batch_plan.hpp: postLmBlockCount + postFacBlockCount + the tail block)"""
    return (min((L + 15) // 16, 1024) if L > 0 and N > 0 else 0) + (min((F + 3) // 4, 1024) if F > 0 else 0) + 1


def three_obs_with_blocks(target):
    """P = 3, three observations per landmark, L such that the post-solve launch has exactly `target` blocks: the smallest L that
    does (one landmark more than the largest L of target - 1 blocks)"""
    F = 4   # at most four small factors in a three-frame euroc window: one factor block (asserted on the hook's own counts)
    L = 16 * (target - 1 - (F + 3) // 4 - 1) + 1
    assert post_blocks(L, 3 * L, F) == target and post_blocks(L - 1, 3 * (L - 1), F) == target - 1
    return op.design_three_observations(L)


def short_tracks(P, L, rig="euroc"):
    """every landmark on three consecutive poses, every pose observed"""
    spec = op.full_window(P, L, rig, 1)
    tracks = {l: [((l + j) % P, (l + j) % 2) for j in range(3)] for l in range(L)}
    op.keep_tracks(spec, tracks)
    return op.Design(spec=spec, tracks=tracks)


# name -> (design, mus, expectations on the hook's own counts)
CASES = {
    "narrow_L1": (lambda: op.build("narrow_L1"), (1e-4,), dict(L=1)),
    "narrow_L15": (lambda: op.build("narrow_L15"), (1e-4,), dict(L=15)),
    "narrow_L16": (lambda: op.build("narrow_L16"), (1e-4,), dict(L=16, post_lm=1)),
    "narrow_L17": (lambda: op.build("narrow_L17"), (1e-4,), dict(L=17, post_lm=2)),
    "narrow_P10_fixed": (lambda: op.build("narrow_P10_fixed"), (1e-4,), dict(constant=1)),
    "narrow_P10_min3": (lambda: op.build("narrow_P10_min3"), (1e-4, 0.0), dict()),
    "ext_P6_fixed": (lambda: op.build("ext_P6_fixed"), (1e-4,), dict(constant=1, ext_variable=True)),
    "tracks_15_to_34": (lambda: op.design_track_lengths(), (1e-4,), dict(L=16)),
    "blocks_256": (lambda: three_obs_with_blocks(256), (1e-4,), dict(blocks=256)),
    "blocks_257": (lambda: three_obs_with_blocks(257), (1e-4,), dict(blocks=257)),
    "blocks_512": (lambda: three_obs_with_blocks(512), (1e-4,), dict(blocks=512)),
    "blocks_513": (lambda: three_obs_with_blocks(513), (1e-4,), dict(blocks=513)),
    "L2048": (lambda: op.design_three_observations(2048), (1e-4,), dict(L=2048)),
    "L2049": (lambda: op.design_three_observations(2049), (1e-4,), dict(L=2049)),
    "L16400": (lambda: op.design_three_observations(16400), (1e-4,), dict(L=16400, post_lm=1024, no_fused_tail=True)),
    "items_96": (lambda: short_tracks(47, 96), (1e-4,), dict(items=96)),
    "items_98": (lambda: short_tracks(48, 96), (1e-4,), dict(items=98)),
    "split_63": (lambda: short_tracks(21, 63, "test4"), (1e-4,), dict(pose_ext=63, ext_variable=True)),
    "split_66": (lambda: short_tracks(22, 66, "test4"), (1e-4,), dict(pose_ext=66, ext_variable=True)),
    "poses_128": (lambda: short_tracks(128, 256), (1e-4,), dict(poses=128)),
    "poses_129": (lambda: short_tracks(129, 258), (1e-4,), dict(poses=129)),
    "ext_P64_fixed": (lambda: op.build("ext_P64_fixed"), (1e-4,), dict(constant=1, ext_variable=True, d_above=1024)),
    "wide_P48_fixed": (lambda: op.build("wide_P48_fixed"), (1e-4,), dict(constant=1, resorted=True)),
}


def state_of(est, res):
    """values of every block and landmark at the linearisation point, in the hook's order"""
    xb = [((KIND[int(k)], int(b)), est.get_parameter_block(int(b))) for b, k in zip(res["block_ids"], res["block_kind"])]
    lm = np.array([est.get_landmark(int(i))["point"] for i in res["lm_ids"]]).reshape(-1, 4)
    return xb, lm


def check_step(name, est, P, blocks, mu, res, cache, x_blocks, lm_x, prior=None):
    """every Stage A / Stage B quantity of one call of the hook against its bound; returns the worst ratios"""
    worst, branch, aux = st.judge(P, mu, res, x_blocks, lm_x, prior, cache)
    assert res["scalars"]["failMax"] == 0 and res["scalars"]["cholFail"] == 0
    bad = {n: w for n, w in worst.items() if not w <= 1.0}
    assert not bad, "%s form %d radius %.6g: outside the rounding bound: %s" % (name, res["form"], res["radius"], bad)
    return worst, branch, aux


def run_case(name, est, design, mus, expect, debug_option, prior_of=None):
    t_start = time.time()
    recs, describe = gpu_records(est)
    record = {}
    for mu in mus:
        lin = est.linearize(mu)
        kinds = [describe(int(b))[1] for b in lin["block_ids"]]
        blocks = [((KIND[k], int(b)), int(o), DIM[k]) for b, o, k in zip(lin["block_ids"], lin["block_off"], kinds)]
        prior = None if prior_of is None else prior_of(blocks)
        first = est.debug_trust_region_step(mu, 1e4, 0)
        assert first["d"] == lin["d"] and first["form"] == first["form_solve"] == DEFERRED, "optimize() defers the landmark step on these windows"
        # what the window was built to be, on the hook's own counts
        nk = [int((first["block_kind"] == k).sum()) for k in range(3)]
        n_post = first["post_lm_blocks"] + first["post_fac_blocks"] + 1
        print("%s: d %d, L %d, blocks %s, post-solve launch %d + %d + 1, step launch %d" %
              (name, first["d"], first["L"], nk, first["post_lm_blocks"], first["post_fac_blocks"], first["step_blocks"]))
        assert first["post_lm_blocks"] == min((first["L"] + 15) // 16, 1024)
        if "L" in expect:
            assert first["L"] == expect["L"]
        if "post_lm" in expect:
            assert first["post_lm_blocks"] == expect["post_lm"]
        if "blocks" in expect:
            assert n_post == expect["blocks"]
        if "items" in expect:
            assert sum(nk) == expect["items"]
        if "pose_ext" in expect:
            assert nk[0] + nk[1] == expect["pose_ext"] and sum(nk) <= 96 and nk[2] <= 64
        if "poses" in expect:
            assert nk[0] == expect["poses"]
        if "d_above" in expect:
            assert first["d"] > expect["d_above"]
        if expect.get("constant"):
            assert len(blocks) < sum(nk), "no constant block in the window"
        assert (kinds.count(1) > 0) == bool(expect.get("ext_variable"))
        if expect.get("resorted"):
            assert [int(i) for i in first["lm_ids"]] != sorted(int(i) for i in first["lm_ids"]), "the device kept the landmarks in id order"
        P = st.prepare(recs, blocks, lm_order=first["lm_ids"])
        x_blocks, lm_x = state_of(est, first)
        cache = {}
        first["radius"] = 1e4
        _, _, aux = check_step(name, est, P, blocks, mu, first, cache, x_blocks, lm_x, prior)
        # the hook's Gauss-Newton step is the one the reduced solve's own hook returns
        y_solve = est.debug_reduced_solve(mu, fused=True)
        dy = np.abs(first["y_C"] - y_solve).max() / np.abs(y_solve).max()
        assert dy < (1e-10 if mu >= 1e-4 else 1e-6), dy
        va = cache[first["y_C"].tobytes()][0]
        gn, ag = float(np.sqrt(va["gnHatSq"])), float(va["gHatSq"] * np.sqrt(va["gHatSq"]) / va["jgSq"])
        # (a state moved far from a prior of 1e8 and more: the scaled gradient and the Gauss-Newton step are all but parallel and the
        # Cauchy point may lie beyond the Gauss-Newton step; then no radius interpolates)
        assert ag < gn or expect.get("prior_dominates")
        radii = [2 * gn, 0.5 * ag] + [float(x) for x in np.linspace(ag, gn, 5)[1:4]] + [float(np.sqrt(np.float64(first["scalars"]["gnHatSq"])))]
        forms = [DEFERRED, SEPARATE] + ([] if expect.get("no_fused_tail") else [FUSED])
        if expect.get("no_fused_tail"):
            with pytest.raises(RuntimeError):
                est.debug_trust_region_step(mu, radii[0], FUSED)
        branches, worst = set(), {}
        for radius in radii:
            got = {}
            for form in forms:
                res = est.debug_trust_region_step(mu, radius, form)
                assert res["form"] == form, "asked for form %d, form %d ran" % (form, res["form"])
                res["radius"] = radius
                w, br, _ = check_step(name, est, P, blocks, mu, res, cache, x_blocks, lm_x, prior)
                branches.add(br)
                for k, x in w.items():
                    worst[k] = max(worst.get(k, 0.0), x)
                got[form] = res
            base = got[forms[0]]
            for form in forms[1:]:
                res = got[form]
                same_start = all(np.array_equal(res[k], base[k]) for k in ("y_C", "v_C", "y_L", "v_L")) and \
                    all(res["scalars"][k] == base["scalars"][k] for k in st.GROUP_B)
                ulps = max([int(np.abs(a.view(np.int64) - b.view(np.int64)).max()) for a, b in zip(res["block_cand"], base["block_cand"])] +
                           [int(np.abs(res["lm_cand"].view(np.int64) - base["lm_cand"].view(np.int64)).max())])
                if same_start:
                    assert ulps == 0, "forms %d and %d: candidates %d ulp apart from the same vectors and sums" % (forms[0], form, ulps)
                else:
                    print("%s radius %.6g: forms %d and %d started from different bits (the build's sums are not ordered); candidates %d ulp apart" %
                          (name, radius, forms[0], form, ulps))
        assert branches == ({st.NEWTON, st.CAUCHY, st.INTERP} if ag < gn else {st.NEWTON, st.CAUCHY}), branches
        record[mu] = worst
        print("%s mu %g: worst error / tol  %s  (max kappa %.3g, %d calls, %d distinct y_C)" %
              (name, mu, "  ".join("%s %.3g" % kv for kv in sorted(worst.items())), float(aux["kappa"].max()), 1 + len(radii) * len(forms), len(cache)))
    # commit: the step is accepted as optimize() accepts one
    mu = mus[0]
    res = est.debug_trust_region_step(mu, radii[2], 0, commit=True)
    for (kind, bid), c in zip([(KIND[int(k)], int(b)) for b, k in zip(res["block_ids"], res["block_kind"])], res["block_cand"]):
        assert np.array_equal(est.get_parameter_block(bid).view(np.uint64), c.view(np.uint64)), (kind, bid)
    after = np.array([est.get_landmark(int(i))["point"] for i in res["lm_ids"]]).reshape(-1, 4)
    assert np.array_equal(after.view(np.uint64), res["lm_cand"].view(np.uint64))
    recs2, _ = gpu_records(est)
    lin = est.linearize(mu)
    kinds = [describe(int(b))[1] for b in lin["block_ids"]]
    blocks = [((KIND[k], int(b)), int(o), DIM[k]) for b, o, k in zip(lin["block_ids"], lin["block_off"], kinds)]
    # (a prior handed over AT its linearisation point: the committed state lies away from that point and is out of that form's scope;
    # the moved form of prior_reference is evaluated again at the committed state)
    prior2 = None if prior_of is None else prior_of(blocks)
    rf = sr.assemble(recs2, blocks, mu, prior=prior2) if prior2 is None or isinstance(prior2, dict) else None
    if rf is not None:
        rc = abs(res["scalars"]["cost"] - float(rf["cost"])) / rf["tol_cost"]
        print("%s: candidate cost against the committed state: error / tol %.3g" % (name, rc))
        assert rc <= 1.0
    if isinstance(prior2, dict):   # the build at the committed state: it consumes what the candidate evaluation left (dchi, grad, M3)
        rS, rg = sr.worst_ratio(lin["S"], lin["g"], rf)
        rc = abs(lin["cost"] - float(rf["cost"])) / rf["tol_cost"]
        print("%s: linearize() at the committed state: worst error / tol  S %.3g  g %.3g  cost %.3g" % (name, rS, rg, rc))
        assert rS <= 1.0 and rg <= 1.0 and rc <= 1.0, "the reduced system at the committed state leaves its rounding bound"
    print("%s: %.1f s" % (name, time.time() - t_start))
    return record


@pytest.mark.parametrize("name", list(CASES))
def test_step_against_long_double(gpu_lib, debug_option, name):
    if not sr.have_long_double():
        pytest.skip("np.longdouble is not wider than float64 on this machine")
    from svin_amd.estimator import Estimator
    make, mus, expect = CASES[name]
    design = make()
    est = Estimator(0)
    fids, _ = syn.feed(est, design.spec)
    if design.fixed_frame is not None:
        ev = est.eval_reprojection()
        pose_of = {est.describe_block(int(b))[0]: int(b) for b in np.unique(ev["pose_id"])}
        assert est.set_parameter_block_constant(pose_of[fids[design.fixed_frame]])
    run_case(name, est, design, mus, expect, debug_option)


def test_step_with_marginalisation_prior(gpu_lib, debug_option):
    """a window straight after its FIRST marginalisation, nothing optimised in between: the prior sits at its linearisation point
    (M3 = I, dchi = 0) and enters k_post_solve's last block as the quadratic form of est.marg()'s J and e0"""
    if not sr.have_long_double():
        pytest.skip("np.longdouble is not wider than float64 on this machine")
    from svin_amd.estimator import Estimator
    spec = syn.make_window(P=7, L=200, n_obs=2000, seed=9, keyframe_every=2, frame_dt=0.3)
    est = Estimator(0)
    done = []

    def on_frame(k, fid):
        if done:
            return
        est.optimize(4)
        est.apply_marginalization(2, 2)
        m = est.marg()
        if m is None:
            return
        done.append(k)

        def prior_of(blocks):
            pc = st.prior_columns(m, blocks)
            assert (pc >= 0).sum() >= 6, "the prior touches no variable block"
            return (m["J"], m["e0"], pc)
        run_case("prior_P7", est, None, (1e-4,), dict(), debug_option, prior_of=prior_of)
    syn.feed(est, spec, on_frame=on_frame)
    assert done, "no marginalisation happened"


@pytest.mark.parametrize("name,move", [(n, m) for n in ("euroc_P7", "rig_v2_P9") for m in ("optimised", "large")])
def test_step_with_moved_prior(gpu_lib, debug_option, name, move):
    """the windows of tests/test_gpu_prior_edges.py with the prior away from its linearisation point -- moved by hand (`large`) or by one
    more frame and optimize(3) (`optimised`): k_post_solve's last block forms (Mv)^T H (Mv), (Mv)^T grad and their y counterparts with
    M3 != I, the candidate evaluation writes the prior's dchi / grad / M3 of the candidate, and the build after the commit consumes them"""
    if not sr.have_long_double():
        pytest.skip("np.longdouble is not wider than float64 on this machine")
    import prior_moves as pm
    import prior_reference as pr
    import test_gpu_prior_edges as pe
    from svin_amd.estimator import Estimator
    est = Estimator(0)
    ran = []

    def run():
        prior = pe.device_prior(est)

        def prior_of(blocks):
            ref = pe.moved_prior(est, prior, blocks)
            assert (ref["columns"] >= 0).sum() >= 6 and float(np.abs(ref["dchi"]).max()) > 1e-9, "the prior sits at its linearisation point"
            return ref
        run_case("%s_%s" % (name, move), est, None, (1e-4,), dict(ext_variable=name.startswith("rig_v2"), prior_dominates=move == "large"), debug_option,
                 prior_of=prior_of)
        ran.append(move)

    def at_prior(before):
        if move == "large":
            rows = [(pr.KIND_OF[b["kind"]], b["id"]) for b in est.marg()["blocks"] if b["mdim"] > 0]
            pm.apply("large", rows, est.get_parameter_block, est.set_parameter_block)
            run()
            raise pe.Done

    def at_optimised():
        run()
    pe.slide(est, name, at_prior, at_optimised)
    assert ran == [move]
