"""The marginalisation prior AWAY from its linearisation point (K3: priorEvalBlock in every evaluation launch, priorAccumulateBlock in
every build) against the long-double reference of tests/helpers/prior_reference.py, inside schur_reference.assemble.

Per window (the smallest that produce the structure): a euroc window after its FIRST marginalisation (poses and speed / bias blocks,
m * m no multiple of 256), a rig_v2 window with sonar and depth after THREE chained marginalisations with optimize() in between (its
linearisation points are first estimates; extrinsics blocks, and the first frame's fixed extrinsics: a block with mdim = 0), a test4
window after two (per-frame extrinsics, all variable), and one wide window -- 45 frames fed, then apply_marginalization(40, 3): m > 64, form 2000, where the
prior is accumulated on a side stream beside the landmark elimination.
Per move (tests/helpers/prior_moves.py, applied to every block of the prior through set_parameter_block; what get_parameter_block
returns afterwards is the data): at_lin, tiny, large, flipped, constant (one pose of the prior constant: its rows and columns vanish
from S while its dchi still enters grad), and optimised (one more frame, then optimize(3)).
Per form the window can take (default, SVIN_SPLIT_EVAL, SVIN_LINEARIZE_EVAL_BUILD, SVIN_SCHUR_PAIRWISE): every entry of linearize()'s S
(both triangles), g and the cost must lie inside the reference's a-priori rounding bound, and SVIN_LAST_SCHUR_FORM must be the form
expected.  The reference takes the prior as data: the device's H, b0, e0 (marg()), the linearisation points (svin_ba_get_prior_lin)
and the blocks' current values.  The printed `error / tol` ratios and times are a record, not the criterion;
tests/test_prior_reference_host.py shows that the bound is tight enough to catch a wrong M3, dchi, grad or cost.
(The device normalises every quaternion it stores, so |q| = |q_lin| = 1 to rounding here: the two normalisation rules of the
definition are exercised by the host tests alone.)

The getter: after a first marginalisation the linearisation points are, bit for bit, the values read just before
apply_marginalization; on the chained window they agree with the oracle's to the pose parity tolerance of
tests/test_gpu_parity.py::test_marginalization_sequence_parity.
"""
import os
import sys
import time

import numpy as np
import pytest

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "helpers"))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import prior_moves as pm           # noqa: E402
import prior_reference as pr       # noqa: E402
import schur_reference as sr       # noqa: E402
import step_reference as st        # noqa: E402
from test_gpu_schur_edges import DIM, KIND, gpu_records   # noqa: E402

from svin_amd import synthetic as syn   # noqa: E402

pytestmark = pytest.mark.gpu

MU = 1e-4
# name -> window, marginalisation arguments, the frame at which the sliding starts, marginalisations to chain, optimize() iterations
WINDOWS = {
    "euroc_P7": dict(make=dict(P=7, L=150, n_obs=1500, seed=9, keyframe_every=2, frame_dt=0.3), marg=(2, 2), start=0, chain=1, iters=4,
                     expect=dict(kinds={0, 2}, mm_not_256=True, form=1090, pairwise=True)),
    "rig_v2_P9": dict(make=dict(P=9, L=200, n_obs=2000, seed=45, rig="rig_v2", sonar=True, depth=True, keyframe_every=2, frame_dt=0.3),
                      marg=(2, 2), start=0, chain=3, iters=4, expect=dict(kinds={0, 1, 2}, fixed_block=True, form=1091, pairwise=True)),
    "test4_P6": dict(make=dict(P=6, L=150, n_obs=1500, seed=12, rig="test4", keyframe_every=2, frame_dt=0.3), marg=(2, 2), start=0,
                     chain=2, iters=4, expect=dict(kinds={0, 1, 2}, form=1091, pairwise=True)),   # (the second marginalisation brings the extrinsics in)
    "wide_P46": dict(make=dict(P=46, L=400, n_obs=5000, seed=31, frame_dt=0.3), marg=(40, 3), start=44, chain=1, iters=3,
                     expect=dict(kinds={0, 2}, fixed_block=True, mm_not_256=True, m_above_64=True, form=2000)),   # (the rig's fixed extrinsics: mdim = 0)
}
FORMS = (("default", {}), ("split_eval", dict(SVIN_SPLIT_EVAL=1)), ("eval_build", dict(SVIN_LINEARIZE_EVAL_BUILD=1)),
         ("pairwise", dict(SVIN_SCHUR_PAIRWISE=1)))


class Done(Exception):
    pass


def slide(est, name, at_prior=None, at_optimised=None):
    """feeds the window; from frame `start` on optimize(iters) + apply_marginalization per frame until `chain` marginalisations have
    produced a prior: at_prior(values of every block just before that marginalisation); then one more frame, optimize(3),
    at_optimised()"""
    w = WINDOWS[name]
    spec = syn.make_window(**w["make"])
    state = dict(count=0, done=False)

    def on_frame(k, fid):
        if state["done"]:
            est.optimize(3)
            if at_optimised is not None:
                at_optimised()
            raise Done
        if k < w["start"]:
            return
        est.optimize(w["iters"])
        before = {int(b): est.get_parameter_block(int(b)) for b in est.parameter_block_ids()} if at_prior is not None else None
        ok, _ = est.apply_marginalization(*w["marg"])
        assert ok
        if est.marg() is None:
            return
        state["count"] += 1
        if state["count"] >= w["chain"]:
            state["done"] = True
            if at_prior is not None:
                at_prior(before)
    with pytest.raises(Done):
        syn.feed(est, spec, on_frame=on_frame)


def device_prior(est):
    """the prior as the solver holds it, from marg(): (H, b, c0, dH, db, dc0, marg()).  The Cholesky route of the marginalisation hands
    the solver the symmetrised H, -b0 and e0 . e0 (J is then triangular); the eigen-solve computes J^T J, J^T e0 on the device."""
    m = est.marg()
    n = m["n"]
    if np.array_equal(m["J"], np.triu(m["J"])):
        c0 = np.asarray(m["e0"], pr.LD) @ np.asarray(m["e0"], pr.LD)
        return 0.5 * (m["H"] + m["H"].T), -m["b0"], c0, None, None, pr.EPS * (n + pr.C0) * c0, m
    return pr.from_factor(m["J"], m["e0"]) + (m,)


def moved_prior(est, prior, blocks):
    """prior_reference.moved at the blocks' current values, for the block table of linearize()"""
    H, b, c0, dH, db, dc0, m = prior
    pb = [dict(kind=pr.KIND_OF.get(bl["kind"]), ordering=bl["ordering"], mdim=bl["mdim"], lin=bl["lin"],
               x=est.get_parameter_block(bl["id"]) if bl["mdim"] > 0 else None) for bl in m["blocks"]]
    return pr.moved(H, b, c0, pb, st.prior_columns(m, blocks), dH, db, dc0)


def block_table(est, lin, describe):
    kinds = [describe(int(b))[1] for b in lin["block_ids"]]
    return [((KIND[k], int(b)), int(o), DIM[k]) for b, o, k in zip(lin["block_ids"], lin["block_off"], kinds)]


def check_state(name, move, est, prior, debug_option, expect, n_constant=0):
    """linearize() in every form against assemble() with the moved prior, at the estimator's current state"""
    from svin_amd.estimator import Estimator
    t0 = time.time()
    recs, describe = gpu_records(est)
    rf, default_form, out = None, None, {}
    for tag, opts in FORMS:
        for k, v in opts.items():
            debug_option(k, v)
        launches = Estimator.debug_get_option("SVIN_EVAL_BUILD_LAUNCHES")
        lin = est.linearize(MU)
        form = Estimator.debug_get_option("SVIN_LAST_SCHUR_FORM")
        launched = Estimator.debug_get_option("SVIN_EVAL_BUILD_LAUNCHES") - launches
        for k in opts:
            debug_option(k, 0)
        if tag == "default":
            default_form = form
            # (a constant pose takes the wide window to 42 variable pose blocks: whichever dense form the device then chooses)
            assert (n_constant or form == expect["form"]) and (form == 2000 or 1000 < form < 2000), form
            blocks = block_table(est, lin, describe)
            ref_prior = moved_prior(est, prior, blocks)
            assert (ref_prior["columns"] < 0).sum() == 6 * n_constant, "rows of the prior without columns"
            rf = sr.assemble(recs, blocks, MU, prior=ref_prior)
            assert rf["d"] == lin["d"] and rf["ref_ratio"] < 1e-3
        elif tag == "pairwise":
            if form == default_form:
                assert not expect.get("pairwise"), "the window did not take the pairwise form"
                continue   # (the window cannot take it: same launches as the default)
            assert form in (4000, 4001), form
        else:
            assert form == default_form, (tag, form)
            if tag == "eval_build" and not launched:
                continue   # (a window k_eval_build does not take: same launches as the default)
        rS, rg = sr.worst_ratio(lin["S"], lin["g"], rf)
        rc = abs(lin["cost"] - float(rf["cost"])) / rf["tol_cost"]
        out[tag] = (rS, rg, rc)
        print("%s %s %s form %d: worst error / tol  S %.3g  g %.3g  cost %.3g  (d %d, prior m %d, |dchi| max %.3g)" %
              (name, move, tag, form, rS, rg, rc, lin["d"], ref_prior["m"], float(np.abs(ref_prior["dchi"]).max())))
        assert rS <= 1.0 and rg <= 1.0, "the reduced system leaves its rounding bound"
        assert rc <= 1.0, "the cost leaves its rounding bound"
    print("%s %s: %.1f s" % (name, move, time.time() - t0))
    return out, ref_prior


@pytest.mark.parametrize("name", list(WINDOWS))
def test_moved_prior_against_long_double(gpu_lib, debug_option, name):
    if not sr.have_long_double():
        pytest.skip("np.longdouble is not wider than float64 on this machine")
    from svin_amd.estimator import Estimator
    t_start = time.time()
    w = WINDOWS[name]
    expect = w["expect"]
    est = Estimator(0)
    seen = []

    def at_prior(before):
        prior = device_prior(est)
        m = prior[-1]
        rows = [(pr.KIND_OF[b["kind"]], b["id"]) for b in m["blocks"] if b["mdim"] > 0]
        print("%s: prior m %d, blocks %s, route %s" % (name, m["n"], [(b["kind"], b["mdim"]) for b in m["blocks"]],
                                                       "cholesky" if prior[3] is None else "eigen"))
        assert {b["kind"] for b in m["blocks"] if b["mdim"] > 0} == expect["kinds"]
        assert any(b["mdim"] == 0 for b in m["blocks"]) == bool(expect.get("fixed_block"))
        if expect.get("mm_not_256"):
            assert m["n"] * m["n"] % 256 != 0
        if expect.get("m_above_64"):
            assert m["n"] > 64
        if w["chain"] == 1:   # the getter: the points are the values the blocks had when they were linearised
            for b in m["blocks"]:
                x = before[b["id"]]
                assert np.array_equal(b["lin"][:len(x)].view(np.uint64), x.view(np.uint64)), b
        after = {bid: est.get_parameter_block(bid) for _, bid in rows}
        held = [b["id"] for b in m["blocks"] if b["kind"] == 0 and b["mdim"] > 0][-1]
        for move in pm.MOVES:
            for bid, x in after.items():
                est.set_parameter_block(bid, x)
            kept = pm.apply("large" if move == "constant" else move, rows, est.get_parameter_block, est.set_parameter_block)
            if move == "flipped" and kept == 0:   # the setter canonicalises the sign: nothing to test
                assert all(est.get_parameter_block(bid)[6] >= 0 for kind, bid in rows if kind != "s")
                continue
            if move == "constant":
                assert est.set_parameter_block_constant(held)
            _, ref = check_state(name, move, est, prior, debug_option, expect, n_constant=int(move == "constant"))
            if move == "constant":
                assert est.set_parameter_block_constant(held, False)
            if move == "at_lin" and w["chain"] == 1:
                assert float(np.abs(ref["dchi"]).max()) < 1e-15
            seen.append(move)
        for bid, x in after.items():
            est.set_parameter_block(bid, x)
        seen.append(prior)

    def at_optimised():
        prior = device_prior(est)
        assert prior[-1]["n"] == seen[-1][-1]["n"] and np.array_equal(prior[-1]["H"], seen[-1][-1]["H"])
        _, ref = check_state(name, "optimised", est, prior, debug_option, expect)
        assert float(np.abs(ref["dchi"]).max()) > 1e-9, "optimize() left the prior at its linearisation point"
        seen.append("optimised")
    slide(est, name, at_prior, at_optimised)
    assert "optimised" in seen and "large" in seen and "constant" in seen
    print("%s: %.1f s" % (name, time.time() - t_start))


def test_chained_linearisation_points_against_oracle(gpu_lib):
    """after three chained marginalisations the points are first estimates: they agree with the oracle's marg()["lin"], block by block,
    to the bar tests/test_gpu_parity.py::test_marginalization_sequence_parity holds the poses to (rig_v2: at least 1e-4, else 30 x
    the distance of the oracle from itself with its initial landmarks moved by 1e-13 m)"""
    from oracle import orc
    from svin_amd.estimator import Estimator
    from test_gpu_parity import pose_diff
    name = "rig_v2_P9"

    def run(est, shift=None):
        w = WINDOWS[name]
        spec = syn.make_window(**w["make"])
        if shift is not None:
            spec.lm_init[:, :3] += shift * np.random.default_rng(1).normal(size=(spec.L, 3))
        state = dict(count=0)
        est.set_solver_options(1e-12, 1e-12, 1e-12)

        def on_frame(k, fid):
            est.optimize(w["iters"])
            est.apply_marginalization(*w["marg"])
            if est.marg() is not None:
                state["count"] += 1
                if state["count"] >= w["chain"]:
                    raise Done
        with pytest.raises(Done):
            syn.feed(est, spec, on_frame=on_frame)
        return {(b["frame"], b["kind"], b["index"]): b for b in est.marg()["blocks"]}

    def distance(a, b):
        assert sorted(a) == sorted(b)
        worst = 0.0
        for key, ba in a.items():
            bb = b[key]
            assert (ba["mdim"], ba["ordering"]) == (bb["mdim"], bb["ordering"])
            worst = max(worst, float(np.abs(ba["lin"] - bb["lin"]).max()) if key[1] == 2 else pose_diff(ba["lin"][:7], bb["lin"][:7]))
        return worst
    gpu, cpu, cpu2 = run(Estimator(0)), run(orc.OracleEstimator()), run(orc.OracleEstimator(), 1e-13)
    worst, sens = distance(gpu, cpu), distance(cpu2, cpu)
    print("chained linearisation points: device against oracle %.3g, oracle against itself with landmarks moved by 1e-13 m %.3g" % (worst, sens))
    assert worst < max(1e-4, 30 * sens)
    assert any(np.any(b["lin"]) for b in gpu.values())
