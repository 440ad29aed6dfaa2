"""The landmark elimination (K5) in every device form against the long-double reference of tests/helpers/schur_reference.py,
on windows with designed observation structure (tests/helpers/obs_patterns.py: device landmark counts 1 / 15 / 16 / 17 and
16 k / 16 k + 1 / 16 k + 15, a chunk of landmarks seen only by a constant pose and such landmarks inside a chunk -- asserted on
the device's own landmark order --, track lengths 1 / stereo pair / 64 /
65 / 2 P, a constant pose, outliers, and for wide windows the panel patterns including an empty pair list, a one-landmark pair
list and lists that reach the record and word caps of a batch).

Per case: eval_reprojection(robust=True) and eval_factors() give the records the build consumes, the reference is assembled from
them, and every entry of linearize()'s S (both triangles: every form writes both) and g must lie inside the reference's a-priori
rounding bound, the cost inside its own.  The form that ran is read from the library (SVIN_LAST_SCHUR_FORM) and asserted.  The
printed `error / tol` ratios are a record, not the criterion.

Not covered here: the batched Schur form (k_schur_dense_batch) and the sharded path.  (The landmark back-substitution and the rest
of k_post_solve: tests/test_gpu_step_edges.py; a marginalisation prior away from its linearisation point: tests/test_gpu_prior_edges.py.)
"""
import os
import sys
import time

import numpy as np
import pytest

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "helpers"))
import obs_patterns as op          # noqa: E402
import schur_reference as sr       # noqa: E402

from svin_amd import synthetic as syn   # noqa: E402

pytestmark = pytest.mark.gpu

KIND = {0: "p", 1: "e", 2: "s"}
DIM = {0: 6, 1: 6, 2: 9}


def gpu_records(est):
    """the records of the current linearisation point as the build consumes them"""
    from svin_amd.estimator import SVIN_LOSS_NONE
    ev, raw = est.eval_reprojection(robust=True), est.eval_reprojection(robust=False)
    desc = {}

    def describe(b):
        if b not in desc:
            desc[b] = est.describe_block(b)
        return desc[b]
    ext_of = {}
    for b in est.parameter_block_ids():
        dsc = describe(b)
        if dsc is not None and dsc[1] == 1:
            ext_of[(dsc[0], dsc[2])] = b
    recs = []
    for i in range(len(ev["r"])):
        pose = int(ev["pose_id"][i])
        s = float(raw["r"][i] @ raw["r"][i])
        bl = [(("p", pose), ev["Jp"][i]), (("l", int(ev["lm_id"][i])), ev["Jl"][i])]
        e = ext_of.get((describe(pose)[0], int(ev["cam"][i])))
        if e is not None:
            bl.append((("e", e), ev["Je"][i]))
        recs.append((ev["r"][i], bl, 0.5 * np.log1p(s)))   # CauchyLoss(1): rho = log(1 + s)
    for f in est.eval_factors():
        assert est.map_get_residual_loss(f["res_id"])[0] == SVIN_LOSS_NONE, "a small factor with a loss: its corrector is not in eval_factors()"
        bl, o = [], 0
        for b in f["blocks"]:
            kind = describe(b)[1]
            bl.append(((KIND[kind], b), f["J"][:, o:o + DIM[kind]]))
            o += DIM[kind]
        assert o == f["J"].shape[1]
        recs.append((f["r"], bl))
    return recs, describe


def device_landmark_order(est, lm_ids):
    """landmark indices in the order of the device's CSR (observation_ids follows pack())"""
    index = {int(i): l for l, i in enumerate(lm_ids)}
    seen, order = set(), []
    for i in est.eval_reprojection()["lm_id"]:
        if int(i) not in seen:
            seen.add(int(i))
            order.append(index[int(i)])
    return order


# (window, debug options, every pose block constant, the code kernels.hpp lists for the form)
PLANNED = [("narrow_L17", {}, False, 1090), ("narrow_L17", op.PAIR, False, 4000), ("ext_P6_fixed", {}, False, 1091),
           ("ext_P6_fixed", op.TILE, False, 1092), ("narrow_L1", {}, True, 5000)]


@pytest.mark.parametrize("name, opts, fix_poses, code", PLANNED)
def test_the_form_that_ran_is_the_planned_one(gpu_lib, debug_option, tmp_path, name, opts, fix_poses, code):
    """SVIN_LAST_SCHUR_FORM after linearize() against planBuild (svin_amd/csrc/build_plan.hpp through the CPU shim of
    tests/test_build_plan_host.py) on the window's own integers: narrow dense with fixed and with variable extrinsics, pairwise
    by its switch, and a window whose poses are all constant, which leaves the small factors alone"""
    import build_plan_lib as bpl
    from svin_amd.estimator import Estimator
    lib = bpl.build_shim(tmp_path)
    design = op.build(name)
    for k, v in opts.items():
        debug_option(k, v)
    est = Estimator(0)
    fids, _ = syn.feed(est, design.spec)
    fixed = [design.fixed_frame] if design.fixed_frame is not None else []
    for b in est.parameter_block_ids():
        dsc = est.describe_block(b)
        if dsc is not None and dsc[1] == 0 and (fix_poses or dsc[0] in [fids[f] for f in fixed]):
            assert est.set_parameter_block_constant(b)
    ev = est.eval_reprojection()
    lin = est.linearize(1e-4)
    ran = Estimator.debug_get_option("SVIN_LAST_SCHUR_FORM")
    kinds = [est.describe_block(int(b))[1] for b in lin["block_ids"]]
    switches = (bpl.PAIRWISE if "SVIN_SCHUR_PAIRWISE" in opts else 0) | (bpl.A_MFMA if "SVIN_SCHUR_A_MFMA" in opts else 0)
    row = bpl.row(6 * (kinds.count(0) + kinds.count(1)), len(set(int(i) for i in ev["lm_id"])), len(ev["r"]), dCPose=6 * kinds.count(0),
                  any_ext=int(kinds.count(1) > 0), F=len(est.eval_factors()), priorM=0, nPose=design.spec.P, switches=switches)
    planned = int(bpl.plan(lib, [row], 120, 133584)["formCode"][0])   # (the two sizes do not enter the form)
    print(name, opts, "dC", row[0], "dCPose", row[1], "L", row[3], "N", row[4], "ran", ran, "planned", planned)
    assert ran == planned == code
    del est


@pytest.mark.parametrize("name", sorted(op.CASES))
def test_reduced_system_against_long_double(gpu_lib, debug_option, name):
    if not sr.have_long_double():
        pytest.skip("np.longdouble is not wider than float64 on this machine")
    import torch
    from svin_amd.estimator import Estimator
    t_start = time.time()
    args, forms = op.CASES[name]
    design = op.build(name)
    spec = design.spec
    P, with_ext = spec.P, args.get("rig", "euroc") == "test4"
    nP = P - (design.fixed_frame is not None)
    if args.get("wide"):
        st = op.work_list_stats(design, torch.cuda.get_device_properties(0).multi_processor_count)
        print(name, "work list: workgroups per pair", st["workgroups"], "pairs without entries", st["pairs_without_entries"],
              "record cap", st["record_cap"], "word cap", st["word_cap"])
        if args.get("sparse_pairs"):
            assert st["pairs_without_entries"] and 1 in st["entries"].values()
        elif args.get("n_comb"):   # the windows built to reach the caps
            assert st["record_cap"] and st["word_cap"] and max(st["workgroups"].values()) >= 2
    mus = [1e-4] + ([0.0] if design.min_obs >= 3 else [])
    for opts, form in forms:
        for k, v in opts.items():
            debug_option(k, v)
        est = Estimator(0)
        fids, lm_ids = syn.feed(est, spec)
        if design.fixed_frame is not None:
            ev = est.eval_reprojection()
            pose_of = {est.describe_block(int(b))[0]: int(b) for b in np.unique(ev["pose_id"])}
            assert est.set_parameter_block_constant(pose_of[fids[design.fixed_frame]])
        recs, describe = gpu_records(est)
        # what the device holds: every landmark (L % 16 as designed), in index order unless pack() re-sorts; with a constant pose
        # one chunk of sixteen landmarks without slots or rows, and a chunk that mixes such landmarks with others
        order = device_landmark_order(est, lm_ids)
        assert sorted(order) == list(range(spec.L)) and len(order) % 16 == args["L"] % 16, (len(order), spec.L)
        if nP <= op.RESORT_ABOVE:
            assert order == list(range(spec.L))
        chunks = [order[i:i + 16] for i in range(0, len(order), 16)]
        if design.fixed_frame is not None and spec.L >= 33:
            lone = set(design.roles["fixed_only"])
            assert any(len(c) == 16 and set(c) <= lone for c in chunks), "no chunk without rows on the device"
            assert any(0 < len(set(c) & lone) < len(c) for c in chunks), "no chunk with holes on the device"
        for mu in mus:
            lin = est.linearize(mu)
            assert Estimator.debug_get_option("SVIN_LAST_SCHUR_FORM") == form, (name, opts, Estimator.debug_get_option("SVIN_LAST_SCHUR_FORM"))
            kinds = [describe(int(b))[1] for b in lin["block_ids"]]
            blocks = [((KIND[k], int(b)), int(o), DIM[k]) for b, o, k in zip(lin["block_ids"], lin["block_off"], kinds)]
            assert kinds.count(0) == nP and kinds.count(2) == P and kinds.count(1) == (2 * P if with_ext else 0), kinds
            assert lin["d"] == 6 * nP + 9 * P + (12 * P if with_ext else 0)
            assert sorted(o for _, o, _ in blocks) == list(np.cumsum([0] + [n for _, _, n in sorted(blocks, key=lambda b: b[1])])[:-1])
            if design.fixed_frame is not None:
                assert all(describe(int(b))[0] != fids[design.fixed_frame] or k != 0 for b, k in zip(lin["block_ids"], kinds))
            rf = sr.assemble(recs, blocks, mu)
            assert rf["d"] == lin["d"]
            rS, rg = sr.worst_ratio(lin["S"], lin["g"], rf)
            rc = abs(lin["cost"] - float(rf["cost"])) / rf["tol_cost"]
            print("%s form %d %s mu %g: worst error / tol  S %.3g  g %.3g  cost %.3g  (d %d, N %d, max kappa %.3g)" %
                  (name, form, opts, mu, rS, rg, rc, lin["d"], spec.N, max(rf["kappa"].values())))
            assert rS <= 1.0 and rg <= 1.0, "the reduced system leaves its rounding bound"
            assert rc <= 1.0, "the cost leaves its rounding bound"
        for k in opts:
            debug_option(k, 0)
        del est
    print("%s: %.1f s" % (name, time.time() - t_start))
