"""The designed systems, the long-double reference and the bars of tests/helpers/marg_reference.py on the CPU (read its text
for the construction).  tests/test_gpu_marg_edges.py hands the same cases to the job's launches through svin_ba_debug_marginalize.

1. The long-double reference equals the independent 40-digit one (tests/mp_marg.py marginalize_mp, which follows the reference's
   algorithm with its rank rule) to 2^-60 in scaled units, on every case of at most 48 unknowns.
2. The float64 restatement of the kernels' arithmetic meets every bar on every case (the constants are 8 x its own worst case, so
   this says the bars are consistent and prints what they are).
3. Every edge the cases are there for is reached: the plan fields per case through marg_plan_lib, so that a change of the plan
   that leaves an edge uncovered fails here.
4. The eigenvalue condition holds on every case (build() redraws until it does; here it is asserted on what build() returned)."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "helpers"))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import marg_plan_lib as mpl          # noqa: E402
import marg_reference as mr          # noqa: E402

LD = mr.LD


@pytest.fixture(scope="module")
def lib(tmp_path_factory):
    return mpl.build_shim(tmp_path_factory.mktemp("marg_ref_host"))


@pytest.fixture(scope="module")
def cases(lib):
    return [mr.build(s) for s in mr.all_specs(lib)]


def test_reference_equals_the_40_digit_one(cases):
    import mp_marg
    small = [c for c in cases if c["ds"]["m"] + 3 * c["ds"]["Lm"] <= 48 and c["ds"]["m"] > 0
             and (c["ds"]["nk"] > 0 or not c["stages"] & mr.STAGE_DENSE)]
    assert len(small) >= 80
    tol, worst = 2.0 ** -60, (0.0, "")
    for c in small:
        ds, ref = c["ds"], c["ref"]
        m, Lm = ds["m"], ds["Lm"]
        H = np.zeros((m + 3 * Lm, m + 3 * Lm))
        H[:m, :m], H[:m, m:], H[m:, :m] = ds["U"], ds["W"], ds["W"].T
        for l in range(Lm):
            H[m + 3 * l:m + 3 * l + 3, m + 3 * l:m + 3 * l + 3] = ds["V"][l].reshape(3, 3)
        b = np.concatenate([ds["ba"], ds["bb"]])
        runs = [(int(a), int(np.flatnonzero(np.diff(np.r_[ds["marg"][i:], -9]) != 1)[0]) + 1) for i, a in enumerate(ds["marg"])
                if i == 0 or ds["marg"][i - 1] != a - 1]
        dense = bool(c["stages"] & mr.STAGE_DENSE)   # (a landmark-only case: what the landmark part leaves, U | ba)
        out = _mp(mp_marg, H, b, [(m + 3 * l, 3) for l in range(Lm)], runs if dense else [])
        Href, bref = (ref["Hk"], ref["bk"]) if dense else (ref["U"], ref["ba"])
        s = mr._scale(np.diag(Href))
        errs = dict(H=mr._mat_err(out["H"], Href, s), b0=mr._vec_err(out["b0"], bref, s))
        if ref["JtJ"] is not None:
            errs.update(JtJ=mr._mat_err(out["JtJ"], ref["JtJ"], s), Jte0=mr._vec_err(out["Jte0"], ref["Jte0"], s))
            assert out["rank"] == ds["rk"], c["name"]
        for q, e in errs.items():
            if e > worst[0]:
                worst = (e, "%s, %s" % (c["name"], q))
            assert e <= tol, "%s: %s differs from the 40-digit reference by %.3g (2^-60 = %.3g)" % (c["name"], q, e, tol)
    print("long double against 40 digits, %d cases: worst %.3g (%s); 2^-60 = %.3g" % (len(small), worst[0], worst[1], tol))


def _mp(mp_marg, H, b, lm_ranges, dense_ranges):
    """marginalize_mp with its matrices as long double (a float would round them to 2^-53): each entry as the sum of two doubles"""
    res = mp_marg.marginalize_mp(H, b, lm_ranges, dense_ranges, raw=True)
    n = res["n"]

    def ld(x):
        hi = float(x)
        return LD(hi) + LD(float(x - hi))
    out = dict(rank=res["rank"])
    for k in ("H", "JtJ"):
        out[k] = np.array([[ld(res[k][i, j]) for j in range(n)] for i in range(n)], dtype=LD).reshape(n, n)
    for k in ("b0", "Jte0"):
        out[k] = np.array([ld(res[k][i]) for i in range(n)], dtype=LD)
    return out


def test_restatement_meets_every_bar(cases):
    consts = mr.constants(cases)
    for cls, what in ((1, "c1 (identities)"), (3, "c3 (identities, the rule's units)"), (2, "c2 (forward errors)")):
        print("%s = %.4g, set by %s" % (what, consts[cls][0], consts[cls][1]))
    for c in cases:
        for q, v in mr.ratios(c, c["restated"], consts).items():
            assert v <= 1.0, "%s: %s at %.3g of its bar" % (c["name"], q, v)
        if c["restated"]["dropped"] is not None:
            assert c["restated"]["dropped"] == c["ds"]["nk"] - c["ds"]["rk"], c["name"]


def test_eigenvalue_condition(cases):
    for c in cases:
        ok, kappa = mr.check_condition(c["ds"], c["ref"], c["stages"], c.get("margin", mr.MARGIN), c.get("cert", False))
        assert ok, c["name"]
        assert kappa == c["kappa"]
    by = {c["name"]: c for c in cases}
    # family C is ill conditioned where it says, family A is not
    assert 1e4 < by["dense-C-nk17-nm17-k7"]["kappa"]["kappa_M"] < 1e7 < by["dense-C-nk17-nm17-k13"]["kappa"]["kappa_M"] < 1e10
    assert 1e4 < by["final-C-n33-k7"]["kappa"]["kappa_K"] < 1e7 < by["final-C-n33-k13"]["kappa"]["kappa_K"] < 1e10
    assert all(max(c["kappa"].values()) < 1e3 for c in cases if c["family"] == "A")
    # family D reaches the 1e-3 branch of every preconditioner
    for name, block in (("lm-D-Lm129-m17", "V"), ("dense-D-nk17-nm17", "marg"), ("final-D-n17", "Hk")):
        c = by[name]
        d = {"V": c["ds"]["V"][:, [0, 4, 8]].ravel(), "marg": np.diag(c["ds"]["U"])[c["ds"]["marg"]],
             "Hk": np.diag(c["ds"]["U"])}[block]
        assert (d < 1e-9).any() and (d > 1e-9).any() and d.min() > 0, name
        assert c["ds"]["U"].max() > 1e6 and np.abs(c["ds"]["U"])[c["ds"]["U"] != 0].min() < 1e-9


def test_every_edge_is_reached(lib, cases):
    by = {c["name"]: c for c in cases}
    K = mpl.constants(lib)

    def plan(name, eig=0):
        return mr.masked_plan(lib, by[name], eig)
    # ---- landmark part: the blocks of k_marg_lm_prepare (128), one workgroup per row, 16 x 16 tiles, K = 3 Lm in steps of 4
    for Lm, grid in ((1, 1), (127, 1), (128, 1), (129, 2), (255, 2), (256, 2), (257, 3)):
        for m, tiles in ((1, 1), (15, 1), (16, 1), (17, 4), (33, 9)):
            q = plan("lm-A-Lm%d-m%d" % (Lm, m))
            assert (q["lmPrepare_grid"], q["lmApply_grid"], q["lmUpdate_grid"]) == (grid, m, tiles), (Lm, m, q)
    assert plan("lm-A-Lm0-m17")["lmPrepare_grid"] == 0
    assert {3 * Lm % 4 for Lm in mr.LM_SIZES} == {0, 1, 2, 3}          # the k < K predicate of k_marg_lm_update on every remainder
    assert {Lm % 256 for Lm in mr.LM_SIZES} >= {0, 1, 255}             # the stride of k_marg_lm_apply
    kinds = set(by["lm-B-Lm4-m17"]["ds"]["kinds"])
    assert kinds == {"one", "rank1", "zero", "full"} and by["lm-B-Lm1-m1"]["ds"]["kinds"] == ["one"]
    for name in ("lm-A-Lm129-m17", "lm-B-Lm129-m33"):                  # rows of W that are zero: U's rows must come back as they went
        W = by[name]["ds"]["W"]
        assert (~W.any(axis=1)).any() and W.any(axis=1).any(), name
    assert any(c["interleaved"] for c in cases if c["group"] == "landmark") and not all(c["interleaved"] for c in cases if c["group"] == "landmark")
    # ---- dense part
    for c in cases:
        if c["group"] == "dense":
            q = mr.masked_plan(lib, c)
            ds = c["ds"]
            if ds["nk"] and ds["nm"]:
                assert (q["dense_grid"], q["denseTileChol"], q["denseUseLds"], q["copyPair"]) == (1, 1, 1, 0), c["name"]
            elif ds["nk"]:
                assert (q["dense_grid"], q["copyPair"]) == (0, 1), c["name"]
            else:
                assert (q["dense_grid"], q["copyPair"], q["final_grid"]) == (0, 0, 0), c["name"]
    last, first = [n for n in by if n.endswith("-prodLds-last")][0], [n for n in by if n.endswith("-prodLds-first-global")][0]
    assert plan(last)["denseProdLds"] == 1 and plan(first)["denseProdLds"] == 0 and by[first]["ds"]["nk"] == by[last]["ds"]["nk"] + 1
    assert plan("dense-A-nk117-nm27")["denseProdLds"] == 1
    assert {by[n]["ds"]["nm"] - by[n]["ds"]["rm"] for n in by if n.startswith("dense-B")} == {1, 6, 11}
    ds = by["dense-A-nk17-nm6-interleaved"]["ds"]
    assert np.diff(ds["marg"]).max() > 1 and np.diff(ds["keep"]).max() > 1
    # ---- M3: the sizes at which planMargJob changes its answer
    sizes, first6 = mr.final_sizes(lib)
    assert sizes[-1] == first6 and plan("final-A-n%d" % (first6 - 1))["finalMode"] == 4 and plan("final-A-n%d" % first6)["finalMode"] == 6
    maxn = K["kSymEigMaxN"]
    assert maxn in sizes and maxn + 1 in sizes
    q, q1 = plan("final-A-n%d" % maxn), plan("final-A-n%d" % (maxn + 1))
    assert q["finalChol_grid"] == q["finalDc_grid"] == q["finalSkipIfDone"] == 1 and q1["finalChol_grid"] == q1["finalDc_grid"] == q1["finalSkipIfDone"] == 0
    # the fall-back keeps G and Q in LDS up to a size of its own (SVIN_MARG_EIG=jacobi: mode 1 | 0; default: finalFallbackLds)
    lds_both = max(n for n in sizes if mpl.lds(lib, "jacobiLdsBytes", n))
    assert lds_both + 1 in sizes and not mpl.lds(lib, "jacobiLdsBytes", lds_both + 1)
    assert plan("final-A-n%d" % lds_both, 3)["finalMode"] == 1 and plan("final-A-n%d" % (lds_both + 1), 3)["finalMode"] == 0
    assert plan("final-A-n%d" % lds_both)["finalFallbackLds"] == 1 and plan("final-A-n%d" % (lds_both + 1))["finalFallbackLds"] == 0
    for n in sizes:
        modes = mr.final_modes(lib, n)
        assert modes == (["default", "direct", "cholesky", "jacobi"] if n <= maxn else ["default", "jacobi"]), (n, modes)
    for n in (17, 33, maxn, first6):
        for fam_tag in ("B-n%d-null", "C-n%d-k7", "C-n%d-k13"):
            assert "final-" + fam_tag % n in by
    c = by["final-B-n33-null"]
    assert c["ds"]["zero_kept"] == 1 and c["ds"]["rk"] == 33 - 11 - 1 and (np.diag(c["ds"]["U"]) == 0).sum() == 1
    assert by["final-B-n33-short"]["ds"]["rk"] == 22 == by["final-B-n33-short"]["ds"]["Gs"].shape[0]
    c = by["final-C-n17-cert"]
    assert c["ds"]["Gs"].shape[0] <= 32 and set(np.unique(c["ds"]["Gs"] - np.round(c["ds"]["Gs"])) != 0) and c["ds"]["rk"] == 17
    # ---- the whole job
    for Lm, nk, nm in mr.WHOLE_SIZES:
        for fam in "ABCD":
            q = plan("whole-%s-Lm%d-nk%d-nm%d" % (fam, Lm, nk, nm))
            assert q["lmPrepare_grid"] and q["dense_grid"] and q["finalChol_grid"] and q["final_grid"]
    assert plan("whole-A-nothing-kept")["final_grid"] == 0 and plan("whole-A-nothing-kept")["lmPrepare_grid"] == 1
    assert plan("whole-A-no-dense-rows")["lmPrepare_grid"] == 0
