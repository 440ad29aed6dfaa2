"""The marginalisation algebra M2 / M3 (svin_amd/csrc/marg.hip from k_marg_lm_prepare to k_marg_final) on systems handed to it
directly, at the edges of every route marg_plan.hpp knows: through svin_ba_debug_marginalize, which runs the job's own launches
(the function Window::launchMarginalization calls) on a caller-given system after M1, against the long-double reference and the
bars of tests/helpers/marg_reference.py (read its text for the designs, the reference and where each bar comes from;
tests/test_marg_reference_host.py shows on the CPU that the reference equals the 40-digit one and that a float64 restatement
meets every bar).  The constants of the bars are recomputed here from that restatement: nothing in them comes from the device.

Per case: the plan the library walked is the plan the planner gives with the masked stages taken out (a test that silently ran
another route would prove nothing), the route the device took (flag[5] of the dense part; flag[3], flag[4] of M3) is the one the
design predicts, and every quantity is within its bar.  Every line printed is `case; route; the quantity nearest its bar, in
units of the bar`; the last lines give the worst case per route (DESIGN.md quotes them)."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "helpers"))
import marg_plan_lib as mpl          # noqa: E402
import marg_reference as mr          # noqa: E402

pytestmark = pytest.mark.gpu
ROUTE_NAMES = {-8: "k_marg_final_chol (certified)", -7: "k_marg_final_dc", -4: "k_marg_final mode 4", -6: "k_marg_final mode 6",
               0: "k_marg_final fall-back"}


@pytest.fixture(scope="module")
def planner(tmp_path_factory):
    return mpl.build_shim(tmp_path_factory.mktemp("marg_gpu_edges"))


@pytest.fixture(scope="module")
def suite(planner):
    """every case (built once, shared, never modified), the constants of the bars, and the per-route record the run prints last"""
    cases = [mr.build(s) for s in mr.all_specs(planner)]
    consts = mr.constants(cases)
    record = {}
    yield dict(cases=cases, consts=consts, record=record, by={c["name"]: c for c in cases})
    print("\nworst case per route, in units of its bar (c1 = %.4g, c3 = %.4g, c2 = %.4g):" % (consts[1][0], consts[3][0], consts[2][0]))
    for route in sorted(record):
        v, who = record[route]
        print("  %-40s %.3g  (%s)" % (route, v, who))


def run(case, stages=None):
    from svin_amd.estimator import Estimator
    ds = case["ds"]
    return Estimator.debug_marginalize(ds["U"], ds["ba"], ds["W"], ds["V"], ds["bb"], ds["marg_rows"], case["stages"] if stages is None else stages)


def assert_plan_taken(res, planner, case, eig=0):
    want = mr.masked_plan(planner, case, eig)
    got = {k: res[k] for k in mr.PLAN_FIELDS}
    assert got == want, "%s: the library walked %s, the planner gives %s" % (case["name"], got, want)
    assert (res["nk"], res["nm"]) == (case["ds"]["nk"], case["ds"]["nm"])


RULE_UNITS = " (rule units)"


def check_bars(suite, case, res, routes, rule_units=None):
    """every quantity of the case within its bar; records the worst under each route name.  rule_units: None all quantities,
    False without / True only the identities in the units of the rule's preconditioner"""
    ratios = {q: v for q, v in mr.ratios(case, res, suite["consts"]).items() if rule_units is None or q.endswith(RULE_UNITS) == rule_units}
    for k in ("U", "ba", "Hk", "bk", "J", "e0", "Ht", "bp"):
        assert res[k] is None or np.all(np.isfinite(res[k])), "%s: %s is not finite" % (case["name"], k)
    worst = max(ratios.items(), key=lambda kv: kv[1], default=("nothing to compare", 0.0))
    print("%s; %s; %s at %.3g" % (case["name"], " + ".join(routes) or "no launch", worst[0], worst[1]))
    for q, v in ratios.items():
        stage = "landmark part" if q in ("U", "ba", "U symmetry") else routes[-1] if q not in ("Hk", "bk") else [r for r in routes if r.startswith(("k_marg_dense", "copy"))][0]
        if v > suite["record"].get(stage, (-1.0, ""))[0]:
            suite["record"][stage] = (v, "%s, %s" % (case["name"], q))
    for q, v in ratios.items():
        assert v <= 1.0, "%s: %s at %.3g of its bar" % (case["name"], q, v)
    return ratios


def for_each(cases, body):
    """body(case) on every case; the failures of all of them in one assertion (one failing case does not hide the next)"""
    failures = []
    for case in cases:
        try:
            body(case)
        except AssertionError as e:
            failures.append((str(e).splitlines() or [case["name"]])[0])
    assert not failures, "%d of %d cases fail:\n%s" % (len(failures), len(cases), "\n".join(failures))


def dense_route(res):
    if res["copyPair"]:
        return "copy pair"
    return "k_marg_dense %s, products %s" % ("certified Cholesky" if res["flags"][5] == 1 else "eigen-solve", "in LDS" if res["denseProdLds"] else "from global memory")


def test_invalid_arguments_are_refused():
    from svin_amd.estimator import Estimator
    U, ba, z = np.eye(2), np.zeros(2), np.zeros(0)
    for rows, stages in (([0, 2], 7), ([0, 1], 0), ([0, 1], 8), ([0, 1], 4), ([0, 1], 5)):
        with pytest.raises(RuntimeError, match="-1"):
            Estimator.debug_marginalize(U, ba, z, z, z, rows, stages)


def test_landmark_part(planner, suite):
    def body(case):
        ds, res = case["ds"], run(case)
        assert_plan_taken(res, planner, case)
        assert res["Hk"] is None and res["J"] is None
        check_bars(suite, case, res, ["landmark part"] if ds["Lm"] else [])
        untouched = ~ds["W"].any(axis=1) if ds["Lm"] else np.ones(ds["m"], bool)
        # a row W does not touch comes back bit for bit (Lm = 0: nothing is launched and all of U | ba does)
        assert np.array_equal(res["U"][untouched], ds["U"][untouched]) and np.array_equal(res["U"][:, untouched], ds["U"][:, untouched]), case["name"]
        assert np.array_equal(res["ba"][untouched], ds["ba"][untouched]), case["name"]
    for_each([c for c in suite["cases"] if c["group"] == "landmark"], body)


def test_dense_part(planner, suite):
    def body(case):
        ds, res = case["ds"], run(case)
        assert_plan_taken(res, planner, case)
        assert res["J"] is None
        if ds["nk"] == 0:
            assert res["Hk"] is None and np.array_equal(res["U"], ds["U"]), case["name"]
            return
        lm = ["landmark part"] if case["stages"] & mr.STAGE_LM else []
        check_bars(suite, case, res, lm + [dense_route(res)])
        if ds["nm"] == 0:     # the copy pair returns what the landmark part left, bit for bit
            assert np.array_equal(res["Hk"], res["U"]) and np.array_equal(res["bk"], res["ba"]), case["name"]
            if not lm:
                assert np.array_equal(res["Hk"], ds["U"]) and np.array_equal(res["bk"], ds["ba"]), case["name"]
            return
        assert np.array_equal(res["U"], ds["U"]) and np.array_equal(res["ba"], ds["ba"]), case["name"]   # (the dense part reads U | ba only)
        if case["family"] == "A" or case.get("pair_m") == 7:
            assert res["flags"][5] == 1, "%s: the certified Cholesky route was expected" % case["name"]
        elif case["family"] == "B":
            assert res["flags"][5] == 0, "%s: a rank-deficient block went through the certificate" % case["name"]
    for_each([c for c in suite["cases"] if c["group"] == "dense"], body)


def final_route(res):
    return ROUTE_NAMES[res["flags"][3]]


def final_results(planner, suite, debug_option, case):
    """{SVIN_MARG_EIG setting: the hook's result} of an M3 case under every setting whose plan differs, run once per session"""
    cache = suite.setdefault("final_results", {})
    if case["name"] not in cache:
        cache[case["name"]] = {}
        for mode in mr.final_modes(planner, case["ds"]["nk"]):
            debug_option("SVIN_MARG_EIG", mr.EIG_MODES.index(mode))
            cache[case["name"]][mode] = run(case)
    return cache[case["name"]]


def test_final_routes(planner, suite, debug_option):
    """M3 over the n grid x SVIN_MARG_EIG: the route taken, the dropped directions, the four identities and c0 in the units
    s = sqrt(diag), and the routes against one another.  (The identities in the rule's units: the next test.)"""
    consts = suite["consts"]

    def body(case):
        ds, n = case["ds"], case["ds"]["nk"]
        results, problems = {}, []

        def one_mode(mode, eig, res):
            what = "%s, SVIN_MARG_EIG=%s" % (case["name"], mode)
            assert_plan_taken(res, planner, case, eig)
            assert np.array_equal(res["Hk"], ds["U"]) and np.array_equal(res["bk"], ds["ba"]), what
            want = mr.expected_final_route(case, mode, mr.masked_plan(planner, case, eig))
            assert res["flags"][3] == want, "%s: route %s, expected %s" % (what, ROUTE_NAMES.get(res["flags"][3]), ROUTE_NAMES[want])
            assert res["flags"][4] == (1 if want in (-8, -7) else 0), what
            dropped = res["flags"][2]
            assert ds["zero_kept"] <= dropped <= n - ds["rk"], "%s: %d eigen-directions dropped, %d rows are zero and the rank is %d" % (what, dropped, ds["zero_kept"], ds["rk"])
            if case.get("cert"):
                assert dropped == 0, what
            zero_rows = ~res["J"].any(axis=1)
            assert zero_rows.sum() == dropped and not res["e0"][zero_rows].any(), "%s: rows of J / entries of e0 of dropped directions" % what
            check_bars(suite, dict(case, name=what), res, ["copy pair", final_route(res)], rule_units=False)
        results.update(final_results(planner, suite, debug_option, case))
        for mode in results:
            eig = mr.EIG_MODES.index(mode)
            try:
                one_mode(mode, eig, results[mode])
            except AssertionError as e:
                problems.append((str(e).splitlines() or [mode])[0])
        assert not problems, " | ".join(problems)
        # the routes agree with one another within the sum of their bars
        ref = case["ref"]
        s1 = mr._scale(np.diag(ref["Hk"]))
        modes = list(results)
        for i, a in enumerate(modes):
            for b in modes[i + 1:]:
                ra, rb = results[a], results[b]
                Ja, Jb = np.asarray(ra["J"], dtype=mr.LD), np.asarray(rb["J"], dtype=mr.LD)
                ea, eb = np.asarray(ra["e0"], dtype=mr.LD), np.asarray(rb["e0"], dtype=mr.LD)
                bar = 2 * consts[1][0] * n * mr.EPS
                assert mr._mat_err(Ja.T @ Ja, Jb.T @ Jb, s1) <= bar, "%s: J^T J of %s and %s" % (case["name"], a, b)
                assert mr._vec_err(Ja.T @ ea, Jb.T @ eb, s1) <= bar, "%s: J^T e0 of %s and %s" % (case["name"], a, b)
                bar = 2 * consts[2][0] * case["kappa"]["kappa_K"] * n * mr.EPS
                assert abs(ra["c0"] - rb["c0"]) / max(1.0, float(ref["c0"])) <= bar, "%s: c0 of %s and %s" % (case["name"], a, b)
    for_each([c for c in suite["cases"] if c["group"] == "final"], body)


def test_final_identities_in_rule_units(planner, suite, debug_option):
    """The four identities of M3 in the units of the rule's own preconditioner, with the constant c3 (marg_reference.py: the
    tighter of the two bars, since family D does not set it), and the routes against one another in the same units.

    This is the bar that found two defects, repaired in the same change (DESIGN.md section 19d has the figures before and after):
    k_marg_final_chol's products with explicit inverses on an ill-conditioned prior that passes its certificate (J^T e0 at 24.5 of
    the bar at n = 33, kappa 7e8) and the orthogonality k_marg_final's Cholesky-preconditioned Jacobi stops at (J^T e0 at 1.25 of
    the bar at n = 17)."""
    consts = suite["consts"]

    def body(case):
        n, ref = case["ds"]["nk"], case["ref"]
        results, problems = final_results(planner, suite, debug_option, case), []
        for mode, res in results.items():
            try:
                check_bars(suite, dict(case, name="%s, SVIN_MARG_EIG=%s" % (case["name"], mode)), res, ["copy pair", final_route(res)], rule_units=True)
            except AssertionError as e:
                problems.append((str(e).splitlines() or [mode])[0])
        s3 = np.asarray(mr.p_rule(np.diag(ref["Hk"]).astype(np.float64)), dtype=mr.LD)
        bar = 2 * consts[3][0] * n * mr.EPS
        modes = list(results)
        for i, a in enumerate(modes):
            for b in modes[i + 1:]:
                Ja, Jb = np.asarray(results[a]["J"], dtype=mr.LD), np.asarray(results[b]["J"], dtype=mr.LD)
                ea, eb = np.asarray(results[a]["e0"], dtype=mr.LD), np.asarray(results[b]["e0"], dtype=mr.LD)
                if mr._mat_err(Ja.T @ Ja, Jb.T @ Jb, s3) > bar or mr._vec_err(Ja.T @ ea, Jb.T @ eb, s3) > bar:
                    problems.append("%s: J^T J / J^T e0 of %s and %s differ by more than the sum of their bars" % (case["name"], a, b))
        assert not problems, " | ".join(problems)
    for_each([c for c in suite["cases"] if c["group"] == "final"], body)


def test_whole_job(planner, suite):
    keys = ("U", "ba", "Hk", "bk", "J", "e0", "Ht", "bp", "scal")

    def body(case):
        ds, res, again = case["ds"], run(case), run(case)
        assert_plan_taken(res, planner, case)
        for k in keys:     # the job sums in a fixed order: the same bits twice
            assert (res[k] is None and again[k] is None) or np.array_equal(res[k], again[k], equal_nan=True), "%s: %s differs between two calls" % (case["name"], k)
        assert res["flags"] == again["flags"], case["name"]
        if ds["nk"] == 0:
            assert res["Hk"] is None and res["J"] is None and res["c0"] is None, case["name"]
            check_bars(suite, case, res, ["landmark part"] if ds["m"] else [])
            return
        check_bars(suite, case, res, ["landmark part", dense_route(res), final_route(res)])
        if case["family"] in "AC":
            assert res["flags"][5] == 1 and res["flags"][3] == -8 and res["flags"][2] == 0, case["name"]
        elif case["family"] == "B":
            assert res["flags"][5] == 0 and res["flags"][3] == -7, case["name"]
            assert ds["zero_kept"] <= res["flags"][2] <= ds["nk"] - ds["rk"], case["name"]
            assert (~res["J"].any(axis=1)).sum() == res["flags"][2], case["name"]
    for_each([c for c in suite["cases"] if c["group"] == "whole"], body)
