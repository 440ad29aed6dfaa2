"""doglegCoefficients (svin_amd/csrc/trust_region.hpp: the function k_post_solve and k_step_retract call) on the CPU against mpmath
at 50 digits: the three branches (Gauss-Newton step inside the region, Cauchy point outside, interpolation), both signs of cc in
the interpolation -- cc <= 0 needs a Gauss-Newton step that barely leads past the Cauchy point, which a real window only
produces under heavy damping --, and the radii at which a branch changes or a difference cancels.

Tolerance, per output f and without a tuned constant:   tol = n_ops * eps * sum_i |x_i df/dx_i|,
the condition number of the exact expression (derivatives by mp.diff with respect to each of the nine inputs) times the
length of the longest chain of roundings from an input to f, counted off the code with every operation rounding once (a
contracted multiply-add rounds less often):
    gnorm 1, gnnorm 1, alpha 1;  b_dot_a = alpha * gDotGn 2;  a_sq = (alpha gnorm)^2: 3 + 3 + 1 = 7;
    b_minus_a_sq: max(7, 2, gnnorm^2 = 3) + 2 additions = 9;  cc = b_dot_a - a_sq 8;  radius^2 - a_sq 8;
    dd = sqrt(cc cc + b_minus_a_sq (radius^2 - a_sq)): max(17, 9 + 8 + 1) + 1 + 1 = 20;
    beta = (dd - cc) / b_minus_a_sq: 21 + 9 + 1 = 31  (the other form: 8 + 21 + 1 = 30);
    cn = beta 31;  cg = -alpha (1 - beta): 32 + 1 + 1 = 34;
    stepNorm = sqrt(cg cg gHatSq + 2 cg cn gDotGn + cn cn gnHatSq): max(70, 67, 64) + 2 + 1 = 73;
    jdSq = cg cg jgSq - 2 cg cn jvDotJy + cn cn jySq: max(70, 67, 64) + 2 = 72;  jdDotR = cg jvDotR - cn jyDotR: 35 + 1 = 36.
N_OPS below holds the five counts.  The model behind the product: every rounding is a relative perturbation of an intermediate,
and the sensitivity of the result to it is that of the inputs it was formed from -- including where radius^2 - a_sq or 1 - beta
cancel, which is exactly where the derivatives grow.  A perturbation of that size can also carry the inputs across a branch
condition (sqrt(gnHatSq) against radius, alpha sqrt(gHatSq) against radius), and at the Cauchy edge the step is NOT continuous
when cc < 0 (the segment from the Cauchy point to the Gauss-Newton step first dips into the region: beta jumps from 0 to
-2 cc / |b - a|^2, in Ceres as here).  So at an edge the branch is part of the case: it is the one the code's own roundings of
sqrt and alpha select (computed here with the same two IEEE operations), it must lie within a relative distance 3.5 * 73 eps of
the inputs in exact arithmetic (a perturbation delta of every input moves alpha sqrt(gHatSq) / radius by at most 3.5 delta),
and value and condition number are those of that branch's expressions.
Where the code must be exact it is asserted to be: radius == sqrt(gnHatSq) as the code rounds it gives cg = 0, cn = 1."""
import ctypes as C
import os
import subprocess

import sys

import mpmath as mp
import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests", "helpers"))
import step_reference as st        # noqa: E402  (the exact expressions and N_OPS live there: the GPU tests use them too)

EPS = float(np.finfo(np.float64).eps)
N_OPS = st.N_OPS   # cg, cn, stepNorm, jdSq, jdDotR = 34, 31, 73, 72, 36
NAMES = ("cg", "cn", "stepNorm", "jdSq", "jdDotR")
NEWTON, CAUCHY, INTERP = st.NEWTON, st.CAUCHY, st.INTERP


@pytest.fixture(scope="module")
def dogleg(tmp_path_factory):
    so = str(tmp_path_factory.mktemp("dogleg") / "libtr.so")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-Wall", "-Wextra", "-Werror", "-shared", "-fPIC",
                           os.path.join(ROOT, "tests", "csrc", "trust_region_shim.cpp"), "-o", so])
    L = C.CDLL(so)
    L.tr_dogleg.argtypes = [C.POINTER(C.c_double), C.POINTER(C.c_double)]
    L.tr_dogleg.restype = None

    def call(x):
        i, o = (C.c_double * 9)(*[float(v) for v in x]), (C.c_double * 5)()
        L.tr_dogleg(i, o)
        return np.array(list(o))
    return call


def exact_branch(x):
    gHatSq, jgSq, gnHatSq, radius = x[0], x[1], x[2], x[8]
    if mp.sqrt(gnHatSq) <= radius:
        return NEWTON
    if mp.sqrt(gHatSq) * gHatSq / jgSq >= radius:
        return CAUCHY
    return INTERP


def reference(x, code_branch):
    """(values and tolerances of the branch the code takes, exact branch, branches within reach) of one input vector of doubles"""
    with mp.workdps(50):
        xm = [mp.mpf(float(v)) for v in x]
        br = exact_branch(xm)
        reach = {br}
        for s in (-1, 1):
            y = list(xm)
            y[8] = xm[8] * (1 + s * mp.mpf(3.5 * max(N_OPS) * EPS))
            reach.add(exact_branch(y))
        val, tol = st.dogleg_reference(x, code_branch)
        return [float(v) for v in val], [float(t) for t in tol], br, sorted(reach)


def base(seed, cc_positive):
    """nine inputs of a consistent problem: g_hat, gn_hat are vectors of R^6 and |Jv|, |Jy|, r likewise, so that every
    Cauchy-Schwarz inequality the expressions rely on holds; cc > 0 (the usual case) or cc <= 0"""
    rng = np.random.default_rng(seed)
    for _ in range(10000):
        g, gn = rng.normal(size=6), rng.normal(size=6)
        gn *= -np.sign(g @ gn)                       # g_hat . gn_hat < 0 (the device accumulates -g . y)
        gn *= 10.0 ** rng.uniform(0, 2)
        jv, jy, r = rng.normal(size=8) * 10.0 ** rng.uniform(-1, 1), rng.normal(size=8) * 10.0 ** rng.uniform(-1, 1), rng.normal(size=8)
        x = [g @ g, jv @ jv, gn @ gn, g @ gn, jy @ jy, jv @ jy, jv @ r, jy @ r, 0.0]
        alpha = x[0] / x[1]
        a, b = alpha * np.sqrt(x[0]), np.sqrt(x[2])
        cc = -alpha * x[3] - a * a
        if a < 0.7 * b and (cc > 0.05 * a * a) == cc_positive and (cc_positive or cc < -0.05 * a * a):
            return x, a, b
    raise AssertionError("no sample")


def up(v, n=1):
    for _ in range(n):
        v = np.nextafter(v, np.inf)
    return v


def cases():
    out = []
    for seed in range(3):
        for pos in (True, False):
            x, a, b = base(seed, pos)
            gnn = float(np.sqrt(np.float64(x[2])))                              # as the code rounds them
            ag = float(np.sqrt(np.float64(x[0])) * (np.float64(x[0]) / np.float64(x[1])))
            tag = "s%d_cc%s" % (seed, "pos" if pos else "neg")
            radii = [("newton", 2 * gnn, NEWTON), ("cauchy", 0.5 * ag, CAUCHY), ("interp_mid", 0.5 * (ag + gnn), INTERP),
                     ("interp_low", ag + 0.01 * (gnn - ag), INTERP), ("interp_high", gnn - 0.01 * (gnn - ag), INTERP),
                     ("radius_eq_gnnorm", gnn, NEWTON), ("radius_below_gnnorm", float(np.nextafter(gnn, 0)), INTERP),
                     ("radius_eq_cauchy", ag, CAUCHY), ("radius_below_cauchy", float(np.nextafter(ag, 0)), CAUCHY),
                     ("radius_above_cauchy", float(up(ag)), INTERP)]
            radii += [("cancel_%dulp" % n, float(up(ag, n)), INTERP) for n in (2, 5, 40)]
            for name, rad, br in radii:
                out.append(pytest.param(x[:8] + [rad], br, pos, id="%s_%s" % (tag, name)))
    return out


@pytest.mark.parametrize("x,code_branch,cc_positive", cases())
def test_dogleg_coefficients_against_mpmath(dogleg, x, code_branch, cc_positive):
    got = dogleg(x)
    val, tol, br, reach = reference(x, code_branch)
    assert code_branch == st.code_branch(x) and code_branch in reach, "the case does not sit where it was designed to sit"
    with mp.workdps(50):
        alpha = mp.mpf(x[0]) / mp.mpf(x[1])
        assert ((-alpha * mp.mpf(x[3]) - alpha ** 2 * mp.mpf(x[0])) > 0) == cc_positive
    ratios = [abs(g - v) / t if t > 0 else (0.0 if g == v else float("inf")) for g, v, t in zip(got, val, tol)]
    print("branch %d (exact arithmetic: %d, within reach %s): error / tol %s" % (code_branch, br, reach, " ".join("%s %.3g" % nr for nr in zip(NAMES, ratios))))
    assert max(ratios) <= 1.0, dict(zip(NAMES, zip(got, val, tol)))
    if code_branch == NEWTON:
        assert got[0] == 0.0 and got[1] == 1.0 and got[2] == float(np.sqrt(np.float64(x[2])))
    if code_branch == CAUCHY:
        assert got[1] == 0.0 and got[2] == x[8]


def test_all_branches_and_both_signs_are_reached():
    seen = set()
    for p in cases():
        x, br, pos = p.values
        seen.add((br, pos))
    assert seen == {(b, s) for b in (NEWTON, CAUCHY, INTERP) for s in (True, False)}


def test_the_difference_of_squares_cancels_in_the_cancellation_cases():
    """radius^2 - a_sq keeps only a few bits in the cases named cancel_*: they test what they say"""
    for p in cases():
        if "cancel_2ulp" in p.id or "radius_above_cauchy" in p.id:
            x = p.values[0]
            a = np.sqrt(np.float64(x[0])) * (np.float64(x[0]) / np.float64(x[1]))
            assert 0 <= x[8] * x[8] - a * a < 64 * EPS * a * a
