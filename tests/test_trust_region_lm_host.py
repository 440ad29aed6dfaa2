"""The Levenberg-Marquardt choice of the host's trust-region state machine (svin_amd/csrc/trust_region.hpp) on the CPU.

Ceres 2.2 LevenbergMarquardtStrategy: the damping is 1 / radius; an accepted step takes radius / max(1/3, 1 - (2 rho - 1)^3),
at most max_radius, and resets the decrease factor to 2; a rejected or invalid step divides the radius by the decrease factor
and doubles the factor; a failed factorisation is an invalid step (no mu ladder); after either the same linearisation is solved
again under the new damping (reuse = false).  The terminations and the five-invalid-steps failure are the minimiser's and the
same for both strategies.  A state machine that is never configured -- and one configured to dogleg with the default radii --
takes the dogleg decisions it took before the strategy existed: DoglegRules below restates those in Python floats."""
import ctypes as C
import math
import os
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ACCEPTED, REJECTED, INVALID, TERMINATED = 0, 1, 2, 3
DOGLEG, LM = 0, 1
KEYS = ("radius", "mu", "x_cost", "reuse", "initScale", "invalid", "iteration", "successful", "termination", "mu_after_accept",
        "decrease_factor", "step_radius", "strategy", "initial_radius", "max_radius")


@pytest.fixture(scope="module")
def lib(tmp_path_factory):
    so = str(tmp_path_factory.mktemp("trlm") / "libtrlm.so")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-Wall", "-Wextra", "-Werror", "-shared", "-fPIC",
                           os.path.join(ROOT, "tests", "csrc", "trust_region_lm_shim.cpp"), "-o", so])
    L = C.CDLL(so)
    pd = C.POINTER(C.c_double)
    L.trlm_create.restype = C.c_void_p
    L.trlm_create.argtypes = [C.c_int, C.c_double, C.c_double, C.c_double, C.c_double, C.c_double, C.c_int, C.c_double]
    L.trlm_destroy.argtypes = [C.c_void_p]
    L.trlm_begin.argtypes = [C.c_void_p, C.c_int]
    L.trlm_retry.argtypes = [C.c_void_p, pd]
    L.trlm_end.argtypes = [C.c_void_p, pd, pd]
    L.trlm_state.argtypes = [C.c_void_p, pd]
    L.trlm_dogleg.argtypes = [pd, pd]
    return L


class TR:
    def __init__(self, L, cost0, strategy=LM, r0=1e4, rmax=1e16, max_it=10, ftol=1e-6, gtol=1e-10, ptol=1e-8):
        self.L, self.h = L, L.trlm_create(strategy, r0, rmax, ftol, gtol, ptol, max_it, cost0)
        self.row = None

    def begin(self, stop=False):
        return bool(self.L.trlm_begin(self.h, 1 if stop else 0))

    @staticmethod
    def _v(cost, step2=1e-2, x2=1e2, grad=1.0, fail=0.0, jd2=0.0, jdr=0.0, dog=0.1):
        return (C.c_double * 8)(cost, step2, x2, grad, fail, jd2, jdr, dog)

    def retry(self, **kw):
        return bool(self.L.trlm_retry(self.h, self._v(**kw)))

    def end(self, **kw):
        row = (C.c_double * 6)(*([float("nan")] * 6))
        o = self.L.trlm_end(self.h, self._v(**kw), row)
        self.row = list(row)
        return o

    def state(self):
        o = (C.c_double * 15)()
        self.L.trlm_state(self.h, o)
        return dict(zip(KEYS, list(o)))


def model(decrease):
    """jdSq / jdDotR such that model_cost_change = -(jdDotR + jdSq / 2) = decrease"""
    return dict(jd2=2.0 * decrease, jdr=-2.0 * decrease)


def step_with_rho(t, rho, decrease=100.0):
    """one iteration whose relative decrease is rho (cost change rho * decrease against a model change of `decrease`)"""
    x = t.state()["x_cost"]
    assert t.begin()
    assert t.state()["mu"] == 1.0 / t.state()["radius"]          # the damping of every build is 1 / radius
    assert not t.retry(cost=x - rho * decrease)
    return t.end(cost=x - rho * decrease, **model(decrease))


def accepted_radius(radius, rho, rmax):
    return min(rmax, radius / max(1.0 / 3.0, 1.0 - math.pow(2.0 * rho - 1.0, 3)))


def test_radius_and_decrease_factor_follow_scripted_rho(lib):
    t = TR(lib, 1000.0, max_it=100)
    s = t.state()
    assert s["radius"] == 1e4 and s["mu"] == 1e-4 and s["decrease_factor"] == 2.0 and s["step_radius"] == math.inf and s["strategy"] == LM
    radius = 1e4
    # the clamp max(1/3, .) is active above rho = (1 + (2/3)^(1/3)) / 2 = 0.9368: both sides of it, and well inside either region
    for rho in (0.99, 0.938, 0.936, 0.5, 0.2, 0.0011):
        spec = t.state()["mu_after_accept"]
        assert step_with_rho(t, rho) == ACCEPTED
        seen = t.row[1]      # (rho as the state machine formed it from the costs: the script's to a rounding)
        assert abs(seen - rho) < 1e-12
        radius = accepted_radius(radius, seen, 1e16)
        s = t.state()
        assert s["radius"] == radius and s["mu"] == 1.0 / radius and s["decrease_factor"] == 2.0 and s["reuse"] == 0
        clamped = 1.0 - math.pow(2.0 * seen - 1.0, 3) <= 1.0 / 3.0
        assert clamped == (rho > 0.937)
        assert (spec == s["mu"]) == clamped      # bitwise: what the speculative build assumed is what the clamped step leaves
        assert t.row[2] == radius and t.row[5] == ACCEPTED and t.row[0] == s["x_cost"]
    # rho = 0.5: the factor is exactly 1; rho = 0.2 shrinks (1 - (-0.6)^3 = 1.216); checked against the closed forms
    assert accepted_radius(1.0, 0.5, 1e16) == 1.0 and np.isclose(accepted_radius(1.0, 0.2, 1e16), 1.0 / 1.216, rtol=1e-15)
    # rejected steps: radius / 2, / 4, / 8; the factor doubles; the linearisation is solved again (reuse stays false)
    for k, rho in enumerate((5e-4, -0.3, 9e-4)):       # (min_relative_decrease is 1e-3)
        mu_used = t.state()["mu"]
        assert step_with_rho(t, rho) == REJECTED
        radius = radius / 2.0 ** (k + 1)
        s = t.state()
        assert s["radius"] == radius and s["mu"] == 1.0 / radius and s["decrease_factor"] == 2.0 ** (k + 2) and s["reuse"] == 0
        assert t.row[4] == mu_used and t.row[5] == REJECTED and t.row[2] == radius
    # an accepted step resets the factor
    assert step_with_rho(t, 0.6) == ACCEPTED and t.state()["decrease_factor"] == 2.0
    assert step_with_rho(t, -0.1) == REJECTED and t.state()["decrease_factor"] == 4.0


def test_cap_at_max_radius(lib):
    t = TR(lib, 1000.0, r0=4.0, rmax=20.0, max_it=100)
    assert step_with_rho(t, 0.99) == ACCEPTED and t.state()["radius"] == 4.0 / (1.0 / 3.0)
    assert t.state()["mu_after_accept"] == 1.0 / 20.0          # the speculation knows the cap
    assert step_with_rho(t, 0.99) == ACCEPTED and t.state()["radius"] == 20.0 and t.state()["mu"] == 1.0 / 20.0
    assert step_with_rho(t, 0.99) == ACCEPTED and t.state()["radius"] == 20.0
    # both radii apply to dogleg as well
    d = TR(lib, 1.0, strategy=DOGLEG, r0=7.0, rmax=50.0)
    assert d.state()["radius"] == 7.0 and d.state()["mu"] == 1e-8 and d.state()["step_radius"] == 7.0
    assert d.begin() and d.end(cost=0.1, dog=1e3, **model(0.9)) == ACCEPTED and d.state()["radius"] == 50.0


def test_invalid_steps(lib):
    t = TR(lib, 10.0, max_it=100)
    # a failed factorisation: never retried (no mu ladder), the step is invalid even if the model looks fine
    assert t.begin() and not t.retry(cost=9.0, fail=1.0)
    assert t.state()["mu"] == 1e-4
    assert t.end(cost=9.0, **model(1.0)) == INVALID
    s = t.state()
    assert s["radius"] == 5e3 and s["mu"] == 1.0 / 5e3 and s["decrease_factor"] == 4.0 and s["reuse"] == 0 and s["invalid"] == 1
    assert s["x_cost"] == 10.0 and s["initScale"] == 0
    assert t.row[1] == 0.0 and t.row[3] == 0.0 and t.row[4] == 1e-4 and t.row[5] == INVALID and t.row[2] == 5e3
    # every failure bit below 4 counts (1 = reduced system, 2 = a landmark block, 3 = both)
    for fail in (2.0, 3.0):
        assert t.begin() and not t.retry(cost=9.0, fail=fail) and t.end(cost=9.0, **model(1.0)) == INVALID
    assert t.state()["radius"] == 5e3 / 4.0 / 8.0 and t.state()["invalid"] == 3
    # a non-positive model change is invalid too; a valid step resets the count
    assert t.begin() and not t.retry(cost=9.0) and t.end(cost=9.0, **model(-1.0)) == INVALID and t.state()["invalid"] == 4
    assert step_with_rho(t, 0.5) == ACCEPTED and t.state()["invalid"] == 0 and t.state()["decrease_factor"] == 2.0
    # five in a row: FAILURE
    for k in range(1, 5):
        assert t.begin() and t.end(cost=9.0, **model(0.0)) == INVALID and t.state()["invalid"] == k
    assert t.begin() and t.end(cost=9.0, **model(0.0)) == TERMINATED and t.state()["termination"] == 3


def test_terminations_are_the_minimisers(lib):
    t = TR(lib, 5.0)
    assert t.begin() and t.end(cost=5.0, grad=1e-11, **model(1.0)) == TERMINATED and t.state()["termination"] == 0 and t.state()["iteration"] == 0
    t = TR(lib, 5.0)
    assert t.begin() and t.end(cost=4.0, step2=1e-20, x2=1.0, **model(1.0)) == TERMINATED and t.state()["termination"] == 0
    t = TR(lib, 5.0)
    assert t.begin() and t.end(cost=5.0 - 1e-7, **model(1.0)) == TERMINATED and t.state()["termination"] == 0
    # the gradient test comes before the validity of the step, the parameter test before the function test (as in dogleg mode)
    t = TR(lib, 5.0)
    assert t.begin() and t.end(cost=4.0, grad=1e-11, **model(-1.0)) == TERMINATED and t.state()["invalid"] == 0
    t = TR(lib, 5.0, max_it=2)
    for _ in range(2):
        assert step_with_rho(t, 0.5) == ACCEPTED
    assert not t.begin() and t.state()["termination"] == 1
    t = TR(lib, 5.0)
    assert not t.begin(stop=True) and t.state()["termination"] == 2
    # rejected steps collapse the radius much faster than dogleg's halving: 2^(k (k + 1) / 2)
    t = TR(lib, 5.0, max_it=500)
    n = 0
    while t.begin():
        assert t.end(cost=6.0, **model(1.0)) == REJECTED
        n += 1
    assert t.state()["termination"] == 0 and t.state()["radius"] <= 1e-32 and 10 < n < 20


def test_the_step_of_an_infinite_radius_is_the_gauss_newton_step(lib):
    """what the driver hands the device in Levenberg-Marquardt mode: doglegCoefficients at radius = +inf is cg = 0, cn = 1,
    |J delta|^2 = |J y|^2 and (J delta).r = -(J y).r to the bit, whatever the other sums hold"""
    rng = np.random.default_rng(5)
    for _ in range(200):
        v = np.concatenate([rng.uniform(1e-8, 1e8, 3), rng.normal(0, 1e3, 1), rng.uniform(1e-8, 1e8, 1), rng.normal(0, 1e3, 3), [np.inf]])
        out = np.zeros(5)
        lib.trlm_dogleg(v.ctypes.data_as(C.POINTER(C.c_double)), out.ctypes.data_as(C.POINTER(C.c_double)))
        assert out[0] == 0.0 and out[1] == 1.0 and out[2] == math.sqrt(v[2]) and out[3] == v[4] and out[4] == -v[7]


class DoglegRules:
    """the dogleg decisions as they stood before the strategy existed, in Python floats (IEEE doubles, the same operations)"""

    def __init__(self, cost0, max_it, ftol=1e-6, gtol=1e-10, ptol=1e-8):
        self.ftol, self.gtol, self.ptol, self.max_it = ftol, gtol, ptol, max_it
        self.radius, self.mu, self.x_cost = 1e4, 1e-8, cost0
        self.reuse, self.init_scale, self.invalid, self.iteration, self.successful, self.termination, self.step_ok = False, True, 0, 0, 0, 1, True

    def begin(self, stop):
        if stop:
            self.termination = 2
            return False
        if self.iteration >= self.max_it:
            self.termination = 1
            return False
        if self.radius <= 1e-32:
            self.termination = 0
            return False
        self.iteration += 1
        self.step_ok = True
        return True

    def mu_after_accept(self):
        return max(1e-8, 2.0 * self.mu / 10.0)

    def retry(self, fail):
        if self.reuse or fail == 0.0:
            return False
        self.mu *= 10.0
        if self.mu < 1.0:
            return True
        self.step_ok = False
        return False

    def end(self, cost, step2, x2, grad, jd2, jdr, dog):
        if not self.reuse:
            self.init_scale, self.reuse = False, True
        if grad <= self.gtol:
            self.iteration -= 1
            self.termination = 0
            return TERMINATED
        mcc = -(jdr + 0.5 * jd2)
        if not self.step_ok or not (mcc > 0.0):
            self.invalid += 1
            if self.invalid >= 5:
                self.termination = 3
                return TERMINATED
            self.mu *= 10.0
            self.reuse = False
            return INVALID
        self.invalid = 0
        if math.sqrt(step2) <= self.ptol * (math.sqrt(x2) + self.ptol):
            self.termination = 0
            return TERMINATED
        change = self.x_cost - cost
        if abs(change) <= self.ftol * self.x_cost:
            self.termination = 0
            return TERMINATED
        rho = change / mcc
        if rho > 1e-3:
            self.x_cost = cost
            self.successful += 1
            if rho < 0.25:
                self.radius *= 0.5
            if rho > 0.75:
                self.radius = max(self.radius, 3.0 * dog)
            self.radius = min(self.radius, 1e16)
            self.mu = self.mu_after_accept()
            self.reuse = False
            return ACCEPTED
        self.radius *= 0.5
        self.reuse = True
        return REJECTED

    def state(self):
        return dict(radius=self.radius, mu=self.mu, x_cost=self.x_cost, reuse=float(self.reuse), initScale=float(self.init_scale),
                    invalid=float(self.invalid), iteration=float(self.iteration), successful=float(self.successful),
                    termination=float(self.termination), mu_after_accept=self.mu_after_accept())


@pytest.mark.parametrize("configured", [False, True])
def test_a_default_object_takes_the_dogleg_decisions_it_always_took(lib, configured):
    """the random trajectory of test_trust_region_host.py's two-ranks test (same generator, same seed, same draws) and the scripted
    ladder of its mu test, replayed on the state machine -- never configured, or configured to dogleg with the default radii -- and
    on DoglegRules: every decision and every state field equal to the bit"""
    def make(cost0, max_it):
        return TR(lib, cost0, strategy=DOGLEG if configured else -1, max_it=max_it), DoglegRules(cost0, max_it)

    def same(a, b):
        sa, sb = a.state(), b.state()
        assert {k: sa[k] for k in sb} == sb and sa["step_radius"] == sa["radius"] and sa["strategy"] == DOGLEG
    rng = np.random.default_rng(17)
    a, b = make(50.0, 400)
    steps, outcomes = 0, set()
    while True:
        stop = steps == 350
        ra, rb = a.begin(stop), b.begin(stop)
        assert ra == rb
        if not ra:
            break
        fail_rounds = int(rng.integers(0, 3)) if rng.random() < 0.2 else 0
        for k in range(fail_rounds + 1):
            rec = dict(cost=float(a.state()["x_cost"] * rng.uniform(0.5, 1.05)), fail=1.0 if k < fail_rounds else 0.0)
            qa, qb = a.retry(**rec), b.retry(rec["fail"])
            assert qa == qb
            same(a, b)
            if not qa:
                break
        dec = float(a.state()["x_cost"] * rng.uniform(-0.05, 0.3))
        rec = dict(cost=float(a.state()["x_cost"] - dec * rng.uniform(0.0, 1.2)), step2=float(rng.uniform(1e-6, 1.0)), x2=100.0,
                   grad=float(rng.uniform(1e-3, 10.0)), dog=float(rng.uniform(0.01, 1e5)), **model(dec))
        oa, ob = a.end(**rec), b.end(**rec)
        assert oa == ob
        same(a, b)
        outcomes.add(oa)
        steps += 1
        if oa == TERMINATED:
            break
    assert steps > 20 and {ACCEPTED, REJECTED, INVALID}.issubset(outcomes)
    # the mu ladder up to max_mu, the invalid step behind it and the failure after five
    a, b = make(10.0, 10)
    assert a.begin() and b.begin(False)
    while True:
        qa, qb = a.retry(cost=10.0, fail=1.0), b.retry(1.0)
        assert qa == qb
        same(a, b)
        if not qa:
            break
    for k in range(5):
        rec = dict(cost=9.0, step2=1e-2, x2=1e2, grad=1.0, dog=0.1, **model(1.0 if k == 0 else -1.0))
        assert a.end(**rec) == b.end(**rec)
        same(a, b)
        if k < 4:
            assert a.begin() and b.begin(False)
    assert a.state()["termination"] == 3
