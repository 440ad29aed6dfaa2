"""Ceres 2.2's TrustRegionMinimizer with both trust-region strategies' ComputeStep -- TRADITIONAL_DOGLEG and
LevenbergMarquardtStrategy -- restated in float64 numpy on a DENSE Jacobian: the reference the device's Levenberg-Marquardt solve
is held against, because the oracle's Map::solve is dogleg only.

The minimiser and the dogleg step follow oracle/orc_map.cpp's Map::solve line by line (Jacobi scaling 1 / (1 + sqrt(h)) fixed at
iteration 0, the diagonal clamped to [1e-6, 1e32] in the scaled system, the mu ladder, monotonic steps, min_relative_decrease
1e-3, five invalid steps = failure, step and state norms in ambient coordinates).  The Levenberg-Marquardt strategy follows
oracle/orc_posegraph.cpp's reading of levenberg_marquardt_strategy.cc: D^2 = clamp(diag(J'J)) / radius, the step of
(J'J + D^2) taken whole, radius / max(1/3, 1 - (2 rho - 1)^3) capped at max_radius after an accepted step, radius /=
decrease_factor and decrease_factor *= 2 after a rejected or invalid one, a failed factorisation an invalid step.

The problem comes from an oracle Map (anything with residual_ids / parameters_of / dims / eval / is_constant / get_param /
set_param / residual_kind): the Jacobian is assembled from the per-residual evaluation -- minimal Jacobians, the loss applied as
Ceres' Corrector does (both losses have rho'' <= 0: residual and Jacobian scale by sqrt(rho')), constant blocks without columns --
and (J'J + D^2) is solved densely by Cholesky.  Candidates are formed by the manifolds' Plus, restated here, and written with
set_param.  Dogleg mode must reproduce the oracle's own solve (tests/test_lm_reference_host.py): that is what licenses the
Levenberg-Marquardt mode as a reference.  Nothing of the library under test is imported."""
import math
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from tiny_window_cost import pose_oplus  # noqa: E402

ACCEPTED, REJECTED, INVALID = 0, 1, 2
LOSS_NONE, LOSS_CAUCHY, LOSS_HUBER = 0, 1, 2
COLUMNS = ("cost", "relative_decrease", "radius", "step_norm", "mu", "outcome")


def default_loss(m, rid):
    """what an Estimator-built window has: CauchyLoss(1) on reprojection residuals (kind 0), none elsewhere"""
    return (LOSS_CAUCHY, 1.0) if m.residual_kind(rid) == 0 else (LOSS_NONE, 1.0)


def loss_rho(kind, a, s):
    """rho(s), rho'(s) of ceres::CauchyLoss(a) / HuberLoss(a) / no loss"""
    if kind == LOSS_CAUCHY:
        b = a * a
        return b * math.log1p(s / b), 1.0 / (1.0 + s / b)
    if kind == LOSS_HUBER:
        b = a * a
        if s <= b:
            return s, 1.0
        r = math.sqrt(s)
        return 2.0 * a * r - b, max(a / r, np.finfo(float).tiny)
    return s, 1.0


def plus(dims, x, d):
    """Manifold::Plus by block shape: (7, 6) PoseManifold (Transformation::oplus), (9, 9) Euclidean, (4, 3) HomogeneousPointManifold"""
    if dims == (7, 6):
        return pose_oplus(x, d)
    if dims == (9, 9):
        return x + d
    if dims == (4, 3):
        return np.r_[x[:3] + d, x[3] + 0.0]
    raise NotImplementedError("block of shape %r (reduced pose manifolds are not restated here)" % (dims,))


class DenseProblem:
    def __init__(self, m, loss_of=None):
        self.m = m
        self.loss_of = loss_of or (lambda rid: default_loss(m, rid))
        self.rids = m.residual_ids()
        self.res, shape, self.M = [], {}, 0
        for rid in self.rids:
            pids = m.parameters_of(rid)
            mm, blocks = m.dims(rid)
            for p, b in zip(pids, blocks):
                shape[p] = b
            self.res.append((rid, pids, mm, self.M, self.loss_of(rid)))
            self.M += mm
        # variable blocks referenced by a residual, in parameter-id order (the oracle's order)
        self.var = [p for p in sorted(shape) if not m.is_constant(p)]
        self.shape = shape
        self.off, self.n = {}, 0
        for p in self.var:
            self.off[p] = self.n
            self.n += shape[p][1]

    def snapshot(self):
        return [np.array(self.m.get_param(p), float) for p in self.var]

    def restore(self, xs):
        for p, x in zip(self.var, xs):
            self.m.set_param(p, x)

    def apply(self, xs, delta):
        out = []
        for p, x in zip(self.var, xs):
            xp = plus(self.shape[p], x, delta[self.off[p]:self.off[p] + self.shape[p][1]])
            self.m.set_param(p, xp)
            out.append(np.array(self.m.get_param(p), float))   # (as the map holds it)
        return out

    def evaluate(self, jac):
        """cost, and with jac the corrected residual vector and dense Jacobian at the map's current values (without: the residuals
        as the error terms return them, no Jacobian)"""
        cost = 0.0
        r = np.zeros(self.M)
        J = np.zeros((self.M, self.n)) if jac else None
        for rid, pids, mm, row, (kind, a) in self.res:
            if jac:
                rr, _, Jms = self.m.eval(rid)
            else:
                rr = self.m.eval(rid, jac=False)
            s = float(rr @ rr)
            rho0, rho1 = loss_rho(kind, a, s)
            cost += 0.5 * rho0
            r[row:row + mm] = rr
            if jac:
                w = math.sqrt(rho1)
                r[row:row + mm] = w * rr
                for p, Jm in zip(pids, Jms):
                    if p in self.off:
                        J[row:row + mm, self.off[p]:self.off[p] + Jm.shape[1]] += w * Jm   # (+=: a block may appear twice)
        return cost, r, J


def minimize(m, strategy="lm", max_iterations=50, function_tolerance=1e-6, gradient_tolerance=1e-10, parameter_tolerance=1e-8,
             initial_radius=1e4, max_radius=1e16, loss_of=None, defect=None, oracle_residual_vector=False):
    """Solve the map in place.  strategy "dogleg" | "lm".  Returns dict(log=(n, 6) array -- cost held after the iteration, relative
    decrease, radius after, step norm, mu used, outcome 0 accepted / 1 rejected / 2 invalid; an iteration on which the solve ends has
    no row --, iterations, successful, termination (0 convergence, 1 iteration limit, 3 failure), initial_cost, final_cost,
    cost_history (the oracle's: one entry per iteration incl. the start), grad_max, last_cost_change).
    defect: None, or a planted deviation from LevenbergMarquardtStrategy for the tests of the log comparison --
    "no_doubling" (the decrease factor stays 2), "clamp_half" (max(1/2, .)), "reject_keeps_damping" (a rejected step shrinks the
    radius but the next system is built with the old damping).
    oracle_residual_vector (dogleg only): oracle/orc_map.cpp keeps ONE residual vector, which the candidate evaluation overwrites with
    the candidate's uncorrected residuals; after a rejected step its model cost change (J delta).r is formed with that vector until
    the next accepted step evaluates again.  Ceres keeps the residuals of x.  True reproduces the oracle's arithmetic, for the
    comparison with the oracle's own solve; the default is Ceres'."""
    assert strategy in ("dogleg", "lm") and (defect is None or strategy == "lm")
    lm = strategy == "lm"
    p = DenseProblem(m, loss_of)
    n = p.n
    x = p.snapshot()
    vnorm = lambda xs: math.sqrt(sum(float(v @ v) for v in xs))   # noqa: E731
    x_norm = vnorm(x)
    x_cost, r, J = p.evaluate(True)
    out = dict(initial_cost=x_cost, cost_history=[x_cost], successful=0, last_cost_change=math.inf)
    g, h = J.T @ r, np.einsum("ij,ij->j", J, J)
    scale = 1.0 / (1.0 + np.sqrt(h))
    radius, mu, reuse = initial_radius, (1.0 / initial_radius if lm else 1e-8), False
    decrease_factor, stale_mu = 2.0, None
    invalid, iteration, log = 0, 0, []
    htil = ghat = gnhat = delta = None
    alpha = dogleg_step_norm = 0.0

    def solve(damp):
        try:
            Lc = np.linalg.cholesky(J.T @ J + np.diag(damp))
        except np.linalg.LinAlgError:
            return None
        y = np.linalg.solve(Lc.T, np.linalg.solve(Lc, g))
        return y if np.all(np.isfinite(y)) else None

    def finish(term):
        out.update(termination=term, final_cost=x_cost, iterations=iteration, log=np.array(log, float).reshape(-1, 6),
                   grad_max=float(np.max(np.abs(g))) if n else 0.0)
        return out

    while True:
        if iteration >= max_iterations:
            return finish(1)
        if np.max(np.abs(g)) <= gradient_tolerance:
            return finish(0)
        if radius <= 1e-32:
            return finish(0)
        iteration += 1
        step_ok = True
        if lm or not reuse:
            htil = np.clip(h * scale * scale, 1e-6, 1e32) / (scale * scale)
        if lm:
            mu = 1.0 / radius
            if defect == "reject_keeps_damping" and stale_mu is not None:
                mu = stale_mu
            y = solve(mu * htil)
            if y is None:
                step_ok = False
            else:
                delta = -y
        else:
            if not reuse:
                reuse = True
                ghat = g / np.sqrt(htil)
                Jv = J @ (g / htil)
                alpha = float(ghat @ ghat) / float(Jv @ Jv)
                y = None
                while mu < 1.0:
                    y = solve(mu * htil)
                    if y is not None:
                        break
                    mu *= 10.0
                if y is None:
                    step_ok = False
                else:
                    gnhat = -np.sqrt(htil) * y
            if step_ok:
                gnorm, gnnorm = math.sqrt(float(ghat @ ghat)), math.sqrt(float(gnhat @ gnhat))
                if gnnorm <= radius:
                    stephat, dogleg_step_norm = gnhat, gnnorm
                elif gnorm * alpha >= radius:
                    stephat, dogleg_step_norm = -(radius / gnorm) * ghat, radius
                else:
                    b_dot_a = float(np.sum(-alpha * ghat * gnhat))
                    a_sq = (alpha * gnorm) * (alpha * gnorm)
                    b_minus_a_sq = a_sq - 2 * b_dot_a + gnnorm * gnnorm
                    c = b_dot_a - a_sq
                    dd = math.sqrt(c * c + b_minus_a_sq * (radius * radius - a_sq))
                    beta = (dd - c) / b_minus_a_sq if c <= 0 else (radius * radius - a_sq) / (dd + c)
                    stephat = (-alpha * (1.0 - beta)) * ghat + beta * gnhat
                    dogleg_step_norm = math.sqrt(float(stephat @ stephat))
                delta = stephat / np.sqrt(htil)
        mu_used = mu
        model_cost_change = 0.0
        if step_ok:
            Jd = J @ delta
            model_cost_change = -(float(Jd @ r) + 0.5 * float(Jd @ Jd))
        if not step_ok or not (model_cost_change > 0.0):
            invalid += 1
            if invalid >= 5:
                return finish(3)
            if lm:
                radius /= decrease_factor
                decrease_factor *= 1.0 if defect == "no_doubling" else 2.0
                stale_mu = None
            else:
                mu *= 10.0
                reuse = False
            out["cost_history"].append(x_cost)
            log.append([x_cost, 0.0, radius, 0.0, mu_used, INVALID])
            continue
        invalid = 0
        xcand = p.apply(x, delta)
        candidate_cost, r_candidate, _ = p.evaluate(False)
        step_norm = math.sqrt(sum(float((a - b) @ (a - b)) for a, b in zip(x, xcand)))
        if step_norm <= parameter_tolerance * (x_norm + parameter_tolerance):
            p.restore(x)
            return finish(0)
        cost_change = x_cost - candidate_cost
        out["last_cost_change"] = abs(cost_change)
        if abs(cost_change) <= function_tolerance * x_cost:
            p.restore(x)
            return finish(0)
        rho = cost_change / model_cost_change
        if rho > 1e-3:
            x, x_norm = xcand, vnorm(xcand)
            x_cost, r, J = p.evaluate(True)
            g, h = J.T @ r, np.einsum("ij,ij->j", J, J)
            out["successful"] += 1
            if lm:
                radius = min(max_radius, radius / max(0.5 if defect == "clamp_half" else 1.0 / 3.0, 1.0 - math.pow(2.0 * rho - 1.0, 3)))
                decrease_factor, stale_mu = 2.0, None
            else:
                if rho < 0.25:
                    radius *= 0.5
                if rho > 0.75:
                    radius = max(radius, 3.0 * dogleg_step_norm)
                radius = min(radius, max_radius)
                mu = max(1e-8, 2.0 * mu / 10.0)
                reuse = False
            outcome = ACCEPTED
        else:
            p.restore(x)
            if lm:
                radius /= decrease_factor
                decrease_factor *= 1.0 if defect == "no_doubling" else 2.0
                stale_mu = mu_used
            else:
                radius *= 0.5
                reuse = True
                if oracle_residual_vector:
                    r = r_candidate
            outcome = REJECTED
        out["cost_history"].append(x_cost)
        log.append([x_cost, rho, radius, step_norm, mu_used, outcome])


def compare_logs(got, ref, cost_rtol, radius_rtol):
    """The comparison the GPU tests hold an iteration log to: the same number of rows, the same outcome in every row, and the cost,
    radius and mu columns within the relative bounds.  Returns None, or a sentence saying what differs first."""
    got, ref = np.asarray(got, float).reshape(-1, 6), np.asarray(ref, float).reshape(-1, 6)
    if got.shape != ref.shape:
        return "%d rows against the reference's %d" % (len(got), len(ref))
    for i, (a, b) in enumerate(zip(got, ref)):
        if a[5] != b[5]:
            return "iteration %d: outcome %d against the reference's %d" % (i + 1, int(a[5]), int(b[5]))
        for col, tol in ((0, cost_rtol), (2, radius_rtol), (4, radius_rtol)):
            if not abs(a[col] - b[col]) <= tol * abs(b[col]):
                return "iteration %d: %s %.17g against the reference's %.17g" % (i + 1, COLUMNS[col], a[col], b[col])
    return None


def log_events(log):
    """what a Levenberg-Marquardt log exercises: accepted steps with the 1/3 clamp active / inactive (read off the radius column:
    tripled or not), and the longest run of consecutive rejected steps"""
    log = np.asarray(log, float).reshape(-1, 6)
    clamped = unclamped = run = longest = 0
    for row in log:
        if row[5] == ACCEPTED:
            if 1.0 - math.pow(2.0 * row[1] - 1.0, 3) <= 1.0 / 3.0:
                clamped += 1
            else:
                unclamped += 1
        run = run + 1 if row[5] == REJECTED else 0
        longest = max(longest, run)
    return dict(clamped=clamped, unclamped=unclamped, rejected_run=longest)
