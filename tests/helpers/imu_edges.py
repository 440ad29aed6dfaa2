"""Shared by test_imu_edges_host.py and test_gpu_imu_edges.py: the cases of tests/golden/imu_edges.npz
(make_golden_imu_edges.py) and the scale-free errors every implementation is held to.  Each error is divided by its bar,
so a value <= 1 passes."""
import os

import numpy as np

GOLD = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "golden")
NAMES = ("a_max", "g_max", "sigma_g_c", "sigma_a_c", "sigma_bg", "sigma_ba", "sigma_gw_c", "sigma_aw_c", "tau", "g")
IU15, IU30 = np.triu_indices(15), np.triu_indices(30)

# the same bars for every sample count: the imu.npz bars, plus scale-free forms of J^T J and J^T r.  Position and velocity
# are at 10x the worst error of the serial FP64 loops (1.95e-13 / 1.29e-13 after 639 steps, test_imu_edges_host.py).
BARS = dict(p=2e-12, q=1e-13, v=1.3e-12, integ=1e-13, cov=1e-12, jac=1e-12, chi2=1e-9, e=1e-8, H=1e-9, g=1e-9)


def load():
    return np.load(os.path.join(GOLD, "imu_edges.npz"))


def params(g):
    par = dict(zip(NAMES, [float(v) for v in g["params"]]))
    par["a0"] = [0.0, 0.0, 0.0]
    return par


def sym(ut, n):
    A = np.zeros((n, n))
    A[np.triu_indices(n)] = ut
    return A + np.triu(A, 1).T


def samples(g, stream, first, count):
    key = "ab"[int(stream)]
    t = np.ascontiguousarray(g[key + "_t"][first:first + count])
    m = np.ascontiguousarray(g[key + "_m"][first:first + count].astype(np.float64))
    return t, m


def case(g, i):
    """(samples t, samples m, t0, t1) of case i"""
    t, m = samples(g, g["stream"][i], int(g["first"][i]), int(g["count"][i]))
    return t, m, tuple(int(v) for v in g["t0"][i]), tuple(int(v) for v in g["t1"][i])


def chain_case(g, k):
    t, m = samples(g, 0, int(g["chain_first"][k]), int(g["chain_count"][k]))
    return t, m, tuple(int(v) for v in g["chain_t"][k]), tuple(int(v) for v in g["chain_t"][k + 1])


def quat_angle(a, b):
    return 2.0 * min(np.linalg.norm(a - b), np.linalg.norm(a + b))


def prop_errors(g, i, T, v, cov, jac, integ=None):
    """propagation: positions / velocities / integrals relative to max(1, |x|), rotation angle, covariance and Jacobian
    relative to their largest entry"""
    rel = lambda a, b: float(np.max(np.abs(a - b) / np.maximum(1.0, np.abs(b))))  # noqa: E731
    ref_cov, ref_F = sym(g["cov"][i], 15), g["F"][i]
    err = dict(p=rel(T[:3], g["T_pred"][i][:3]), q=quat_angle(T[3:], g["T_pred"][i][3:]), v=rel(v, g["v_pred"][i]),
               cov=float(np.max(np.abs(cov - ref_cov)) / np.max(np.abs(ref_cov))),
               jac=float(np.max(np.abs(jac - ref_F)) / np.max(np.abs(ref_F))))
    if integ is not None:
        err["integ"] = rel(integ, g["integrals"][i])
    return {k: x / BARS[k] for k, x in err.items()}


def factor_errors(r, J, e, chi2, P_delta, gv, H):
    """an IMU factor's weighted residual r (15) and minimal Jacobian J (15 x 30) against the fixture: chi^2, e (r unweighted
    with the fixture's P_delta), H = J^T J per sqrt(H_ii H_jj), g = J^T r per sqrt(H_ii) max(1, |r|)"""
    H = sym(H, 30)
    P = sym(P_delta, 15)
    Lc = np.linalg.cholesky(np.linalg.inv(P))
    d = np.sqrt(np.diag(H))
    err = dict(chi2=abs(float(r @ r) - chi2) / chi2,
               e=float(np.max(np.abs(np.linalg.solve(Lc.T, r) - e)) / np.max(np.abs(e))),
               H=float(np.max(np.abs(J.T @ J - H) / np.outer(d, d))),
               g=float(np.max(np.abs(J.T @ r - gv) / d)) / max(1.0, float(np.linalg.norm(r))))
    return {k: x / BARS[k] for k, x in err.items()}


def fold(worst, err, where):
    """worst[k] = (error / bar, case) over the cases seen so far; a case over a bar is printed as it is met"""
    for k, x in err.items():
        if not x <= 1.0:
            print("over the bar: %s, %s %.2e" % (where, k, x * BARS[k]))
        if k not in worst or x > worst[k][0]:
            worst[k] = (x, where)


def report(worst):
    return ", ".join("%s %.2e (%s)" % (k, x * BARS[k], w) for k, (x, w) in sorted(worst.items()))


def failures(worst):
    return {k: (x * BARS[k], w) for k, (x, w) in worst.items() if not x <= 1.0}
