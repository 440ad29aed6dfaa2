#!/usr/bin/env python3
"""Golden fixture for IMU pre-integration at the sample counts and interval edges where a tiled implementation can go wrong
(tests/golden/imu_edges.npz), from the same INDEPENDENT 50-digit mpmath restatement as imu.npz (make_golden_imu.py:
integrate(), quat_to_R, the IMU parameters) -- nothing here calls the oracle or the product.

Cases are slices (first sample, count, t0, t1) of two shared sample streams, with measurements exact in float32:
  A  200 Hz, smooth random motion
  B  100 Hz with defects: a duplicate stamp pair (100/101), a gyroscope-saturated sample (200) and an accelerometer-saturated
     one (264), and four IMU gaps whose steps reach |omega| dt = 0.45, 0.55, 0.95, 1.05 rad (either side of the series /
     closed-form switches of the right Jacobian and of dq; the 0.55 and 1.05 rad steps are also over g_max)
The chain window takes consecutive slices of A.
`count` is the number of samples handed to the integration.

Stored per case
  propagation flavour (ImuError.cpp:266-476): used, predicted T and v, the integrals (acc_doubleintegral, acc_integral,
    Delta_t), the 15x15 covariance (upper triangle) and the 15x15 Jacobian F (:452-462)
  factor (redo flavour, :76-263 and :739-791) at states T1 / sb1 near the prediction: e, chi^2 = e^T P_delta^-1 e, P_delta
    (upper triangle) and the weighted invariants g = F_all^T P_delta^-1 e (30), H = F_all^T P_delta^-1 F_all (30 x 30, upper
    triangle), F_all = [F0 F1] the minimal Jacobians of :752-784 (plus / oplus: okvis_kinematics operators.hpp)
  for the `bias_case` entries, two more evaluations of the same factor after a first one at sb0 (which pre-integrates at sb0):
    a  sb0 + Delta_b with |Delta_b_g| Delta_t = 0.5e-4 (below the 1e-4 redo threshold): the linearised correction
       Dq = deltaQ(-dalpha_db_g Delta_b_g) Delta_q and the F0.block<3,6>(., 9) Delta_b terms of e
    b  sb0 + Delta_b with |Delta_b_g| Delta_t = 2e-4: the factor re-integrates at the new biases
  chain: six frames whose five consecutive IMU intervals hold 3, 64, 129, 9, 257 samples, each factor as above
A case with used = -1 (last sample older than t1) stores zeros for everything but its inputs.
Run:  python tests/golden/make_golden_imu_edges.py      (writes imu_edges.npz; about a minute)
"""
import os
import sys
import time

import mpmath as mp
import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from make_golden import qmul  # noqa: E402
from make_golden_imu import M, cross_mx, fl, integrate, quat_to_R  # noqa: E402

mp.mp.dps = 50
HERE = os.path.dirname(os.path.abspath(__file__))
NS = 1_000_000_000
PAR_F = dict(a_max=176.0, g_max=7.8, sigma_g_c=12.0e-4, sigma_a_c=8.0e-3, sigma_bg=0.03, sigma_ba=0.1, sigma_gw_c=4.0e-6,
             sigma_aw_c=4.0e-5, tau=3600.0, g=9.81007)
PAR_NAMES = ("a_max", "g_max", "sigma_g_c", "sigma_a_c", "sigma_bg", "sigma_ba", "sigma_gw_c", "sigma_aw_c", "tau", "g")
PAR = {k: mp.mpf(v) for k, v in PAR_F.items()}
IU15, IU30 = np.triu_indices(15), np.triu_indices(30)
COUNT_SWEEP = (2, 3, 4, 5, 7, 8, 9, 12, 15, 16, 17, 31, 32, 33, 63, 64, 65, 66, 127, 128, 129, 130, 192, 193, 256, 257, 640)
BIAS_COUNTS = (3, 9, 17, 33, 65, 129, 193, 257)
CHAIN_COUNTS = (3, 64, 129, 9, 257)


def smooth(rng, n, rate, amp, freqs):
    """sum of three sinusoids per axis, random phases and amplitudes"""
    t = np.arange(n) / rate
    out = np.zeros((n, 3))
    for f in freqs:
        out += rng.uniform(0.3, 1.0, 3) * amp * np.sin(2 * np.pi * f * t[:, None] + rng.uniform(0, 2 * np.pi, 3))
    return out


def quantise(m):
    """measurements exact in single precision (stored as float32; an IMU's samples are short integers anyway)"""
    return m.astype(np.float32).astype(np.float64)


def stream_a(rng):
    n, rate = 720, 200
    ns = 200 * NS + 3_000_000 + np.arange(n, dtype=np.int64) * (NS // rate)
    gyr = smooth(rng, n, rate, 0.8, (0.3, 1.1, 2.3))
    acc = smooth(rng, n, rate, 1.5, (0.2, 0.9, 1.7)) + np.array([0.0, 0.0, 9.81])
    return ns, quantise(np.c_[gyr, acc])


def stream_b(rng):
    n, rate = 420, 100
    dts = np.full(n - 1, NS // rate, dtype=np.int64)
    dts[100] = 0                                       # samples 100 and 101 share a stamp
    gyr = smooth(rng, n, rate, 0.5, (0.25, 0.8, 1.9))
    acc = smooth(rng, n, rate, 1.0, (0.15, 0.7, 1.3)) + np.array([0.0, 0.0, 9.81])
    gyr[200] = [9.0, -0.4, 0.2]                        # gyroscope saturation (g_max 7.8)
    acc[264] = [0.5, -1.0, 180.0]                      # accelerometer saturation (a_max 176)
    # IMU gaps: sample k and k + 1 carry the same rate, dt of the gap chosen for the target |omega| dt
    for k, w, angle in ((350, [1.8, -2.0, 1.2], 0.45), (352, [8.0, 0.6, 0.2], 0.55), (354, [-4.4, 4.6, -4.1], 0.95),
                        (356, [0.5, -8.4, 0.3], 1.05)):
        w = np.array(w)
        gyr[k] = gyr[k + 1] = w
        dts[k] = int(round(angle / np.linalg.norm(w) * NS))
    ns = 300 * NS + 7_000_000 + np.r_[0, np.cumsum(dts)]
    return ns, quantise(np.c_[gyr, acc])


def between(ns, k, frac):
    return int(ns[k] + int(round(frac * (ns[k + 1] - ns[k]))))


def stamp(x):
    return [int(x) // NS, int(x) % NS]


def mpq(q):
    q = [mp.mpf(float(c)) for c in q]
    n = mp.sqrt(sum(c * c for c in q))
    return [c / n for c in q]


def expq(v):
    """okvis::kinematics::deltaQ: [sinc(|v|/2) v / 2, cos(|v|/2)]"""
    h = mp.sqrt(v[0] ** 2 + v[1] ** 2 + v[2] ** 2) / 2
    s = mp.sin(h) / h / 2 if h > 0 else mp.mpf(1) / 2
    return [s * v[0], s * v[1], s * v[2], mp.cos(h)]


def qinv(q):
    n = sum(c * c for c in q)
    return [-q[0] / n, -q[1] / n, -q[2] / n, q[3] / n]


def plus4(q):
    x, y, z, w = q
    return M([[w, -z, y, x], [z, w, -x, y], [-y, x, w, z], [-x, -y, -z, w]])


def oplus4(q):
    x, y, z, w = q
    return M([[w, z, -y, x], [-z, w, x, y], [y, -x, w, z], [-x, -y, -z, w]])


def tl3(A):
    return M([[A[i, j] for j in range(3)] for i in range(3)])


def setb(F, r0, c0, B):
    for a in range(3):
        for b in range(3):
            F[r0 + a, c0 + b] = B[a, b]


def vec(x):
    return M([mp.mpf(float(v)) for v in x])


def rand_pose(rng, scale=1.0):
    a = rng.uniform(-0.5, 0.5, 3)
    th = np.linalg.norm(a)
    return np.r_[rng.uniform(-1, 1, 3) * scale, np.sin(th / 2) * a / th, np.cos(th / 2)]


def perturbed_pose(rng, r, q):
    """float pose near (r, q): 2 cm, 0.01 rad; quaternion normalised in mp so that the stored floats are what the states hold"""
    da = rng.normal(size=3) * 0.01
    th = np.linalg.norm(da)
    dq = [mp.mpf(float(x)) for x in np.r_[np.sin(th / 2) * da / th, np.cos(th / 2)]]
    q1 = mpq([float(c) for c in qmul(dq, q)])
    return np.r_[fl(r)[:, 0] + rng.normal(size=3) * 0.02, [float(c) for c in q1]]


def slice_mp(stream, first, count):
    ns, meas = stream
    t = [mp.mpf(int(x)) / NS for x in ns[first:first + count]]
    mg = [[mp.mpf(float(x)) for x in r[:3]] for r in meas[first:first + count]]
    ma = [[mp.mpf(float(x)) for x in r[3:]] for r in meas[first:first + count]]
    return t, mg, ma


def predict(pr, T0, sb0):
    """prediction of ImuError::propagation (:452-458) from the pre-integrated quantities"""
    q0, r0, v0 = mpq(T0[3:]), vec(T0[:3]), vec(sb0[:3])
    C0, Dt, gW = quat_to_R(q0), pr["Dt"], M([0, 0, PAR["g"]])
    r1 = r0 + v0 * Dt + C0 * pr["adi"] - gW * Dt * Dt / 2
    q1 = qmul(q0, pr["Dq"])
    n1 = mp.sqrt(sum(c * c for c in q1))
    return r1, [c / n1 for c in q1], v0 + C0 * pr["ai"] - gW * Dt


def factor(rd, Dt, T0, sb0, T1, sb1, sb_ref):
    """ImuError::EvaluateWithMinimalJacobians (:717-791) with the pre-integration rd done at the biases of sb_ref:
    e, chi^2, P_delta, g = F_all^T P^-1 e, H = F_all^T P^-1 F_all"""
    q0, q1 = mpq(T0[3:]), mpq(T1[3:])
    r0, r1, v0, v1 = vec(T0[:3]), vec(T1[:3]), vec(sb0[:3]), vec(sb1[:3])
    db = [mp.mpf(float(sb0[3 + i])) - mp.mpf(float(sb_ref[3 + i])) for i in range(6)]
    dbg, dba = M(db[:3]), M(db[3:])
    C0 = quat_to_R(q0)
    CT = C0.T
    gW = M([0, 0, PAR["g"]])
    dp_est = r0 - r1 + v0 * Dt - gW * Dt * Dt / 2
    dv_est = v0 - v1 - gW * Dt
    Dq = qmul(expq(-rd["dal"] * dbg), rd["Dq"])
    q1i = qinv(q1)
    F0 = mp.eye(15)
    setb(F0, 0, 0, CT)
    setb(F0, 0, 3, CT * cross_mx(dp_est))
    setb(F0, 0, 6, CT * Dt)
    setb(F0, 0, 9, rd["dp"])
    setb(F0, 0, 12, -rd["Cdi"])
    setb(F0, 3, 3, tl3(plus4(qmul(Dq, q1i)) * oplus4(q0)))
    setb(F0, 3, 9, tl3(oplus4(qmul(q1i, q0)) * oplus4(Dq)) * (-rd["dal"]))
    setb(F0, 6, 3, CT * cross_mx(dv_est))
    setb(F0, 6, 6, CT)
    setb(F0, 6, 9, rd["dv"])
    setb(F0, 6, 12, -rd["Ci"])
    F1 = -mp.eye(15)
    setb(F1, 0, 0, -CT)
    setb(F1, 3, 3, -tl3(plus4(Dq) * oplus4(q0) * plus4(q1i)))
    setb(F1, 6, 6, -CT)
    eq = qmul(Dq, qmul(q1i, q0))
    e0 = CT * dp_est + rd["adi"] + rd["dp"] * dbg - rd["Cdi"] * dba
    e2 = CT * dv_est + rd["ai"] + rd["dv"] * dbg - rd["Ci"] * dba
    e = M(list(e0) + [2 * eq[0], 2 * eq[1], 2 * eq[2]] + list(e2) +
          [mp.mpf(float(sb0[3 + i])) - mp.mpf(float(sb1[3 + i])) for i in range(6)])
    P = (rd["P"] + rd["P"].T) / 2
    Pi = mp.inverse(P)
    Fa = mp.zeros(15, 30)
    for i in range(15):
        for j in range(15):
            Fa[i, j], Fa[i, 15 + j] = F0[i, j], F1[i, j]
    Pe = Pi * e
    PF = Pi * Fa
    return dict(e=fl(e)[:, 0], chi2=float((e.T * Pe)[0, 0]), P_delta=fl(P)[IU15], g=fl(Fa.T * Pe)[:, 0], H=fl(Fa.T * PF)[IU30])


def propagation(stream, first, count, t0, t1, T0, sb0):
    t, mg, ma = slice_mp(stream, first, count)
    bg, ba = vec(sb0[3:6]), vec(sb0[6:9])
    pr = integrate(t, mg, ma, PAR, bg, ba, t0, t1, redo=False)
    r1, q1, v1 = predict(pr, T0, sb0)
    C0 = quat_to_R(mpq(T0[3:]))
    Tm = mp.eye(15)
    for blk in range(3):
        setb(Tm, 3 * blk, 3 * blk, C0)
    cov = Tm * pr["P"] * Tm.T
    F = mp.eye(15)
    setb(F, 0, 3, -cross_mx(C0 * pr["adi"]))
    setb(F, 0, 6, mp.eye(3) * pr["Dt"])
    setb(F, 0, 9, C0 * pr["dp"])
    setb(F, 0, 12, -C0 * pr["Cdi"])
    setb(F, 3, 9, -C0 * pr["dal"])
    setb(F, 6, 3, -cross_mx(C0 * pr["ai"]))
    setb(F, 6, 9, C0 * pr["dv"])
    setb(F, 6, 12, -C0 * pr["Ci"])
    return pr, r1, q1, v1, dict(used=pr["used"], T_pred=np.r_[fl(r1)[:, 0], [float(c) for c in q1]], v_pred=fl(v1)[:, 0],
                                integrals=np.r_[fl(pr["adi"])[:, 0], fl(pr["ai"])[:, 0], float(pr["Dt"])], cov=fl(cov)[IU15], F=fl(F))


def redo(stream, first, count, t0, t1, sb):
    t, mg, ma = slice_mp(stream, first, count)
    return integrate(t, mg, ma, PAR, vec(sb[3:6]), vec(sb[6:9]), t0, t1, redo=True)


def case_list(A, B):
    ns_a, ns_b = A[0], B[0]
    cases = []

    def add(name, s, first, count, t0, t1, bias=False):
        cases.append(dict(name=name, stream=s, first=first, count=count, t0=t0, t1=t1, bias=bias))
    for i, c in enumerate(COUNT_SWEEP):
        first = (37 * i) % (len(ns_a) - c)
        add("count %d" % c, 0, first, c, between(ns_a, first, 0.37), between(ns_a, first + c - 2, 0.61), c in BIAS_COUNTS)
    add("t0 on the first sample", 0, 11, 20, int(ns_a[11]), between(ns_a, 29, 0.5))
    add("t1 on the last sample", 0, 13, 20, between(ns_a, 13, 0.4), int(ns_a[32]))
    add("t0 and t1 on samples", 0, 15, 20, int(ns_a[15]), int(ns_a[34]))
    add("t0, t1 in one sample interval", 0, 17, 6, between(ns_a, 19, 0.2), between(ns_a, 19, 0.7))
    add("70 samples before t0", 0, 40, 100, between(ns_a, 110, 0.45), between(ns_a, 138, 0.5))
    add("130 samples before t0", 0, 50, 160, between(ns_a, 180, 0.3), between(ns_a, 208, 0.55))
    add("101 samples after t1", 0, 60, 130, between(ns_a, 60, 0.5), between(ns_a, 88, 0.5))
    add("duplicate stamps at 63/64", 1, 37, 100, between(ns_b, 37, 0.5), between(ns_b, 135, 0.5))
    add("gyro saturation at 63, acc at 127", 1, 137, 150, between(ns_b, 137, 0.5), between(ns_b, 285, 0.5))
    add("gyro saturation at 64, acc at 128", 1, 136, 140, between(ns_b, 136, 0.25), between(ns_b, 274, 0.75))
    add("IMU gaps at 60..66", 1, 290, 80, between(ns_b, 290, 0.5), between(ns_b, 368, 0.5))
    for name, j, span in (("100 Hz over 1/15 s", 20, NS // 15), ("100 Hz over 1/13 s", 40, NS // 13)):
        t0 = between(ns_b, j, 0.3)
        t1 = t0 + span
        last = int(np.searchsorted(ns_b, t1)) + 1          # the sample after t1, plus one margin sample
        add(name, 1, j - 1, last - (j - 1) + 1, t0, t1)
    add("last sample older than t1", 0, 5, 10, between(ns_a, 5, 0.5), int(ns_a[14]) + 2_000_000)
    return cases


def main():
    t_start = time.time()
    rng = np.random.default_rng(20261016)
    A, B = stream_a(rng), stream_b(rng)
    streams = (A, B)
    cases = case_list(A, B)
    rows, bias_rows = [], []
    for ci, c in enumerate(cases):
        S = streams[c["stream"]]
        ns = S[0]
        assert ns[c["first"]] <= c["t0"] < c["t1"] and c["first"] + c["count"] <= len(ns)
        T0, v0 = rand_pose(rng), rng.normal(size=3)
        sb0 = np.r_[v0, rng.normal(size=3) * 0.01, rng.normal(size=3) * 0.05]
        t0, t1 = mp.mpf(c["t0"]) / NS, mp.mpf(c["t1"]) / NS
        row = dict(stream=c["stream"], first=c["first"], count=c["count"], t0=stamp(c["t0"]), t1=stamp(c["t1"]),
                   T0=np.r_[T0[:3], [float(x) for x in mpq(T0[3:])]], sb0=sb0)
        if ns[c["first"] + c["count"] - 1] < c["t1"]:       # ImuError.cpp:279
            row.update(used=-1, T_pred=np.zeros(7), v_pred=np.zeros(3), integrals=np.zeros(7), cov=np.zeros(120), F=np.zeros((15, 15)),
                       T1=np.zeros(7), sb1=np.zeros(9), e=np.zeros(15), chi2=0.0, P_delta=np.zeros(120), g=np.zeros(30), H=np.zeros(465))
            rows.append(row)
            continue
        pr, r1, q1, v1, out = propagation(S, c["first"], c["count"], t0, t1, row["T0"], sb0)
        row.update(out)
        T1 = perturbed_pose(rng, r1, q1)
        sb1 = np.r_[fl(v1)[:, 0] + rng.normal(size=3) * 0.02, sb0[3:6] + rng.normal(size=3) * 1e-3, sb0[6:9] + rng.normal(size=3) * 1e-3]
        rd = redo(S, c["first"], c["count"], t0, t1, sb0)
        row.update(T1=T1, sb1=sb1, **factor(rd, t1 - t0, row["T0"], sb0, T1, sb1, sb0))
        rows.append(row)
        if c["bias"]:
            Dt = float(t1 - t0)
            br = dict(bias_case=ci)
            for tag, gyro in (("a", 0.5e-4), ("b", 2e-4)):
                d = rng.normal(size=3)
                da = rng.normal(size=3)
                sbx = sb0.copy()
                sbx[3:6] += d / np.linalg.norm(d) * gyro / Dt
                sbx[6:9] += da / np.linalg.norm(da) * 1e-2
                if tag == "a":       # linearised correction around the pre-integration at sb0
                    f = factor(rd, t1 - t0, row["T0"], sbx, T1, sb1, sb0)
                else:                # re-integrated at the new biases
                    f = factor(redo(S, c["first"], c["count"], t0, t1, sbx), t1 - t0, row["T0"], sbx, T1, sb1, sbx)
                br["sb0" + tag] = sbx
                for k in ("e", "chi2", "g", "H") + (("P_delta",) if tag == "b" else ()):
                    br[k + "_" + tag] = f[k]
            bias_rows.append(br)
        print("%-36s count %4d used %4d chi2 %.6e  (%.0f s)" % (c["name"], c["count"], row["used"], row["chi2"], time.time() - t_start), flush=True)
    # the chain window: consecutive slices of stream A, frame k + 1 stamped inside the last interval of slice k
    ns_a = A[0]
    first = 100
    ch = dict(chain_first=[], chain_count=[], chain_t=[between(ns_a, first, 0.4)], chain_e=[], chain_chi2=[], chain_P_delta=[],
              chain_g=[], chain_H=[])
    T = rand_pose(rng)
    T = np.r_[T[:3], [float(x) for x in mpq(T[3:])]]
    sb = np.r_[rng.normal(size=3), rng.normal(size=3) * 0.01, rng.normal(size=3) * 0.05]
    ch_T, ch_sb = [T], [sb]
    for c in CHAIN_COUNTS:
        tk = between(ns_a, first + c - 2, float(rng.uniform(0.2, 0.8)))
        t0, t1 = mp.mpf(ch["chain_t"][-1]) / NS, mp.mpf(tk) / NS
        rd = redo(A, first, c, t0, t1, sb)
        r1, q1, v1 = predict(rd, T, sb)       # Delta_q and the integrals are the same in both flavours
        T1 = perturbed_pose(rng, r1, q1)
        sb1 = np.r_[fl(v1)[:, 0] + rng.normal(size=3) * 0.02, sb[3:6] + rng.normal(size=3) * 1e-3, sb[6:9] + rng.normal(size=3) * 1e-3]
        f = factor(rd, t1 - t0, T, sb, T1, sb1, sb)
        for k in ("e", "chi2", "P_delta", "g", "H"):
            ch["chain_" + k].append(f[k])
        ch["chain_first"].append(first)
        ch["chain_count"].append(c)
        ch["chain_t"].append(tk)
        ch_T.append(T1)
        ch_sb.append(sb1)
        T, sb, first = T1, sb1, first + c - 2
        print("chain interval of %d samples: chi2 %.6e  (%.0f s)" % (c, f["chi2"], time.time() - t_start), flush=True)
    ch["chain_t"] = [stamp(x) for x in ch["chain_t"]]
    ch["chain_T"], ch["chain_sb"] = ch_T, ch_sb
    out = {"params": np.array([PAR_F[k] for k in PAR_NAMES]),
           "a_t": np.array([stamp(x) for x in A[0]], np.uint32), "a_m": A[1].astype(np.float32),
           "b_t": np.array([stamp(x) for x in B[0]], np.uint32), "b_m": B[1].astype(np.float32),
           "name": np.array([c["name"] for c in cases])}
    for key in rows[0]:
        out[key] = np.array([r[key] for r in rows])
    for key in ("stream", "first", "count", "used"):
        out[key] = out[key].astype(np.int32)
    out["t0"], out["t1"] = out["t0"].astype(np.uint32), out["t1"].astype(np.uint32)
    for key in bias_rows[0]:
        out[key] = np.array([r[key] for r in bias_rows])
    for key, v in ch.items():
        out[key] = np.array(v)
    out["chain_t"] = out["chain_t"].astype(np.uint32)
    path = os.path.join(HERE, "imu_edges.npz")
    np.savez_compressed(path, **out)
    print("wrote imu_edges.npz: %d cases, %d with bias steps, a chain of %d intervals; %d bytes, %.0f s" %
          (len(rows), len(bias_rows), len(CHAIN_COUNTS), os.path.getsize(path), time.time() - t_start))


if __name__ == "__main__":
    main()
