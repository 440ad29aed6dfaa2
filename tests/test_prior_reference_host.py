"""tests/helpers/prior_reference.py -- the long-double reference of the marginalisation prior away from its linearisation point --
checked on the CPU before the GPU tests rely on it.  Priors come from the oracle: sliding windows, marg() with its linearisation
points (one window after its FIRST marginalisation, one after THREE chained ones with optimize() in between, whose points are first
estimates), states then moved by tests/helpers/prior_moves.py.  Quaternions are stored RAW here (the oracle's map takes what it is
given): every pose / extrinsics block is scaled by 1 -+ O(1e-3) before each marginalisation and after each move, so that the two
normalisation rules of the definition (lift at the raw q_lin, PlusJacobian at the normalised q) are visible at all.

  agreement   M^T H M, M^T grad and the cost agree with the oracle's own linearisation of its MarginalizationError at the moved state
              -- e = e0 + J dchi and ambient Jacobians J lift(x_lin), times the oracle's PlusJacobian(x): another formulation, through
              7-column blocks -- to the helper's bound plus the oracle's float64 rounding, taken as the same bound once more
  inside      a float64 restatement of the device arithmetic, summed forwards and backwards, stays inside the bound on every case
  mutations   on every moved case each of the eight mutations of that restatement leaves the bound in an entry of S, g or the cost
  scatter     schur_reference.assemble(prior=moved) puts the same numbers at the reduced system's rows
  derivative  M is the derivative of delta -> (x [+] delta) [-] x_lin at 0 (central differences in long double)
"""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "helpers"))
import prior_moves as pm           # noqa: E402
import prior_reference as pr       # noqa: E402
import schur_reference as sr       # noqa: E402
import step_reference as st        # noqa: E402

from svin_amd import synthetic as syn   # noqa: E402

EPS, C0, LD = pr.EPS, pr.C0, pr.LD
KIND_MARGINALIZATION = 8   # orc_errors.hpp: ErrorTerm::Kind
MOVED = ("optimised", "tiny", "large", "flipped", "constant")
MUTATIONS = ("M3_transposed", "M3_identity", "q_not_normalised", "lin_normalised", "factor_2_dropped", "grad_without_H_dchi",
             "cost_without_quadratic", "constant_not_skipped")
WINDOWS = {
    "euroc_first": (dict(P=7, L=150, n_obs=1500, seed=9, keyframe_every=2, frame_dt=0.3), (2, 2), 1),
    "rig_v2_chained": (dict(P=9, L=200, n_obs=2000, seed=45, rig="rig_v2", sonar=True, depth=True, keyframe_every=2, frame_dt=0.3), (2, 2), 3),
}


class Done(Exception):
    pass


def scale_quaternions(mp, ids, base):
    for k, pid in enumerate(ids):
        x = mp.get_param(pid)
        if len(x) == 7:
            x[3:7] *= 1.0 + base * (1 + k % 3)
            mp.set_param(pid, x)


def pose_like_ids(mp):
    ids = set()
    for rid in mp.residual_ids():
        ids.update(mp.parameters_of(rid))
    return sorted(p for p in ids if len(mp.get_param(p)) == 7)


def build_window(name):
    """the oracle after `chain` marginalisations, one more frame and optimize(3): (estimator, map, marg(), values straight after the
    last marginalisation)"""
    from oracle import orc
    kw, (n_kf, n_imu), chain = WINDOWS[name]
    spec = syn.make_window(**kw)
    est = orc.OracleEstimator()
    mp = est.map()
    state = dict(count=0, marg=None, x_lin_state=None)

    def on_frame(k, fid):
        if state["marg"] is not None:
            est.optimize(3)
            raise Done
        est.optimize(4)
        scale_quaternions(mp, pose_like_ids(mp), -2e-3)   # raw linearisation quaternions
        est.apply_marginalization(n_kf, n_imu)
        m = est.marg()
        if m is None:
            return
        state["count"] += 1
        if state["count"] >= chain:
            state["marg"] = m
            state["x_lin_state"] = {b["id"]: mp.get_param(b["id"]) for b in m["blocks"]}
    with pytest.raises(Done):
        syn.feed(est, spec, on_frame=on_frame)
    return est, mp, state["marg"], state["x_lin_state"]


@pytest.fixture(scope="module")
def windows(oracle_lib):
    if not sr.have_long_double():
        pytest.skip("np.longdouble is not wider than float64 on this machine")
    return {name: build_window(name) for name in WINDOWS}


def cases_of(window):
    """(move, marg, blocks with x, columns without and with a constant pose), the oracle's map left at the moved state"""
    est, mp, m, x_after = window
    optimised = {b["id"]: mp.get_param(b["id"]) for b in m["blocks"]}
    rows = [(pr.KIND_OF[b["kind"]], b["id"]) for b in m["blocks"] if b["mdim"] > 0]
    poses = [b for b in m["blocks"] if b["kind"] == 0 and b["mdim"] > 0]
    assert len(poses) >= 2
    for move in ("at_lin",) + MOVED:
        for bid, x in (optimised if move == "optimised" else x_after).items():
            mp.set_param(bid, x)
        if move != "optimised":
            kept = pm.apply("large" if move == "constant" else move, rows, mp.get_param, mp.set_param)
            assert move != "flipped" or kept > 0
        if move != "at_lin":
            scale_quaternions(mp, [bid for _, bid in rows], 1e-3)   # raw current quaternions
        blocks = [dict(kind=pr.KIND_OF[b["kind"]], ordering=b["ordering"], mdim=b["mdim"], lin=b["lin"], x=mp.get_param(b["id"]), id=b["id"])
                  for b in m["blocks"]]
        free = np.arange(m["n"])
        held = free.copy()
        held[poses[1]["ordering"]:poses[1]["ordering"] + 6] = -1
        yield move, m, blocks, free, held


def oracle_linearisation(est, mp, m):
    """S, g, cost of the oracle's MarginalizationError at the map's current values, over the prior's own rows"""
    from oracle import orc
    rid = [r for r in mp.residual_ids() if mp.residual_kind(r) == KIND_MARGINALIZATION]
    assert len(rid) == 1
    r, Js, _ = mp.eval(rid[0])
    params = mp.parameters_of(rid[0])
    by_id = {b["id"]: b for b in m["blocks"]}
    Jeff = np.zeros((len(r), m["n"]))
    for pid, J in zip(params, Js):
        b = by_id[pid]
        if b["mdim"] == 0:
            continue
        x = orc.arr(mp.get_param(pid))
        Jp = np.zeros((J.shape[1], b["mdim"]))
        mp.L.orc_manifold_plus_jacobian(orc.BLOCK_POSE if J.shape[1] == 7 else orc.BLOCK_SPEEDBIAS, orc.dptr(x), orc.dptr(Jp))
        Jeff[:, b["ordering"]:b["ordering"] + b["mdim"]] = J @ Jp
    return Jeff.T @ Jeff, Jeff.T @ r, 0.5 * float(r @ r)


def tolerances(ref):
    """the bound of every entry over the prior's own rows; rows of a constant block hold exact zeros"""
    on = ref["columns"] >= 0
    tS = np.asarray(EPS * (ref["n_S"] + C0) * ref["M_S"] + ref["P_S"], np.float64) * np.outer(on, on)
    tg = np.asarray(EPS * (ref["n_g"] + C0) * ref["M_g"] + ref["P_g"], np.float64) * on
    return tS, tg, ref["tol_cost"]


def ratios(ref, S, g, cost, factor=1.0):
    on = ref["columns"] >= 0
    tS, tg, tc = tolerances(ref)
    S0, g0 = ref["S"] * np.outer(on, on), ref["g"] * on
    return st.ratio(S, S0, factor * tS), st.ratio(g, g0, factor * tg), st.ratio(cost, ref["cost"], factor * tc)


def _sum(terms, axis, order):
    """a float64 sum along `axis`, term after term, forwards (order 0) or backwards (order 1)"""
    terms = np.flip(terms, axis) if order else terms
    return np.take(np.cumsum(terms, axis=axis), -1, axis=axis)


def device64(H, b, c0, blocks, columns, order=0, mutate=None):
    """the arithmetic of the device in float64: dchi = x [-] x_lin, M3 = [oplus(conj q_lin) oplus(q / |q|)]_3x3, grad = b + H dchi,
    cost = 0.5 c0 + sum dchi (b + 0.5 H dchi), M^T H M and M^T grad with the rows of constant blocks skipped"""
    H, b = np.asarray(H, np.float64), np.asarray(b, np.float64)
    m = len(b)
    dchi, M = np.zeros(m), np.eye(m)
    for blk in blocks:
        o = blk["ordering"]
        if blk["mdim"] == 0:
            continue
        x, lin = np.asarray(blk["x"], np.float64), np.asarray(blk["lin"], np.float64)
        if blk["kind"] == "s":
            dchi[o:o + 9] = x[:9] - lin[:9]
            continue
        dchi[o:o + 3] = x[:3] - lin[:3]
        q, ql = x[3:7], lin[3:7]
        conj = np.array([-ql[0], -ql[1], -ql[2], ql[3]])
        dq = pm.quat_mul(q, conj / (ql @ ql))
        dchi[o + 3:o + 6] = (1.0 if mutate == "factor_2_dropped" else 2.0) * dq[:3]
        qc = q if mutate == "q_not_normalised" else q / np.sqrt(q @ q)
        if mutate == "lin_normalised":
            conj = conj / np.sqrt(ql @ ql)
        M3 = _sum(pr.oplus(conj)[:3, :, None] * pr.oplus(qc)[None, :, :3], 1, order)
        if mutate == "M3_transposed":
            M3 = M3.T.copy()
        if mutate == "M3_identity":
            M3 = np.eye(3)
        M[o + 3:o + 6, o + 3:o + 6] = M3
    s = _sum(H * dchi[None, :], 1, order)
    grad = b + (0.0 if mutate == "grad_without_H_dchi" else s)
    cost = 0.5 * float(c0) + float(_sum(dchi * (b + (0.0 if mutate == "cost_without_quadratic" else 0.5 * s)), 0, order))
    left = _sum(M[:, :, None] * H[:, None, :], 0, order)        # (M^T H)[i, b] = sum_a M[a, i] H[a, b]
    S = _sum(left[:, :, None] * M[None, :, :], 1, order)
    g = _sum(M * grad[:, None], 0, order)
    if mutate != "constant_not_skipped":
        on = np.asarray(columns) >= 0
        S, g = S * np.outer(on, on), g * on
    return S, g, cost


def test_oplus_is_the_quaternion_product():
    rng = np.random.Generator(np.random.PCG64(3))
    for _ in range(5):
        p, q = rng.normal(size=4), rng.normal(size=4)
        assert np.allclose(pr.oplus(q) @ p, pm.quat_mul(p, q), rtol=0, atol=1e-15)


def test_tangent_map_is_the_derivative_of_minus_after_plus():
    """M = d / d delta [(x [+] delta) [-] x_lin] at delta = 0, x [+] delta by Transformation::oplus (step_reference.pose_oplus, checked
    against mpmath in tests/test_step_reference_host.py), [-] by PoseManifold::minus; central differences in long double"""
    if not sr.have_long_double():
        pytest.skip("np.longdouble is not wider than float64 on this machine")
    rng = np.random.Generator(np.random.PCG64(11))
    for _ in range(4):
        x, lin = rng.normal(size=7), rng.normal(size=7)
        x[3:7] /= np.linalg.norm(x[3:7])    # (x [+] delta normalises x first: its derivative is taken at the normalised x)
        lin[3:7] /= np.linalg.norm(lin[3:7])    # (minus divides by |q_lin|^2 and the lift does not: the two agree at a unit q_lin only)
        blk = dict(kind="p", ordering=0, mdim=6, lin=lin, x=x)
        ref = pr.moved(np.eye(6), np.zeros(6), 0.0, [blk], np.arange(6))
        h = LD(1e-6)
        D = np.zeros((6, 6), LD)
        for c in range(6):
            d = np.zeros(6, LD)
            d[c] = h
            hi = pr.moved(np.eye(6), np.zeros(6), 0.0, [dict(blk, x=st.pose_oplus(np.asarray(x, LD), d))], np.arange(6))["dchi"]
            lo = pr.moved(np.eye(6), np.zeros(6), 0.0, [dict(blk, x=st.pose_oplus(np.asarray(x, LD), -d))], np.arange(6))["dchi"]
            D[:, c] = (hi - lo) / (2 * h)
        assert np.abs(np.asarray(D - ref["M"], np.float64)).max() < 1e-10, np.asarray(D - ref["M"], np.float64)


def test_reference_against_oracle_and_mutations(windows):
    report = []
    for name, window in windows.items():
        est, mp = window[0], window[1]
        for move, m, blocks, free, held in cases_of(window):
            H, b, c0, dH, db, dc0 = pr.from_factor(m["J"], m["e0"])
            H64, b64, c64 = m["J"].T @ m["J"], m["J"].T @ m["e0"], float(m["e0"] @ m["e0"])
            So, go, co = oracle_linearisation(est, mp, m)
            worst = {}
            for label, columns in (("free", free), ("held", held)):
                ref = pr.moved(H, b, c0, blocks, columns, dH, db, dc0)
                on = columns >= 0
                # agreement with the oracle's own linearisation (the rows of the held block masked: it has no columns)
                w = ratios(ref, So * np.outer(on, on), go * on, co, factor=2.0)
                worst["oracle " + label] = max(w)
                assert max(w) <= 1.0, (name, move, label, "oracle", w)
                for order in (0, 1):
                    w = ratios(ref, *device64(H64, b64, c64, blocks, columns, order))
                    worst["float64 " + label] = max(worst.get("float64 " + label, 0.0), *w)
                    assert max(w) <= 1.0, (name, move, label, "float64 order %d" % order, w)
                if move == "at_lin":
                    continue
                for mut in MUTATIONS:
                    if (mut == "constant_not_skipped") != (label == "held"):
                        continue
                    w = ratios(ref, *device64(H64, b64, c64, blocks, columns, 0, mut))
                    worst[mut] = max(w)
                    assert max(w) > 1.0, "%s %s: mutation %s stays inside the bound: %s" % (name, move, mut, (w,))
            if move == "at_lin" and name == "euroc_first":
                ref = pr.moved(H, b, c0, blocks, free, dH, db, dc0)
                assert np.abs(ref["dchi"]).max() < 1e-18, "straight after the first marginalisation the states are the linearisation points"
            report.append("%s %s (m %d): %s" % (name, move, m["n"], "  ".join("%s %.3g" % kv for kv in worst.items())))
    print("\n".join(report))


def test_assemble_scatters_the_moved_prior(windows):
    """schur_reference.assemble(prior=moved) with no other record: the prior's M^T H M, M^T grad and cost at the rows the block table
    gives, with exactly the prior's own bound; a constant block has neither rows nor columns"""
    est, mp, m, _ = windows["euroc_first"]
    move, m, blocks, free, held = next(c for c in cases_of(windows["euroc_first"]) if c[0] == "large")
    H, b, c0, dH, db, dc0 = pr.from_factor(m["J"], m["e0"])
    held_id = next(bl["id"] for bl in blocks if held[bl["ordering"]] < 0 and bl["mdim"] > 0)
    table, off = [], 5   # rows in another order than the prior's, starting past a block the prior does not touch
    for bl in reversed(blocks):
        if bl["mdim"] > 0 and bl["id"] != held_id:
            table.append(((bl["kind"], bl["id"]), off, bl["mdim"]))
            off += bl["mdim"]
    table.append((("s", -1), 0, 5))
    pc = st.prior_columns(dict(n=m["n"], blocks=blocks), table)
    assert ((pc >= 0) == (held >= 0)).all()
    ref = pr.moved(H, b, c0, blocks, pc, dH, db, dc0)
    out = sr.assemble([], table, 0.0, prior=ref)
    sel = np.nonzero(pc >= 0)[0]
    tS, tg, tc = tolerances(ref)
    assert np.array_equal(out["S"][np.ix_(pc[sel], pc[sel])], ref["S"][np.ix_(sel, sel)]) and np.array_equal(out["g"][pc[sel]], ref["g"][sel])
    assert not np.any(out["S"][:5]) and not np.any(out["S"][:, :5]) and out["cost"] == ref["cost"]
    assert np.allclose(out["tol_S"][np.ix_(pc[sel], pc[sel])], tS[np.ix_(sel, sel)], rtol=1e-12, atol=0)
    assert np.allclose(out["tol_g"][pc[sel]], tg[sel], rtol=1e-12, atol=0)
    assert out["tol_cost"] >= tc and out["ref_ratio"] < 1e-3


def test_moved_prior_is_one_more_record():
    """step_reference.stage_a and schur_reference.assemble with the moved prior of a random J, e0 (a constant block among its rows) give
    what the same prior gives handed over as a record of its own -- residual e0 + J dchi, Jacobian J M --, to the long-double share of the
    bounds: the five sums through Mv, My, the gradient M^T grad, the column norms diag(M^T H M), the cost"""
    if not sr.have_long_double():
        pytest.skip("np.longdouble is not wider than float64 on this machine")
    import test_step_reference_host as tsh
    recs, blocks, lm_ids, x_blocks, lm_x, y_C, P, _ = tsh.setup(2)
    rng = np.random.Generator(np.random.PCG64(78))
    m = 6 + 6 + 9
    J, e0 = np.triu(rng.normal(size=(m, m))) * 3, rng.normal(size=m)
    pblocks = []
    for k, (kind, bid, o, md) in enumerate((("p", 1, 0, 6), ("p", 99, 6, 6), ("s", 200, 12, 9))):
        lin = rng.normal(size=9 if kind == "s" else 7)
        if kind == "p":
            lin[3:7] /= np.linalg.norm(lin[3:7])
        pblocks.append(dict(kind=kind, id=bid, ordering=o, mdim=md, lin=lin, x=pm.moved_value("large", kind, k, lin)))
    pc = st.prior_columns(dict(n=m, blocks=pblocks), blocks)
    assert (pc[6:12] == -1).all() and (pc >= 0).sum() == 15
    H, b, c0, dH, db, dc0 = pr.from_factor(J, e0)
    ref = pr.moved(H, b, c0, pblocks, pc, dH, db, dc0)
    Jeff, e = np.asarray(J, LD) @ ref["M"], np.asarray(e0, LD) + np.asarray(J, LD) @ ref["dchi"]
    rec = (e, [(("p", 1), Jeff[:, 0:6]), (("p", 99), Jeff[:, 6:12]), (("s", 200), Jeff[:, 12:21])])
    va, ta, aux = st.stage_a(P, tsh.MU, y_C, ref)
    vb, tb, _ = st.stage_a(st.prepare(recs + [rec], blocks, lm_order=lm_ids), tsh.MU, y_C)
    for n in ("v_C", "y_L", "v_L") + st.SCALARS_A:
        assert st.ratio(va[n], vb[n], aux["ref_ratio"] * np.asarray(ta[n])) <= 1.0, n
    ra, rb = sr.assemble(recs, blocks, tsh.MU, prior=ref), sr.assemble(recs + [rec], blocks, tsh.MU)
    assert st.ratio(ra["S"], rb["S"], ra["ref_ratio"] * ra["tol_S"]) <= 1.0 and st.ratio(ra["g"], rb["g"], ra["ref_ratio"] * ra["tol_g"]) <= 1.0
    assert abs(float(ra["cost"] - rb["cost"])) <= ra["ref_ratio"] * ra["tol_cost"]
    # ... and Stage B's direct J delta sums take the prior through the same map
    scal = {n: float(va[n]) for n in st.GROUP_B}
    args = (scal, 0.5 * float(np.sqrt(va["gnHatSq"])), np.asarray(y_C, np.float64), np.asarray(va["v_C"], np.float64),
            np.asarray(va["y_L"], np.float64), np.asarray(va["v_L"], np.float64), x_blocks, lm_x, ta)
    wa, _ = st.stage_b(P, *args, prior=aux["prior"])
    wb, twb = st.stage_b(st.prepare(recs + [rec], blocks, lm_order=lm_ids), *args)
    for n in ("jdSq_direct", "jdDotR_direct"):
        assert st.ratio(wa[n], wb[n], aux["ref_ratio"] * twb[n]) <= 1.0, n
