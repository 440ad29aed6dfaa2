"""Host-only checks of the long-double step reference (tests/helpers/step_reference.py) and of its rounding bounds, on three
seeded synthetic record sets small enough for mpmath to redo everything densely:
 (a) the reference agrees with a dense 50-digit restatement -- full J, the damped normal equations solved densely, the
     traditional dogleg of Ceres written in scaled coordinates -- to long-double rounding (Stage A) and to the dogleg tolerance
     (Stage B: its inputs are the group-B sums rounded to float64, as the device hands them over);
 (b) a plain float64 numpy replay of the kernel's arithmetic (`replay`) stays inside every bound;
 (c) each of eight seeded mutations of that replay -- the bugs the issue names -- leaves at least one bound.
Every set has a constant pose, an extrinsics block, small factors, tracks of 3 .. 8 observations and one far landmark whose
V_kk is small enough for the metric's clamp to act (ht_k != V_kk: without it mutation 5 would be no mutation)."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "helpers"))
import schur_reference as sr       # noqa: E402
import step_reference as st        # noqa: E402

pytestmark = pytest.mark.skipif(not sr.have_long_double(), reason="np.longdouble is not wider than float64 on this machine")
MU = 1e-4
SEEDS = (1, 2, 3)


def problem(seed, n_lm=6):
    rng = np.random.Generator(np.random.PCG64(seed))
    poses = [("p", i) for i in range(3)]
    ext, sbs, fixed = ("e", 100), [("s", 200), ("s", 201)], ("p", 99)
    blocks, off = [], 0
    for key in poses + [ext] + sbs:
        dim = 9 if key[0] == "s" else 6
        blocks.append((key, off, dim))
        off += dim
    recs = []
    for l in range(n_lm):
        far = 1e-5 if l == n_lm - 1 else 1.0   # the far landmark: V_kk ~ 1e-9, the clamp of the metric acts
        for k in range([3, 4, 5, 8, 3, 4][l % 6]):
            pk = fixed if (l == 2 and k == 0) else poses[int(rng.integers(len(poses)))]
            sc = 10.0 ** rng.uniform(-0.5, 1)
            recs.append((rng.normal(size=2), [(pk, sc * rng.normal(size=(2, 6))), (("l", 1000 + l), far * sc * rng.normal(size=(2, 3))),
                                              (ext, sc * rng.normal(size=(2, 6)))]))
    for a, b in zip(poses[:-1], poses[1:]):
        recs.append((rng.normal(size=15), [(a, rng.normal(size=(15, 6))), (sbs[0], rng.normal(size=(15, 9))),
                                           (b, rng.normal(size=(15, 6))), (sbs[1], rng.normal(size=(15, 9)))]))
    recs.append((1e-2 * rng.normal(size=6), [(poses[0], 1e2 * np.eye(6))]))
    x_blocks = []
    for key in poses + [fixed, ext] + sbs:
        x = rng.normal(size=9 if key[0] == "s" else 7)
        if key[0] != "s":
            x[3:] /= np.linalg.norm(x[3:])
        x_blocks.append((key, x))
    lm_x = np.concatenate([rng.normal(size=(n_lm, 3)) * 5, np.ones((n_lm, 1))], 1)
    return recs, blocks, [1000 + l for l in range(n_lm)], x_blocks, lm_x


# ------------------------------------------------------------------------------------------------ float64 replay of the kernels
def dogleg64(gHatSq, jgSq, gnHatSq, gDotGn, jySq, jvDotJy, jvDotR, jyDotR, radius, plus=False):
    """doglegCoefficients line by line in float64"""
    f = np.float64
    gnorm, gnnorm, alpha = np.sqrt(f(gHatSq)), np.sqrt(f(gnHatSq)), f(gHatSq) / f(jgSq)
    if gnnorm <= radius:
        cg, cn, step = f(0), f(1), gnnorm
    elif gnorm * alpha >= radius:
        cg, cn, step = -(radius / gnorm), f(0), f(radius)
    else:
        b_dot_a = -alpha * gDotGn
        a_sq = (alpha * gnorm) * (alpha * gnorm)
        b_minus_a_sq = a_sq - 2 * b_dot_a + gnnorm * gnnorm
        cc = b_dot_a - a_sq
        dd = np.sqrt(cc * cc + b_minus_a_sq * (radius * radius - a_sq))
        beta = (dd - cc) / b_minus_a_sq if cc <= 0 else (radius * radius - a_sq) / (dd + cc)
        cg, cn = -alpha * (1.0 - beta), beta
        step = np.sqrt(max(cg * cg * gHatSq + 2 * cg * cn * gDotGn + cn * cn * gnHatSq, 0.0))
    s = 1.0 if plus else -1.0
    return cg, cn, step, cg * cg * jgSq + s * 2.0 * cg * cn * jvDotJy + cn * cn * jySq, cg * jvDotR - cn * jyDotR


def replay(recs, blocks, lm_ids, x_blocks, lm_x, mu, y_C, radius, mutation=None):
    """k_post_solve + the fused step in float64, landmark by landmark and record by record as the kernel walks them; returns the
    layout of Estimator.debug_trust_region_step.  mutation: one of MUTATIONS."""
    col = {k: (o, n) for k, o, n in blocks}
    d = max(o + n for _, o, n in blocks)
    y = np.asarray(y_C, np.float64)
    g, h = np.zeros(d), np.zeros(d)
    by_lm, facs = {}, []
    for r, bl in recs:
        r = np.asarray(r, np.float64)
        idx, Js, lm, Jl = [], [], None, None
        for key, J in bl:
            if key[0] == "l":
                lm, Jl = key[1], np.asarray(J, np.float64)
            elif key in col:
                idx.append(np.arange(col[key][0], col[key][0] + col[key][1]))
                Js.append(np.asarray(J, np.float64))
        idx, Jc = np.concatenate(idx), np.concatenate(Js, 1)
        g[idx] += Jc.T @ r
        h[idx] += (Jc * Jc).sum(0)
        (by_lm.setdefault(lm, []) if lm is not None else facs).append((idx, Jc, Jl, r))

    def metric(hh):
        sc = 1.0 / (1.0 + np.sqrt(hh))
        return np.minimum(np.maximum(hh * sc * sc, 1e-6), 1e32) / (sc * sc)
    ht = metric(h)
    v = g / ht
    acc = np.zeros(8)   # jgSq jySq jvDotJy jvDotR jyDotR gHat gnHat gDotGn
    gmax = np.abs(g).max()
    yL, vL = np.zeros((len(lm_ids), 3)), np.zeros((len(lm_ids), 3))
    for li, lm in enumerate(lm_ids):
        rows = by_lm[lm]
        V = sum(Jl.T @ Jl for _, _, Jl, _ in rows)
        b = sum(Jl.T @ r for _, _, Jl, r in rows)
        hl = metric(np.diag(V))
        X = np.linalg.inv(V + mu * np.diag(hl))
        us = [(Jc @ y[idx], Jc @ v[idx]) for idx, Jc, _, _ in rows]
        t = np.zeros(3)
        for k, ((_, _, Jl, _), (uy, _)) in enumerate(zip(rows, us)):
            if mutation == "dropped_observation" and li == 1 and k == len(rows) - 1:
                continue
            t += Jl.T @ uy
            if mutation == "doubled_observation" and li == 1 and k == 0:
                t += Jl.T @ uy
        yl = X @ (b - t)
        vl = b / (np.diag(V) if mutation == "v_by_V_kk" else hl)
        yL[li], vL[li] = yl, vl
        acc[5] += (b * b / hl).sum()
        acc[6] += (hl * yl * yl).sum()
        acc[7] += -(b @ yl)
        gmax = max(gmax, np.abs(b).max())
        for (_, _, Jl, r), (uy, uv) in zip(rows, us):
            jv, jy = uv + Jl @ vl, uy + Jl @ yl
            acc[:5] += [jv @ jv, jy @ jy, jv @ jy, jv @ r, jy @ r]
    if mutation == "neighbour_y":
        yL[2] = yL[3]
    for idx, Jc, _, r in facs:
        jv, jy = Jc @ v[idx], Jc @ y[idx]
        acc[:5] += [jv @ jv, jy @ jy, jv @ jy, jv @ r, jy @ r]
    acc[5] += (g * g / ht).sum()
    acc[6] += (ht * y * y).sum()
    acc[7] += -(g @ y)
    scal = dict(gHatSq=acc[5], jgSq=acc[0], gnHatSq=acc[6], gDotGn=acc[7], jySq=acc[1], jvDotJy=acc[2], jvDotR=acc[3], jyDotR=acc[4],
                gradMax=gmax)
    cg, cn, step, jd_sq, jd_r = dogleg64(*[scal[k] for k in st.GROUP_B], radius, plus=mutation == "plus_on_jvDotJy")
    scal.update(doglegStepNorm=step, jdSq=jd_sq, jdDotR=jd_r, spareA0=cg, spareA1=cn)
    cand, step_sq, x_sq = [], 0.0, 0.0
    for key, x in x_blocks:
        x = np.asarray(x, np.float64)
        if key in col:
            dl = cg * v[col[key][0]:col[key][0] + col[key][1]] - cn * y[col[key][0]:col[key][0] + col[key][1]]
            xo = x + dl if key[0] == "s" else st.pose_oplus(x, dl)
            step_sq += (x - xo) @ (x - xo)
            x_sq += x @ x
        elif mutation == "constant_block_moved":
            xo = x.copy()
            xo[:3] += cg * v[:3] - cn * y[:3]
        else:
            xo = x.copy()
        cand.append(xo)
    lm_c = np.asarray(lm_x, np.float64).copy()
    lm_c[:, :3] += cg * vL - cn * yL
    if mutation == "w_one_ulp":
        lm_c[1, 3] = np.nextafter(lm_c[1, 3], 2.0)
    step_sq += ((lm_x[:, :3] - lm_c[:, :3]) ** 2).sum()
    x_sq += (lm_x[:, :3] ** 2).sum() + (0.0 if mutation == "x_norm_without_w" else (lm_x[:, 3] ** 2).sum())
    scal.update(stepNormSq=step_sq, xNormSq=x_sq)
    return dict(scalars=scal, y_C=y, v_C=v, y_L=yL, v_L=vL, block_cand=cand, lm_cand=lm_c, form=st.DEFERRED, radius=radius)


MUTATIONS = ("dropped_observation", "doubled_observation", "plus_on_jvDotJy", "neighbour_y", "v_by_V_kk", "constant_block_moved",
             "w_one_ulp", "x_norm_without_w")


def setup(seed):
    recs, blocks, lm_ids, x_blocks, lm_x = problem(seed)
    f64 = sr.assemble(recs, blocks, MU, dtype=np.float64)
    y_C = np.linalg.solve(np.asarray(f64["S"], np.float64), np.asarray(f64["g"], np.float64))
    P = st.prepare(recs, blocks, lm_order=lm_ids)
    va, ta, aux = st.stage_a(P, MU, y_C)
    gn, ag = float(np.sqrt(va["gnHatSq"])), float(va["gHatSq"] * np.sqrt(va["gHatSq"]) / va["jgSq"])
    assert ag < gn
    return recs, blocks, lm_ids, x_blocks, lm_x, y_C, P, (gn, ag)


@pytest.fixture(scope="module", params=SEEDS)
def case(request):
    return setup(request.param)


def test_float64_replay_stays_inside_every_bound(case):
    recs, blocks, lm_ids, x_blocks, lm_x, y_C, P, (gn, ag) = case
    branches = set()
    for radius in (2 * gn, 0.5 * ag, 0.5 * (ag + gn), ag + 0.1 * (gn - ag)):
        res = replay(recs, blocks, lm_ids, x_blocks, lm_x, MU, y_C, radius)
        worst, br, _ = st.judge(P, MU, res, x_blocks, lm_x)
        branches.add(br)
        print("radius %.4g branch %d: %s" % (radius, br, "  ".join("%s %.2g" % kv for kv in sorted(worst.items()))))
        assert max(worst.values()) <= 1.0, {k: w for k, w in worst.items() if w > 1.0}
    assert branches == {st.NEWTON, st.CAUCHY, st.INTERP}


@pytest.mark.parametrize("mutation", MUTATIONS)
def test_every_mutation_leaves_a_bound(case, mutation):
    recs, blocks, lm_ids, x_blocks, lm_x, y_C, P, (gn, ag) = case
    radius = 0.5 * (ag + gn)   # the interpolation: both coefficients are at work
    res = replay(recs, blocks, lm_ids, x_blocks, lm_x, MU, y_C, radius, mutation)
    worst, br, _ = st.judge(P, MU, res, x_blocks, lm_x)
    assert br == st.INTERP
    out = {k: w for k, w in worst.items() if w > 1.0}
    print("%s: outside %s" % (mutation, "  ".join("%s %.3g" % kv for kv in sorted(out.items()))))
    assert out, "the mutation %s stays inside every bound" % mutation


# ------------------------------------------------------------------------------------------------ dense mpmath restatement
def mp_dense(recs, blocks, lm_ids, mu, radius):
    import mpmath as mp
    col = {k: (o, n) for k, o, n in blocks}
    d = max(o + n for _, o, n in blocks)
    lcol = {l: d + 3 * i for i, l in enumerate(lm_ids)}
    n = d + 3 * len(lm_ids)
    rows, rr = [], []
    for r, bl in recs:
        m = len(r)
        block = [[mp.mpf(0)] * n for _ in range(m)]
        for k, J in bl:
            o = lcol[k[1]] if k[0] == "l" else (col[k][0] if k in col else None)
            if o is None:
                continue
            J = np.asarray(J, np.float64).reshape(m, -1)
            for a in range(m):
                for c in range(J.shape[1]):
                    block[a][o + c] = mp.mpf(float(J[a, c]))
        rows += block
        rr += [mp.mpf(float(x)) for x in r]
    J, r = mp.matrix(rows), mp.matrix(rr)
    H, g = J.T * J, J.T * r
    ht = []
    for i in range(n):
        sc = 1 / (1 + mp.sqrt(H[i, i]))
        ht.append(min(max(H[i, i] * sc * sc, mp.mpf(1e-6)), mp.mpf(1e32)) / (sc * sc))   # (the clamps are the doubles 1e-6 and 1e32)
    Hd = H.copy()
    for i in range(n):
        Hd[i, i] += mp.mpf(mu) * ht[i]
    y = mp.lu_solve(Hd, g)
    v = mp.matrix([g[i] / ht[i] for i in range(n)])
    Jv, Jy = J * v, J * y
    dot = lambda a, b: sum(a[i] * b[i] for i in range(len(a)))
    out = dict(y=y, v=v, d=d, jgSq=dot(Jv, Jv), jySq=dot(Jy, Jy), jvDotJy=dot(Jv, Jy), jvDotR=dot(Jv, r), jyDotR=dot(Jy, r),
               gHatSq=sum(g[i] ** 2 / ht[i] for i in range(n)), gnHatSq=sum(ht[i] * y[i] ** 2 for i in range(n)),
               gDotGn=-dot(g, y), gradMax=max(abs(g[i]) for i in range(n)))
    # traditional dogleg (ceres dogleg_strategy.cc) in the scaled coordinates x_hat = D x, D = sqrt(ht): gradient D^-1 g,
    # Gauss-Newton step -D y, Cauchy point -alpha g_hat with alpha = |g_hat|^2 / |J D^-1 g_hat|^2
    D = [mp.sqrt(t) for t in ht]
    g_hat = mp.matrix([g[i] / D[i] for i in range(n)])
    gn_hat = mp.matrix([-D[i] * y[i] for i in range(n)])
    Jg = J * mp.matrix([g_hat[i] / D[i] for i in range(n)])
    alpha = dot(g_hat, g_hat) / dot(Jg, Jg)
    norm = lambda a: mp.sqrt(dot(a, a))
    if norm(gn_hat) <= radius:
        s_hat, branch = gn_hat, st.NEWTON
    elif alpha * norm(g_hat) >= radius:
        s_hat, branch = -(radius / norm(g_hat)) * g_hat, st.CAUCHY
    else:
        a, b = -alpha * g_hat, gn_hat
        ba = b - a
        # |a + beta (b - a)| = radius, the root in (0, 1]
        qa, qb, qc = dot(ba, ba), 2 * dot(a, ba), dot(a, a) - mp.mpf(radius) ** 2
        beta = (-qb + mp.sqrt(qb * qb - 4 * qa * qc)) / (2 * qa)
        s_hat, branch = a + beta * ba, st.INTERP
    step = mp.matrix([s_hat[i] / D[i] for i in range(n)])
    Js = J * step
    out.update(step=step, stepNorm=norm(s_hat), jdSq=dot(Js, Js), jdDotR=dot(Js, r), branch=branch)
    return out


def to_ld(v):
    hi = float(v)
    return st.LD(hi) + st.LD(float(v - hi))


@pytest.mark.parametrize("seed", SEEDS)
def test_reference_against_dense_mpmath(seed):
    mp = pytest.importorskip("mpmath")
    recs, blocks, lm_ids, x_blocks, lm_x, _, P, (gn, ag) = setup(seed)
    with mp.workdps(50):
        for radius in (2 * gn, 0.5 * ag, 0.5 * (ag + gn)):
            dense = mp_dense(recs, blocks, lm_ids, MU, radius)
            d, L = dense["d"], len(lm_ids)
            y_C = np.array([to_ld(dense["y"][i]) for i in range(d)])
            va, ta, aux = st.stage_a(P, MU, y_C)
            share = aux["ref_ratio"]
            worst = {}
            worst["v_C"] = st.ratio(va["v_C"], np.array([to_ld(dense["v"][i]) for i in range(d)]), share * ta["v_C"])
            for n, src in (("y_L", "y"), ("v_L", "v")):
                worst[n] = st.ratio(va[n], np.array([to_ld(dense[src][d + i]) for i in range(3 * L)]).reshape(L, 3), share * ta[n])
            for n in st.SCALARS_A:
                worst[n] = st.ratio(va[n], to_ld(dense[n]), share * ta[n])
            # Stage B from the sums as the device hands them over: rounded to float64
            scal = {n: float(va[n]) for n in st.GROUP_B}
            y64, v64 = np.asarray(y_C, np.float64), np.asarray(va["v_C"], np.float64)
            vb, tb = st.stage_b(P, scal, radius, y64, v64, np.asarray(va["y_L"], np.float64), np.asarray(va["v_L"], np.float64),
                                x_blocks, lm_x, ta)
            assert vb["branch"] == dense["branch"]
            for n in ("stepNorm", "jdSq", "jdDotR"):
                worst[n] = st.ratio(vb[n], to_ld(dense[n]), tb[n])
                if n != "stepNorm":
                    worst[n + "_direct"] = st.ratio(vb[n + "_direct"], to_ld(dense[n]), tb[n + "_direct"])
            # the step itself: delta = cg v - cn y on every block and landmark
            step = np.array([to_ld(dense["step"][i]) for i in range(d + 3 * L)])
            for (key, x), c, t in zip(x_blocks, vb["block_cand"], tb["block_cand"]):
                if key[0] == "s":
                    off = dict((k, o) for k, o, _ in blocks)[key]
                    worst["sb"] = max(worst.get("sb", 0.0), st.ratio(c - np.asarray(x, st.LD), step[off:off + 9], t))
            worst["landmarks"] = st.ratio(vb["lm_cand"][:, :3] - lm_x[:, :3], step[d:].reshape(L, 3), tb["lm_cand"])
            print("seed %d radius %.4g branch %d: %s" % (seed, radius, dense["branch"], "  ".join("%s %.2g" % kv for kv in sorted(worst.items()))))
            assert max(worst.values()) <= 1.0, {k: w for k, w in worst.items() if w > 1.0}


def test_prior_is_one_more_record():
    """the prior handed over as (J, e0, columns) gives the values of the same J and e0 handed over as a record of its own, with
    bounds at least as wide (the device sums the prior's products over its rows first), also with a constant block among its rows;
    schur_reference.assemble takes the same prior as H = J^T J, b0 = J^T e0, c0 = e0 . e0 / 2"""
    recs, blocks, lm_ids, x_blocks, lm_x, y_C, P, _ = setup(2)
    rng = np.random.Generator(np.random.PCG64(77))
    m = 6 + 6 + 9
    J, e0 = np.triu(rng.normal(size=(m, m))) * 3, rng.normal(size=m)
    marg = dict(n=m, blocks=[dict(id=1, ordering=0, mdim=6), dict(id=99, ordering=6, mdim=6), dict(id=200, ordering=12, mdim=9)])
    pc = st.prior_columns(marg, blocks)
    assert (pc[6:12] == -1).all() and pc[0] == 6 and pc[12] == dict((k, o) for k, o, _ in blocks)[("s", 200)]
    va, ta, aux = st.stage_a(P, MU, y_C, (J, e0, pc))
    rec = (e0, [(("p", 1), J[:, 0:6]), (("p", 99), J[:, 6:12]), (("s", 200), J[:, 12:21])])
    P2 = st.prepare(recs + [rec], blocks, lm_order=lm_ids)
    vb, tb, _ = st.stage_a(P2, MU, y_C)
    for n in ("v_C", "y_L", "v_L") + st.SCALARS_A:
        assert st.ratio(va[n], vb[n], aux["ref_ratio"] * np.asarray(tb[n])) <= 1.0, n
        assert np.all(np.asarray(ta[n]) >= np.asarray(tb[n]) * (1 - 1e-12)), n
    sel = pc >= 0
    H, b0 = J.T @ J, J.T @ e0
    ra = sr.assemble(recs, blocks, MU, prior=(H, b0, 0.5 * e0 @ e0, pc))
    rb = sr.assemble(recs + [rec], blocks, MU)
    assert np.abs(np.asarray(ra["S"] - rb["S"], np.float64)).max() <= 1e-12 * np.abs(np.asarray(rb["S"], np.float64)).max()
    assert np.abs(np.asarray(ra["g"] - rb["g"], np.float64)).max() <= 1e-12 * np.abs(np.asarray(rb["g"], np.float64)).max()
    assert abs(float(ra["cost"] - rb["cost"])) <= 1e-14 * float(rb["cost"]) and sel.sum() == 15


def test_pose_oplus_is_the_definition():
    """x [+] delta in long double against mpmath: normalise, exp(delta / 2) from the left, normalise"""
    mp = pytest.importorskip("mpmath")
    rng = np.random.Generator(np.random.PCG64(5))
    with mp.workdps(50):
        for _ in range(5):
            x, dl = rng.normal(size=7), rng.normal(size=6) * 10.0 ** rng.uniform(-8, 0)
            got = st.pose_oplus(np.asarray(x, st.LD), np.asarray(dl, st.LD))
            q = [mp.mpf(float(c)) for c in x[3:]]
            nq = mp.sqrt(sum(c * c for c in q))
            q = [c / nq for c in q]
            w = [mp.mpf(float(c)) for c in dl[3:]]
            th = mp.sqrt(sum(c * c for c in w))
            dq = [mp.sin(th / 2) / th * c for c in w] + [mp.cos(th / 2)]
            a, b = dq, q
            qn = [a[3] * b[0] + a[0] * b[3] + a[1] * b[2] - a[2] * b[1], a[3] * b[1] + a[1] * b[3] + a[2] * b[0] - a[0] * b[2],
                  a[3] * b[2] + a[2] * b[3] + a[0] * b[1] - a[1] * b[0], a[3] * b[3] - a[0] * b[0] - a[1] * b[1] - a[2] * b[2]]
            nn = mp.sqrt(sum(c * c for c in qn))
            want = [mp.mpf(float(x[k])) + mp.mpf(float(dl[k])) for k in range(3)] + [c / nn for c in qn]
            assert max(abs(to_ld_mp(got[k]) - want[k]) for k in range(7)) < st.Q_OPS * float(np.finfo(st.LD).eps)


def to_ld_mp(x):
    import mpmath as mp
    hi = float(x)
    return mp.mpf(hi) + mp.mpf(float(x - np.longdouble(hi)))
