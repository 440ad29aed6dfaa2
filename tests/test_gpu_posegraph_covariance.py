"""Marginal covariances of pose-graph keyframes (svin_pg_get_covariance_blocks) against the long-double reference
(tests/helpers/pg_cov_reference.py) on the case graphs of tests/helpers/pg_cases.py.

  columns        every case but `breaks` (and `radius_small`, the graph of pieces60 again), both DoF: whole columns of Sigma for
                 column keyframes picked by role from the captured partition (an interior keyframe of the first and of the last piece,
                 a cut keyframe -- a level-2 interior where level 2 is active --, a cover / root keyframe, the first free and the
                 last keyframe).  A is built from the debug step's own Ja, Jb and scales at radius = inf, as check_solve builds its
                 matrix; column j of the result, y = Sigma[:, j] / (s s_j), has to solve A y = e_j under pg_reference's stage-3 rule
                 unchanged: eta <= eta_ceiling(n, R), eta <= 8 max(eta(LAPACK), eps), forward error against the long-double
                 inverse <= kappa_2(A) x that bar.  Constant rows are exactly zero, (a, b) and (b, a) are transposes bit for bit,
                 and the case's edge was reached on the captured partition.
  determinism    the same call twice and a fresh handle return the same bits; the factor is reused (counters) until
                 add_keyframe, optimize, set_partition or another (earliest, cur).
  batch edges    B - 1, B, B + 1, 2B + 1 column keyframes in one call: every block equals the single-pair call's bit for bit and
                 the substitution passes are ceil(columns / B).
  optimised      after an optimisation the blocks follow the long-double reference at the returned poses (forward bar only:
                 the returned poses carry a rounding of their own).
  interference   covariance calls between optimisations leave poses, summary and every debug-step array as a handle that never
                 asked has them.
  singular       `breaks` and a graph with a floating second sequence return SVIN_PG_ERR_SINGULAR, name a keyframe, keep
                 nothing, and the handle then optimises to the bits of a fresh one.
  arguments      every -1 / -2 condition leaves a sentinel-filled buffer untouched; cov == NULL sizes.
  config #5      5 000 keyframes, 4-DoF: whole columns of the last keyframe and of the latest loop's partner under the backward-error
                 rule with scipy's sparse LU on the sparse A as the yardstick.

Measured on an MI355X on 2026-10-20 (`pytest -s` prints the line of every case): over the 36 case / DoF pairs the worst column has
eta = 0.8 - 4.4 x max(eta(LAPACK), eps) (bar 8; the largest: level2_fallback_6 4.38, heavy_6 3.81, level2_wide_6 3.17) and a forward
error of 0.002 - 0.036 of kappa x bar; after an optimisation 0.005 - 0.062 of it; config #5 eta 0.9e-16 - 4.3e-16 against
7e-17 - 9e-17 of the sparse LU.  The whole file: 60 tests in 13 s.
"""
import ctypes as C
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "helpers"))
import pg_cases as pc  # noqa: E402
import pg_cov_reference as cr  # noqa: E402
import pg_reference as pr  # noqa: E402

from svin_amd import synthetic_pg as spg  # noqa: E402

pytestmark = [pytest.mark.gpu, pytest.mark.skipif(not pr.have_long_double(), reason="np.longdouble is not an extended type on this platform")]

CASES = [c for c in pc.build_cases() if c.name != "radius_small"]
BY_NAME = {c.name: c for c in CASES}
CASE_DOFS = [(c, six) for c in CASES for six in c.dofs if c.name != "breaks"]
IDS = ["%s-%ddof" % (c.name, 6 if six else 4) for c, six in CASE_DOFS]
B = 8   # kPgCovBatch (include/svin_pg.h)


def handle(case, six):
    from svin_amd.posegraph import PoseGraph
    g = PoseGraph(0, six_dof=six)
    case.configure(g)
    spg.feed(g, case.spec)
    return g


def ask(g, case, local_pairs):
    """blocks of pairs given in local keyframes (keyframe index = list position, the range starts at case.earliest)"""
    e = case.earliest
    return g.covariance_blocks(e, case.cur, [(e + a, e + b) for a, b in local_pairs])


def counters(g):
    c = g.covariance_counters()
    return c["factorisations"], c["passes"], c["columns"]


@pytest.mark.parametrize("case,six", CASE_DOFS, ids=IDS)
def test_columns(gpu_lib, case, six):
    g = handle(case, six)
    cap = g.debug_step(case.earliest, case.cur, case.radius)
    assert cap is not None
    part = case.partition(cap, six)
    pr.check_partition(cap, part)
    case.reach(part, cap, six)
    A, _ = pr.system(cap["Ja"], cap["Jb"], cap["res"], cap["scale"], cap, six, np.inf)
    nn = len(cap["off"])
    cols = cr.role_columns(cap, cap)
    pairs = cr.column_pairs(nn, cols)
    blocks = ask(g, case, pairs)
    sigma = cr.columns_from_blocks(cap, six, cols, blocks)       # (asserts the constant rows are exactly zero)
    worst = cr.check_columns(A, cap["scale"], cap, six, cols, sigma)
    print("cov %s %d-DoF: n %d, %d column keyframes, worst eta %.3e, eta / max(eta(LAPACK), eps) %.2f, forward / (kappa bar) %.3f" %
          (case.name, 6 if six else 4, A.shape[0], len(cols), worst["eta"], worst["ratio"], worst["fwd"]))
    cr.check_transposes(blocks, ask(g, case, [(b, a) for a, b in pairs]))
    g.close()


@pytest.mark.parametrize("name,six", [("pieces60", False), ("level2_6", True), ("dense40", True)])
def test_determinism_and_reuse(gpu_lib, name, six):
    case = BY_NAME[name]
    g = handle(case, six)
    nn = case.cur - case.earliest + 1
    pairs = [(a, b) for b in (nn - 1, nn // 2, 3) for a in (1, nn // 3, nn // 2, nn - 1)]
    c0 = counters(g)
    first = ask(g, case, pairs)
    c1 = counters(g)
    again = ask(g, case, pairs)
    c2 = counters(g)
    assert c1[0] == c0[0] + 1 and c2[0] == c1[0], "the factor of the first call was not reused"
    assert np.array_equal(first, again)
    h = handle(case, six)
    assert np.array_equal(first, ask(h, case, pairs)), "a fresh handle returns other bits"
    h.close()
    # everything that invalidates the factor
    n = case.spec.n
    g.add_keyframe(n, int(case.spec.sequence[n - 1]), case.spec.t_svin[n - 1] + 0.1, case.spec.q_svin[n - 1])
    assert np.array_equal(first, ask(g, case, pairs)) and counters(g)[0] == c2[0] + 1      # (the new keyframe is outside the range)
    g.set_partition(case.piece, case.dense)
    ask(g, case, pairs)
    assert counters(g)[0] == c2[0] + 2
    g.set_levels(case.levels, case.l2)
    ask(g, case, pairs)
    assert counters(g)[0] == c2[0] + 3
    sub = [(a, b) for a, b in pairs if a < nn - 1 and b < nn - 1]
    e = case.earliest
    g.covariance_blocks(e, case.cur - 1, [(e + a, e + b) for a, b in sub])
    assert counters(g)[0] == c2[0] + 4, "another (earliest, cur) reused the factor"
    ask(g, case, pairs)
    assert counters(g)[0] == c2[0] + 5
    g.optimize(case.earliest, case.cur)
    ask(g, case, pairs)
    ask(g, case, pairs)
    assert counters(g)[0] == c2[0] + 6
    g.close()


@pytest.mark.parametrize("name,six", [("nodes129", False), ("nodes129", True), ("level2_4", False), ("level2_6", True)])
def test_batch_edges(gpu_lib, name, six):
    case = BY_NAME[name]
    g = handle(case, six)
    nn = case.cur - case.earliest + 1
    step = max(1, (nn - 2) // (2 * B + 1))
    spread = list(range(nn - 1, 0, -step))[:2 * B + 1]      # column keyframes spread over the whole range, the last one included
    assert len(spread) == 2 * B + 1
    single = {}
    for c in spread:
        single[c] = (ask(g, case, [(c, c)])[0], ask(g, case, [(1, c)])[0])
    for ncol in (B - 1, B, B + 1, 2 * B + 1):
        cols = spread[:ncol]
        pairs = [(c, c) for c in cols] + [(1, c) for c in cols]
        before = counters(g)
        out = ask(g, case, pairs)
        after = counters(g)
        assert after[1] - before[1] == -(-ncol // B) and after[2] - before[2] == ncol and after[0] == before[0]
        for i, c in enumerate(cols):
            assert np.array_equal(out[i], single[c][0]) and np.array_equal(out[ncol + i], single[c][1]), (ncol, c)
    g.close()


@pytest.mark.parametrize("name,six", [("dense40", False), ("dense40", True), ("level2_4", False), ("level2_6", True), ("huber_4", False),
                                      ("huber_6", True)])
def test_after_an_optimisation(gpu_lib, name, six):
    case = BY_NAME[name]
    g = handle(case, six)
    g.optimize(case.earliest, case.cur)
    T, Q = g.poses()
    P = case.problem(six)
    part = case.partition(P, six)
    states = cr.states_from_poses(P, T[case.earliest:case.cur + 1], Q[case.earliest:case.cur + 1], six, pc._r2ypr)
    assert np.max(np.abs(states["t"] - P["t"])) > 1e-6, "the optimisation moved nothing"
    ref = cr.Reference(P, states, six)
    nn = len(P["off"])
    cols = cr.role_columns(part, P)
    pairs = cr.column_pairs(nn, cols)
    blocks = ask(g, case, pairs)
    sigma = cr.columns_from_blocks(P, six, cols, blocks)
    worst = cr.check_columns(ref.A, ref.s, P, six, cols, sigma, ref_cols={k: ref.column_block(k) for k in cols}, forward_only=True)
    print("cov after optimize %s %d-DoF: forward / (kappa bar) %.3f" % (name, 6 if six else 4, worst["fwd"]))
    cr.check_blocks(ref, pairs[::5], blocks[::5])
    # at the SVIn poses the same blocks would be somewhere else: the call did take the returned poses
    ref0 = cr.Reference(P, P, six)
    with pytest.raises(AssertionError):
        cr.check_blocks(ref0, pairs, blocks)
    g.close()


@pytest.mark.parametrize("name,six", [("pieces60", False), ("level2_6", True)])
def test_no_interference(gpu_lib, name, six):
    case = BY_NAME[name]
    e, cur = case.earliest, case.cur
    x, y = handle(case, six), handle(case, six)
    pairs = [(e + 1, cur), (cur, cur), (e + 5, e + 9)]
    sx = x.optimize(e, cur)
    y.covariance_blocks(e, cur, pairs)
    sy = y.optimize(e, cur)
    y.covariance_blocks(e, cur, pairs)
    for key in ("initial_cost", "final_cost", "iterations", "termination", "successful"):
        assert sx[key] == sy[key], key
    assert y.summary()["final_cost"] == sy["final_cost"] and y.summary()["iterations"] == sy["iterations"]
    px, py = x.partition(), y.partition()
    for key in ("free", "separators", "pieces", "max_rows", "tiles", "separator_unknowns", "dense_solves", "level2_pieces"):
        assert px[key] == py[key], key
    for a, b in zip(x.poses() + x.drift()[1:], y.poses() + y.drift()[1:]):
        assert np.array_equal(a, b)
    assert x.drift()[0] == y.drift()[0]
    cx, cy = x.debug_step(e, cur, case.radius), y.debug_step(e, cur, case.radius)
    for key in cx:
        assert np.array_equal(np.asarray(cx[key]), np.asarray(cy[key])), key
    x.close()
    y.close()


def _singular_cases():
    out = [(BY_NAME["breaks"], six) for six in (False, True)]
    for six in (False, True):
        out.append((cr.second_sequence_case(), six))                                   # dense regime: the pivot is the root's
        out.append((cr.second_sequence_case(piece=8, dense=0, levels=1), six))       # pieces: the pivot is a piece's
    return out


@pytest.mark.parametrize("case,six", _singular_cases(), ids=lambda v: getattr(v, "name", None) and "%s-p%d" % (v.name, v.piece))
def test_singular(gpu_lib, case, six):
    from svin_amd.posegraph import SingularError
    P = case.problem(six)
    A, _ = cr.scaled_system(P, P, six)
    assert cr.smallest_pivot_ratio(A) < cr.PIVOT_TOL or not np.all(np.diag(A) > 0)      # singular by the rule in the reference
    g = handle(case, six)
    before = counters(g)
    named = r"keyframe \d+" if case.name == "breaks" else r"keyframe \d+|root"
    with pytest.raises(SingularError, match=named):
        ask(g, case, [(2, 5)])
    assert counters(g) == before, "a failed pass was counted or kept"
    with pytest.raises(SingularError, match=named):
        ask(g, case, [(2, 5)])
    fresh = handle(case, six)
    sg, sf = g.optimize(case.earliest, case.cur), fresh.optimize(case.earliest, case.cur)
    for key in ("initial_cost", "final_cost", "iterations", "termination", "successful"):
        assert sg[key] == sf[key], key
    for a, b in zip(g.poses(), fresh.poses()):
        assert np.array_equal(a, b)
    g.close()
    fresh.close()


@pytest.mark.parametrize("six", [False, True])
def test_arguments(gpu_lib, six):
    case = BY_NAME["pieces60"]
    g = handle(case, six)
    L, h, D = g.L, g.h, 6 if six else 4
    e, cur = case.earliest, case.cur
    ip = C.POINTER(C.c_int)

    def call(handle_, earliest, cur_, n, a, b, buf, cap):
        ia = None if a is None else np.ascontiguousarray(a, np.int32)
        ib = None if b is None else np.ascontiguousarray(b, np.int32)
        return L.svin_pg_get_covariance_blocks(handle_, earliest, cur_, n, None if ia is None else ia.ctypes.data_as(ip),
                                               None if ib is None else ib.ctypes.data_as(ip),
                                               buf.ctypes.data_as(C.POINTER(C.c_double)) if buf is not None else None, cap)
    sentinel = -123.25
    buf = np.full(2 * D * D + 3, sentinel)
    assert call(None, e, cur, 1, [e + 1], [e + 2], buf, buf.size) == -1
    assert call(h, e, cur, -1, [e + 1], [e + 2], buf, buf.size) == -1
    assert call(h, cur, e, 1, [e + 1], [e + 2], buf, buf.size) == -1
    assert call(h, e, cur, 2, [e + 1, e + 2], [e + 2, e + 3], buf, 2 * D * D - 1) == -1
    assert call(h, e, cur, 1, None, [e + 2], buf, buf.size) == -1
    assert call(h, e, cur, 1, [e + 1], None, buf, buf.size) == -1
    assert call(h, e, cur, 1, [e + 1], [10 ** 6], buf, buf.size) == -2              # unknown
    assert call(h, e, cur - 3, 1, [e + 1], [cur], buf, buf.size) == -2              # behind cur
    assert call(h, e + 2, cur, 1, [e + 1], [cur], buf, buf.size) == -2              # ahead of the range
    assert L.svin_pg_get_covariance(h, e, cur, e + 1, e + 2, buf.ctypes.data_as(C.POINTER(C.c_double)), D * D - 1) == -1
    assert np.all(buf == sentinel), "a refused call wrote to the buffer"
    assert g.covariance_counters()["factorisations"] == 0
    assert call(h, e, cur, 2, [e + 1, e + 2], [e + 2, e + 3], None, 0) == 2 * D * D      # cov == NULL only sizes
    assert call(h, e, cur, 0, None, None, None, 0) == 0
    assert g.covariance_counters()["factorisations"] == 0
    assert call(h, e, cur, 2, [e + 1, e + 2], [e + 2, e + 3], buf, buf.size) == 2 * D * D
    assert np.all(buf[2 * D * D:] == sentinel) and np.all(buf[:2 * D * D] != sentinel)
    one = np.full(D * D, sentinel)
    assert L.svin_pg_get_covariance(h, e, cur, e + 1, e + 2, one.ctypes.data_as(C.POINTER(C.c_double)), D * D) == D * D
    assert np.array_equal(one, buf[:D * D])
    assert g.covariance(e, cur, e + 1, e + 2).shape == (D, D)
    g.close()


def test_config5_columns(gpu_lib):
    import scipy.sparse as sp
    import scipy.sparse.linalg as spl
    from svin_amd.posegraph import PoseGraph
    six, D = False, 4
    spec = spg.make_pose_graph(n=5000, laps=20, loop_every=25, seed=7)
    g = PoseGraph(0, six_dof=six)
    earliest, cur = spg.feed(g, spec)
    cap = g.debug_step(earliest, cur)
    off, ea, eb = cap["off"], cap["ea"], cap["eb"]
    nn, n = len(off), len(cap["scale"])
    last_loop = max(spec.loops)
    partner = spec.loops[last_loop][0]
    cols = [cur - earliest, partner - earliest]
    assert off[cols[0]] >= 0 and off[cols[1]] >= 0 and cols[0] != cols[1]
    e = earliest
    blocks = g.covariance_blocks(e, cur, [(e + a, e + b) for a, b in cr.column_pairs(nn, cols)])
    sigma = cr.columns_from_blocks(cap, six, cols, blocks)
    # sparse A = S J^T J S from the captured blocks: entries in long double (COO, duplicates summed by the products below)
    Ja, Jb = np.asarray(cap["Ja"], pr.LD).reshape(-1, D, D), np.asarray(cap["Jb"], pr.LD).reshape(-1, D, D)
    s = np.asarray(cap["scale"], pr.LD)
    rows, colsI, vals = [], [], []

    def add(o_r, o_c, blk, mask):      # blk: ne x D x D (rows of o_r, columns of o_c)
        idx_r = (o_r[mask][:, None, None] + np.arange(D)[None, :, None]) + np.zeros((1, 1, D), int)
        idx_c = (o_c[mask][:, None, None] + np.arange(D)[None, None, :]) + np.zeros((1, D, 1), int)
        rows.append(idx_r.reshape(-1)); colsI.append(idx_c.reshape(-1)); vals.append(blk[mask].reshape(-1))
    oa, ob = off[ea], off[eb]
    add(oa, oa, np.einsum("eki,ekj->eij", Ja, Ja), oa >= 0)
    add(ob, ob, np.einsum("eki,ekj->eij", Jb, Jb), ob >= 0)
    both = (oa >= 0) & (ob >= 0)
    cross = np.einsum("eki,ekj->eij", Jb, Ja)
    add(ob, oa, cross, both)
    add(oa, ob, np.transpose(cross, (0, 2, 1)), both)
    rows, colsI, vals = np.concatenate(rows), np.concatenate(colsI), np.concatenate(vals)
    vals = vals * s[rows] * s[colsI]

    def matvec_ld(y):
        out = np.zeros(n, pr.LD)
        np.add.at(out, rows, vals * y[colsI])
        return out
    A64 = sp.coo_matrix((np.asarray(vals, np.float64), (rows, colsI)), shape=(n, n)).tocsc()
    normA = float(spl.eigsh(A64, k=1, which="LA", return_eigenvectors=False)[0])
    lu = spl.splu(A64)
    for node in cols:
        for j in range(D):
            u = off[node] + j
            unit = np.zeros(n)
            unit[u] = 1.0
            y = np.asarray(sigma[node][:, j], pr.LD) / (s * s[u])

            def eta(v):
                v = np.asarray(v, pr.LD)
                r = np.asarray(unit, pr.LD) - matvec_ld(v)
                return float(np.sqrt(r @ r)) / (normA * float(np.sqrt(v @ v)) + 1.0)
            eta_dev, eta_lu = eta(y), eta(lu.solve(unit))
            print("cov config #5 keyframe %d column %d: eta %.3e eta(splu) %.3e ceiling %.3e" % (node, j, eta_dev, eta_lu, pr.eta_ceiling(n, D)))
            assert eta_dev <= pr.eta_ceiling(n, D)
            assert eta_dev <= pr.ETA_MARGIN * max(eta_lu, pr.EPS64), (node, j, eta_dev, eta_lu)
    cr.check_transposes(blocks[:8], g.covariance_blocks(e, cur, [(e + b, e + a) for a, b in cr.column_pairs(nn, cols)[:8]]))
    g.close()
