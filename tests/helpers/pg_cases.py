"""The case graphs of tests/test_gpu_posegraph_stages.py and tests/test_pg_reference_host.py: the smallest pose graphs that
reach each edge of the pose-graph kernels and of the host's symbolic step, and a restatement of the local problem
optimize() builds from the keyframe list (so that the host tests see the problems the GPU tests run)."""
from dataclasses import dataclass, field

import numpy as np

from svin_amd import synthetic_pg as spg

import pg_reference as pr


def _r2ypr(q):
    """hostR2ypr: degrees, from the quaternion's rotation matrix"""
    R = spg.q2R(q)
    yw = np.arctan2(R[1, 0], R[0, 0])
    p = np.arctan2(-R[2, 0], R[0, 0] * np.cos(yw) + R[1, 0] * np.sin(yw))
    r = np.arctan2(R[0, 2] * np.sin(yw) - R[1, 2] * np.cos(yw), -R[0, 1] * np.sin(yw) + R[1, 1] * np.cos(yw))
    return np.array([yw, p, r]) / np.pi * 180.0


def _qmul(a, b):
    return np.array([a[3] * b[0] + a[0] * b[3] + a[1] * b[2] - a[2] * b[1], a[3] * b[1] + a[1] * b[3] + a[2] * b[0] - a[0] * b[2],
                     a[3] * b[2] + a[2] * b[3] + a[0] * b[1] - a[1] * b[0], a[3] * b[3] - a[0] * b[0] - a[1] * b[1] - a[2] * b[2]])


def local_problem(spec, six, earliest, cur):
    """optimize()'s problem construction (keyframe index = list position, as spg.feed adds them): the arrays debug_step
    captures under the same names, float64"""
    yaw, pitch, roll, t, q, seq, fixed = [], [], [], [], [], [], []
    ea, eb, eloop, et, eyaw, epitch, eroll, eq, esq = [], [], [], [], [], [], [], [], []
    local_of = {}
    i = 0
    for k in range(spec.n):
        if k < earliest:
            continue
        local_of[k] = i
        ypr = _r2ypr(spec.q_svin[k])
        yaw.append(ypr[0]); pitch.append(ypr[1]); roll.append(ypr[2])
        t.append(spec.t_svin[k]); q.append(spec.q_svin[k]); seq.append(int(spec.sequence[k]))
        fixed.append((k == earliest or seq[-1] == 0) if six else (k <= earliest))
        for j in range(1, (4 if six else 2) + 1):
            if i - j >= 0 and seq[i] == seq[i - j]:
                qa = q[i - j]
                Ra = spg.q2R(qa)
                et.append(Ra.T @ (t[i] - t[i - j]))
                ea.append(i - j); eb.append(i); eloop.append(0)
                eyaw.append(yaw[i] - yaw[i - j]); epitch.append(pitch[i - j]); eroll.append(roll[i - j])
                n2 = qa @ qa
                eq.append(_qmul(np.array([-qa[0], -qa[1], -qa[2], qa[3]]) / n2, q[i]))
                esq.append([20, 20, 20, 100, 100, 57.3])
        if k in spec.loops:
            old, rt, rq, ry = spec.loops[k]
            if old in local_of:
                ci = local_of[old]
                ea.append(ci); eb.append(i); eloop.append(1)
                et.append(np.asarray(rt, float)); eyaw.append(float(ry)); epitch.append(pitch[ci]); eroll.append(roll[ci])
                eq.append(np.asarray(rq, float)); esq.append([20, 20, 20, 100, 100, 100])
        i += 1
        if k == cur:
            break
    D = 6 if six else 4
    off, n = [], 0
    for f in fixed:
        off.append(-1 if f else n)
        n += 0 if f else D
    f64 = lambda a, w: np.asarray(a, np.float64).reshape(-1, w).reshape(-1)   # noqa: E731
    return dict(ea=np.array(ea, int), eb=np.array(eb, int), eloop=np.array(eloop, int), off=np.array(off, int),
                et=f64(et, 3), eyaw=f64(eyaw, 1), epitch=f64(epitch, 1), eroll=f64(eroll, 1), eq=f64(eq, 4), esq=f64(esq, 6),
                yaw=f64(yaw, 1), pitch=f64(pitch, 1), roll=f64(roll, 1), t=f64(t, 3), q=f64(q, 4))


PROBLEM_KEYS = ("ea", "eb", "eloop", "off", "et", "eyaw", "epitch", "eroll", "eq", "esq", "yaw", "pitch", "roll", "t", "q")


def set_loops(spec, pairs, seed, noise_t=0.002, noise_deg=0.02, offsets=None):
    """replace the spec's loop edges by (cur, old) pairs measured from the true geometry as make_pose_graph does;
    offsets: {cur: (dt[3], dyaw_deg)} added to the measurement"""
    rng = np.random.default_rng(seed)
    spec.loops = {}
    for k, old in pairs:
        Ro, Rc = spec.R_true[old], spec.R_true[k] @ spg.ypr2R(rng.normal(0, noise_deg, 3))
        rel_t = Ro.T @ (spec.t_true[k] - spec.t_true[old]) + rng.normal(0, noise_t, 3)
        yaw = spg.R2ypr(Rc)[0] - spg.R2ypr(Ro)[0]
        if offsets and k in offsets:
            rel_t = rel_t + np.asarray(offsets[k][0], float)
            yaw += offsets[k][1]
        yaw = yaw - 360.0 if yaw > 180.0 else (yaw + 360.0 if yaw < -180.0 else yaw)
        spec.loops[int(k)] = (int(old), rel_t, spg.R2q(Ro.T @ Rc), float(yaw))
    return spec


@dataclass
class Case:
    name: str
    spec: object
    piece: int = 0              # set_partition(piece, dense); 0 = the default length
    dense: int = 128
    levels: int = 2
    l2: int = 0                 # set_levels(levels, l2); 0 = the default length
    radius: float = 1e4
    dofs: tuple = (False, True)
    reach: object = None        # reach(part, problem, six, ref=None): asserts that the planned edge was reached
    earliest: int = 0
    extra: dict = field(default_factory=dict)

    @property
    def cur(self):
        return self.spec.n - 1

    def lengths(self, six):
        return (self.piece or (64 if six else 32)), (self.l2 or (32 if six else 16))

    def problem(self, six):
        return local_problem(self.spec, six, self.earliest, self.cur)

    def partition(self, problem, six):
        piece, l2 = self.lengths(six)
        return pr.partition(problem, six, piece, self.dense, self.levels, l2)

    def configure(self, pg):
        pg.set_partition(self.piece, self.dense)
        pg.set_levels(self.levels, self.l2)


def _graph(n, pairs, seed, sequence=None, **kw):
    spec = spg.make_pose_graph(n=n, laps=1, loop_every=10 ** 6, seed=seed)
    set_loops(spec, pairs, seed + 1, **kw)
    if sequence is not None:
        spec.sequence[:] = sequence
    return spec


def _earliest(spec):
    return min((v[0] for v in spec.loops.values()), default=0)


def _case(name, spec, reach, **kw):
    return Case(name=name, spec=spec, reach=reach, earliest=_earliest(spec), **kw)


def _free(problem):
    return int(np.sum(np.asarray(problem["off"]) >= 0))


# ---- reach predicates
def reach_dense(part, problem, six, ref=None):
    assert part["nPieces"] == 0 and part["nS"] == _free(problem) * (6 if six else 4)


def reach_pieces(part, problem, six, ref=None):
    assert part["nPieces"] >= 2 and part["nPieces2"] == 0 and np.all(part["rows"] > 0)


def reach_short_last(part, problem, six, ref=None):
    D = 6 if six else 4
    assert part["nPieces"] >= 2 and part["rows"][-1] == D < part["BW"]


def reach_counts(ne=None, nn=None):
    def f(part, problem, six, ref=None):
        if ne is not None:
            assert len(problem["ea"]) == ne[1 if six else 0], len(problem["ea"])
        if nn is not None:
            assert len(problem["off"]) == nn, len(problem["off"])
    return f


def reach_level2(part, problem, six, ref=None):
    assert part["nPieces"] >= 8 and part["nPieces2"] >= 2 and part["nR"] < part["nS"]


def reach_level2_control(part, problem, six, ref=None):
    assert part["nPieces"] >= 8 and part["nPieces2"] == 0 and part["nR"] == part["nS"]


def reach_fallback(part, problem, six, ref=None):
    assert part["level2_requested"] and part["nPieces2"] == 0 and part["nPieces"] >= 8


def reach_adjacency(lo, hi, closed):
    """the fullest piece's columns within (lo, hi]; closed: it was closed by the separators it touches, not by its length
    (256 / D keyframes) and not by the end of the chain"""
    def f(part, problem, six, ref=None):
        D = 6 if six else 4
        full = int(np.argmax(part["cols"]))
        assert lo < int(part["cols"][full]) <= hi, int(part["cols"][full])
        if closed:
            assert full < part["nPieces"] - 1 and part["rows"][full] < (256 // D) * D, "the fullest piece was not closed by adjacency"
    return f


def reach_level2_wide(part, problem, six, ref=None):
    assert part["nPieces2"] >= 2 and 192 < int(np.max(part["cols2"])) <= 256, part["cols2"]


def _shared_kinds(part, problem):
    """kinds (1 sep-sep, 2 band, 3 coupling) of the destination blocks that a loop edge shares with a sequential edge"""
    ea, eb, lp, off = problem["ea"], problem["eb"], problem["eloop"], problem["off"]
    seqs = {(int(a), int(b)) for a, b, l in zip(ea, eb, lp) if not l}
    kinds = set()
    for a, b, l in zip(ea, eb, lp):
        if l and (int(a), int(b)) in seqs and off[a] >= 0 and off[b] >= 0:
            sa, sb = part["isSep"][a], part["isSep"][b]
            kinds.add(1 if sa and sb else (2 if not sa and not sb else 3))
    return kinds


def reach_shared(kind):
    def f(part, problem, six, ref=None):
        assert kind in _shared_kinds(part, problem), _shared_kinds(part, problem)
    return f


def reach_breaks(part, problem, six, ref=None):
    D = 6 if six else 4
    off, ea, eb = problem["off"], problem["ea"], problem["eb"]
    deg = np.zeros(len(off), int)
    np.add.at(deg, ea, 1)
    np.add.at(deg, eb, 1)
    assert off[-1] >= 0 and deg[-1] == 0, "the last keyframe is not isolated"
    assert part["nPieces"] >= 2
    # a chain break inside a piece: two consecutive interior keyframes of one piece with no edge between them
    pairs = {(int(a), int(b)) for a, b in zip(ea, eb)}
    assert any(part["nodePiece"][k] >= 0 and part["nodePiece"][k] == part["nodePiece"][k + 1] and (k, k + 1) not in pairs
               for k in range(len(off) - 1)), "no chain break inside a piece"


def reach_constant_middle(part, problem, six, ref=None):
    off, ea, eb = problem["off"], problem["ea"], problem["eb"]
    one = np.sum((off[ea] < 0) != (off[eb] < 0))
    both = np.sum((off[ea] < 0) & (off[eb] < 0))
    assert one > 0 and both > 0, (one, both)
    assert part["nPieces"] >= 2


def reach_huber(part, problem, six, ref=None):
    E = pr.edges(problem, problem, six)
    s = np.asarray(E["s"].v, float)[np.asarray(problem["eloop"]) != 0]
    assert np.any((s > 0.0098) & (s < 0.01)) and np.any((s > 0.01) & (s < 0.0102)) and np.any(s > 1.0) and np.any(s == 0.0), np.sort(s)


def reach_wrap(part, problem, six, ref=None):
    """ref: dict with yawC (the candidate yaws of the step under test) once a step is at hand"""
    yaw, ea, eb = problem["yaw"], problem["ea"], problem["eb"]
    raw = yaw[eb] - yaw[ea] - problem["eyaw"]
    assert np.any(np.abs(raw) > 180.0), "no residual wraps"
    if ref is not None:
        assert np.any(np.abs(np.asarray(ref["yawC"], float) - yaw) > 300.0), "no candidate yaw crossed +-180"


def _ring(n, every, back):
    return [(k, k - back) for k in range(back, n) if k % every == 0]


def _exact_loop(spec, k, old, six_too=True):
    """a loop measurement that the SVIn poses satisfy exactly in float64 (residual exactly zero): the same expressions
    optimize() uses for the sequential measurements"""
    qa, qb = spec.q_svin[old], spec.q_svin[k]
    rel_t = spg.q2R(qa).T @ (spec.t_svin[k] - spec.t_svin[old])
    n2 = qa @ qa
    rel_q = _qmul(np.array([-qa[0], -qa[1], -qa[2], qa[3]]) / n2, qb)
    return (int(old), rel_t, rel_q, float(_r2ypr(qb)[0] - _r2ypr(qa)[0]))


def build_cases():
    C = []
    # baseline: one dense solve
    C.append(_case("dense40", _graph(41, [(20, 0), (33, 6), (40, 12)], 101), reach_dense))
    # ordinary pieces, one level
    C.append(_case("pieces60", _graph(61, [(30, 0), (44, 9), (58, 21)], 103), reach_pieces, piece=8, dense=0, levels=1))
    # the last piece holds one keyframe: rows = D < BW (n chosen per DoF; the loops sit early so the tail is a plain chain)
    for six, n in ((False, _search_short_last(False)), (True, _search_short_last(True))):
        C.append(_case("short_last_%d" % (6 if six else 4), _graph(n, [(12, 0), (25, 4)], 105), reach_short_last, piece=8, dense=0,
                       levels=1, dofs=(six,)))
    # block edges of the 128-thread kernels: 127 / 128 / 129 edges (4-DoF: 64 nodes, 6-DoF: 33 nodes), 128 / 129 nodes
    for i, ne in enumerate((127, 128, 129)):
        lp = [(40, 0), (50, 3), (60, 7), (63, 20)][:2 + i]
        C.append(_case("edges%d_4" % ne, _graph(64, lp, 107 + i), reach_counts(ne=(ne, None), nn=64), dofs=(False,)))
        lp6 = [(12, 0), (16, 1), (20, 2), (24, 3), (28, 5), (30, 9), (32, 14)][:5 + i]
        C.append(_case("edges%d_6" % ne, _graph(33, lp6, 117 + i), reach_counts(ne=(None, ne), nn=33), dofs=(True,)))
    for nn in (128, 129):
        C.append(_case("nodes%d" % nn, _graph(nn, [(60, 0), (100, 30), (nn - 1, 64)], 121 + nn), reach_counts(nn=nn)))
    # level 2 and its one-level control
    for six, n in ((False, 161), (True, 111)):
        tag = "6" if six else "4"
        lp = _ring(n, 23, 40)
        C.append(_case("level2_" + tag, _graph(n, [(40, 0)] + lp[1:], 131), reach_level2, piece=8, dense=0, levels=2, l2=8, dofs=(six,)))
        C.append(_case("level2_control_" + tag, _graph(n, [(40, 0)] + lp[1:], 131), reach_level2_control, piece=8, dense=0, levels=1,
                       l2=8, dofs=(six,)))
    # pieces closed by the separators they touch (a loop on every keyframe into one earlier stretch, distinct targets: every
    # target is a cover), the fullest one within one keyframe of the 256-column budget: _budget_pairs
    C.append(_case("heavy_hi_4", _graph(_budget_pairs(False)[-1][0] + 3, _budget_pairs(False), 141), reach_adjacency(252, 256, closed=True), piece=64, dense=0,
                   levels=1, dofs=(False,)))
    hv4 = [(k, k - 78) for k in range(80, 124)]
    C.append(_case("heavy_lo_4", _graph(124, hv4, 141), reach_adjacency(128, 192, closed=False), piece=64, dense=0, levels=1,
                   dofs=(False,)))
    C.append(_case("heavy_6", _graph(_budget_pairs(True)[-1][0] + 3, _budget_pairs(True), 143), reach_adjacency(250, 256, closed=True), piece=42, dense=0,
                   levels=1, dofs=(True,)))
    # level 2 requested, validated and refused (a level-2 piece would touch too many root separators): one level after all
    C.append(_case("level2_fallback_6", _graph(170, [(k, 2 + (k * 7) % 60) for k in range(66, 170)], 145), reach_fallback, piece=12,
                   dense=0, levels=2, l2=8, dofs=(True,)))
    # level-2 pieces that come near the column budget themselves (wave 0 of <4,3> takes columns after it has factorised)
    C.append(_case("level2_wide_4", _graph(190, [(k, 2 + (k * 7) % 60) for k in range(66, 190)], 147), reach_level2_wide, piece=8,
                   dense=0, levels=2, l2=8, dofs=(False,)))
    C.append(_case("level2_wide_6", _graph(170, [(k, 2 + (k * 7) % 45) for k in range(51, 170)], 149), reach_level2_wide, piece=12,
                   dense=0, levels=2, l2=8, dofs=(True,)))
    # a loop edge and a sequential edge on the same pair of keyframes: one destination block, as a separator-separator,
    # a band and a coupling block
    for six in (False, True):
        for kind, name in ((1, "sep"), (2, "band"), (3, "coupling")):
            C.append(_case("shared_%s_%d" % (name, 6 if six else 4), _search_shared(six, kind), reach_shared(kind), piece=8, dense=0,
                           levels=1, dofs=(six,)))
    # two sequences alternating in blocks of five (no sequential edge across a block boundary), every block tied to an
    # earlier one by a loop; the last keyframe opens a third sequence and has no edge at all
    n = 62
    seq = np.array([1 + (k // 5) % 2 for k in range(n)])
    seq[-1] = 3
    C.append(_case("breaks", _graph(n, [(k, k - 7) for k in range(10, n - 1, 5)] + [(k, k - 13) for k in range(23, n - 1, 10)], 151,
                                    sequence=seq), reach_breaks, piece=8, dense=0, levels=1))
    # 6-DoF: sequence 0 (constant) in the middle of the list
    seq = np.ones(70, int)
    seq[25:40] = 0
    C.append(_case("constant_middle_6", _graph(70, [(30, 2), (45, 28), (50, 33), (60, 10), (66, 37)], 153, sequence=seq),
                   reach_constant_middle, piece=8, dense=0, levels=1, dofs=(True,)))
    # Huber: |r|^2 just below and just above 0.01, far outside, exactly zero
    for six in (False, True):
        C.append(_case("huber_%d" % (6 if six else 4), _huber_graph(six), reach_huber, piece=8, dense=0, levels=1, dofs=(six,)))
    # yaws near +-180 degrees: loop residuals that wrap, and a step that carries candidates across
    wr = _graph(121, [(40, 20), (100, 5), (120, 0)], 157, offsets={120: ((0, 0, 0), 12.0)})
    k = int(np.argmin([180.0 - _r2ypr(q)[0] if _r2ypr(q)[0] > 0 else 999.0 for q in wr.q_svin]))
    gap = 180.0 - _r2ypr(wr.q_svin[k])[0] - 0.01      # turn that keyframe to 179.99 degrees: the step (+0.04) carries it across
    wr.q_svin[k] = spg.R2q(spg.ypr2R([gap, 0.0, 0.0]) @ spg.q2R(wr.q_svin[k]))
    C.append(_case("wrap_4", wr, reach_wrap, piece=8, dense=0, levels=1, dofs=(False,)))
    # the damping term dominant instead of small
    C.append(_case("radius_small", _graph(61, [(30, 0), (44, 9), (58, 21)], 103), reach_pieces, piece=8, dense=0, levels=1, radius=1e-2))
    return C


def _budget_pairs(six):
    """The closing rule `adj + 1 >= maxAdj` counts the preceding cut group twice (its 2w head start and the walk's stamp), so a
    piece whose separators arrive one per keyframe is closed at 60 (4-DoF) / 37 (6-DoF) of them.  To come within one keyframe of
    the 256 columns the closing keyframe X has to meet several new separators at once: X has no loop of its own, m later
    keyframes loop back to X, and each of those is made a cover (not X) by m later loops into it (degree m + 1 > m).  The loops
    after that complete the run of targets, so that the walk closes the first piece right behind the run."""
    w, sh, s0, X, m, run_end = (4, 60, 64, 93, 6, 59) if six else (2, 78, 80, 136, 4, 71)
    pairs = {s: s - sh for s in range(s0, X)}
    ks = [X + w + 2 + j for j in range(m)]
    for k in ks:
        pairs[k] = X
    nxt = ks[-1] + w + 1
    for k in ks:
        for _ in range(m):
            pairs[nxt] = k
            nxt += 1
    for tgt in range(X - sh, run_end + 1):
        pairs[nxt] = tgt
        nxt += 1
    return sorted(pairs.items())


def _search_shared(six, kind):
    w = 4 if six else 2
    for k in range(12, 50):
        spec = _graph(61, [(30, 0), (k, k - 1 - (k % w)), (58, 21)], 161)
        c = Case("probe", spec, piece=8, dense=0, levels=1)
        p = c.problem(six)
        if _shared_kinds(c.partition(p, six), p) == {kind}:
            return spec
    raise AssertionError("no position gives a shared block of kind %d" % kind)


def _huber_graph(six):
    """loops whose translation residual is set to a chosen vector (the rotation part is left at its small natural value)"""
    pairs = [(20, 0), (31, 8), (42, 15), (53, 27), (59, 36)]
    spec = _graph(61, pairs, 155)
    scale = 1.0 / 20.0 if six else 1.0          # sqrt_info of the 6-DoF translation rows
    want = {20: 0.1 * (1 - 5e-4), 31: 0.1 * (1 + 5e-4), 42: 3.0}
    for k, norm in want.items():
        old, rt, rq, ry = _exact_loop(spec, k, spec.loops[k][0])
        v = np.array([0.6, -0.48, 0.64]) * norm * scale
        spec.loops[k] = (old, rt - v, rq, ry)
    # exactly zero: keyframe 53 stands exactly where keyframe 27 stands and measures the identity
    spec.t_svin[53], spec.q_svin[53] = spec.t_svin[27], spec.q_svin[27]
    spec.loops[53] = (27, np.zeros(3), np.array([0.0, 0, 0, 1]), 0.0)
    return spec


def _search_short_last(six):
    for n in range(56, 90):
        spec = _graph(n, [(12, 0), (25, 4)], 105)
        c = Case("probe", spec, piece=8, dense=0, levels=1)
        p = c.problem(six)
        part = c.partition(p, six)
        if part["nPieces"] >= 2 and part["rows"][-1] == (6 if six else 4):
            return n
    raise AssertionError("no size leaves one keyframe in the last piece")
