"""The case graphs of tests/test_gpu_posegraph_edges.py and tests/test_pg_edge_reference_host.py: pg_cases.py's graphs with
caller-given edges (svin_pg_add_edge) placed where the generalised evaluation, the shared-destination assembly and the symbolic
step can go wrong.  A case's `callers` are pg_edge_reference.caller_edge dicts; keyframe index = list position."""
import copy
from dataclasses import dataclass, field

import numpy as np

import pg_cases as pc
import pg_edge_reference as er

NONE, CAUCHY, HUBER = er.LOSS_NONE, er.LOSS_CAUCHY, er.LOSS_HUBER


def dense_info(six, seed=5, cond=50.0):
    """a dense symmetric positive definite information of the size of the 6-DoF / 4-DoF weights"""
    D = 6 if six else 4
    rng = np.random.default_rng(seed)
    Q, _ = np.linalg.qr(rng.normal(size=(D, D)))
    w = np.geomspace(1.0, cond, D) * (100.0 if six else 1.0)
    A = (Q * w) @ Q.T
    return (A + A.T) / 2


def diag_info(six):
    return np.diag([300.0, 500, 700, 9000, 8000, 7000] if six else [2.0, 3.0, 0.5, 0.02])


def eye_info(six):
    return np.eye(6 if six else 4)


def loop_weights_squared(six):
    return np.diag(np.array([20.0, 20, 20, 100, 100, 100] if six else [1.0, 1, 1, 0.1]) ** 2)


@dataclass
class EdgeCase(pc.Case):
    callers: list = field(default_factory=list)

    def problem(self, six):
        return er.local_problem(self.spec, six, self.earliest, self.cur, self.callers)


def _case(name, spec, callers, reach, earliest=None, **kw):
    earliest = pc._earliest(spec) if earliest is None else earliest
    if hasattr(reach, "earliest"):
        reach.earliest = earliest
    return EdgeCase(name=name, spec=spec, reach=reach, earliest=earliest, callers=callers, **kw)


def _callers(problem):
    return np.where(np.asarray(problem["eloop"]) == 2)[0]


def _kind_of(part, problem, a, b):
    sa, sb = part["isSep"][a], part["isSep"][b]
    return 1 if sa and sb else (2 if not sa and not sb else 3)


# ---- reach predicates
def reach_positions(part, problem, six, ref=None):
    c = set(_callers(problem).tolist())
    assert {127, 128, 129} <= c and 126 not in c and 125 not in c, sorted(c)
    assert len(problem["ea"]) > 129


def reach_losses(part, problem, six, ref=None):
    E = er.edges(problem, problem, six)
    s = np.asarray(E["s"].v, float)
    kl = np.asarray(problem["eloss"]).reshape(-1, 2)
    for kind in (HUBER, CAUCHY, NONE):
        sel = (np.asarray(problem["eloop"]) == 2) & (kl[:, 0] == kind) & (kl[:, 1] == (1.0 if kind == NONE else 0.5))
        ss, b = s[sel], 0.25
        assert np.any((ss > 0.99 * b) & (ss < b)) and np.any((ss > b) & (ss < 1.01 * b)) and np.any(ss > 20 * b) and np.any(ss == 0.0), (kind, ss)
    # the kinds of information: dense, diagonal (not identity), identity, default
    S = np.asarray(problem["einfo"]).reshape(len(s), -1)
    R = 6 if six else 4
    S = S.reshape(-1, R, R)[_callers(problem)]
    offd = np.array([np.any(np.triu(x, 1) != 0) for x in S])
    ident = np.array([np.array_equal(x, np.eye(R)) for x in S])
    dflt = np.array([np.array_equal(x, er.default_factor(six)) for x in S])
    assert offd.any() and ident.any() and dflt.any() and (~offd & ~ident & ~dflt).any()


def reach_shared(kind, count):
    def f(part, problem, six, ref=None):
        got = {(_kind_of(part, problem, a, b), len(es)) for (a, b), es in er.shared_pairs(problem).items()}
        assert (kind, count) in got, got
        es = next(es for (a, b), es in er.shared_pairs(problem).items() if len(es) == count)
        assert len({(int(problem["ea"][e]) < int(problem["eb"][e])) for e in es}) == 2, "one orientation only"
    return f


def reach_cover(hub, others):
    def f(part, problem, six, ref=None):
        lo = hub - f.earliest
        assert part["nPieces"] >= 2 and part["isCover"][lo] == 1
        assert all(part["isCover"][o - f.earliest] == 0 for o in others)
        c = _callers(problem)
        assert np.sum((problem["ea"][c] == lo) | (problem["eb"][c] == lo)) == 5
        assert np.any(problem["ea"][c] > problem["eb"][c]) and np.any(problem["ea"][c] < problem["eb"][c])
    f.earliest = 0
    return f


def reach_constants(both):
    def f(part, problem, six, ref=None):
        off, c = problem["off"], _callers(problem)
        ca, cb = off[problem["ea"][c]] < 0, off[problem["eb"][c]] < 0
        assert np.any(ca != cb)
        if both:
            assert np.any(ca & cb)
    return f


def reach_two_sequences(seq):
    def f(part, problem, six, ref=None):
        c = _callers(problem)
        assert len(c) and all(seq[problem["ea"][e] + f.earliest] != seq[problem["eb"][e] + f.earliest] for e in c)
        assert part["nPieces"] >= 2
    f.earliest = 0
    return f


def reach_left_out(n_callers, n_in):
    def f(part, problem, six, ref=None):
        assert len(_callers(problem)) == n_in < n_callers
    return f


def reach_level2(part, problem, six, ref=None):
    pc.reach_level2(part, problem, six)
    c = _callers(problem)
    w = 4 if six else 2
    assert np.sum(np.abs(problem["ea"][c] - problem["eb"][c]) > w + 2) >= 3
    assert any(part["isRoot"][problem["ea"][e]] or part["isRoot"][problem["eb"][e]] for e in c)


# ---- builders
def _positions_case(six):
    n = 33 if six else 64
    spec = pc._graph(n, [], 171)
    base = len(pc.local_problem(spec, six, 0, n - 1)["ea"])
    assert base <= 127
    far = [3, 9, 15, 21, 27, 1, 5]
    callers = [er.caller_edge(spec, far[i], n - 2, info=[None, dense_info, diag_info][i % 3], loss=[NONE, HUBER, CAUCHY][i % 3],
                              scale=0.3, seed=200 + i) for i in range(127 - base)]
    callers += [er.caller_edge(spec, n - 1, 7, info=dense_info, loss=CAUCHY, scale=0.2, seed=210),       # a later than b
                er.caller_edge(spec, 11, n - 1, info=None, loss=HUBER, scale=0.1, seed=211),
                er.caller_edge(spec, 13, n - 1, info=eye_info, loss=NONE, seed=212),
                er.caller_edge(spec, n - 1, 17, info=diag_info, loss=HUBER, scale=2.0, seed=213)]
    return _case("positions_%d" % (6 if six else 4), spec, callers, reach_positions, earliest=0, dofs=(six,))


def _exact(spec, a, b):
    old, rt, rq, ry = pc._exact_loop(spec, b, a)
    return rt, rq, ry


def _loss_case():
    """identity information: s = |u|^2; the translation residual of each edge set to a chosen vector as pg_cases._huber_graph
    does; a pair of keyframes standing in one place for s = 0 exactly; then the other kinds of information on natural noise"""
    spec = pc._graph(61, [(20, 0)], 173)
    spec.t_svin[53], spec.q_svin[53] = spec.t_svin[27], spec.q_svin[27]
    callers = []
    a = 0.5
    for kind in (HUBER, CAUCHY, NONE):
        for i, norm in enumerate((a * (1 - 5e-4), a * (1 + 5e-4), 6.0 * a)):
            ka, kb = 5 + 3 * i, 31 + 4 * i + kind
            rt, rq, ry = _exact(spec, ka, kb)
            callers.append(dict(a=ka, b=kb, t=rt - np.array([0.6, -0.48, 0.64]) * norm, q=rq, yaw=ry, info=eye_info, loss=kind, scale=a))
        callers.append(dict(a=27, b=53, t=np.zeros(3), q=np.array([0.0, 0, 0, 1]), yaw=0.0, info=eye_info, loss=kind, scale=a))
    for i, (info, kind) in enumerate(((dense_info, CAUCHY), (dense_info, HUBER), (diag_info, NONE), (None, HUBER), (None, NONE),
                                      (diag_info, CAUCHY))):
        callers.append(er.caller_edge(spec, 2 + 5 * i, 40 + 3 * i, info=info, loss=kind, scale=0.1 * (i + 1), seed=220 + i))
    return _case("losses", spec, callers, reach_losses, piece=8, dense=0, levels=1)


def _shared_cases():
    out = []
    for six in (False, True):
        w = 4 if six else 2
        for kind, name in ((1, "sep"), (2, "band"), (3, "coupling")):
            base = pc._search_shared(six, kind)
            k = next(k for k, v in base.loops.items() if 0 < k - v[0] <= w)
            old = base.loops[k][0]
            for count in (3, 4):
                spec = copy.deepcopy(base)
                callers = [er.caller_edge(spec, k, old, info=dense_info, loss=CAUCHY, scale=0.5, seed=230)]     # reversed
                if count == 4:
                    callers.append(er.caller_edge(spec, old, k, info=diag_info, loss=NONE, seed=231))
                out.append(_case("shared%d_%s_%d" % (count, name, 6 if six else 4), spec, callers, reach_shared(kind, count),
                                 piece=8, dense=0, levels=1, dofs=(six,)))
    return out


def _cover_case():
    spec = pc._graph(71, [(30, 0)], 175)
    others = [4, 12, 19, 47, 56]
    callers = [er.caller_edge(spec, 33, o, info=dense_info if i % 2 else None, loss=HUBER, scale=0.2, seed=240 + i) if i % 2 else
               er.caller_edge(spec, o, 33, info=diag_info, loss=CAUCHY, scale=0.3, seed=240 + i) for i, o in enumerate(others)]
    return _case("cover5", spec, callers, reach_cover(33, others), piece=8, dense=0, levels=1)


def _two_sequences_case():
    n = 62
    seq = np.array([1 + (k // 5) % 2 for k in range(n)])
    spec = pc._graph(n, [(k, k - 7) for k in range(10, n - 1, 10)], 177, sequence=seq)
    callers = [er.caller_edge(spec, 3, 8, info=dense_info, seed=250), er.caller_edge(spec, 26, 12, info=None, loss=HUBER, scale=0.1, seed=251),
               er.caller_edge(spec, 44, 49, info=diag_info, loss=CAUCHY, scale=1.0, seed=252), er.caller_edge(spec, 61, 56, seed=253)]
    return _case("two_sequences", spec, callers, reach_two_sequences(seq), piece=8, dense=0, levels=1)


def _constants_cases():
    seq = np.ones(70, int)
    seq[25:40] = 0
    spec = pc._graph(70, [(30, 2), (45, 28), (50, 33), (60, 10), (66, 37)], 153, sequence=seq)
    callers = [er.caller_edge(spec, 30, 55, info=dense_info, loss=CAUCHY, scale=0.5, seed=260),      # a constant
               er.caller_edge(spec, 12, 36, info=None, loss=HUBER, scale=0.1, seed=261),             # b constant
               er.caller_edge(spec, 28, 33, info=diag_info, seed=262),                               # both constant: cost only
               er.caller_edge(spec, 2, 64, info=eye_info, seed=263)]                                 # a = earliest: constant
    six6 = _case("constants_6", spec, callers, reach_constants(True), piece=8, dense=0, levels=1, dofs=(True,))
    spec4 = pc._graph(61, [(30, 4), (58, 21)], 179)
    c4 = [er.caller_edge(spec4, 4, 40, info=dense_info, loss=HUBER, scale=0.3, seed=264),
          er.caller_edge(spec4, 50, 4, info=None, loss=CAUCHY, scale=0.3, seed=265)]
    return [six6, _case("constants_4", spec4, c4, reach_constants(False), piece=8, dense=0, levels=1, dofs=(False,))]


def _left_out_case():
    spec = pc._graph(61, [(30, 6), (58, 21)], 181)
    callers = [er.caller_edge(spec, 2, 40, info=dense_info, seed=270), er.caller_edge(spec, 45, 5, seed=271),
               er.caller_edge(spec, 8, 50, info=diag_info, loss=CAUCHY, scale=0.4, seed=272)]
    return _case("left_out", spec, callers, reach_left_out(3, 1), piece=8, dense=0, levels=1)


def _level2_cases():
    out = []
    for six, n in ((False, 161), (True, 111)):
        lp = pc._ring(n, 23, 40)
        spec = pc._graph(n, [(40, 0)] + lp[1:], 131)
        callers = [er.caller_edge(spec, 10, 90, info=dense_info, loss=CAUCHY, scale=0.5, seed=280),
                   er.caller_edge(spec, 100, 35, info=None, loss=HUBER, scale=0.1, seed=281),
                   er.caller_edge(spec, 60, n - 3, info=diag_info, seed=282),
                   er.caller_edge(spec, 61, 62, info=dense_info, seed=283)]          # a short one next to them
        out.append(_case("level2_%d" % (6 if six else 4), spec, callers, reach_level2, piece=8, dense=0, levels=2, l2=8, dofs=(six,)))
    return out


def build_cases():
    C = [_positions_case(False), _positions_case(True), _loss_case()]
    C += _shared_cases()
    C += [_cover_case(), _two_sequences_case()] + _constants_cases() + [_left_out_case()] + _level2_cases()
    return C


def shared_cases(cases):
    return [c for c in cases if c.name.startswith("shared")]
