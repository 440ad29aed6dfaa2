"""The case graphs of tests/test_gpu_posegraph_priors.py and tests/test_pg_prior_reference_host.py: pg_cases.py's and
pg_edge_cases.py's graphs with absolute keyframe measurements (svin_pg_add_prior) and a free gauge (svin_pg_set_gauge) placed where
the one-ended evaluation, the list construction and the symbolic step can go wrong.  A case's `priors` are
pg_prior_reference.prior dicts (information possibly a callable of six); keyframe index = list position.  The keyframes start at
their SVIn poses, so a measurement at spec.t_svin[k] - v has the unit residual v there."""
import copy
from dataclasses import dataclass, field

import numpy as np

from svin_amd import synthetic_pg as spg

import pg_cases as pc
import pg_edge_cases as ec
import pg_prior_reference as rr
import pg_reference as pr

NONE, CAUCHY, HUBER = rr.LOSS_NONE, rr.LOSS_CAUCHY, rr.LOSS_HUBER
POSE, POSITION, DEPTH = rr.POSE, rr.POSITION, rr.DEPTH


def spd(m, seed, cond, scale=1.0):
    rng = np.random.default_rng(seed)
    Q, _ = np.linalg.qr(rng.normal(size=(m, m)))
    A = (Q * (np.geomspace(1.0, cond, m) * scale)) @ Q.T
    return (A + A.T) / 2


def pose_info(seed=5, cond=50.0, scale=1.0):
    """a dense D x D information for a POSE prior of either DoF"""
    return lambda six: spd(6 if six else 4, seed, cond, scale)


def pose_diag(six):
    return np.diag([3.0, 5.0, 7.0, 90.0, 80.0, 70.0] if six else [2.0, 3.0, 0.5, 0.02])


def pose_eye(six):
    return np.eye(6 if six else 4)


@dataclass
class PriorCase(ec.EdgeCase):
    priors: list = field(default_factory=list)
    gauge: int = 0

    def problem(self, six):
        return rr.local_problem(self.spec, six, self.earliest, self.cur, self.callers, self.priors, self.gauge)


def _case(name, spec, priors, reach, callers=(), earliest=None, **kw):
    earliest = pc._earliest(spec) if earliest is None else earliest
    return PriorCase(name=name, spec=spec, reach=reach, earliest=earliest, callers=list(callers), priors=priors, **kw)


def near(spec, k, kind, v=(0.0, 0.0, 0.0), dyaw=0.0, dq_deg=(0.0, 0.0, 0.0), **kw):
    """a prior whose unit residual at the SVIn poses is [v, dyaw] (4-DoF) / [v, about 2 sin(dq / 2)] (6-DoF)"""
    Rm = spg.q2R(spec.q_svin[k]) @ spg.ypr2R(list(dq_deg))
    yaw = pc._r2ypr(spec.q_svin[k])[0] - dyaw
    return rr.prior(k, kind, spec.t_svin[k] - np.asarray(v, float), spg.R2q(Rm), yaw, **kw)


def _priors(problem):
    return np.where(np.asarray(problem["eloop"]) == 3)[0]


# ---- reach predicates
def reach_positions(part, problem, six, ref=None):
    p = set(_priors(problem).tolist())
    assert {126, 127, 128, 129, 130} <= p and len(problem["ea"]) > 130
    last = len(problem["off"]) - 1
    on_last = [e for e in p if problem["ea"][e] == last]
    assert len(on_last) >= 5 and set(problem["eprior"][on_last].tolist()) == {POSE, POSITION, DEPTH}
    assert part["nPieces"] == 0


def reach_losses(part, problem, six, ref=None):
    R = 6 if six else 4
    E = rr.edges(problem, problem, six)
    s = np.asarray(E["s"].v, float)
    kl = np.asarray(problem["eloss"]).reshape(-1, 2)
    S = np.asarray(problem["einfo"]).reshape(-1, R, R)
    pe = np.asarray(problem["eloop"]) == 3
    ident = np.array([np.array_equal(x[:3, :3], np.eye(3)) and problem["eprior"][e] == POSITION for e, x in enumerate(S)])
    b = 0.25
    for kind in (HUBER, CAUCHY, NONE):
        ss = s[pe & ident & (kl[:, 0] == kind) & (kl[:, 1] == (1.0 if kind == NONE else 0.5))]
        assert np.any(ss == b) and np.any((ss > 0.99 * b) & (ss < b)) and np.any((ss > b) & (ss < 1.01 * b)) and np.any(ss > 20 * b) \
            and np.any(ss == 0.0), (kind, ss)
    # the kinds of information: identity, diagonal, dense at condition 1e6
    Sp = S[pe]
    offd = np.array([np.any(np.triu(x, 1) != 0) for x in Sp])
    conds = [np.linalg.cond(x[np.ix_(np.diag(x) != 0, np.diag(x) != 0)]) for x in Sp]
    assert offd.any() and (~offd).any() and max(conds) > 500.0        # (cond(S) = sqrt(cond(information)))
    # a prior on the constant keyframe, on interior keyframes and on a cut keyframe; every kind
    off = np.asarray(problem["off"])
    nodes = problem["ea"][_priors(problem)]
    assert np.any(off[nodes] < 0) and np.any((off[nodes] >= 0) & (part["isSep"][nodes] == 0)) and np.any(part["isSep"][nodes] == 1)
    assert set(problem["eprior"][pe].tolist()) == {POSE, POSITION, DEPTH} and part["nPieces"] >= 2


def reach_roles(part, problem, six, ref=None):
    pc.reach_level2(part, problem, six)
    nodes = problem["ea"][_priors(problem)]
    sep, cover, root = part["isSep"][nodes], part["isCover"][nodes], part["isRoot"][nodes]
    assert np.any(sep == 0) and np.any((sep == 1) & (root == 0)) and np.any(cover == 1) and np.any((root == 1) & (cover == 0))


def reach_left_out(n_priors, n_in):
    def f(part, problem, six, ref=None):
        assert len(_priors(problem)) == n_in < n_priors
        assert np.any(np.asarray(problem["off"])[problem["ea"][_priors(problem)]] < 0)
    return f


def reach_mixed(kind, count):
    inner = ec.reach_shared(kind, count)

    def f(part, problem, six, ref=None):
        two = dict(problem)
        keep = np.asarray(problem["eloop"]) != 3      # (pg_edge_reference.shared_pairs does not know the one-ended entries)
        two["ea"], two["eb"] = problem["ea"][keep], problem["eb"][keep]
        inner(part, two, six)
        (lo, hi), _ = next(iter(rr.er.shared_pairs(two).items()))
        nodes = set(problem["ea"][_priors(problem)].tolist())
        assert {lo, hi} <= nodes and np.sum(problem["eloop"] == 2) >= 1
    return f


def reach_gauge(regime):
    def f(part, problem, six, ref=None):
        off = np.asarray(problem["off"])
        assert np.all(off >= 0) and len(_priors(problem)) >= 1
        if regime == "dense":
            assert part["nPieces"] == 0
        elif regime == "one_level":
            assert part["nPieces"] >= 2 and part["nPieces2"] == 0 and part["isSep"][0] == 0
        else:
            assert part["nPieces2"] >= 2
    return f


# ---- builders
def _positions_case(six):
    n = 31 if six else 60
    spec = pc._graph(n, [], 271)
    base = len(pc.local_problem(spec, six, 0, n - 1)["ea"])
    assert base <= 120
    kinds = [POSE, POSITION, DEPTH]
    infos = {POSE: [None, pose_info(7, 50.0), pose_diag], POSITION: [None, spd(3, 8, 30.0), np.diag([4.0, 2.0, 9.0])],
             DEPTH: [None, np.array([[25.0]]), np.array([[0.04]])]}
    priors = []
    for i in range(126 - base):     # on keyframes along the chain: the entries behind them move up
        k = 2 + (i * 5) % (n - 4)
        priors.append(near(spec, k, kinds[i % 3], v=(0.01 * (i % 7), -0.02, 0.015), dyaw=0.3, dq_deg=(0.2, -0.1, 0.1),
                           info=infos[kinds[i % 3]][(i // 3) % 3], loss=[NONE, HUBER, CAUCHY][i % 3], scale=0.3))
    for i in range(5):              # the last keyframe's: positions 126 .. 130 once the chain's have moved everything up
        kind = kinds[i % 3]
        priors.append(near(spec, n - 1, kind, v=(0.05, 0.02 * i, -0.03), dyaw=-0.4, dq_deg=(0.1, 0.3, -0.2), info=infos[kind][(i + 1) % 3],
                           loss=[CAUCHY, NONE, HUBER][i % 3], scale=0.2))
    return _case("positions_%d" % (6 if six else 4), spec, priors, reach_positions, earliest=0, dofs=(six,))


def _exact_half(spec, lo, hi):
    """a keyframe whose x coordinate gives back 0.5 exactly from x - (x - 0.5)"""
    for k in range(lo, hi):
        x = spec.t_svin[k][0]
        if x - (x - 0.5) == 0.5:
            return k
    raise AssertionError("no keyframe with an exact half")


def _loss_case():
    """identity information on POSITION priors: s = |u|^2 set to a chosen value; then the other kinds and informations"""
    spec = pc._graph(61, [(20, 0)], 273)
    a = 0.5
    priors = []
    for kind in (HUBER, CAUCHY, NONE):
        for i, norm in enumerate((a * (1 - 5e-4), a * (1 + 5e-4), 6.0 * a)):
            k = 3 + 5 * i + kind
            priors.append(near(spec, k, POSITION, v=np.array([0.6, -0.48, 0.64]) * norm, info=np.eye(3), loss=kind, scale=a))
        k = _exact_half(spec, 22 + 9 * kind, 60)
        priors.append(rr.prior(k, POSITION, spec.t_svin[k] - np.array([0.5, 0.0, 0.0]), info=np.eye(3),
                               loss=kind, scale=a))                                                           # s = a^2 exactly
        priors.append(near(spec, 40 + kind, POSITION, info=np.eye(3), loss=kind, scale=a))                    # s = 0 exactly
    extra = [(POSE, pose_info(9, 1.0), CAUCHY), (POSE, pose_info(9, 1e6), HUBER), (POSE, pose_diag, NONE), (POSE, pose_eye, CAUCHY),
             (POSITION, spd(3, 10, 1e6), CAUCHY), (POSITION, spd(3, 11, 1.0, 4.0), HUBER), (DEPTH, np.array([[400.0]]), HUBER),
             (DEPTH, None, NONE), (DEPTH, np.array([[1e-4]]), CAUCHY)]
    for i, (kind, info, lk) in enumerate(extra):
        priors.append(near(spec, 1 + 6 * i, kind, v=(0.03 * i, -0.05, 0.02 * (i + 1)), dyaw=0.5 - 0.2 * i, dq_deg=(0.3, -0.2, 0.1 * i),
                           info=info, loss=lk, scale=0.1 * (i + 1)))
    priors.append(near(spec, 0, POSE, v=(0.1, 0.2, -0.1), dyaw=1.0, dq_deg=(0.5, 0.0, 0.0), info=pose_info(12, 20.0), loss=HUBER, scale=0.05))
    priors.append(near(spec, 0, DEPTH, v=(0.0, 0.0, 0.3)))                                                   # the constant keyframe
    return _case("losses", spec, priors, reach_losses, piece=8, dense=0, levels=1)


def _roles_cases():
    out = []
    for six, n in ((False, 161), (True, 111)):
        lp = pc._ring(n, 23, 40)
        spec = pc._graph(n, [(40, 0)] + lp[1:], 231)
        bare = pc.local_problem(spec, six, 0, n - 1)
        part = pr.partition(bare, six, 8, 0, 2, 8)
        off = bare["off"]
        roles = [np.where((off >= 0) & (part["isSep"] == 0))[0], np.where((part["isSep"] == 1) & (part["isRoot"] == 0))[0],
                 np.where(part["isCover"] == 1)[0], np.where((part["isRoot"] == 1) & (part["isCover"] == 0))[0]]
        priors = []
        for i, nodes in enumerate(roles):
            for j, k in enumerate(nodes[[len(nodes) // 3, (2 * len(nodes)) // 3]]):
                kind = [POSE, POSITION, DEPTH][(i + j) % 3]
                info = {POSE: pose_info(20 + i, 100.0), POSITION: spd(3, 30 + i, 10.0, 2.0), DEPTH: np.array([[9.0]])}[kind]
                priors.append(near(spec, int(k), kind, v=(0.04, -0.03 * (j + 1), 0.05), dyaw=0.6, dq_deg=(0.2, 0.2, -0.3), info=info,
                                   loss=[NONE, CAUCHY, HUBER][(i + j) % 3], scale=0.4))
        out.append(_case("roles_%d" % (6 if six else 4), spec, priors, reach_roles, piece=8, dense=0, levels=2, l2=8, dofs=(six,)))
    return out


def _left_out_case():
    spec = pc._graph(61, [(30, 6), (58, 21)], 281)
    priors = [near(spec, 2, POSE, v=(0.1, 0.1, 0.1), info=pose_info(40, 10.0)), near(spec, 6, POSITION, v=(0.2, 0.0, -0.1)),
              near(spec, 40, DEPTH, v=(0.0, 0.0, 0.25), info=np.array([[16.0]]), loss=CAUCHY, scale=0.5), near(spec, 5, DEPTH)]
    return _case("left_out", spec, priors, reach_left_out(4, 2), piece=8, dense=0, levels=1)


def _mixed_cases():
    out = []
    shared = {c.name: c for c in ec.build_cases()}
    for name, kind, count in (("shared3_band_4", 2, 3), ("shared4_sep_6", 1, 4), ("shared3_coupling_6", 3, 3)):
        base = shared[name]
        six = base.dofs[0]
        spec = copy.deepcopy(base.spec)
        a, b = base.callers[0]["a"], base.callers[0]["b"]
        priors = [near(spec, a, POSE, v=(0.02, 0.03, -0.04), dyaw=0.2, dq_deg=(0.1, -0.2, 0.3), info=pose_info(50, 1e3), loss=CAUCHY, scale=0.6),
                  near(spec, b, POSITION, v=(-0.05, 0.01, 0.02), info=spd(3, 51, 5.0)),
                  near(spec, b, DEPTH, v=(0.0, 0.0, -0.2), info=np.array([[2.0]]), loss=HUBER, scale=0.1),
                  near(spec, max(a, b) + 3, POSE, v=(0.01, 0.01, 0.01), info=pose_diag)]
        out.append(_case("mixed_" + name, spec, priors, reach_mixed(kind, count), callers=base.callers, earliest=base.earliest, piece=8, dense=0,
                         levels=1, dofs=(six,)))
    return out


def _gauge_cases():
    out = []
    dense = pc._graph(41, [(20, 0), (33, 6)], 283)
    one = pc._graph(70, [(30, 2), (45, 28), (60, 10)], 285)
    for regime, spec_of, cfg in (("dense", lambda six: dense, dict()), ("one_level", lambda six: one, dict(piece=8, dense=0, levels=1)),
                                 ("two_level", None, dict(piece=8, dense=0, levels=2, l2=8))):
        for six in (False, True):
            if spec_of is None:
                n = 111 if six else 161
                spec = pc._graph(n, [(40, 0)] + pc._ring(n, 23, 40)[1:], 231)
            else:
                spec = spec_of(six)
            n = spec.n
            priors = [near(spec, n // 3, POSE, v=(0.1, -0.05, 0.02), dyaw=0.4, dq_deg=(0.2, 0.1, -0.1), info=pose_info(60, 30.0)),
                      near(spec, 0, POSITION, v=(0.03, 0.02, 0.01), info=spd(3, 61, 4.0)),
                      near(spec, n - 1, POSITION, v=(-0.02, 0.04, 0.0), loss=CAUCHY, scale=0.5),
                      near(spec, n // 2, DEPTH, v=(0.0, 0.0, 0.1), info=np.array([[4.0]]))]
            out.append(_case("gauge_%s_%d" % (regime, 6 if six else 4), spec, priors, reach_gauge(regime), earliest=0, gauge=1, dofs=(six,),
                             **cfg))
    return out


def build_cases():
    return [_positions_case(False), _positions_case(True), _loss_case()] + _roles_cases() + [_left_out_case()] + _mixed_cases() + _gauge_cases()


# ---- whole runs
def depth_chain(n=40, slope=0.02, sigma=0.01):
    """a chain without loops whose SVIn poses are the generating ones plus a z drift of `slope` metres per keyframe, and a DEPTH
    prior per keyframe at the generating depth with information 1 / sigma^2 (a pressure sensor good to a centimetre).  The edges hold
    the drifted increments, stiffness K (4-DoF two unit-weight edges, 6-DoF four of weight 20^2 reaching up to four keyframes: K about
    12 000); a linear error profile strains no edge in the interior, so what is left of it after the solve sits at the ends and is of
    the order slope sqrt(K / information) <= 0.03 m, against an rms of 0.45 m before: well beyond tenfold in either DoF."""
    spec = spg.make_pose_graph(n=n, laps=1, loop_every=10 ** 6, seed=41, drift_yaw_deg=0.0, drift_t=0.0)
    spec.t_svin = spec.t_svin.copy()
    spec.t_svin[:, 2] += slope * np.arange(n)
    priors = [rr.prior(k, DEPTH, [0.0, 0.0, spec.t_true[k][2]], info=np.array([[1.0 / sigma ** 2]])) for k in range(n)]
    return spec, priors


def rigid_case(six, n=30):
    """the generating trajectory, noise-free, seen in another frame (4-DoF: turned about the vertical and shifted, pitch and roll not
    being variables there; 6-DoF: any rotation), and POSITION priors at the generating positions of two (4-DoF) / three non-collinear
    (6-DoF) keyframes: with a free gauge the generating poses have zero cost and nothing else has"""
    spec = spg.make_pose_graph(n=n, laps=1, loop_every=10 ** 6, seed=43, drift_yaw_deg=0.0, drift_t=0.0)
    Rg, sh = spg.ypr2R([8.0, 3.0, -2.0] if six else [8.0, 0.0, 0.0]), np.array([1.5, -1.0, 0.3])
    spec.t_svin = (Rg @ spec.t_true.T).T + sh
    spec.q_svin = np.stack([spg.R2q(Rg @ R) for R in spec.R_true])
    where = [2, n // 3 + 1, (2 * n) // 3] if six else [2, (2 * n) // 3]
    priors = [rr.prior(k, POSITION, spec.t_true[k]) for k in where]
    return spec, priors
