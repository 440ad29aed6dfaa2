"""Host-side mirror of pose_graph's optimisation entry points over the C ABI in include/svin_pg.h.

``PoseGraph`` plays the role of the keyframe list + optimisation thread of
/root/reference/pose_graph/src/pose_graph/PoseGraph.cpp (addKeyframe :70-224, optimize4DoFPoseGraph :226-385,
optimize6DoFPoseGraph :387-543); the numerics run on the GPU inside libsvin_ba.so -- there is no CPU path.
"""
import ctypes as C

import numpy as np

from . import estimator

PG_EXPORTS = [
    "svin_pg_create", "svin_pg_destroy", "svin_pg_last_error", "svin_pg_add_keyframe", "svin_pg_num_keyframes",
    "svin_pg_optimize", "svin_pg_get_pose", "svin_pg_get_poses", "svin_pg_get_drift", "svin_pg_summary",
    "svin_pg_set_partition", "svin_pg_get_partition", "svin_pg_set_levels", "svin_pg_debug_step", "svin_pg_debug_array",
    "svin_pg_get_covariance_blocks", "svin_pg_get_covariance", "svin_pg_covariance_counters",
    "svin_pg_add_edge", "svin_pg_remove_edge", "svin_pg_num_edges", "svin_pg_get_edge",
    "svin_pg_add_prior", "svin_pg_remove_prior", "svin_pg_num_priors", "svin_pg_get_prior", "svin_pg_set_gauge", "svin_pg_get_gauge",
]
PRIOR_POSE, PRIOR_POSITION, PRIOR_DEPTH = 0, 1, 2   # svin_pg.h SVIN_PG_PRIOR_*
GAUGE_REFERENCE, GAUGE_FREE = 0, 1
LOSS_NONE, LOSS_CAUCHY, LOSS_HUBER = 0, 1, 2   # svin_ba.h SVIN_LOSS_*
ERR_SINGULAR = -5   # SVIN_PG_ERR_SINGULAR


class SingularError(RuntimeError):
    """J^T J of the covariance pass is not positive definite (SVIN_PG_ERR_SINGULAR); mirrors estimator.SingularError"""
DEBUG_ARRAYS = [
    "ea", "eb", "eloop", "off", "et", "eyaw", "epitch", "eroll", "eq", "esq", "yaw", "pitch", "roll", "t", "q",
    "res", "Ja", "Jb", "g", "scale", "colsq", "nodeBlk", "y", "yS", "cost", "costC", "gradmax", "model", "step2", "x2",
    "cholFail", "yawC", "tC", "qC", "rows", "cols", "rows2", "cols2", "sepOff", "nodePiece", "nodeRow", "isCover",
    "isRoot", "l2PieceOf", "nS", "nR", "nPieces", "nPieces2", "BW", "BW2", "ekind", "einfo", "eloss", "eid", "eprior",
]
_DEBUG_INTS = {"ea", "eb", "eloop", "ekind", "eid", "eprior", "off", "cholFail", "rows", "cols", "rows2", "cols2", "sepOff", "nodePiece", "nodeRow",
               "isCover", "isRoot", "l2PieceOf", "nS", "nR", "nPieces", "nPieces2", "BW", "BW2"}
_DEBUG_SCALARS = {"cost", "costC", "gradmax", "model", "step2", "x2", "cholFail", "nS", "nR", "nPieces", "nPieces2", "BW", "BW2"}

_BOUND = False


def _lib():
    global _BOUND
    L = estimator.load_library()
    if not _BOUND:
        vp, i32, f64, pd = C.c_void_p, C.c_int, C.c_double, C.POINTER(C.c_double)

        def sig(name, res, *args):
            f = getattr(L, name)
            f.restype = res
            f.argtypes = list(args)
        sig("svin_pg_create", vp, i32, i32, i32)
        sig("svin_pg_destroy", None, vp)
        sig("svin_pg_last_error", C.c_char_p)
        sig("svin_pg_add_keyframe", i32, vp, i32, i32, pd, pd, i32, pd, pd, f64)
        sig("svin_pg_num_keyframes", i32, vp)
        sig("svin_pg_optimize", i32, vp, i32, i32)
        sig("svin_pg_get_pose", i32, vp, i32, pd, pd)
        sig("svin_pg_get_poses", i32, vp, i32, pd, pd)
        sig("svin_pg_get_drift", i32, vp, pd, pd, pd)
        sig("svin_pg_summary", i32, vp, pd)
        sig("svin_pg_set_partition", i32, vp, i32, i32)
        sig("svin_pg_get_partition", i32, vp, pd)
        sig("svin_pg_set_levels", i32, vp, i32, i32)
        sig("svin_pg_debug_step", i32, vp, i32, i32, f64)
        sig("svin_pg_debug_array", C.c_longlong, vp, C.c_char_p, pd, C.c_longlong)
        pi = C.POINTER(C.c_int)
        sig("svin_pg_get_covariance_blocks", C.c_longlong, vp, i32, i32, i32, pi, pi, pd, C.c_longlong)
        sig("svin_pg_get_covariance", i32, vp, i32, i32, i32, i32, pd, i32)
        sig("svin_pg_covariance_counters", i32, vp, C.POINTER(C.c_longlong))
        sig("svin_pg_add_edge", i32, vp, i32, i32, pd, pd, f64, pd, i32, f64)
        sig("svin_pg_remove_edge", i32, vp, i32)
        sig("svin_pg_num_edges", i32, vp)
        sig("svin_pg_get_edge", i32, vp, i32, pi, pi, pd, pd, pd, pd, pi, pd)
        sig("svin_pg_add_prior", i32, vp, i32, i32, pd, pd, f64, pd, i32, f64)
        sig("svin_pg_remove_prior", i32, vp, i32)
        sig("svin_pg_num_priors", i32, vp)
        sig("svin_pg_get_prior", i32, vp, i32, pi, pi, pd, pd, pd, pd, pi, pd)
        sig("svin_pg_set_gauge", i32, vp, i32)
        sig("svin_pg_get_gauge", i32, vp)
        _BOUND = True
    return L


def _p(a):
    return a.ctypes.data_as(C.POINTER(C.c_double))


class PoseGraph:
    def __init__(self, device=0, six_dof=False, max_iterations=0):
        self.L = _lib()
        self.six = bool(six_dof)
        self.h = self.L.svin_pg_create(device, 1 if six_dof else 0, max_iterations)
        if not self.h:
            raise RuntimeError("svin_pg_create failed: " + self.L.svin_pg_last_error().decode())

    def close(self):
        if getattr(self, "h", None):
            self.L.svin_pg_destroy(self.h)
            self.h = None

    __del__ = close

    def _check(self, rc, what):
        if rc < 0:
            raise RuntimeError("%s failed (%d): %s" % (what, rc, self.L.svin_pg_last_error().decode()))
        return rc

    def add_keyframe(self, index, sequence, t, q, loop=None):
        """loop = (loop_index, rel_t[3], rel_q[4] xyzw, rel_yaw_deg) or None"""
        t = np.ascontiguousarray(t, np.float64)
        q = np.ascontiguousarray(q, np.float64)
        if loop is None:
            self._check(self.L.svin_pg_add_keyframe(self.h, index, sequence, _p(t), _p(q), -1, None, None, 0.0), "add_keyframe")
        else:
            li, rt, rq, ry = loop
            rt = np.ascontiguousarray(rt, np.float64)
            rq = np.ascontiguousarray(rq, np.float64)
            self._check(self.L.svin_pg_add_keyframe(self.h, index, sequence, _p(t), _p(q), int(li), _p(rt), _p(rq), float(ry)),
                        "add_keyframe")

    def add_edge(self, index_a, index_b, rel_t, rel_q=None, rel_yaw_deg=0.0, information=None, loss=LOSS_NONE, loss_scale=1.0):
        """a caller-given edge: the pose of keyframe b in the frame of keyframe a (rel_t, rel_q xyzw in 6-DoF, rel_yaw_deg in
        4-DoF), information D x D or None for the loop-edge weights, loss one of LOSS_NONE / LOSS_CAUCHY / LOSS_HUBER on
        |S u|^2; returns the edge id"""
        rt = np.ascontiguousarray(rel_t, np.float64)
        rq = None if rel_q is None else np.ascontiguousarray(rel_q, np.float64)
        info = None if information is None else np.ascontiguousarray(information, np.float64)
        return self._check(self.L.svin_pg_add_edge(self.h, int(index_a), int(index_b), _p(rt), None if rq is None else _p(rq),
                                                   float(rel_yaw_deg), None if info is None else _p(info), int(loss),
                                                   float(loss_scale)), "add_edge")

    def remove_edge(self, edge_id):
        self._check(self.L.svin_pg_remove_edge(self.h, int(edge_id)), "remove_edge")

    def num_edges(self):
        return self.L.svin_pg_num_edges(self.h)

    def get_edge(self, edge_id):
        D = 6 if self.six else 4
        ia, ib, lk = C.c_int(0), C.c_int(0), C.c_int(0)
        t, q, yaw, info, ls = np.zeros(3), np.zeros(4), np.zeros(1), np.zeros((D, D)), np.zeros(1)
        self._check(self.L.svin_pg_get_edge(self.h, int(edge_id), C.byref(ia), C.byref(ib), _p(t), _p(q), _p(yaw), _p(info),
                                            C.byref(lk), _p(ls)), "get_edge")
        return dict(index_a=ia.value, index_b=ib.value, rel_t=t, rel_q=q, rel_yaw_deg=float(yaw[0]), information=info,
                    loss=lk.value, loss_scale=float(ls[0]))

    def prior_rows(self, kind):
        return {PRIOR_POSE: 6 if self.six else 4, PRIOR_POSITION: 3, PRIOR_DEPTH: 1}[int(kind)]

    def add_prior(self, index, kind, t, q=None, yaw_deg=0.0, information=None, loss=LOSS_NONE, loss_scale=1.0):
        """an absolute measurement of keyframe `index` in the frame poses() answers in: kind PRIOR_POSE (t, and q xyzw in 6-DoF
        or yaw_deg in 4-DoF), PRIOR_POSITION (t) or PRIOR_DEPTH (t[2]); information m x m (m = prior_rows(kind)) or None for the
        identity; loss as for add_edge; returns the prior id"""
        t = np.ascontiguousarray(t, np.float64)
        q = None if q is None else np.ascontiguousarray(q, np.float64)
        info = None if information is None else np.ascontiguousarray(information, np.float64)
        return self._check(self.L.svin_pg_add_prior(self.h, int(index), int(kind), _p(t), None if q is None else _p(q), float(yaw_deg),
                                                    None if info is None else _p(info), int(loss), float(loss_scale)), "add_prior")

    def remove_prior(self, prior_id):
        self._check(self.L.svin_pg_remove_prior(self.h, int(prior_id)), "remove_prior")

    def num_priors(self):
        return self.L.svin_pg_num_priors(self.h)

    def get_prior(self, prior_id):
        idx, kind, lk = C.c_int(0), C.c_int(0), C.c_int(0)
        t, q, yaw, info, ls = np.zeros(3), np.zeros(4), np.zeros(1), np.zeros(36), np.zeros(1)
        self._check(self.L.svin_pg_get_prior(self.h, int(prior_id), C.byref(idx), C.byref(kind), _p(t), _p(q), _p(yaw), _p(info),
                                             C.byref(lk), _p(ls)), "get_prior")
        m = self.prior_rows(kind.value)
        return dict(index=idx.value, kind=kind.value, t=t, q=q, yaw_deg=float(yaw[0]), information=info[:m * m].reshape(m, m).copy(),
                    loss=lk.value, loss_scale=float(ls[0]))

    def set_gauge(self, gauge):
        """GAUGE_REFERENCE: the reference's constant keyframes (default); GAUGE_FREE: none, the priors tie the graph"""
        self._check(self.L.svin_pg_set_gauge(self.h, int(gauge)), "set_gauge")

    def gauge(self):
        return self.L.svin_pg_get_gauge(self.h)

    def optimize(self, earliest_loop_index, cur_index):
        self._check(self.L.svin_pg_optimize(self.h, earliest_loop_index, cur_index), "optimize")
        return self.summary()

    def summary(self):
        s = np.zeros(6)
        self._check(self.L.svin_pg_summary(self.h, _p(s)), "summary")
        return dict(initial_cost=s[0], final_cost=s[1], iterations=int(s[2]), termination=int(s[3]), successful=int(s[4]),
                    solve_seconds=s[5])

    def poses(self):
        n = self.L.svin_pg_num_keyframes(self.h)
        T, Q = np.zeros((n, 3)), np.zeros((n, 4))
        self._check(self.L.svin_pg_get_poses(self.h, n, _p(T), _p(Q)), "get_poses")
        return T, Q

    def drift(self):
        y, r, t = np.zeros(1), np.zeros((3, 3)), np.zeros(3)
        self._check(self.L.svin_pg_get_drift(self.h, _p(y), _p(r), _p(t)), "get_drift")
        return float(y[0]), r, t

    def set_partition(self, piece_keyframes=0, dense_keyframes=128):
        self._check(self.L.svin_pg_set_partition(self.h, piece_keyframes, dense_keyframes), "set_partition")

    def partition(self):
        s = np.zeros(10)
        self._check(self.L.svin_pg_get_partition(self.h, _p(s)), "get_partition")
        return dict(free=int(s[0]), separators=int(s[1]), pieces=int(s[2]), max_rows=int(s[3]), tiles=int(s[4]),
                    symbolic_seconds=float(s[5]), separator_unknowns=int(s[6]), dense_solves=int(s[7]),
                    dense_solve_seconds=float(s[8]), level2_pieces=int(s[9]))

    def set_levels(self, levels=2, level2_piece_keyframes=0):
        self._check(self.L.svin_pg_set_levels(self.h, levels, level2_piece_keyframes), "set_levels")

    def debug_step(self, earliest_loop_index, cur_index, radius=1e4):
        """one LM step at `radius`, kept stage by stage (svin_pg_debug_step): dict of the arrays named in include/svin_pg.h,
        or None when there is nothing to optimise; poses and drift stay untouched"""
        if self._check(self.L.svin_pg_debug_step(self.h, earliest_loop_index, cur_index, float(radius)), "debug_step") == 0:
            return None
        out = {}
        for name in DEBUG_ARRAYS:
            n = self._check(self.L.svin_pg_debug_array(self.h, name.encode(), None, 0), "debug_array " + name)
            a = np.zeros(max(int(n), 1))
            self._check(self.L.svin_pg_debug_array(self.h, name.encode(), _p(a), int(n)), "debug_array " + name)
            a = a[:int(n)]
            if name in _DEBUG_INTS:
                a = a.astype(np.int64)
            out[name] = a[0].item() if name in _DEBUG_SCALARS else a
        return out

    def covariance_blocks(self, earliest_loop_index, cur_index, pairs):
        """Sigma[a, b] for every (a, b) of `pairs` (keyframe indices): n_pairs x D x D, tangent coordinates and units as
        include/svin_pg.h states them; raises SingularError when J^T J is not positive definite"""
        pairs = np.ascontiguousarray(pairs, np.int32).reshape(-1, 2)
        ia, ib = np.ascontiguousarray(pairs[:, 0]), np.ascontiguousarray(pairs[:, 1])
        D = 6 if self.six else 4
        out = np.zeros((len(pairs), D, D))
        pi = C.POINTER(C.c_int)
        rc = self.L.svin_pg_get_covariance_blocks(self.h, earliest_loop_index, cur_index, len(pairs), ia.ctypes.data_as(pi),
                                                  ib.ctypes.data_as(pi), _p(out), out.size)
        if rc == ERR_SINGULAR:
            raise SingularError(self.L.svin_pg_last_error().decode())
        self._check(rc, "covariance_blocks")
        return out

    def covariance(self, earliest_loop_index, cur_index, a, b):
        """the D x D block Sigma[a, b]"""
        return self.covariance_blocks(earliest_loop_index, cur_index, [(a, b)])[0]

    def covariance_counters(self):
        c = (C.c_longlong * 4)()
        self._check(self.L.svin_pg_covariance_counters(self.h, c), "covariance_counters")
        return dict(factorisations=int(c[0]), passes=int(c[1]), columns=int(c[2]))
