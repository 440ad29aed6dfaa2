"""The host side of the pose graph's caller-given edges (svin_amd/csrc/pg_edges.hpp through tests/csrc/pg_edges_shim.cpp) on the
CPU: which information matrices are accepted, the factor S = L^T they give, the weights of an edge without a matrix, the loss
arguments, and the table of destination blocks that three or more edges share.

The bound on S^T S.  pgEdgeFactor is a Cholesky factorisation in IEEE float64 (correctly rounded sqrt and division), D <= 6.  By
Higham, Accuracy and Stability, theorem 10.3 the computed factor satisfies S^T S = I + dI with |dI| <= gamma_(D+1) |S|^T |S|,
gamma_k = k u / (1 - k u), u = 2^-53.  The test forms S^T S and |S|^T |S| in long double (error 2^-11 of that bound) and holds
every entry to gamma_(D+1) (|S|^T |S|)_ij."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
OK, NOT_FINITE, NOT_SYMMETRIC, NOT_PD = 0, 1, 2, 3
U = 2.0 ** -53


@pytest.fixture(scope="module")
def lib(tmp_path_factory):
    so = os.path.join(str(tmp_path_factory.mktemp("pgedges")), "libpge.so")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-Wall", "-Wextra", "-Werror", "-shared", "-fPIC",
                           os.path.join(ROOT, "tests", "csrc", "pg_edges_shim.cpp"), "-o", so])
    L = C.CDLL(so)
    pd, ip = C.POINTER(C.c_double), C.POINTER(C.c_int)
    L.pge_constant.restype = C.c_int64
    L.pge_factor.argtypes = [pd, C.c_int, pd]
    L.pge_default.argtypes = [C.c_int, pd, pd]
    L.pge_loss_valid.argtypes = [C.c_int, C.c_double]
    L.pge_status_text.restype = C.c_char_p
    L.pge_shared.restype = C.c_int64
    L.pge_shared.argtypes = [C.c_int, ip, ip, ip, C.c_int, C.POINTER(C.c_int64), C.c_int64]
    return L


def _pd(a):
    return a.ctypes.data_as(C.POINTER(C.c_double))


def factor(lib, info):
    info = np.ascontiguousarray(info, np.float64)
    D = info.shape[0]
    S = np.full((D, D), -7.0)
    return lib.pge_factor(_pd(info), D, _pd(S)), S


def spd(D, seed, cond=10.0):
    rng = np.random.default_rng(seed)
    Q, _ = np.linalg.qr(rng.normal(size=(D, D)))
    w = np.geomspace(1.0, cond, D)
    A = (Q * w) @ Q.T
    return (A + A.T) / 2


@pytest.mark.parametrize("D", [4, 6])
@pytest.mark.parametrize("cond", [1.0, 1e3, 1e6, 1e10])
def test_factor_reproduces_the_information(lib, D, cond):
    LD = np.longdouble
    for seed in range(5):
        info = spd(D, 10 * D + seed, cond) * 10.0 ** (seed - 2)
        st, S = factor(lib, info)
        assert st == OK
        assert np.all(np.tril(S, -1) == 0) and np.all(np.diag(S) > 0)
        gram = S.astype(LD).T @ S.astype(LD)
        absgram = np.abs(S).astype(LD).T @ np.abs(S).astype(LD)
        gamma = (D + 1) * U / (1 - (D + 1) * U)
        assert np.all(np.abs(gram - info.astype(LD)) <= gamma * absgram)


def test_diagonal_and_identity_are_exact_where_the_roots_are(lib):
    st, S = factor(lib, np.diag([400.0, 400, 400, 10000, 10000, 10000]))
    assert st == OK and np.array_equal(S, np.diag([20.0, 20, 20, 100, 100, 100]))
    st, S = factor(lib, np.eye(4))
    assert st == OK and np.array_equal(S, np.eye(4))


def test_refused_matrices_leave_the_output_alone(lib):
    good = spd(4, 3)
    cases = []
    a = good.copy(); a[1, 2] = np.nextafter(a[1, 2], np.inf); cases.append((a, NOT_SYMMETRIC))          # one ulp off symmetry
    cases.append((np.diag([1.0, -1.0, 1.0, 1.0]), NOT_PD))                                                # indefinite
    cases.append((np.array([[1.0, 1, 0, 0], [1, 1, 0, 0], [0, 0, 1, 0], [0, 0, 0, 1]]), NOT_PD))          # semi-definite, exactly
    cases.append((np.zeros((4, 4)), NOT_PD))
    v = np.array([1.0, 2, 3, 4, 5, 6]); cases.append((np.outer(v, v), NOT_PD))                            # rank one, 6 x 6
    a = good.copy(); a[0, 0] = np.nan; cases.append((a, NOT_FINITE))
    a = good.copy(); a[1, 3] = a[3, 1] = np.inf; cases.append((a, NOT_FINITE))
    a = good.copy(); a[2, 1] = np.nan; cases.append((a, NOT_FINITE))                                      # NaN is reported as NaN, not as asymmetry
    for info, want in cases:
        st, S = factor(lib, info)
        assert st == want, (info, st)
        assert np.all(S == -7.0)
        assert lib.pge_status_text(st) and lib.pge_status_text(st) != b"ok"
    assert factor(lib, good)[0] == OK


def test_defaults(lib):
    for six, w in ((0, [1, 1, 1, 0.1]), (1, [20, 20, 20, 100, 100, 100])):
        D = len(w)
        S, info = np.zeros((D, D)), np.zeros((D, D))
        lib.pge_default(six, _pd(S), _pd(info))
        assert np.array_equal(S, np.diag(np.array(w, np.float64)))
        assert np.array_equal(info, np.diag(np.array(w, np.float64) ** 2))
        st, S2 = factor(lib, info)          # the squared weights written out give the weights back (to a rounding of the root)
        assert st == OK and np.max(np.abs(S2 - S)) <= 2 * U * np.max(w)
    assert lib.pge_constant(0) == 3 and lib.pge_constant(1) == 10 and lib.pge_constant(2) == 21


def test_loss_arguments(lib):
    assert lib.pge_loss_valid(0, float("nan")) == 1 and lib.pge_loss_valid(0, -1.0) == 1
    for kind in (1, 2):
        assert lib.pge_loss_valid(kind, 0.1) == 1
        for bad in (0.0, -0.1, float("inf"), float("nan")):
            assert lib.pge_loss_valid(kind, bad) == 0
    assert lib.pge_loss_valid(3, 1.0) == 0 and lib.pge_loss_valid(-1, 1.0) == 0


def shared(lib, edges, off, min_count=3):
    ip = C.POINTER(C.c_int)
    ea = np.ascontiguousarray([a for a, _ in edges], np.int32)
    eb = np.ascontiguousarray([b for _, b in edges], np.int32)
    off = np.ascontiguousarray(off, np.int32)
    args = (len(edges), ea.ctypes.data_as(ip), eb.ctypes.data_as(ip), off.ctypes.data_as(ip), min_count)
    need = lib.pge_shared(*args, None, 0)
    o = np.zeros(need, np.int64)
    assert lib.pge_shared(*args, o.ctypes.data_as(C.POINTER(C.c_int64)), need) == need
    it = iter(o.tolist())
    out = []
    for _ in range(next(it)):
        lo, hi, cnt = next(it), next(it), next(it)
        out.append((lo, hi, [next(it) for _ in range(cnt)]))
    assert next(it, None) is None
    return out


def test_shared_destinations_by_multiplicity_and_orientation(lib):
    off = [-1] + [4 * k for k in range(9)]
    # pair (1,2) once, (2,3) twice, (3,4) three times (one reversed), (5,4) four times in both orientations, (0,6) three times
    # on a constant keyframe, interleaved
    edges = [(1, 2), (2, 3), (3, 4), (5, 4), (0, 6), (3, 2), (4, 3), (4, 5), (0, 6), (3, 4), (5, 4), (6, 0), (4, 5), (7, 8)]
    got = shared(lib, edges, off)
    assert got == [(3, 4, [2, 6, 9]), (4, 5, [3, 7, 10, 12])]
    # every multiplicity from two on
    got2 = shared(lib, edges, off, 2)
    assert got2 == [(2, 3, [1, 5]), (3, 4, [2, 6, 9]), (4, 5, [3, 7, 10, 12])]
    assert shared(lib, edges, off, 5) == []
    assert shared(lib, [], off) == []


def test_shared_groups_come_in_the_order_of_their_first_edge(lib):
    off = [0, 4, 8, 12]
    edges = [(2, 3), (0, 1), (3, 2), (1, 0), (0, 1), (2, 3)]
    assert shared(lib, edges, off) == [(2, 3, [0, 2, 5]), (0, 1, [1, 3, 4])]
