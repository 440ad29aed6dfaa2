"""General 2x2 information matrices on reprojection residuals, host side (no GPU needed).

``svin_amd/csrc/dmath.hpp`` holds the square-root information helper (S = L^T of information = L L^T, Eigen's LLT on the lower
triangle) and the general form of ``reprojEval`` (r = S e, Jw = S J3 ahead of the rotation chain) that the evaluation kernels run
per lane.  tests/csrc/reproj_info_shim.cpp compiles both for the host; they are compared with numpy's Cholesky factor, with the
oracle's Map (``add_reproj`` + ``orc_map_eval``) and with the isotropic form.
"""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

from oracle import orc

HERE = os.path.dirname(os.path.abspath(__file__))
pd = C.POINTER(C.c_double)


@pytest.fixture(scope="module")
def shim(tmp_path_factory):
    out = str(tmp_path_factory.mktemp("reproj_info") / "svin_reproj_info_shim.so")
    subprocess.check_call(["g++", "-O2", "-std=c++17", "-shared", "-fPIC", "-o", out,
                           os.path.join(HERE, "csrc", "reproj_info_shim.cpp")])
    return C.CDLL(out)


def d(a):
    return a.ctypes.data_as(pd)


def rotated(l0, l1, deg):
    c, s = np.cos(np.radians(deg)), np.sin(np.radians(deg))
    R = np.array([[c, -s], [s, c]])
    M = R @ np.diag([l0, l1]) @ R.T
    return 0.5 * (M + M.T)


# isotropic, diagonal, rotated by 30 degrees with eigenvalue ratio 25, and ratio 1e4
MATRICES = {
    "isotropic": np.array([[0.64, 0.0], [0.0, 0.64]]),
    "diagonal": np.array([[2.5, 0.0], [0.0, 0.4]]),
    "rot30_ratio25": rotated(5.0, 0.2, 30.0),
    "rot30_ratio1e4": rotated(40.0, 0.004, 30.0),
}


@pytest.mark.parametrize("name", sorted(MATRICES))
def test_square_root_information_matches_numpy_cholesky(shim, name):
    info = np.ascontiguousarray(MATRICES[name])
    S = np.zeros(3)
    assert shim.ri_sqrt_information(d(info.reshape(-1)), d(S)) == 1
    ref = np.linalg.cholesky(info).T
    got = np.array([[S[0], S[1]], [0.0, S[2]]])
    err = np.max(np.abs(got - ref)) / np.max(np.abs(ref))
    print("sqrt information %s: relative error %.3e" % (name, err))
    assert err <= 1e-15, err
    assert np.max(np.abs(got.T @ got - info)) <= 4e-16 * np.max(np.abs(info))


def rand_pose(rng, tr=1.0, rot=0.5):
    a = rng.uniform(-rot, rot, 3)
    th = np.linalg.norm(a)
    return np.r_[rng.uniform(-tr, tr, 3), np.sin(th / 2) * a / th, np.cos(th / 2)]


def apply(T, p):
    x, y, z, w = T[3:]
    R = np.array([[1 - 2 * (y * y + z * z), 2 * (x * y - z * w), 2 * (x * z + y * w)],
                  [2 * (x * y + z * w), 1 - 2 * (x * x + z * z), 2 * (y * z - x * w)],
                  [2 * (x * z - y * w), 2 * (y * z + x * w), 1 - 2 * (x * x + y * y)]])
    return np.r_[R @ p[:3] + T[:3] * p[3], p[3]]


MODELS = {orc.DIST_NONE: [], orc.DIST_RADTAN: [-0.28, 0.07, 0.0002, 0.00002],
          orc.DIST_EQUIDISTANT: [-0.21, 0.14, 0.0006, 0.0003],
          orc.DIST_RADTAN8: [-0.16, 0.15, 0.0003, 0.0002, 0.01, 0.02, -0.01, 0.005]}
INTR = [458.0, 457.0, 367.0, 248.0]


def camera_row(model):
    cam = np.zeros(12)
    cam[:4] = INTR
    cam[4:4 + len(MODELS[model])] = MODELS[model]
    return cam


def geometry(rng, k):
    """pose, extrinsics, homogeneous point and measurement of case k: k % 7 == 0 may lie closer than 0.2 m (invalid: zero
    Jacobians), k % 11 == 3 is a point at infinity (|hw| <= 1e-8: the validity test is skipped)"""
    L = orc.lib()
    T_WS, T_SC = rand_pose(rng), rand_pose(rng, 0.2, 0.2)
    TW = np.zeros(7)
    L.orc_transformation_compose(d(T_WS), d(T_SC), d(TW))
    hw = 1.0 if k % 5 else rng.uniform(0.5, 2.0)
    z = rng.uniform(0.05, 0.19) if k % 7 == 0 else rng.uniform(1.0, 8.0)
    pc = np.r_[rng.uniform(-0.5, 0.5, 2) * z, z, 1.0]
    hp = apply(TW, pc) * hw
    if k % 11 == 3:
        hp = np.r_[apply(TW, pc)[:3] - TW[:3], 0.0]   # a direction: hw = 0
        hp[3] = 1e-9 if k % 2 else 0.0
    uv = np.array([300.0, 200.0]) + rng.normal(size=2) * 30
    return T_WS, T_SC, hp, uv


@pytest.mark.parametrize("name", sorted(MATRICES))
@pytest.mark.parametrize("model", sorted(MODELS))
def test_general_reprojection_matches_oracle_map(shim, model, name):
    """the tolerance of test_device_math_host.py's reprojEval check: 1e-11 of max(1, |reference|)"""
    rng = np.random.default_rng(300 + model)
    info = np.ascontiguousarray(MATRICES[name])
    S = np.zeros(3)
    assert shim.ri_information_valid(d(info.reshape(-1)), d(S)) == 1
    cam = camera_row(model)
    m = orc.OracleMap()
    pid, worst, n_invalid, n_inf = 1, 0.0, 0, 0
    for k in range(120):
        T_WS, T_SC, hp, uv = geometry(rng, k)
        m.add_param(pid, orc.BLOCK_POSE, T_WS)
        m.add_param(pid + 1, orc.BLOCK_HPOINT, hp)
        m.add_param(pid + 2, orc.BLOCK_POSE, T_SC)
        rid = m.add_reproj(model, INTR, MODELS[model], uv, info, orc.LOSS_NONE, pid, pid + 1, pid + 2)
        r, Js, Jm = m.eval(rid)
        ro, Jp, Jl, Je = np.zeros(2), np.zeros(12), np.zeros(6), np.zeros(12)
        shim.ri_reproj_general(d(cam), model, d(T_WS), d(hp), d(T_SC), C.c_double(uv[0]), C.c_double(uv[1]), d(S), d(ro), d(Jp),
                               d(Jl), d(Je))
        if k % 7 == 0 and k % 11 != 3:
            assert not Jp.any() and not Jl.any() and not Je.any() and ro.any()   # invalid: weighted residual kept, Jacobians zero
            n_invalid += 1
        if abs(hp[3]) <= 1e-8:
            n_inf += 1
        for a, b in ((ro, r), (Jp.reshape(2, 6), Jm[0]), (Jl.reshape(2, 3), Jm[1]), (Je.reshape(2, 6), Jm[2])):
            worst = max(worst, np.max(np.abs(a - b)) / max(1.0, np.max(np.abs(b))))
        pid += 3
    print("general reprojEval model %d %s: worst %.3e (%d invalid, %d at infinity)" % (model, name, worst, n_invalid, n_inf))
    assert n_invalid > 0 and n_inf > 0
    assert worst < 1e-11, worst


@pytest.mark.parametrize("model", sorted(MODELS))
def test_isotropic_matrix_through_the_general_form_equals_the_scalar_form(shim, model):
    rng = np.random.default_rng(500 + model)
    cam = camera_row(model)
    for k in range(120):
        T_WS, T_SC, hp, uv = geometry(rng, k)
        w = np.sqrt(64.0 / rng.uniform(4, 12) ** 2)
        S = np.array([w, 0.0, w])
        out = []
        for general in (True, False):
            ro, Jp, Jl, Je = np.zeros(2), np.zeros(12), np.zeros(6), np.zeros(12)
            if general:
                shim.ri_reproj_general(d(cam), model, d(T_WS), d(hp), d(T_SC), C.c_double(uv[0]), C.c_double(uv[1]), d(S), d(ro),
                                       d(Jp), d(Jl), d(Je))
            else:
                shim.ri_reproj_scalar(d(cam), model, d(T_WS), d(hp), d(T_SC), C.c_double(uv[0]), C.c_double(uv[1]), C.c_double(w),
                                      d(ro), d(Jp), d(Jl), d(Je))
            out.append(np.r_[ro, Jp, Jl, Je])
        np.testing.assert_allclose(out[0], out[1], rtol=1e-15, atol=0.0)


@pytest.mark.parametrize("name,info", [
    ("asymmetric", [[2.0, 0.3], [0.2, 1.0]]),
    ("indefinite", [[1.0, 2.0], [2.0, 1.0]]),
    ("negative", [[-1.0, 0.0], [0.0, 1.0]]),
    ("zero", [[0.0, 0.0], [0.0, 0.0]]),
    ("nan", [[np.nan, 0.0], [0.0, 1.0]]),
    ("nan_offdiagonal", [[1.0, np.nan], [np.nan, 1.0]]),
    ("inf", [[np.inf, 0.0], [0.0, 1.0]]),
])
def test_bad_information_matrices_are_refused(shim, name, info):
    S = np.zeros(3)
    assert shim.ri_information_valid(d(np.ascontiguousarray(info, np.float64).reshape(-1)), d(S)) == 0
