"""Map::getLhs on the GPU (svin_ba_get_lhs / svin_ba_get_lhs_blocks; kernels in svin_amd/csrc/lhs.hip) against the oracle's
Map::getLhs (oracle/orc_map.cpp, the CPU restatement of okvis_ceres/src/Map.cpp:105-150) at identical states on both sides.

H of a block = sum of J^T J over its residuals, minimal Jacobians, no loss.  Bars: |dH|_F / |H|_F <= 1e-10; blocks an IMU factor
touches 1e-7 (the rule of test_gpu_parity.check_small_factors: the IMU rows carry the square root of an ill-conditioned
information matrix that the two sides invert by different algorithms); after a marginalisation 1e-9 in units of sqrt(diag)."""
import ctypes as C
import subprocess

import numpy as np
import pytest

from svin_amd import synthetic as syn
from test_gpu_parity import drop_underdetermined_landmarks, inject_states, log, make_pair, oracle_describe, snapshot_states

pytestmark = pytest.mark.gpu


def gpu_blocks(gpu):
    """every block of the GPU window: (id, key) with key (frame, kind, index) or ("lm", id)"""
    lms = set(gpu.landmark_ids())
    out = []
    for b in gpu.parameter_block_ids():
        d = gpu.describe_block(b)
        if d is not None:
            out.append((int(b), d))
        elif b in lms:
            out.append((int(b), ("lm", int(b))))
    return out


def oracle_lhs(cpu, keys):
    """the oracle's getLhs of the blocks named by `keys` (the GPU's keys; frame and landmark ids are the same on both sides)"""
    m = cpu.map()
    ids = {}
    for rid in m.residual_ids():
        for b in m.parameters_of(rid):
            d = oracle_describe(cpu, b)
            if d is not None:
                ids[d] = b
    lms = set(cpu.landmark_ids())
    out = {}
    for k in keys:
        if k[0] == "lm":
            if k[1] in lms:
                out[k] = m.get_lhs(k[1], 3)
        elif k in ids:
            out[k] = m.get_lhs(ids[k], 9 if k[1] == 2 else 6)
    return out


def imu_touched(gpu):
    return {b for f in gpu.eval_factors() if f["kind"] == 0 for b in f["blocks"]}


def optimised_states(spec, iters=6):
    from svin_amd.estimator import Estimator
    e = Estimator(0)
    syn.feed(e, spec)
    e.optimize(iters)
    return snapshot_states(e)


def all_lhs(gpu):
    blocks = gpu_blocks(gpu)
    Hs = gpu.get_lhs_blocks([b for b, _ in blocks])
    return {k: H for (b, k), H in zip(blocks, Hs)}, {k: b for b, k in blocks}


def compare_with_oracle(gpu, cpu, tag, imu_blocks=(), bar=1e-10, imu_bar=1e-7, skip=()):
    Hg, ids = all_lhs(gpu)
    Hc = oracle_lhs(cpu, list(Hg))
    worst, n = {}, 0
    for k, H in Hg.items():
        if k not in Hc:   # a block no residual touches: zero by definition
            assert not np.any(H), (tag, k)
            continue
        ref = Hc[k]
        assert H.shape == ref.shape, (tag, k)
        if ids[k] in skip:
            continue
        nr = np.linalg.norm(ref)
        d = np.linalg.norm(H - ref) / nr if nr > 0 else np.linalg.norm(H)
        kind = 3 if k[0] == "lm" else k[1]
        worst[kind] = max(worst.get(kind, 0.0), d)
        tol = imu_bar if ids[k] in imu_blocks else bar
        assert d <= tol, (tag, k, d)
        n += 1
    log(tag, "blocks", n, "worst |dH|_F / |H|_F by kind (0 pose, 1 extrinsics, 2 speed/bias, 3 landmark):", worst)
    assert set(worst) >= ({3} if skip else {0, 3})
    return Hg


@pytest.mark.parametrize("rig,kw", [("euroc", {}), ("test4", {}), ("rig_v2", dict(sonar=True, depth=True))])
def test_narrow_window_lhs_against_oracle(gpu_lib, rig, kw):
    """every pose, extrinsics, speed/bias and landmark block at the initial states, then at the GPU's optimised states put into the
    oracle (rig_v2: sonar, depth, per-frame extrinsics with relative-extrinsics factors)"""
    spec = syn.make_window(P=10, L=600, n_obs=6000, seed=41, rig=rig, **kw)
    gpu, cpu, fg, fc, lg, lc = make_pair(spec)
    assert fg == fc and lg == lc
    imu = imu_touched(gpu)
    H0 = compare_with_oracle(gpu, cpu, "%s initial" % rig, imu)
    assert {k[1] for k in H0 if k[0] != "lm"} == {0, 1, 2}
    # optimised states from a third estimator into both: an estimator that optimised itself has re-integrated its IMU factors at
    # the biases ITS history visited (ImuError.cpp:581-592), so the two sides get the same states AND the same history
    snap = optimised_states(spec)
    inject_states(gpu, snap)
    inject_states(cpu, snap)
    H1 = compare_with_oracle(gpu, cpu, "%s optimised" % rig, imu)
    assert any(not np.array_equal(H0[k], H1[k]) for k in H0)


def test_lhs_with_marginalisation_prior_against_oracle(gpu_lib):
    """the idea of test_gpu_parity.one_shot_pass: the oracle's optimised states into both sides, ONE marginalisation, every block
    compared before anything is optimised again -- the prior contributes its diagonal block of J^T J (a block fixed when it was
    marginalised contributes nothing); in units of sqrt(diag) at 1e-9"""
    from svin_amd.estimator import Estimator
    from oracle import orc
    spec = syn.make_window(P=7, L=500, n_obs=4000, seed=52, rig="rig_v2", keyframe_every=2, frame_dt=0.3, sonar=True, depth=True)
    snaps = []

    def record(k, fid, est):
        if k == 5:
            est.optimize(12)
            snaps.append(snapshot_states(est))
    ref = orc.OracleEstimator()
    syn.feed(ref, spec, on_frame=lambda k, fid: record(k, fid, ref))
    out = {}

    def run(est, name):
        def cb(k, fid):
            if k != 5:
                return
            inject_states(est, snaps[0])
            if name == "gpu":
                out["before"] = all_lhs(est)[0]
            ok, removed = est.apply_marginalization(2, 2)
            assert ok and len(removed) >= 1
            assert est.marg() is not None
            if name == "gpu":   # the same handle as "before": the marginalisation has dropped the kept result
                n0 = est.lhs_pass_count()
                out["gpu"], out["ids"] = all_lhs(est)
                assert est.lhs_pass_count() == n0 + 1
                out["imu"] = imu_touched(est)
            else:
                out["cpu"] = oracle_lhs(est, list(out["gpu"]))
        syn.feed(est, spec, on_frame=cb)
    run(Estimator(0), "gpu")
    run(orc.OracleEstimator(), "cpu")
    Hg, Hc, ids = out["gpu"], out["cpu"], out["ids"]
    worst, prior_blocks = 0.0, 0
    for k, H in Hg.items():
        if k not in Hc:
            assert not np.any(H), k
            continue
        sd = np.sqrt(np.maximum(np.abs(np.diag(Hc[k])), 1e-300))
        d = float(np.max(np.abs(H - Hc[k]) / np.outer(sd, sd)))
        worst = max(worst, d)
        assert d <= 1e-9, (k, d)
        prior_blocks += k in out["before"] and not np.array_equal(out["before"][k], H)
    log("getLhs after one marginalisation: blocks", len(Hg), "changed by it", prior_blocks, "worst in sqrt(diag) units", worst)
    assert prior_blocks >= 1


def test_wide_window_lhs_against_oracle(gpu_lib):
    """P = 48, L = 1 500: the shape of test_wide_window_panels_against_oracle (host-packed observation table, panel order)"""
    spec = drop_underdetermined_landmarks(syn.make_window(P=48, L=1500, n_obs=15000, seed=31, frame_dt=0.25))
    gpu, cpu, fg, fc, lg, lc = make_pair(spec)
    assert fg == fc and lg == lc
    compare_with_oracle(gpu, cpu, "wide window P = 48", imu_touched(gpu))


def _rot(qv):
    x, y, z, w = qv
    return np.array([[1 - 2 * (y * y + z * z), 2 * (x * y - z * w), 2 * (x * z + y * w)],
                     [2 * (x * y + z * w), 1 - 2 * (x * x + z * z), 2 * (y * z - x * w)],
                     [2 * (x * z - y * w), 2 * (y * z + x * w), 1 - 2 * (x * x + y * y)]])


def build_map_window(est, m, host_pose_error):
    """the builder of test_gpu_map.test_map_built_window_against_oracle_map, smaller: one pose (Pose4d manifold, PoseError built in
    or as a host cost function), a constant extrinsics block, 120 landmarks -- every third constant, the others under a
    HomogeneousPointError -- with Cauchy-robustified reprojection residuals of an equidistant camera"""
    from svin_amd import estimator
    from oracle import orc
    rng = np.random.default_rng(11)
    intr, dist = [350.0, 360.0, 378.0, 238.0], [-0.21, 0.14, 0.0006, 0.0003]
    T_WS = np.r_[rng.uniform(-3, 3, 3), 0, 0, 0, 1.0]
    q = rng.normal(size=4)
    T_WS[3:] = q / np.linalg.norm(q)
    T_SC = np.r_[0.1, -0.05, 0.02, 0.0, 0.0, 0.0, 1.0]
    est.add_camera(syn.DIST_EQUIDISTANT, intr, dist, 752, 480, [0, 0, 0, 0])
    T_init = T_WS.copy()
    T_init[:3] += 0.05 * rng.normal(size=3)
    assert est.map_add_parameter_block(1, est.BLOCK_POSE, T_init) and est.map_add_parameter_block(2, est.BLOCK_POSE, T_SC)
    assert est.set_parameter_block_constant(2)
    m.add_param(1, orc.BLOCK_POSE, T_init)
    m.add_param(2, orc.BLOCK_POSE, T_SC)
    m.set_constant(2)
    A6 = rng.standard_normal((6, 6))
    info6 = A6 @ A6.T + 10.0 * np.eye(6)
    meas = T_init + np.r_[0.02, -0.01, 0.03, 0, 0, 0, 0]
    if host_pose_error:
        def pose_cost(ps):
            r, Jm, _ = estimator.host_pose_error(meas, info6, ps[0])
            return r, [Jm]
        assert est.map_add_host_residual([1], [7], 6, pose_cost) != 0
    else:
        assert est.map_add_pose_error(1, meas, info6) != 0
    orc.lib().orc_map_add_pose_error(m.h, orc.dptr(orc.arr(meas)), orc.dptr(orc.arr(info6)), 1)
    Rws, Rsc = _rot(T_WS[3:]), _rot(T_SC[3:])
    for i in range(120):
        pc = np.r_[rng.uniform(-1.5, 1.5, 2), 1.0] * (3.0 * (i % 10) + 2.0)
        pw = Rws @ (Rsc @ pc + T_SC[:3]) + T_WS[:3]
        r = np.hypot(pc[0], pc[1])
        th = np.arctan2(r, pc[2])
        thd = th * (1 + dist[0] * th ** 2 + dist[1] * th ** 4 + dist[2] * th ** 6 + dist[3] * th ** 8)
        s = thd / r if r > 1e-8 else 1.0
        uv = np.array([intr[0] * s * pc[0] + intr[2], intr[1] * s * pc[1] + intr[3]]) + rng.uniform(-1, 1, 2)
        hp = np.r_[pw + 0.05 * rng.normal(size=3), 1.0]
        assert est.map_add_parameter_block(10 + i, est.BLOCK_HOMOGENEOUS_POINT, hp)
        m.add_param(10 + i, orc.BLOCK_HPOINT, hp)
        assert est.map_add_reprojection_error(1, 10 + i, 2, 0, uv, np.eye(2)) != 0
        m.add_reproj(orc.DIST_EQUIDISTANT, intr, dist, uv, np.eye(2), orc.LOSS_CAUCHY, 1, 10 + i, 2)
        if i % 3 == 0:
            assert est.set_parameter_block_constant(10 + i)
            m.set_constant(10 + i)
        else:
            est.add_homogeneous_point_error(10 + i, hp, variance=4.0)
            m.add_hpoint_error(hp, 4.0, 10 + i)
    assert est.reset_parameterization(1, 3)   # Map::Pose4d: getLhs keeps six columns
    m.reset_parameterization(1, 4)
    return [1, 2] + [10 + i for i in range(120)]


def test_map_built_graph_lhs_and_host_pose_error(gpu_lib):
    """constant landmarks (|w| of their observations), HomogeneousPointErrors, a pose on a reduced manifold, and a PoseError given
    as an F_HOST callback: the same H as the built-in PoseError and as the oracle's"""
    from svin_amd.estimator import Estimator
    from oracle import orc
    res = {}
    for host in (False, True):
        est, m = Estimator(0), orc.OracleMap()
        ids = build_map_window(est, m, host)
        Hs = est.get_lhs_blocks(ids)
        dims = [6, 6] + [3] * 120
        for b, H, d in zip(ids, Hs, dims):
            ref = m.get_lhs(b, d)
            dd = np.linalg.norm(H - ref) / np.linalg.norm(ref)
            assert dd <= 1e-10, (host, b, dd)
        res[host] = Hs
        # and after a solve (the oracle at the GPU's values)
        est.optimize(5)
        for b in ids:
            m.set_param(b, est.get_parameter_block(b))
        for b, H, d in zip(ids, est.get_lhs_blocks(ids), dims):
            ref = m.get_lhs(b, d)
            assert np.linalg.norm(H - ref) <= 1e-10 * np.linalg.norm(ref), (host, b)
    log("map-built graph: pose block built-in vs host PoseError", np.max(np.abs(res[False][0] - res[True][0])))
    assert np.linalg.norm(res[False][0] - res[True][0]) <= 1e-13 * np.linalg.norm(res[False][0])
    for a, b in zip(res[False][1:], res[True][1:]):
        assert np.array_equal(a, b)


def test_lhs_consistency(gpu_lib):
    """bit-identical from call to call and per block vs batched; host pack mode == resident; landmark qualities; the cached result
    follows set_T_WS / set_landmark / optimize and matches the oracle again"""
    from svin_amd.estimator import Estimator
    spec = syn.make_window(P=8, L=400, n_obs=4000, seed=61)
    gpu, cpu, fg, fc, lg, lc = make_pair(spec)
    H1, ids = all_lhs(gpu)
    gpu.set_T_WS(fg[0], gpu.get_T_WS(fg[0]))   # drops the cached result: the second pass is a fresh computation
    H2, _ = all_lhs(gpu)
    for k in H1:
        assert np.array_equal(H1[k], H2[k]), k
        assert np.array_equal(gpu.get_lhs(ids[k]), H1[k]), k
    # host pack mode against the device-resident observation table
    b = Estimator(0)
    b.set_pack_mode(1)
    syn.feed(b, spec)
    for it in (0, 1):
        Ha, Hb = all_lhs(gpu)[0], all_lhs(b)[0]
        assert Ha.keys() == Hb.keys()
        for k in Ha:
            assert np.array_equal(Ha[k], Hb[k]), (it, k)
        if it == 0:
            gpu.optimize(5)
            b.optimize(5)
    assert gpu.path_counters()["resident_solves"] >= 1 and b.path_counters()["resident_solves"] == 0
    # quality from H (Estimator.cpp:902-923) against the library's own
    lms = gpu.get_landmarks()
    Hl = gpu.get_lhs_blocks(list(lms))
    worst = 0.0
    for (lid, info), H in zip(lms.items(), Hl):
        ev = np.linalg.eigvalsh(H)
        q = 0.0 if ev[0] < 1e-12 else np.sqrt(ev[0]) / np.sqrt(ev[2])
        worst = max(worst, abs(q - info["quality"]))
    log("landmark quality from getLhs vs get_landmark: worst", worst)
    assert worst <= 1e-8
    # the cached result follows every change and matches the oracle again
    g2 = Estimator(0)
    syn.feed(g2, spec)
    Hfresh = all_lhs(g2)[0]
    snap = snapshot_states(gpu)
    inject_states(g2, snap)
    inject_states(cpu, snap)
    gpu = g2
    imu = imu_touched(gpu)
    H0 = compare_with_oracle(gpu, cpu, "consistency: at optimised states", imu)
    assert not np.array_equal(H0[(fg[3], 0, 0)], Hfresh[(fg[3], 0, 0)])
    T = gpu.get_T_WS(fg[3]) + np.r_[0.01, -0.02, 0.005, 0, 0, 0, 0]
    assert gpu.set_T_WS(fg[3], T) and cpu.set_T_WS(fc[3], T)
    Hs = compare_with_oracle(gpu, cpu, "consistency: after set_T_WS", imu)
    assert not np.array_equal(H0[(fg[3], 0, 0)], Hs[(fg[3], 0, 0)])
    lid = gpu.landmark_ids()[5]
    hp = gpu.get_landmark(lid)["point"] + np.r_[0.05, 0.02, -0.03, 0.0]
    assert gpu.set_landmark(lid, hp) and cpu.set_landmark(lid, hp)
    Hl2 = compare_with_oracle(gpu, cpu, "consistency: after set_landmark", imu)
    assert not np.array_equal(Hs[("lm", lid)], Hl2[("lm", lid)])
    # nothing changed since the last comparison: no pass at all
    n0 = gpu.lhs_pass_count()
    gpu.get_lhs(lid)
    assert gpu.lhs_pass_count() == n0
    # read-only queries keep the result: after a change, the reference's loop (getLhs, then parameterBlockPtr) is one pass
    assert gpu.set_T_WS(fg[2], gpu.get_T_WS(fg[2]))
    for l in gpu.landmark_ids():
        gpu.get_lhs(l)
        gpu.parameter_block(l)
        gpu.get_landmark(l)
    gpu.get_T_WS(fg[2])
    gpu.describe_block(gpu.parameter_block_ids()[0])
    gpu.get_lhs(fg[2])
    assert gpu.lhs_pass_count() == n0 + 1
    # optimize on the SAME handle drops it; the oracle at that handle's new states.  Blocks an IMU factor touches are not held to
    # the oracle here: the solve re-integrated the IMU factors at the biases its iterations visited, the oracle did not (its IMU
    # terms are linearised elsewhere, ImuError.cpp:581-592) -- they must only have been recomputed
    gpu.optimize(3)
    inject_states(cpu, snapshot_states(gpu))
    Ho = compare_with_oracle(gpu, cpu, "consistency: after optimize on the same handle", skip=imu)
    assert gpu.lhs_pass_count() == n0 + 2
    assert not np.array_equal(Ho[(fg[3], 0, 0)], Hl2[(fg[3], 0, 0)]) and not np.array_equal(Ho[("lm", lid)], Hl2[("lm", lid)])


def test_lhs_errors(gpu_lib):
    """unknown id, too small a capacity, and landmark-sharded mode (SVIN_ERR_UNSUPPORTED)"""
    from svin_amd.estimator import Estimator
    from svin_amd import distributed as sd
    spec = syn.make_window(P=4, L=100, n_obs=800, seed=7)
    est = Estimator(0)
    fids, lids = syn.feed(est, spec)
    L, h = est.L, est.h
    H = np.zeros(81)
    pH = H.ctypes.data_as(C.POINTER(C.c_double))
    assert L.svin_ba_get_lhs(h, 987654321, pH, 81) == -2
    assert L.svin_ba_get_lhs(h, fids[0], pH, 35) == -6
    assert L.svin_ba_get_lhs(h, lids[0], pH, 8) == -3
    assert L.svin_ba_get_lhs(h, fids[0], pH, 36) == 6 and np.any(H[:36])
    ids = np.array([fids[0], 987654321], np.uint64)
    assert L.svin_ba_get_lhs_blocks(h, 2, ids.ctypes.data_as(C.POINTER(C.c_uint64)), None, None, 0) == -2
    ids = np.array([fids[0], lids[0]], np.uint64)
    dims = np.zeros(2, np.int32)
    assert L.svin_ba_get_lhs_blocks(h, 2, ids.ctypes.data_as(C.POINTER(C.c_uint64)), dims.ctypes.data_as(C.POINTER(C.c_int32)), None, 0) == 45
    assert list(dims) == [6, 3]
    assert L.svin_ba_get_lhs_blocks(h, 2, ids.ctypes.data_as(C.POINTER(C.c_uint64)), None, pH, 44) == -1
    with pytest.raises(RuntimeError):
        est.get_lhs(987654321)
    # sharded mode: not available
    world = 2
    ar = sd.ThreadAllReduce(world)
    e = Estimator(0)
    syn.feed(e, sd.shard_spec(spec, 0, world))
    e.set_distributed(0, world, ar.callback(0))
    assert e.L.svin_ba_get_lhs(e.h, e.frame_ids()[0], pH, 81) == -4
    assert e.L.svin_ba_get_lhs_blocks(e.h, 1, np.array([e.frame_ids()[0]], np.uint64).ctypes.data_as(C.POINTER(C.c_uint64)), None, pH, 81) == -4


def test_shim_getlhs_loop_matches_batched_blocks(gpu_lib, tmp_path):
    """tests/csrc/shim_lhs.cpp: the reference's landmark loop (Estimator.cpp:902-923) through the shim's Map::getLhs, blocks held bit
    for bit against svin_ba_get_lhs_blocks inside the program and against the ctypes mirror driving the same window"""
    from svin_amd.estimator import Estimator
    from test_gpu_shim import dump_window
    from test_shim_compile import _compile
    exe = _compile(tmp_path, "shim_lhs")
    spec = syn.make_window(P=7, L=200, n_obs=1800, seed=23, rig="euroc", keyframe_every=2, frame_dt=0.3)
    path = str(tmp_path / "window.txt")
    dump_window(spec, path, 0, 2, 8)
    p = subprocess.run([exe, path], capture_output=True, text=True, timeout=300)
    assert p.returncode == 0, (p.returncode, p.stdout[-2000:], p.stderr[-2000:])
    lhs, summary = {}, None
    for line in p.stdout.splitlines():
        t = line.split()
        if t[0] == "lhs":
            lhs[int(t[1])] = (np.array([float(v) for v in t[2:11]]).reshape(3, 3), float(t[12]))
        elif t[0] == "blocks":
            summary = dict(n=int(t[1]), match=int(t[3]), pose_dim=int(t[5]), loop_us=float(t[7]), loop_passes=int(t[9]),
                           same_point=int(t[11]))
    log("shim getLhs loop:", summary)
    assert summary is not None and summary["n"] == summary["match"] == len(lhs) > 0 and summary["pose_dim"] == 6
    # getLhs + parameterBlockPtr per landmark, as the reference's loop: ONE all-blocks pass for the whole loop
    assert summary["loop_passes"] == 1 and summary["same_point"] == summary["n"]
    est = Estimator(0)
    syn.feed(est, spec)
    est.optimize(8)
    ids = sorted(lhs)
    assert ids == sorted(est.landmark_ids())
    for lid, H in zip(ids, est.get_lhs_blocks(ids)):
        assert np.array_equal(H, lhs[lid][0]), lid
        assert abs(lhs[lid][1] - est.get_landmark(lid)["quality"]) <= 1e-8
