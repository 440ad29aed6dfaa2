"""The windows the Levenberg-Marquardt tests run on -- tests/test_lm_reference_host.py (CPU: the numpy reference against the oracle
and against the rules) and tests/test_gpu_lm.py (the device against the numpy reference) -- built identically on an oracle object
and on the library's Estimator.  The smallest shapes that reach each route of the reduced solve, from starts perturbed far enough
that the reference's own Levenberg-Marquardt log shows an accepted step with the 1/3 clamp active, one with it inactive, and two
consecutive rejected steps (asserted in test_lm_reference_host.py)."""
import os

import numpy as np

from svin_amd import synthetic as syn

GOLD = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "golden")
TIGHT = (1e-14, 1e-14, 1e-14)

# name -> make_window arguments, iterations.  "imu": poses, speed / bias, IMU factors, reprojection residuals.  "chain": the second rig
# (per-frame extrinsics) with sonar and depth factors -- the chain elimination of the reduced solve.  "prior": the window left after two
# marginalisations on the way (the marginalisation prior in the reduced system).
ESTIMATOR_WINDOWS = {
    "imu": (dict(P=5, L=60, n_obs=600, seed=73, pose_noise=(1.0, 0.25), lm_noise=2.5), 14),
    "imu_mild": (dict(P=4, L=60, n_obs=600, seed=71), 10),
    "chain": (dict(P=4, L=60, n_obs=600, seed=75, rig="rig_v2", sonar=True, depth=True, sonar_patch=(3, 6)), 12),
    "prior": (dict(P=6, L=60, n_obs=700, seed=76, keyframe_every=2, frame_dt=0.3), 12),
}


def feed_estimator(est, name):
    """the named window on an estimator-like object (the oracle's or the library's); returns (frame ids, landmark ids)"""
    kw, _ = ESTIMATOR_WINDOWS[name]
    spec = syn.make_window(**kw)
    if name != "prior":
        return syn.feed(est, spec)
    count = [0]

    def on_frame(k, fid):
        # two marginalisations, at the last two frames but one; the solves in front of them are short dogleg solves on both sides
        if k in (spec.P - 3, spec.P - 2):
            est.optimize(3)
            est.apply_marginalization(2, 2)
            count[0] += 1
    out = syn.feed(est, spec, on_frame=on_frame)
    assert count[0] == 2
    return out


def tiny_start(g, scale):
    """tests/golden/tiny_window.npz's start, moved: the free pose by scale x (0.3 m, 0.1 rad), the landmarks by scale x 0.5 m"""
    rng = np.random.default_rng(11)
    T1 = np.array(g["T1_init"], float)
    T1[:3] += scale * 0.3 * rng.normal(size=3)
    q = T1[3:] + scale * 0.05 * rng.normal(size=4)
    T1[3:] = q / np.linalg.norm(q)
    lm = np.array(g["lm_init"], float) + scale * 0.5 * rng.normal(size=np.shape(g["lm_init"]))
    return T1, lm


def load_tiny():
    return np.load(os.path.join(GOLD, "tiny_window.npz"))


def tiny_on_oracle(orc, g, T1, lm, loss=None):
    """2 poses (one constant), 2 constant extrinsics, 12 landmarks, 48 reprojection residuals (CauchyLoss(1) unless `loss` says
    otherwise) on an OracleMap"""
    m = orc.OracleMap()
    loss = orc.LOSS_CAUCHY if loss is None else loss
    info = 64.0 / float(g["size"]) ** 2 * np.eye(2)
    m.add_param(1, orc.BLOCK_POSE, g["T0"])
    m.set_constant(1)
    m.add_param(2, orc.BLOCK_POSE, T1)
    for c in range(2):
        m.add_param(3 + c, orc.BLOCK_POSE, g["T_SC"][c])
        m.set_constant(3 + c)
    for l in range(len(lm)):
        m.add_param(10 + l, orc.BLOCK_HPOINT, np.r_[lm[l], 1.0])
        for f, pose in enumerate((1, 2)):
            for c in range(2):
                m.add_reproj(orc.DIST_RADTAN, g["intr"], g["dist"], g["uv"][f, c, l], info, loss, pose, 10 + l, 3 + c)
    return m


def tiny_on_device(est, g, T1, lm):
    """the same through the library's Map entry points"""
    info = 64.0 / float(g["size"]) ** 2 * np.eye(2)
    for c in range(2):
        est.add_camera(syn.DIST_RADTAN, g["intr"], g["dist"], 752, 480, [0.0, 0.0, 0.0, 0.0])
    assert est.map_add_parameter_block(1, est.BLOCK_POSE, g["T0"]) and est.set_parameter_block_constant(1)
    assert est.map_add_parameter_block(2, est.BLOCK_POSE, T1)
    for c in range(2):
        assert est.map_add_parameter_block(3 + c, est.BLOCK_POSE, g["T_SC"][c]) and est.set_parameter_block_constant(3 + c)
    for l in range(len(lm)):
        assert est.map_add_parameter_block(10 + l, est.BLOCK_HOMOGENEOUS_POINT, np.r_[lm[l], 1.0])
        for f, pose in enumerate((1, 2)):
            for c in range(2):
                assert est.map_add_reprojection_error(pose, 10 + l, 3 + c, c, g["uv"][f, c, l], info) != 0
    return est
