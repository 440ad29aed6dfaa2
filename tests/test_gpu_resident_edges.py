"""The kernels of the device-resident window (svin_amd/csrc/resident.hip) at their scan, staging and delta edges.

tests/test_gpu_resident.py holds the resident window to the host re-pack through long random sequences; here the reference is the
plain restatement of tests/helpers/resident_model.py -- what the CSR must be from the calls that were made -- and the calls are the
designed scripts of tests/helpers/resident_cases.py, each of which reaches a stated edge (asserted on the script by the model
before any estimator exists: tests/test_resident_cases_host.py does the same without a GPU):

  A  k_window_rebuild phases 0-3, k_window_finish, k_window_store_landmarks: handle ranges of 1 .. 5 000 (one wave of work, the
     workgroup sizes of the per-handle kernels, per = 1 | 2 | 3 handles per thread of the scan) under three occupancies
  B  one flush's delta: many additions to a landmark (phase 3's insertion sort), removals at the ends of a segment, a withdrawn
     addition, a window that loses every observation, flushes that change values only
  C  k_window_order at chunks of 1 024 (the last staged size) and 1 025 observations, and at 1 | 16 | 17 landmarks
  D  k_window_marg_gather over 40 .. 2 049 CSR slots: the marginalisation job gathered on the device against the host-assembled one

Every script runs on a resident estimator and on a host-packed twin (set_pack_mode(1)); each debug_csr of either is held to the
model, array for array, and the two to each other.  The only tolerance is zero."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "helpers"))
import resident_cases as rc        # noqa: E402

from test_gpu_resident import assert_same_csr, same_states   # noqa: E402

pytestmark = pytest.mark.gpu


class GpuRunner(rc.Runner):
    """a = resident, b = host-packed"""

    def __init__(self, sc):
        from svin_amd.estimator import Estimator
        a, b = Estimator(0), Estimator(0)
        b.set_pack_mode(1)
        super().__init__(sc, [a, b])
        self.a, self.b = a, b
        self.csr, self.ordered, self.marg = {}, {}, None

    def checked(self, tag, flush):
        ca, cb = self.a.debug_csr(), self.b.debug_csr()
        assert ca["resident"] and not cb["resident"], tag
        ordered = [self.model.check_csr(c, self.sc.constant_frames, "%s, %s %s" % (self.sc.name, name, tag))
                   for name, c in (("resident", ca), ("host-packed", cb))]
        assert ordered[0] == ordered[1], tag
        self.ordered[tag] = ordered[0]
        assert_same_csr(ca, cb, "%s %s" % (self.sc.name, tag))
        self.csr[tag] = ca

    def landmarks_equal(self, tag):
        la, lb = self.a.get_landmarks(), self.b.get_landmarks()
        assert list(la) == list(lb) == sorted(self.model.lms), tag
        for i in la:
            assert np.array_equal(la[i]["point"], lb[i]["point"]) and la[i]["quality"] == lb[i]["quality"], (tag, i)
            assert la[i]["n_obs"] == lb[i]["n_obs"] == len(self.model.lms[i].obs), (tag, i)
        return la

    def optimized(self, n):
        same_states([self.a, self.b], "%s after optimize(%d)" % (self.sc.name, n))
        la = self.landmarks_equal("%s after optimize(%d)" % (self.sc.name, n))
        for i, lm in self.model.lms.items():
            if not lm.obs or lm.constant:   # a landmark outside the CSR reads back the point it was given, with quality 0
                assert np.array_equal(la[i]["point"], lm.point), i
            if not lm.obs:
                assert la[i]["quality"] == 0.0, i
        self.model.update_points({i: v["point"] for i, v in la.items()})

    def marginalised(self, expected, results, num_kf, num_imu, classes):
        for name, (ok, removed) in zip(("resident", "host-packed"), results):
            assert ok and [int(i) for i in removed] == expected["removed"], "%s: the removed landmarks are not the policy's" % name
        pre = [e.marg_pre() for e in self.ests]
        post = [e.marg() for e in self.ests]
        for name, p in zip(("resident", "host-packed"), pre):
            assert p is not None and p["n_landmarks"] == len(expected["job"]), name
            # the coupling of every job landmark: its rows meet exactly the poses of its linearised observations (none, if constant)
            m = p["m"]
            fid = dict(self.frame_ids)
            fid.update(self.left)
            pose_rows = {k: p["rows_of"][fid[k]] for k in classes["linearised"] if fid[k] in p["rows_of"]}
            for lid, frames, constant in expected["job"]:
                r0, dim = p["rows_of"][lid]
                W = p["H"][:m, r0:r0 + dim]
                seen = {k for k, (o, d) in pose_rows.items() if np.any(W[o:o + d] != 0.0)}
                assert seen == (set() if constant else set(frames)), (name, lid, seen, frames, p["H"][r0:r0 + dim, r0:r0 + dim])
                assert np.any(p["H"][r0:r0 + dim, r0:r0 + dim] != 0.0) == (not constant), (name, lid)
        for key in ("H", "b0"):
            assert np.array_equal(pre[0][key], pre[1][key]), "system after M1: %s differs by %g" % (key, float(np.max(np.abs(pre[0][key] - pre[1][key]))))
            assert np.array_equal(post[0][key], post[1][key]), "prior: %s differs by %g" % (key, float(np.max(np.abs(post[0][key] - post[1][key]))))
        assert [x["id"] for x in post[0]["blocks"]] == [x["id"] for x in post[1]["blocks"]]
        self.marg = dict(expected=expected)

    def do_marginalise(self, num_kf, num_imu, classes):
        self.left = {k: self.frame_ids[k] for k in classes["remove"]}
        super().do_marginalise(num_kf, num_imu, classes)


def run(sc):
    sc.expect(rc.Runner(sc).run())       # the script reaches its edge: asserted by the model before any estimator exists
    r = GpuRunner(sc)
    sc.expect(r.run())
    return r


# ------------------------------------------------------------------------------------------------------------------ A
@pytest.mark.parametrize("H, pattern", rc.handle_cases())
def test_handle_range_sweep(gpu_lib, H, pattern):
    """H landmarks of which some are observed (all / every seventh / the first and last five), one full flush and optimize(2): the
    CSR of both estimators is the model's and the same, the landmarks read back equal, the unobserved ones as they were given"""
    r = run(rc.handle_sweep(H, pattern))
    assert r.a.landmark_handles() == (H, H)      # (5 000 < 8 192: resident and not renumbered)
    pa, pb = r.a.path_counters(), r.b.path_counters()
    assert (pa["resident_solves"], pa["host_pack_solves"], pb["resident_solves"]) == (1, 0, 0)


# ------------------------------------------------------------------------------------------------------------------ B
def test_delta_edges(gpu_lib):
    """one window through fourteen flushes, each with one corner case of the delta (resident_cases.delta_edges)"""
    r = run(rc.delta_edges())
    c = r.csr
    assert c["every observation removed"]["L"] == c["every observation removed"]["N"] == 0 and c["one again"]["N"] == 1
    assert int(np.sum(c["constant set"]["w"] < 0)) == 8 and not np.any(c["constant cleared"]["w"] < 0)
    assert np.array_equal(c["constant cleared"]["w"], c["values only"]["w"]), "the weights come back bit for bit"
    assert np.array_equal(np.abs(c["constant set"]["w"]), c["values only"]["w"])
    pa, pb = r.a.path_counters(), r.b.path_counters()
    print("resident", pa, "host-packed", pb)
    assert pa["host_pack_solves"] == 0 and pa["resident_solves"] == 2 and pb["resident_solves"] == 0 and pb["host_pack_solves"] == 2


# ------------------------------------------------------------------------------------------------------------------ C
def test_pose_order_at_the_staging_boundary(gpu_lib):
    """chunks of 1 024, 1 025 and 528 observations on 33 frames, one of them constant; no solve ahead of the check"""
    r = run(rc.staging_boundary())
    assert r.ordered["full"], "obs_order is all -1: the window did not take the ordered dense form"
    assert len(np.unique(r.csr["full"]["obs_idx"] & 0xfff)) >= 32     # every pose block occurs


@pytest.mark.parametrize("L", rc.ORDER_SMALL)
def test_pose_order_with_variable_extrinsics(gpu_lib, L):
    r = run(rc.order_small(L))
    assert r.ordered["full"], "obs_order is all -1: the window did not take the ordered dense form"
    assert len(np.unique((r.csr["full"]["obs_idx"] >> 12) & 0xfff)) == 8     # an extrinsics block per frame and camera


# ------------------------------------------------------------------------------------------------------------------ D
@pytest.mark.parametrize("L", rc.GATHER_COUNTS)
def test_marginalisation_gather(gpu_lib, debug_option, L):
    """one applyMarginalizationStrategy on L CSR slots of five kinds of landmarks: the removed landmarks, the job's landmark count
    and the coupling of every job landmark are the model's on both estimators; the system after M1 and the prior are equal bit for
    bit between the device-gathered and the host-assembled job; the CSR after the call is the model's again"""
    debug_option("SVIN_MARG_KEEP_PRE", 1)
    r = run(rc.marg_gather(L))
    exp = r.marg["expected"]
    print("L", L, "job landmarks", len(exp["job"]), "of them constant", sum(1 for j in exp["job"] if j[2]), "job observations", exp["n_job_obs"],
          "removed landmarks", len(exp["removed"]), "observations gone", exp["n_removed_obs"])
    assert r.csr["before"]["N"] - r.csr["after"]["N"] == exp["n_removed_obs"] >= exp["n_job_obs"] > 0
    pa, pb = r.a.path_counters(), r.b.path_counters()
    assert (pa["device_gathered_marginalisations"], pa["host_assembled_marginalisations"], pa["host_pack_solves"]) == (1, 0, 0)
    assert (pb["device_gathered_marginalisations"], pb["host_assembled_marginalisations"], pb["resident_solves"]) == (0, 1, 0)
