"""The reference and the scripts of tests/test_gpu_resident_edges.py, without a GPU: every script of helpers/resident_cases.py reaches
the edge it states (asserted by the model on the script alone), the model of helpers/resident_model.py answers hand-written
sequences with the arrays written out here, and its obs_order rule refuses an order that is sorted but not stable."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "helpers"))
import resident_cases as rc        # noqa: E402
import resident_model as rm        # noqa: E402


def all_scenarios():
    out = [("A-%d-%s" % hp, lambda hp=hp: rc.handle_sweep(*hp)) for hp in rc.handle_cases()]
    out += [("B", rc.delta_edges), ("C-staging", rc.staging_boundary)]
    out += [("C-rig_v2-L%d" % L, lambda L=L: rc.order_small(L)) for L in rc.ORDER_SMALL]
    out += [("D-L%d" % L, lambda L=L: rc.marg_gather(L)) for L in rc.GATHER_COUNTS]
    return out


@pytest.mark.parametrize("name, make", all_scenarios(), ids=[n for n, _ in all_scenarios()])
def test_every_script_reaches_its_edge(name, make):
    sc = make()
    trace = rc.Runner(sc).run()
    assert trace and sc.edge
    sc.expect(trace)


def test_the_sweep_visits_the_scan_edges():
    """the handle counts of sweep A against the arithmetic of the scan: one wave of work, 1 023 | 1 024 | 1 025 and 2 048 | 2 049
    (per 1 -> 2 -> 3), the first trailing threads and whole waves without a range"""
    assert len(rc.handle_cases()) == 3 * len(rc.HANDLE_COUNTS) - 1
    stats = {H: rm.scan_ranges(H, np.ones(H, int)) for H in rc.HANDLE_COUNTS}
    assert [stats[H]["per"] for H in (1023, 1024, 1025, 2048, 2049, 5000)] == [1, 1, 2, 2, 3, 5]
    assert stats[63]["threads_with_items"] == 63 and stats[63]["empty_waves"] == 15
    assert stats[1024]["threads_with_items"] == 1024 and stats[1024]["empty_waves"] == 0
    assert stats[1025]["threads_with_items"] == 513 and stats[1025]["empty_waves"] == 7     # the first whole waves without a range
    assert stats[2047]["threads_with_items"] == 1024 and stats[2047]["hi"][1023] - stats[2047]["lo"][1023] == 1   # a short last range
    assert stats[2049]["threads_with_items"] == 683 and stats[2049]["empty_waves"] == 5
    # every seventh handle at per = 1: runs of six threads that sum to zero inside every wave
    r = rm.scan_ranges(1024, (np.arange(1024) % 7 == 0).astype(int))
    assert r["zero_threads"] == 1024 - 147
    # the two ends only: fourteen waves that sum to zero between two that do not
    flags = np.zeros(5000, int)
    flags[rc.observed_handles(5000, "ends")] = 1
    r = rm.scan_ranges(5000, flags)
    assert r["per"] == 5 and r["threads_with_items"] == 1000 and r["zero_waves"] == 14 and int(r["thread_sums"].sum()) == 10


def small_model():
    m = rm.ResidentModel()
    m.add_landmark(10, [1.0, 2.0, 3.0, 1.0])
    m.add_landmark(11, [4.0, 5.0, 6.0, 1.0])           # never observed
    m.add_landmark(12, [7.0, 8.0, 9.0, 1.0])
    m.add_observation(12, 0, 1, 0, [5.0, 6.0], 8.0)
    m.add_observation(10, 0, 0, 0, [1.0, 2.0], 8.0)
    m.add_observation(10, 1, 0, 0, [3.0, 4.0], 4.0)
    return m


def test_model_on_a_hand_written_sequence():
    m = small_model()
    e = m.expected()
    assert (e["L"], e["N"], e["ids"]) == (2, 3, [10, 12])
    assert e["lm_ptr"].tolist() == [0, 2, 3] and e["obs_lm"].tolist() == [0, 0, 1]
    assert e["uv"].tolist() == [[1.0, 2.0], [3.0, 4.0], [5.0, 6.0]]
    assert e["w"].tolist() == [1.0, 2.0, 1.0]                    # sqrt(64 / 8^2), sqrt(64 / 4^2)
    assert e["lm"].tolist() == [[1.0, 2.0, 3.0, 1.0], [7.0, 8.0, 9.0, 1.0]]
    assert e["frame"].tolist() == [0, 1, 0] and e["cam"].tolist() == [0, 0, 1]
    f = m.end_flush()
    assert f["full"] and f["n_adds"] == 3 and f["adds"] == {12: [0], 10: [1, 2]}
    # a constant landmark, a landmark set by the host, an observation on the unobserved landmark, the first of a segment removed
    m.set_constant(12, True)
    m.set_landmark(10, [1.5, 2.0, 3.0, 1.0])
    m.add_observation(11, 1, 1, 0, [9.0, 9.5], 16.0)
    m.remove_observation(10, 0, 0, 0)
    e = m.expected()
    assert e["ids"] == [10, 11, 12] and e["lm_ptr"].tolist() == [0, 1, 2, 3]
    assert e["uv"].tolist() == [[3.0, 4.0], [9.0, 9.5], [5.0, 6.0]] and e["w"].tolist() == [2.0, 0.5, -1.0]
    assert e["lm"][0].tolist() == [1.5, 2.0, 3.0, 1.0]
    f = m.end_flush()
    assert not f["full"] and not f["values_only"] and f["removed"] == {10: [(0, 2)]} and f["const_changes"] == 1
    # withdrawn before it was flushed; then nothing at all
    m.add_observation(10, 2, 0, 0, [0.0, 0.0], 8.0)
    m.remove_observation(10, 2, 0, 0)
    f = m.end_flush()
    assert f["withdrawn"] == 1 and f["n_adds"] == 1 and not f["removed"] and not f["values_only"]
    m.set_constant(12, False)
    assert m.end_flush()["values_only"] and m.expected()["w"].tolist() == [2.0, 0.5, 1.0]


def csr_of(m, pose_slot, order=None):
    """a debug_csr answer made from the model's own arrays with the given frame -> pose slot map"""
    e = m.expected()
    idx = np.array([pose_slot[f] | (0 << 12) | (c << 24) for f, c in zip(e["frame"].tolist(), e["cam"].tolist())], np.uint32)
    out = dict(L=e["L"], N=e["N"], lm_ptr=e["lm_ptr"], obs_lm=e["obs_lm"], obs_idx=idx, uv=e["uv"], w=e["w"], lm=e["lm"])
    out["obs_order"] = np.full(e["N"], -1, np.int32) if order is None else np.asarray(order, np.int32)
    return out


def test_model_checks_a_csr_and_its_slot_rule():
    m = small_model()
    good = csr_of(m, {0: 0, 1: 1})
    assert m.check_csr(good) is False                       # (all -1: no order wanted)
    for key, bad in (("lm_ptr", np.array([0, 1, 3], np.int32)), ("obs_lm", np.array([0, 1, 1], np.int32)),
                     ("w", np.array([1.0, -2.0, 1.0])), ("uv", good["uv"][::-1].copy()), ("lm", good["lm"][::-1].copy())):
        with pytest.raises(AssertionError):
            m.check_csr(dict(good, **{key: bad}))
    with pytest.raises(AssertionError, match="camera"):
        m.check_csr(dict(good, obs_idx=good["obs_idx"] ^ np.uint32(1 << 24)))
    with pytest.raises(AssertionError, match="share a slot"):
        m.check_csr(csr_of(m, {0: 0, 1: 0}))
    assert m.check_csr(csr_of(m, {0: 0, 1: 0}), constant_frames=[1]) is False     # a pose without a block may sit anywhere
    two = good["obs_idx"].copy()
    two[2] |= 1                                              # frame 0 under two slots
    with pytest.raises(AssertionError, match="pose slots"):
        m.check_csr(dict(good, obs_idx=two))


def test_obs_order_rule_refuses_a_sorted_but_unstable_order():
    rng = np.random.Generator(np.random.PCG64(5))
    L, n_pose = 37, 6                                        # two chunks and a partial one
    cnt = rng.integers(1, 9, L)
    lm_ptr = np.r_[0, np.cumsum(cnt)].astype(np.int32)
    N = int(lm_ptr[-1])
    idx = (rng.integers(0, n_pose, N) | (rng.integers(0, 2, N) << 24)).astype(np.uint32)
    good = rm.expected_obs_order(idx, lm_ptr)
    assert rm.check_obs_order(idx, lm_ptr, good) is True
    assert rm.check_obs_order(idx, lm_ptr, np.full(N, -1, np.int32)) is False
    pose = idx & 0xfff
    for c in range(3):                                       # written out: sorted by pose inside the chunk, ties in index order
        seg = good[lm_ptr[16 * c]:lm_ptr[min(L, 16 * c + 16)]]
        assert sorted(seg.tolist()) == list(range(lm_ptr[16 * c], lm_ptr[min(L, 16 * c + 16)]))
        key = list(zip(pose[seg].tolist(), seg.tolist()))
        assert key == sorted(key)
    # the same chunks walked backwards: still sorted by pose, ties reversed
    unstable = good.copy()
    for c in range(3):
        beg, end = int(lm_ptr[16 * c]), int(lm_ptr[min(L, 16 * c + 16)])
        rev = np.arange(end - 1, beg - 1, -1)
        unstable[beg:end] = rev[np.argsort(pose[rev], kind="stable")]
    assert np.all(np.diff(pose[unstable[:lm_ptr[16]]].astype(int)) >= 0) and not np.array_equal(unstable, good)
    with pytest.raises(AssertionError, match="stable"):
        rm.check_obs_order(idx, lm_ptr, unstable)
    # one tie swapped
    one = good.copy()
    k = int(np.nonzero(pose[good[:-1]] == pose[good[1:]])[0][0])
    one[k], one[k + 1] = one[k + 1], one[k]
    with pytest.raises(AssertionError, match="stable"):
        rm.check_obs_order(idx, lm_ptr, one)
    # sorted over the whole array instead of chunk by chunk; a repeated index
    with pytest.raises(AssertionError, match="stable"):
        rm.check_obs_order(idx, lm_ptr, np.argsort(pose, kind="stable").astype(np.int32))
    twice = good.copy()
    twice[3] = twice[4]
    with pytest.raises(AssertionError, match="permutation"):
        rm.check_obs_order(idx, lm_ptr, twice)


def test_model_marginalisation_on_a_hand_written_window():
    """frames 0 .. 5, frame 0 leaves, 0 .. 3 are outside the IMU window, 3 .. 5 are new (resident_cases.MARG_CALL)"""
    m = rm.ResidentModel()
    tracks = {1: [0, 1], 2: [0], 3: [0, 1, 4], 4: [1, 2], 5: [], 6: [0, 0, 2], 7: [0, 3]}
    for lid, frames in tracks.items():
        m.add_landmark(lid, [float(lid), 0.0, 1.0, 1.0])
        for n, f in enumerate(frames):
            m.add_observation(lid, f, n % 2, 10 * lid + n, [float(lid), float(f)], 8.0)
    m.set_constant(6, True)
    out = m.marginalise(**rc.MARG_CALL[2])
    assert out["removed"] == [1, 2, 5, 6]                     # linearised, single observation, unobserved, linearised (constant)
    assert out["job"] == [(1, [0, 1], False), (6, [0, 0, 2], True)] and out["n_job_obs"] == 5
    assert out["n_removed_obs"] == 5 + 1 + 1 + 1              # the job's, landmark 2's, the leaving ones of landmarks 3 and 7
    e = m.expected()
    assert e["ids"] == [3, 4, 7] and e["frame"].tolist() == [1, 4, 1, 2, 3]
