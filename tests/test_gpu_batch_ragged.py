"""Windows of DIFFERENT landmark and observation counts through one launch sequence (svin_ba_solve_prepared_batch; batch_plan.hpp):
what the front end decides anew every frame -- how many landmarks, how many observations -- does not separate the windows of a
fleet, only what the launcher computes once per launch does (reduced system, factors, prior, cameras).  Every window brings the
extent of each launch in its slot; the grid is the largest extent of the lane, a block beyond its window's extent leaves at once.

The yardstick is the product's own single-window path, as in test_gpu_batch.py: every window of a batch ends BIT FOR BIT where
optimize() alone leaves it -- its blocks have the roles, its partial sums the indices and the order of its own launches -- with
the same iteration and step counts, whatever its partners, its position in the call and the number of lanes."""
import numpy as np
import pytest

from svin_amd import synthetic as syn

pytestmark = pytest.mark.gpu


def states_of(est, fids, lids):
    T = np.stack([est.get_T_WS(f) for f in fids])
    sb = np.stack([v if v is not None else np.full(9, np.nan) for v in (est.get_speed_and_bias(f) for f in fids)])   # (old keyframes of a sliding window keep their pose only)
    lms = est.get_landmarks()
    lids = [l for l in lids if l in lms]   # (the generator keeps a landmark only if an observation of it survived the draw)
    lm = np.stack([np.r_[lms[l]["point"], lms[l]["quality"]] for l in lids])
    return T, sb, lm


def build(seed, **kw):
    from svin_amd.estimator import Estimator
    spec = syn.make_window(seed=seed, **kw)
    est = Estimator(0)
    fids, lids = syn.feed(est, spec)
    return est, fids, lids


SUMMARY_KEYS = ("iterations", "successful", "termination", "initial_cost", "final_cost")


def assert_same(est, fids, lids, ref, s_ref, tag):
    s = est.summary()
    assert tuple(s[k] for k in SUMMARY_KEYS) == tuple(s_ref[k] for k in SUMMARY_KEYS), (tag, s, s_ref)
    for a, b, name in zip(states_of(est, fids, lids), ref, ("poses", "speed / bias", "landmarks and quality")):
        assert np.array_equal(a, b, equal_nan=True), "%s: %s differ by %.3e" % (tag, name, float(np.nanmax(np.abs(a - b))))


# P = 6 throughout: 6 poses + 2 extrinsics + 6 speed / bias blocks = 14 parameter blocks in front of the landmarks in the
# retraction's item table.  (L, n_obs) with seeds for which every landmark keeps an observation, so that the packed counts are
# the requested ones (asserted from svin_ba_debug_csr below):
EDGES = [dict(seed=101, L=16, n_obs=129),     # ONE landmark chunk, 16 k;  N = 128 + 1
         dict(seed=108, L=17, n_obs=150),     # 16 k + 1: a second chunk of one landmark
         dict(seed=102, L=400, n_obs=4097),   # 16 k near 400;  N = 256 k + 1
         dict(seed=103, L=401, n_obs=4096),   # 16 k + 1;  N = 256 k
         dict(seed=104, L=242, n_obs=2560),   # 14 + L = 256: the last full table block;  N = 256 k
         dict(seed=105, L=243, n_obs=2561),   # 14 + L = 257: one item into the next;  N = 256 k + 1 = 128 k + 1
         dict(seed=106, L=250, n_obs=2500),   # a pair of identical counts
         dict(seed=107, L=250, n_obs=2500)]
N_ITER = 8


@pytest.fixture(scope="module")
def edges_alone(gpu_lib):
    """every window of EDGES optimised on its own, once for the tests of this file: (packed L, packed N, states, summary)"""
    out = []
    for c in EDGES:
        est, fids, lids = build(P=6, **c)
        est.optimize(N_ITER)
        ref, summary = states_of(est, fids, lids), est.summary()
        csr = est.debug_csr()   # (afterwards: the handle that sets the yardstick does nothing a plain optimize() does not do)
        out.append((csr["L"], csr["N"], ref, summary))
    return out


def run_batch(order, alone, tag):
    from svin_amd import estimator
    batch = [build(P=6, **EDGES[k]) for k in order]
    assert estimator.optimize_batch([b[0] for b in batch], N_ITER) == len(order), tag
    for k, (est, fids, lids) in zip(order, batch):
        assert_same(est, fids, lids, alone[k][2], alone[k][3], "%s, window %d" % (tag, k))


def test_edges_of_every_extent_in_one_group(gpu_lib, edges_alone):
    """eight windows of one fleet whose counts straddle the boundary of every grid expression: landmark chunks of 16 (build,
    post-solve pass), observation blocks of 256 (evaluation) and 128, table blocks of 256 (retraction).  Before the extents were
    per window each distinct count tuple was a group of its own and only the identical pair was batched."""
    from svin_amd.estimator import Estimator
    Ls, Ns = [a[0] for a in edges_alone], [a[1] for a in edges_alone]
    assert Ls == [c["L"] for c in EDGES] and Ns == [c["n_obs"] for c in EDGES], (Ls, Ns)
    assert 16 in Ls and any(l % 16 == 0 and l > 16 for l in Ls) and sum(l % 16 == 1 for l in Ls) >= 2     # L on 16 k and 16 k + 1
    assert min(Ls) <= 16 and any(385 <= l <= 416 for l in Ls)                                              # one chunk; one near 400
    assert any(n % 256 == 0 for n in Ns) and any(n % 256 == 1 for n in Ns) and any(n % 128 == 1 for n in Ns)
    tables = sorted(-(-(14 + l) // 256) for l in Ls)
    assert tables[0] < tables[-1] and 14 + 242 == 256 and 242 in Ls and 243 in Ls                          # the table blocks cross 256
    assert len(set(zip(Ls, Ns))) == len(EDGES) - 1                                                         # exactly one identical pair
    run_batch(list(range(len(EDGES))), edges_alone, "call order")
    idle = Estimator.debug_get_option("SVIN_LAST_BATCH_IDLE_PPM")
    assert 0 < idle < 1000000, idle   # windows of 16 and of 401 landmarks shared lanes: some blocks were launched for nothing


def test_partner_and_position_independence(gpu_lib, edges_alone, debug_option):
    """the same eight windows in another order of the call and with one lane instead of four: other partners in a lane, another
    blockIdx.y, another grid above every window -- the same bits"""
    other = [5, 0, 7, 2, 4, 1, 6, 3]
    for lanes, order in ((4, other), (1, list(range(len(EDGES)))), (1, other)):
        debug_option("SVIN_BATCH_LANES", lanes)
        run_batch(order, edges_alone, "%d lanes, order %s" % (lanes, order))


def test_ragged_batch_with_rejected_steps_and_early_termination(gpu_lib):
    """windows of different sizes whose trust regions go different ways: badly perturbed starts (rejected steps: the round's
    k_step_retract launch, whose grid follows the table blocks), a nearly converged one (terminates early and sits out the
    remaining rounds, so the lane's grids shrink to the windows still taking part)"""
    from svin_amd import estimator
    cfgs = [dict(seed=71, L=120, pose_noise=(0.6, 0.15), lm_noise=1.5), dict(seed=72, L=250, pose_noise=(1.0, 0.25), lm_noise=2.5),
            dict(seed=73, L=330, pose_noise=(1.5, 0.4), lm_noise=4.0), dict(seed=74, L=90, pose_noise=(1e-6, 1e-6), lm_noise=1e-6, pixel_noise=1e-3)]
    cfgs = [dict(c, P=6, n_obs=10 * c["L"]) for c in cfgs]
    alone = []
    for c in cfgs:
        est, fids, lids = build(**c)
        est.optimize(25)
        alone.append((states_of(est, fids, lids), est.summary()))
    its = [a[1]["iterations"] for a in alone]
    assert any(a[1]["successful"] < a[1]["iterations"] for a in alone), "no rejected step: raise the perturbation"
    assert min(its) < max(its), its
    batch = [build(**c) for c in cfgs]
    assert estimator.optimize_batch([b[0] for b in batch], 25) == len(cfgs)
    for k, (est, fids, lids) in enumerate(batch):
        assert_same(est, fids, lids, alone[k][0], alone[k][1], "window %d" % k)


def test_ragged_batch_of_sliding_windows_with_marginalisation_priors(gpu_lib):
    """windows in SVIn's operating mode -- fed frame by frame, optimised and marginalised after every frame, each with a
    marginalisation prior -- that saw different numbers of landmarks.  Three handles per size take the identical history; before
    the last optimisation two of them go into the batch, the third is optimised alone.  All six are ONE group: the priors have
    equal size (asserted), the landmark counts do not matter."""
    from svin_amd import estimator
    from svin_amd.estimator import Estimator

    def history(seed, L):
        spec = syn.make_window(P=9, L=L, n_obs=10 * L, seed=seed, keyframe_every=2, frame_dt=0.3)
        est = Estimator(0)

        def on_frame(k, fid):
            if k < spec.P - 1:
                est.optimize(6)
                est.apply_marginalization(3, 2)
        fids, lids = syn.feed(est, spec, on_frame=on_frame)
        est.wait_idle()
        return est, est.frame_ids(), [l for l in lids if l in est.get_landmarks()]

    sizes = [(11, 600), (12, 520), (13, 450)]
    alone = [history(*c) for c in sizes]
    batch = [history(*c) for c in sizes for _ in range(2)]
    for k, (b, fb, lb) in enumerate(batch):
        a, fa, la = alone[k // 2]
        assert a.marg() is not None and fa == fb and la == lb
        for x, y in zip(states_of(a, fa, la), states_of(b, fb, lb)):
            assert np.array_equal(x, y, equal_nan=True), "the histories of a seed differ before the batch"
    priors = [a.marg()["n"] for a, _, _ in alone]
    assert len(set(priors)) == 1, "the priors differ in size: choose seeds for which they agree (%s)" % priors
    assert len({len(la) for _, _, la in alone}) == len(sizes), "the windows are meant to differ in their landmark counts"
    for a, _, _ in alone:
        a.optimize(8)
    assert estimator.optimize_batch([b[0] for b in batch], 8) == len(batch)
    for k, (b, fb, lb) in enumerate(batch):
        a, fa, la = alone[k // 2]
        assert_same(b, fb, lb, states_of(a, fa, la), a.summary(), "window %d" % k)
