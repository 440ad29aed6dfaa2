"""The accumulator ledger and the plan of a pass of Window::solve (svin_amd/csrc/iteration_plan.hpp) on the CPU, through
tests/csrc/iteration_plan_shim.cpp: the loop of solve() with the launches left out, driven by the real TrustRegionHost through
every sequence of six per-pass events (the factorisation fails, a step is accepted and leaves the damping a speculative build
assumes, accepted and leaves another, rejected, invalid, the solve terminates) -- every shorter sequence is a prefix of one.

1. Soundness.  A model that knows nothing of the ledger interprets what every pass enqueues: the accumulators are a multiset of
   builds (point, mu, initScale); a build that zeroes first replaces it, any other adds to it, the post-solve pass empties it, an
   accepted step renames the point.  In front of every reduced solve the multiset must be exactly {(current point, mu, initScale)}.
   Four planted defects, applied to the launch list, must each fail that.
2. Equivalence.  The six locals Window::solve kept before the ledger, transcribed once, give the same launches, zeroFirst flags
   and hit / miss counts.
3. The batched round.  A window of a batched solve plans its passes with the same planPass (one GPU, no speculation, no
   k_eval_build, a ledger of its own, no build behind the initial evaluation); the stages of its round (batchStagesOf) and the
   slot's lmDeferred must be the expressions Window::solveBatchGroup wrote out by hand before, its build {launch, no zeroing}.
4. The same cases through a stand-alone program under AddressSanitizer and UndefinedBehaviorSanitizer
   (tests/csrc/iteration_plan_sanitize.cpp), whose answers must be the shim's.

Everything is evaluated for all 6^6 sequences of a configuration at once: arrays of shape (sequences, passes)."""
import ctypes as C
import itertools
import os
import subprocess

import numpy as np
import pytest

from helpers import iteration_plan_lib as ip
from helpers.iteration_plan_lib import (ACCEPTED, BATCH_EVAL, BATCH_FULL, BATCH_REUSE, BATCHED, BUILD, CALLBACK, FIELDS,   # noqa: F401
                                        INVALID, NATIVE, ONE_GPU, REJECTED, RETRY, STALE, ZERO)

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
N_PASS, N_EVENTS = 6, 6


def configurations():
    """(strategy, SVIN_NO_SPECULATION, SVIN_NO_EVAL_BUILD, mode, numIter, stepInEvalTaken's answer); Levenberg-Marquardt has no
    sharded mode (solve() refuses it)"""
    out = []
    for lm, no_spec, no_eval_build, mode, num_iter in itertools.product((0, 1), (0, 1), (0, 1), (ONE_GPU, NATIVE, CALLBACK), (0, 1, 2, 6)):
        if lm and mode != ONE_GPU:
            continue
        for head in ((0, 1) if mode == ONE_GPU and not no_spec and num_iter > 1 else (0,)):
            out.append((lm, no_spec, no_eval_build, mode, num_iter, head))
    return out


def batched_configurations():
    """a window of a batched solve: dogleg, one GPU, SVIN_NO_SPECULATION set, no k_eval_build; the step mode of the shim's window
    is the fused step with the landmarks deferred, which batchSupported requires"""
    return [(0, 1, 1, BATCHED, num_iter, 0) for num_iter in (0, 1, 2, 6)]


@pytest.fixture(scope="module")
def lib(tmp_path_factory):
    return ip.build_shim(tmp_path_factory.mktemp("iteration_plan"))


def run_all(lib, cfg):
    """{field: array (6^6, 6)} of every sequence of the configuration"""
    c = np.array(cfg, np.int32)
    rows = np.zeros((N_EVENTS ** N_PASS, N_PASS, len(FIELDS)))
    lib.ip_run_all(c.ctypes.data_as(C.c_void_p), N_PASS, rows.ctypes.data_as(C.c_void_p))
    return {name: rows[:, :, k] for k, name in enumerate(FIELDS)}


@pytest.fixture
def runs(lib):
    """(configuration, its rows), one at a time: a configuration's rows are some 50 MB"""
    return ((cfg, run_all(lib, cfg)) for cfg in configurations())


def first_build(cfg):
    return cfg[3] == ONE_GPU and cfg[4] > 0   # enqueued behind the initial evaluation: one GPU, an iteration to use it


# ------------------------------------------------------------------------------------------------ 1. the model
def model(cfg, r, launch=None, zero_first=None):
    """The accumulators as a multiset of builds.  Its size is tracked exactly up to 2 (more is as wrong as 2); where it is 1 the
    build in it is the last one added.  Returns (ok, kept): ok[q, k] -- pass k of sequence q found exactly its own build in front of
    its solve, or had no solve; kept[q, k] -- that build was not launched by the pass itself."""
    launch = r["launch"] if launch is None else launch
    zero_first = r["zeroFirst"] if zero_first is None else zero_first
    nq = r["alive"].shape[0]
    count = np.full(nq, 1 if first_build(cfg) else 0)
    point, mu, init = np.zeros(nq), np.full(nq, r["mu"][:, 0] if first_build(cfg) else 0.0), np.full(nq, 1.0)
    current = np.zeros(nq)   # id of the current point; the candidate of pass k is point k + 1
    ok = np.ones(r["alive"].shape, bool)

    def add(where, zero, p, m, i):
        nonlocal count, point, mu, init
        count = np.where(where, np.where(zero, 1, np.minimum(count + 1, 2)), count)
        point, mu, init = np.where(where, p, point), np.where(where, m, mu), np.where(where, i, init)

    for k in range(N_PASS):
        alive, solve = r["alive"][:, k] > 0, r["solve"][:, k] > 0
        add(alive & solve & (launch[:, k] > 0), zero_first[:, k] > 0, current, r["mu"][:, k], r["initScale"][:, k])
        exact = (count == 1) & (point == current) & (mu == r["mu"][:, k]) & (init == r["initScale"][:, k])
        ok[:, k] = ~(alive & solve) | exact
        count = np.where(alive & solve, 0, count)   # the post-solve pass
        add(alive & (r["specWanted"][:, k] > 0), False, k + 1.0, r["specMu"][:, k], 0.0)
        current = np.where(alive & (r["end"][:, k] == ACCEPTED), k + 1.0, current)
    return ok, (r["alive"] > 0) & (r["solve"] > 0) & ~(launch > 0)


def test_every_reduced_solve_finds_exactly_its_own_build(runs):
    solves = kept_spec = 0
    for cfg, r in runs:
        ok, _ = model(cfg, r)
        assert ok.all(), (cfg, np.argwhere(~ok)[0])
        solves += int(((r["alive"] > 0) & (r["solve"] > 0)).sum())
        kept_spec += int(r["hitsIfClosed"][:, -1].sum())
    assert solves > 10 ** 6 and kept_spec > 10 ** 4   # the sweep solves, and keeps speculative builds


def test_counters_count_the_speculative_builds(runs):
    """hits + misses = speculative builds enqueued, wherever the solve ends; a hit exactly when a pass kept a build that is not the first one"""
    for cfg, r in runs:
        alive = r["alive"] > 0
        enqueued = np.cumsum(alive & (r["specWanted"] > 0), axis=1)
        assert np.array_equal((r["hitsIfClosed"] + r["missesIfClosed"])[alive], enqueued[alive]), cfg
        _, kept = model(cfg, r)
        if first_build(cfg):
            kept[:, 0] = False   # (pass 0 can only keep the first build: nothing speculative exists yet)
        assert np.array_equal(r["hitsIfClosed"][alive], np.cumsum(kept, axis=1)[alive]), cfg
        if cfg[1]:
            assert not r["specWanted"].any() and not r["hitsIfClosed"].any() and not r["missesIfClosed"].any()


def previous(a, fill=0.0):
    return np.concatenate([np.full((a.shape[0], 1), fill), a[:, :-1]], axis=1)


def stale_speculative(r):
    """passes whose build zeroes first: what the accumulators hold is a build nobody can keep"""
    return (r["alive"] > 0) & (r["launch"] > 0) & (r["zeroFirst"] > 0)


@pytest.mark.parametrize("defect", ["never zero first", "keep a speculative build after a rejected step", "keep the first build after a mu retry",
                                    "keep a speculative build whose initScale differs"])
def test_model_rejects_planted_defects(runs, defect):
    caught = 0
    for cfg, r in runs:
        launch, zero_first = r["launch"].copy(), r["zeroFirst"].copy()
        if defect == "never zero first":
            hit = zero_first > 0
            zero_first[:] = 0
        else:
            if defect == "keep a speculative build after a rejected step":
                # the first build behind a rejected step (dogleg: behind the re-used linearisations that follow it) with that pass's
                # speculative build still in the accumulators
                rejected_before = np.zeros(r["alive"].shape, bool)
                pending = np.zeros(r["alive"].shape[0], bool)
                for k in range(N_PASS):
                    rejected_before[:, k] = pending
                    pending = np.where(r["solve"][:, k] > 0, False, pending)
                    pending = pending | ((r["end"][:, k] == REJECTED) & (r["specWanted"][:, k] > 0))
                hit = stale_speculative(r) & rejected_before
            elif defect == "keep the first build after a mu retry":
                hit = np.zeros(r["alive"].shape, bool)
                if first_build(cfg):
                    hit[:, 1] = (r["alive"][:, 1] > 0) & (r["end"][:, 0] == RETRY)
            else:   # a build with initScale where the speculative build (never with it) of the pass before is held
                hit = stale_speculative(r) & (r["initScale"] > 0) & (previous(r["specWanted"]) > 0)
            launch[hit] = 0
        if hit.any():
            ok, _ = model(cfg, r, launch, zero_first)
            assert not ok[hit.any(axis=1)].all(axis=1).any(), cfg   # every sequence the defect touches fails
            caught += int(hit.any(axis=1).sum())
    assert caught > 0, "the sweep never reaches the defect"


# ------------------------------------------------------------------------------------------------ 2. the six locals of before
def six_locals(cfg, r):
    """Window::solve's bookkeeping before the ledger -- firstBuilt, firstMu, accumulatorsClean, specValid, specMu, specPending.on --
    statement by statement, for all sequences at once (x = where(condition, value, x) for `if (condition) x = value`)."""
    lm, no_spec, no_eval_build, mode, num_iter, _ = cfg
    dist, dist_native = mode != ONE_GPU, mode == NATIVE
    nq = r["alive"].shape[0]
    false = np.zeros(nq, bool)
    speculate = (not no_spec) and (not dist or dist_native)
    first_built = np.full(nq, (not dist) and num_iter > 0)
    first_mu = r["mu"][:, 0]
    clean, spec_valid, spec_mu, pending = ~false, false, np.zeros(nq), false
    hits, misses = np.zeros(nq), np.zeros(nq)
    out = {k: np.zeros(r["alive"].shape) for k in ("launch", "zeroFirst", "specWanted", "hitsIfClosed", "missesIfClosed")}
    for k in range(N_PASS):
        alive, fresh = r["alive"][:, k] > 0, r["reuse"][:, k] == 0
        mu, init_scale, end = r["mu"][:, k], r["initScale"][:, k] > 0, r["end"][:, k]
        f = alive & fresh                                             # if (!tr.reuse) {
        have_first = first_built & init_scale & (mu == first_mu)
        clean = np.where(f & first_built & ~have_first, False, clean)
        first_built = np.where(f, False, first_built)
        spec_kept = ~have_first & spec_valid & (spec_mu == mu) & ~init_scale
        hits, misses = hits + (f & pending & spec_kept), misses + (f & pending & ~spec_kept)
        pending = np.where(f, False, pending)
        out["launch"][:, k] = f & ~have_first & ~spec_kept
        out["zeroFirst"][:, k] = f & ~have_first & ~spec_kept & ~clean
        spec_valid = np.where(f, False, spec_valid)
        clean = np.where(f, True, clean)                              #   (launchDoglegPrepare) }
        wanted = alive & speculate & clean & (r["iteration"][:, k] < num_iter)   # specBuildWanted
        spec_mu = np.where(wanted, r["specMu"][:, k], spec_mu)        # (tr.muAfterAccept(): the shim's record of it)
        clean, spec_valid, pending = np.where(wanted, False, clean), np.where(wanted, True, spec_valid), np.where(wanted, True, pending)
        spec_valid = np.where(alive & np.isin(end, (RETRY, INVALID, REJECTED)), False, spec_valid)
        out["specWanted"][:, k] = wanted
        out["hitsIfClosed"][:, k], out["missesIfClosed"][:, k] = np.where(alive, hits, 0), np.where(alive, misses + pending, 0)   # ~SpecPending
    return out


def test_same_launches_as_the_six_locals_of_before(runs):
    for cfg, r in runs:
        old = six_locals(cfg, r)
        for name, was in old.items():
            assert np.array_equal(was, r[name]), (cfg, name, np.argwhere(was != r[name])[0])


# ------------------------------------------------------------------------------------------------ the rest of the pass
def test_pass_fields_follow_the_loop_they_replace(runs):
    for cfg, r in runs:
        lm, no_spec, no_eval_build, mode, num_iter, head = cfg
        dist = mode != ONE_GPU
        fuse = defer = not dist   # (the shim's window: stepModeOf gives the fused step with the landmarks deferred on one GPU)
        alive, fresh = r["alive"] > 0, r["reuse"] == 0
        assert np.array_equal(r["solve"] > 0, alive & fresh)
        assert np.array_equal(r["allReduceSystem"] > 0, alive & fresh & dist)
        assert np.array_equal(r["prepareRadius"][alive], np.where(fresh & fuse, r["stepRadius"], -1.0)[alive])
        assert np.array_equal(r["doglegStep"] > 0, alive & (~fresh | (not fuse)))
        assert np.array_equal(r["lmDeferredPost"] > 0, alive & fresh & defer)
        assert np.array_equal(r["lmDeferredEval"] > 0, alive & fresh & defer)
        eval_build = not dist and not no_spec
        assert np.array_equal(r["specInEval"] > 0, (r["specWanted"] > 0) & eval_build)
        assert np.array_equal(r["stepInEval"] > 0, alive & fresh & bool(head) & eval_build & (r["iteration"] < num_iter))
        assert not ((r["stepInEval"] > 0) & ~(r["specInEval"] > 0)).any()   # the step is never left to a build that is not enqueued
        if lm:
            assert fresh[alive].all() and np.isinf(r["stepRadius"][alive]).all()
        if num_iter == 0:
            assert not alive.any()


def test_ledger_keeps_exactly_the_build_asked_for(lib):
    """need() on every state, the unreachable ones too: kept only as kBuild on the current point with the asked mu and initScale"""
    for contents, held_init, on_cand, pending, ask_init in itertools.product((ZERO, BUILD, STALE), (0, 1), (0, 1), (0, 1), (0, 1)):
        for held_mu, ask_mu in ((1e-8, 1e-8), (1e-8, 1e-7)):
            state, out = np.array([contents, held_init, on_cand, pending], np.int32), np.zeros(4, np.int32)
            lib.ip_need(state.ctypes.data_as(C.c_void_p), held_mu, ask_mu, ask_init, out.ctypes.data_as(C.c_void_p))
            kept = contents == BUILD and not on_cand and held_mu == ask_mu and held_init == ask_init
            assert list(out) == [not kept, (not kept) and contents != ZERO, int(bool(pending) and kept), int(bool(pending) and not kept)]
    for contents, speculate, iteration in itertools.product((ZERO, BUILD, STALE), (0, 1), (0, 1, 2, 3)):
        assert lib.ip_spec_wanted(contents, speculate, iteration, 2) == int(bool(speculate) and contents == ZERO and iteration < 2)


def test_replay_of_an_iteration_log_counts_as_the_loop_does(lib):
    """ip_replay (what tests/test_gpu_solve_loop.py holds the device's counters against) on logs written out by hand: rows of
    (cost, rho, radius after, step norm, mu used, outcome 0 accepted / 1 rejected / 2 invalid)"""
    A, R, I = 0.0, 1.0, 2.0
    # dogleg, five iterations allowed: accepted (its build is kept by iteration 2), rejected, the re-used linearisation accepted (no
    # build behind its pass: the accumulators still hold the rejected step's), accepted (its build is pending when the log ends)
    log = [[9, .9, 1e4, 1, 1e-8, A], [9, -1, 5e3, 1, 1e-8, R], [8, .9, 5e3, 1, 1e-8, A], [7, .9, 5e3, 1, 1e-8, A]]
    assert ip.replay(lib, log, "dogleg", 0, 5) == (1, 2, 4)
    assert ip.replay(lib, log, "dogleg", 0, 4) == (1, 1, 4)      # the last iteration of a solve enqueues none
    assert ip.replay(lib, log, "dogleg", 1, 5) == (0, 0, 4)
    assert ip.replay(lib, log, "dogleg", 0, 5, terminated_pass=True) == (2, 1, 5)
    # the mu ladder: iteration 2 starts at 1e-8 and is solved at 1e-6 -- two passes end in a retry, each with a build for nothing
    log = [[9, .9, 1e4, 1, 1e-8, A], [8, .9, 1e4, 1, 1e-6, A], [7, .9, 1e4, 1, 2e-7, A]]
    assert ip.replay(lib, log, "dogleg", 0, 9) == (2, 3, 5)
    # an invalid step: the next iteration is built with ten times the damping, the speculative build assumed an accepted step
    log = [[9, 0, 1e4, 0, 1e-8, I], [8, .9, 1e4, 1, 1e-7, A], [7, .9, 1e4, 1, 2e-8, A]]
    assert ip.replay(lib, log, "dogleg", 0, 9) == (1, 2, 3)
    # Levenberg-Marquardt: kept exactly behind a step accepted with the clamp active (radius x 3)
    r1 = 1e4 / (1.0 / 3.0)
    log = [[9, .99, r1, 1, 1e-4, A], [8, .6, 3.2e4, 1, 1 / r1, A], [8, -1, 1.6e4, 1, 1 / 3.2e4, R], [7, .99, 4.8e4, 1, 1 / 1.6e4, A]]
    assert ip.replay(lib, log, "lm", 0, 9) == (1, 3, 4)


# ------------------------------------------------------------------------------------------------ 3. the batched round
def hand_made_passes():
    """(solve, build.launch, build.zeroFirst, allReduceSystem, stepInEval, doglegStep, specWanted), prepareRadius, cand -> stages, -1
    where batchStagesOf throws; every pass also as the initial evaluation (cand = 0), which reads none of it"""
    fused = 1e4
    cases = {(1, 1, 0, 0, 0, 0, 0): BATCH_FULL | BATCH_EVAL, (0, 0, 0, 0, 0, 1, 0): BATCH_REUSE | BATCH_EVAL,
             (1, 1, 1, 0, 0, 0, 0): -1,    # a zeroing build
             (1, 0, 0, 0, 0, 0, 0): -1,    # a build kept from an earlier round
             (1, 1, 0, 1, 0, 0, 0): -1,    # a system all-reduce
             (1, 1, 0, 0, 0, 0, 1): -1, (0, 0, 0, 0, 0, 1, 1): -1,   # a speculative build
             (1, 1, 0, 0, 1, 0, 0): -1,    # the step left to k_eval_build
             (1, 1, 0, 0, 0, 1, 0): -1,    # a step that is not fused
             (0, 0, 0, 0, 0, 0, 0): -1}    # neither a solve nor a step
    out = []
    for fields, want in cases.items():
        out += [(fields, fused, 1, want), (fields, fused, 0, BATCH_EVAL)]
    return out + [((1, 1, 0, 0, 0, 0, 0), -1.0, 1, -1)]   # the post-solve pass without a radius


HAND_MADE_PASSES = hand_made_passes()


def test_batched_round_is_the_pass_solve_batch_group_wrote_out_by_hand(lib):
    """Every event sequence of a batched window.  Before, Window::solveBatchGroup kept `deferLm = p.L > 0 && p.N > 0` per window and
    issued  stages = !cand ? kBatchEval : (tr.reuse ? kBatchReuse | kBatchEval : kBatchFull | kBatchEval)  and
    lmDeferred = cand && deferLm && !tr.reuse;  the rows are passes, cand = true (the initial evaluation, cand = false, has no pass)."""
    passes = 0
    for cfg in batched_configurations():
        r = run_all(lib, cfg)
        alive, reuse = r["alive"] > 0, r["reuse"] > 0
        defer_lm = True   # the shim's window: L = 100, N = 1000
        stages_before = np.where(reuse, BATCH_REUSE | BATCH_EVAL, BATCH_FULL | BATCH_EVAL)
        assert np.array_equal(r["batchStages"][alive], stages_before[alive]), cfg
        assert np.array_equal(r["lmDeferredEval"][alive] > 0, (defer_lm & ~reuse)[alive]), cfg
        # the build of every pass that has one -- a fresh linearisation, the retry ladder included -- is launched into clean accumulators
        fresh = alive & ~reuse
        assert np.array_equal(r["solve"] > 0, fresh) and (r["launch"][fresh] > 0).all() and not (r["zeroFirst"][alive] > 0).any(), cfg
        assert (r["end"][fresh] == RETRY).any() or cfg[4] == 0
        assert not (r["specWanted"][alive] > 0).any() and not (r["allReduceSystem"][alive] > 0).any() and not (r["stepInEval"][alive] > 0).any()
        assert np.array_equal(r["doglegStep"] > 0, alive & reuse)   # kBatchReuse: k_step_retract alone
        assert np.array_equal(r["prepareRadius"][fresh], r["stepRadius"][fresh])   # (dogleg: the slot's radius, tr.radius)
        ok, kept = model(cfg, r)   # and the accumulators hold exactly that build in front of every reduced solve
        assert ok.all() and not kept.any(), cfg
        passes += int(alive.sum())
    assert passes > 10 ** 5
    # the initial evaluation, and what a round has no launches for
    for fields, radius, cand, want in HAND_MADE_PASSES:
        f = np.array(fields, np.int32)
        assert lib.ip_batch_stages(f.ctypes.data_as(C.c_void_p), radius, cand) == want, (fields, radius, cand)


# ------------------------------------------------------------------------------------------------ 4. under a sanitizer
def test_ledger_and_pass_under_address_and_undefined_behaviour_sanitizers(lib, tmp_path):
    exe, cases, passes = str(tmp_path / "iteration_plan_sanitize"), str(tmp_path / "cases.txt"), str(tmp_path / "passes.txt")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-Wall", "-Wextra", "-Werror", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                           os.path.join(ROOT, "tests", "csrc", "iteration_plan_sanitize.cpp"), "-o", exe])
    rng = np.random.default_rng(5)
    scripts = []
    for cfg in configurations() + batched_configurations():
        for n in (0, 1, 3, 6, 12):
            scripts.append((cfg, [int(v) for v in rng.integers(0, N_EVENTS, n)]))
        scripts.append((cfg, [0] * 9))   # the mu ladder to its end
    with open(cases, "w") as f:
        for cfg, ev in scripts:
            f.write(" ".join(str(v) for v in list(cfg) + [len(ev)] + ev) + "\n")
    with open(passes, "w") as f:   # the hand-made passes of the batched round, the throwing branches of batchStagesOf among them
        for fields, radius, cand, _ in HAND_MADE_PASSES:
            f.write(" ".join(str(v) for v in fields) + " %r %d\n" % (radius, cand))
    out = subprocess.run([exe, cases, passes], stdout=subprocess.PIPE, stderr=subprocess.PIPE, universal_newlines=True)
    assert out.returncode == 0, out.stderr
    lines = out.stdout.strip().split("\n")
    assert len(lines) == len(scripts) + len(HAND_MADE_PASSES)
    stages, lines = lines[len(scripts):], lines[:len(scripts)]
    for (fields, radius, cand, want), line in zip(HAND_MADE_PASSES, stages):
        f = np.array(fields, np.int32)
        assert line == "stages %d" % lib.ip_batch_stages(f.ctypes.data_as(C.c_void_p), radius, cand) == "stages %d" % want, (fields, radius, cand)
    for (cfg, ev), line in zip(scripts, lines):
        c, e, rows = np.array(cfg, np.int32), np.array(ev + [0], np.int32), np.zeros(len(ev) * len(FIELDS))
        ran = lib.ip_run(c.ctypes.data_as(C.c_void_p), e.ctypes.data_as(C.c_void_p), len(ev), rows.ctypes.data_as(C.c_void_p))
        got = [float(v) for v in line.split()]
        assert got[0] == ran and np.array_equal(np.array(got[1:]), rows), (cfg, ev)
