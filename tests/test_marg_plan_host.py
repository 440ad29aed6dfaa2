"""The host planning of the marginalisation (svin_amd/csrc/marg_plan.hpp through tests/csrc/marg_plan_shim.cpp) on the CPU.

1. planMargJob against the expressions Window::applyMarginalizationStrategy formed inline before the planning moved into the header
   (commit 9bfafa1, svin_amd/csrc/marg.hip: the reservations :1620-1670, the launches and the carve-up of the buffers :1752-1856;
   the LDS sizes :267, :430-438, :526-529, :1041), restated here once, over the sweep of tests/helpers/marg_plan_lib.py.
2. Properties over the same sweep: regions inside their buffers and disjoint while they live together, LDS within a workgroup's
   160 KiB, no launch behind one that is not issued, exactly one of {dense kernel, copy pair, nothing}.
3. selectMargFrames against Estimator.cpp:499-540 restated in Python, over every keyframe pattern of up to 8 frames.
4. Every function of the header in a stand-alone program under AddressSanitizer and UndefinedBehaviorSanitizer."""
import itertools
import os
import subprocess
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "helpers"))
import marg_plan_lib as mpl          # noqa: E402

ROOT = mpl.ROOT
JS = mpl.JACOBI_SHARED


@pytest.fixture(scope="module")
def lib(tmp_path_factory):
    return mpl.build_shim(tmp_path_factory.mktemp("margplan"))


@pytest.fixture(scope="module")
def swept(lib):
    rows = mpl.sweep()
    d = {name: rows[:, k].astype(np.int64) for k, name in enumerate(mpl.INPUTS)}
    return d, mpl.plan(lib, rows)


# ------------------------------------------------------------------------------------------------ the parent's expressions
def jacobi_ld(n):                      # :267
    return ((n + 15) & ~15) | 1


LIMIT = 158 * 1024 - JS                # :430


def jacobi_lds_bytes(n):               # :431-434
    b = 2 * n * jacobi_ld(n) * 8
    return np.where(b <= LIMIT, b, 0)


def jacobi_lds_bytes_g_only(n):        # :435-438
    b = n * jacobi_ld(n) * 8
    return np.where((b <= LIMIT) & (n <= 144), b, 0)


def marg_chol_lds_bytes(n):            # :526-529
    nT = (n + 15) // 16
    NP = 16 * nT
    return (NP * (NP + 1) + nT * 16 * 17 + NP) * 8


def sym_eig_lds_bytes(n):              # :1041
    return n * (n | 1) * 8


def parent_plan(d):
    """what 9bfafa1 reserved, launched and carved up for the inputs d (arrays), as {field of marg_plan_lib.FIELDS: array}"""
    m, Lm, N, F, nk, nm = (d[k] for k in ("m", "Lm", "N", "F", "nk", "nm"))
    zero = np.zeros_like(m)
    w = {}
    mm, L3 = np.maximum(m, 1), np.maximum(3 * Lm, 1)                       # :1620
    w["bU"], w["bW2"], w["bV"], w["bVec"] = mm * mm + 2, mm * L3 + 2, 9 * np.maximum(Lm, 1) + 2, mm + 2 * L3 + 16   # :1621
    w["clearU"], w["clearW2"], w["clearV"], w["clearVec"] = mm * mm, mm * L3, 9 * np.maximum(Lm, 1), mm + 2 * L3 + 14   # :1626-1629
    w["gLm"], w["gUv"], w["gW"] = np.maximum(4 * Lm, 1), np.maximum(2 * N, 1), np.maximum(N, 1)   # :1644
    w["gLmPtr"], w["gObsLm"], w["gIdx"] = Lm + 1, np.maximum(N, 1), np.maximum(N, 1)              # :1645
    w["bLin"], w["bFacLin"] = np.maximum(32 * N, 1), np.maximum(F, 1)                             # :1653-1654
    w["bPartial"], w["bScal"], w["bFlag"] = zero + 16 * 4096, zero + 1, zero + 8                  # :1655-1657
    w["bHk"] = np.maximum(nk * nk + nk, 1)                                                        # :1667
    w["bScratch"] = np.where((nk > 0) & (nm > 0), 2 * nm * nm + nk * nm + 2 * nm + 16, 0)         # :1668
    n2 = nk * nk                                                                                  # :1669
    w["bOut"] = np.where(nk > 0, 5 * n2 + 4 * nk + 16, 0)                                         # :1670
    # the old prior (H | b0), copied into U and ba                                                  :1722-1727
    old = d["oldPriorM"]
    w["oldH_off"], w["oldH_len"], w["oldB0_off"], w["oldB0_len"] = zero, old * old, old * old, old
    # DeviceProblem's linearisation tables and MargDev                                              :1743, :1749-1750
    w["linR_off"], w["linJp_off"], w["linJl_off"], w["linJe_off"] = zero, 2 * N, 14 * N, 20 * N
    w["ba_off"], w["bb_off"], w["vb_off"] = zero, mm, mm + L3
    # M1                                                                                            :1752-1766
    rep = N > 0
    w["reproj"], w["factors"] = rep, F > 0
    w["accumLm_grid"] = np.where(rep, (Lm + 63) // 64, 0)
    w["accumCamX"] = np.where(rep, d["nPose"] + d["nExt"], 0)
    w["accumCamY"] = np.where(rep, np.where(d["anyExtVar"] != 0, 1 + d["nCam"], 1), 0)
    w["accumFactors_grid"] = np.where(F > 0, 1, 0)
    # M2, landmark part                                                                             :1791-1795
    lm = (Lm > 0) & (m > 0)
    w["lmPrepare_grid"] = np.where(lm, (Lm + 127) // 128, 0)
    w["lmApply_grid"] = np.where(lm, m, 0)
    w["lmUpdate_grid"] = np.where(lm, ((m + 15) // 16) * ((m + 15) // 16), 0)
    for k in ("accumLm", "accumFactors", "lmPrepare", "lmApply", "lmUpdate"):
        w[k + "_lds"] = zero
    # M2, dense part                                                                                :1797-1818
    dense = (nk > 0) & (nm > 0)
    lds_eig = jacobi_lds_bytes(nm)                                           # :1807
    lds_prod = 8 * (2 * nk * nm + nm * nm)                                   # :1808
    prod_lds = lds_prod <= LIMIT                                             # :1809
    lds_tile = marg_chol_lds_bytes(nm)                                       # :1810
    tile_chol = lds_tile <= LIMIT                                            # :1811
    lds = np.maximum(np.maximum(lds_eig, np.where(prod_lds, lds_prod, 0)), np.where(tile_chol, lds_tile, 0))   # :1812
    w["dense_grid"], w["dense_lds"] = np.where(dense, 1, 0), np.where(dense, lds, 0)   # :1813
    w["denseUseLds"] = np.where(dense & (lds_eig != 0), 1, 0)
    w["denseProdLds"], w["denseTileChol"] = np.where(dense & prod_lds, 1, 0), np.where(dense & tile_chol, 1, 0)
    w["copyPair"] = (nk > 0) & (nm == 0)                                     # :1815-1818
    w["Vm_off"], w["Qm_off"], w["denseTmp_off"] = zero, np.where(dense, nm * nm, 0), np.where(dense, 2 * nm * nm, 0)   # :1804
    # (the copy pair moves m * m and m doubles, :1816-1817)
    w["Hk_off"], w["bk_off"] = zero, np.where(nk > 0, np.where(nm > 0, n2, m * m), 0)   # :1803, :1817
    w["Hk_len"] = np.where(nk > 0, np.where(nm > 0, n2, m * m), 0)
    w["bk_len"] = np.where(nk > 0, np.where(nm > 0, nk, m), 0)
    # M3                                                                                            :1820-1856
    fin = nk > 0
    for k, (name, off) in enumerate((("G", zero), ("Q", n2), ("J", 2 * n2), ("Ht", 3 * n2), ("e0", 4 * n2), ("bp", 4 * n2 + nk),
                                     ("scal", 4 * n2 + 2 * nk), ("finalTmp", 4 * n2 + 2 * nk + 8))):   # :1822-1825
        w[name + "_off"] = np.where(fin, off, 0)
    eig = d["margEig"]
    want, force_fallback = eig != 0, eig == 3                                 # :1835-1836
    lds_both, lds_one = jacobi_lds_bytes(nk), jacobi_lds_bytes_g_only(nk)     # :1837
    mode = np.where(force_fallback, np.where(lds_both != 0, 1, 0), np.where(lds_one != 0, 4, 6))   # :1838
    lds_f = np.where(mode == 4, np.maximum(lds_one, lds_both), np.where(mode == 1, lds_both, 0))   # :1839
    direct = (~want | (eig == 1)) & (nk <= 128)                               # :1845-1846
    chol = ~want & (nk <= 128)                                                # :1847
    w["finalChol_grid"], w["finalChol_lds"] = np.where(fin & chol, 1, 0), np.where(fin & chol, marg_chol_lds_bytes(nk), 0)   # :1848-1851
    w["finalDc_grid"], w["finalDc_lds"] = np.where(fin & direct, 1, 0), np.where(fin & direct, sym_eig_lds_bytes(nk), 0)   # :1852-1855
    w["finalDcAfterChol"] = np.where(fin & chol, 1, 0)
    w["final_grid"], w["final_lds"] = np.where(fin, 1, 0), np.where(fin, lds_f, 0)   # :1856
    w["finalMode"] = np.where(fin, mode, 0)
    w["finalFallbackLds"] = np.where(fin & (mode == 4) & (lds_both != 0), 1, 0)
    w["finalSkipIfDone"] = np.where(fin & direct, 1, 0)
    return w


# ------------------------------------------------------------------------------------------------ 1. against the parent
def test_sweep_covers_what_it_claims():
    rows = mpl.sweep()
    d = {name: rows[:, k] for k, name in enumerate(mpl.INPUTS)}
    assert np.all(d["nk"] + d["nm"] == d["m"])
    assert set(d["m"]) >= set(range(5)) | {15, 16, 17, 95, 96, 97, 127, 128, 129, 139, 140, 144, 145, 319, 320} and d["m"].max() == 320
    assert set(d["Lm"]) == set(mpl.LM_VALUES) and set(d["margEig"]) == {0, 1, 2, 3} and set(d["anyExtVar"]) == {0, 1}
    for m in mpl.M_VALUES:   # every split, nk = 0 and nm = 0 included
        assert set(d["nk"][(d["m"] == m)]) == set(range(m + 1)), m
    for k in ("N", "F", "oldPriorM"):
        assert (d[k] == 0).any() and (d[k] > 0).any(), k
    assert set(d["nk"]) >= {127, 128, 129}   # around symeig::kMaxN


def test_helpers_match_the_parent(lib):
    c = mpl.constants(lib)
    assert (c["kJacobiRegLen"], c["kPanelLd"], c["kSymEigMaxN"], c["kMargLdsPerWorkgroup"]) == (144, 17, 128, 163840)
    n = np.arange(0, 400, dtype=np.int64)
    assert mpl.lds(lib, "jacobiLdsLimit", 0) == LIMIT
    for name, want in (("jacobiLd", jacobi_ld(n)), ("jacobiLdsBytes", jacobi_lds_bytes(n)), ("jacobiLdsBytesGOnly", jacobi_lds_bytes_g_only(n)),
                       ("margCholLdsBytes", marg_chol_lds_bytes(n)), ("symEigLdsBytes", sym_eig_lds_bytes(n)),
                       ("margGatherScratchInts", np.maximum(2 * n, 1))):   # :1646
        got = np.array([mpl.lds(lib, name, v) for v in n])
        assert np.array_equal(got, want), name
    # the thresholds the sweep is built around
    assert mpl.lds(lib, "jacobiLdsBytes", 96) > 0 and mpl.lds(lib, "jacobiLdsBytes", 97) == 0
    assert mpl.lds(lib, "jacobiLdsBytesGOnly", 139) > 0 and mpl.lds(lib, "jacobiLdsBytesGOnly", 140) == 0
    assert mpl.lds(lib, "margCholLdsBytes", 128) <= LIMIT < mpl.lds(lib, "margCholLdsBytes", 129)
    # another sizeof(JacobiShared) moves the limit with it
    assert mpl.lds(lib, "jacobiLdsLimit", 0, 4096) == 158 * 1024 - 4096
    assert mpl.lds(lib, "jacobiLdsBytes", 96, 16384) == 0


def test_plan_equals_the_parents_expressions(swept):
    d, q = swept
    want = parent_plan(d)
    assert len(d["m"]) > 50000
    for name in mpl.FIELDS:
        if name in want:
            assert np.array_equal(q[name], np.asarray(want[name]).astype(np.int64)), name
    # fields the parent had no expression for: the extents of the regions (checked as properties below) -- and nothing else
    assert set(mpl.FIELDS) - set(want) == {r + "_len" for r in mpl.REGIONS} - {"Hk_len", "bk_len", "oldH_len", "oldB0_len"}
    # every route is met
    assert set(q["finalMode"][d["nk"] > 0]) == {0, 1, 4, 6}
    for flag in ("denseUseLds", "denseProdLds", "denseTileChol", "finalFallbackLds", "finalSkipIfDone", "finalDcAfterChol", "copyPair"):
        assert set(q[flag]) == {0, 1}, flag


# ------------------------------------------------------------------------------------------------ 2. properties
def test_regions_lie_inside_their_buffers(swept, lib):
    d, q = swept
    for r, buf in mpl.BUFFER_OF.items():
        used = q[r + "_len"] > 0
        assert np.all((q[r + "_off"] + q[r + "_len"])[used] <= q[buf][used]), r
    # extents: what the kernels index (marg.hip: MargDev, DenseArgs' tmp = pm | tv | Mu, FinalArgs' tmp = p | ev | 1 / sigma)
    m, Lm, N, nk, nm = (d[k] for k in ("m", "Lm", "N", "nk", "nm"))
    dense, fin = q["dense_grid"] > 0, nk > 0
    assert np.array_equal(q["ba_len"], m) and np.array_equal(q["bb_len"], 3 * Lm) and np.array_equal(q["vb_len"], 3 * Lm)
    for r, per in (("linR", 2), ("linJp", 12), ("linJl", 6), ("linJe", 12)):
        assert np.array_equal(q[r + "_len"], per * N), r
    assert np.array_equal(q["Vm_len"], np.where(dense, nm * nm, 0)) and np.array_equal(q["Qm_len"], q["Vm_len"])
    assert np.array_equal(q["denseTmp_len"], np.where(dense, 2 * nm + nk * nm, 0))
    for r in ("G", "Q", "J", "Ht"):
        assert np.array_equal(q[r + "_len"], nk * nk), r
    assert np.array_equal(q["e0_len"], nk) and np.array_equal(q["bp_len"], nk)
    assert np.array_equal(q["scal_len"], np.where(fin, 8, 0)) and np.array_equal(q["finalTmp_len"], 3 * nk)
    # the cleared prefixes, and the rows the landmark kernels and the accumulation write, lie inside the accumulators
    for c, buf in zip(mpl.CLEARS, ("bU", "bW2", "bV", "bVec")):
        assert np.all(q[c] <= q[buf]), c
    assert np.all(m * m <= q["clearU"]) and np.all(m * 3 * Lm <= q["clearW2"]) and np.all(9 * Lm <= q["clearV"])
    assert np.all(q["vb_off"] + q["vb_len"] <= q["clearVec"])
    # the index lists of k_marg_dense (keep | marg) are m ints; the old prior was planned as the Hk | bk of a job with nk = oldPriorM
    old = d["oldPriorM"]
    prev = mpl.plan(lib, np.stack([old, 0 * old, 0 * old, 0 * old, old, 0 * old, 1 + 0 * old, 1 + 0 * old, 1 + 0 * old, 0 * old, 0 * old,
                                   0 * old, JS + 0 * old], axis=1))
    assert np.all(q["oldH_off"] + q["oldH_len"] <= q["oldB0_off"]) and np.all(q["oldB0_off"] + q["oldB0_len"] <= prev["bHk"])
    assert np.array_equal(q["oldH_len"], prev["Hk_len"]) and np.array_equal(q["oldB0_off"], prev["bk_off"])
    # ... and its copy lands inside U and ba when it is no larger than the dense part
    fits = old <= m
    assert np.all((old * old)[fits] <= q["clearU"][fits]) and np.all(old[fits] <= q["ba_len"][fits])


def test_regions_that_live_together_do_not_overlap(swept):
    _, q = swept
    together = (("ba", "bb", "vb"), ("linR", "linJp", "linJl", "linJe"), ("Vm", "Qm", "denseTmp"), ("Hk", "bk"),
                ("G", "Q", "J", "Ht", "e0", "bp", "scal", "finalTmp"))
    for group in together:
        for a, b in itertools.combinations(group, 2):
            both = (q[a + "_len"] > 0) & (q[b + "_len"] > 0)
            a0, a1, b0, b1 = q[a + "_off"], q[a + "_off"] + q[a + "_len"], q[b + "_off"], q[b + "_off"] + q[b + "_len"]
            assert np.all(((a1 <= b0) | (b1 <= a0))[both]), (a, b)


def test_lds_requests_fit_a_workgroup(swept):
    _, q = swept
    for name in mpl.LAUNCHES_M1 + mpl.LAUNCHES_LM + ("dense",) + mpl.LAUNCHES_M3:
        assert np.all(q[name + "_lds"] + JS <= 163840), name
        assert np.all(q[name + "_lds"][q[name + "_grid"] == 0] == 0), name


def test_no_launch_behind_one_that_is_not_issued(swept):
    d, q = swept
    # M1: the accumulation kernels read what the evaluation in front of them wrote
    assert np.all(q["accumLm_grid"][q["reproj"] == 0] == 0) and np.all(q["accumCamX"][q["reproj"] == 0] == 0)
    assert np.all(q["accumCamY"][q["reproj"] == 0] == 0) and np.all(q["accumFactors_grid"][q["factors"] == 0] == 0)
    assert np.all((q["accumCamX"] > 0) == (q["accumCamY"] > 0))
    # M2 landmark part: prepare -> apply -> update
    assert np.all(q["lmApply_grid"][q["lmPrepare_grid"] == 0] == 0) and np.all(q["lmUpdate_grid"][q["lmApply_grid"] == 0] == 0)
    assert np.array_equal(q["lmPrepare_grid"] > 0, q["lmUpdate_grid"] > 0)
    # M3 reads the Hk | bk of the dense kernel or of the copy pair
    produced = (q["dense_grid"] > 0) | (q["copyPair"] != 0)
    for name in mpl.LAUNCHES_M3:
        assert np.all(q[name + "_grid"][~produced] == 0), name
    assert np.array_equal(q["final_grid"] > 0, produced)
    # k_marg_final_dc is told that the Cholesky kernel ran only when it is issued, k_marg_final to skip only behind k_marg_final_dc
    assert np.all(q["finalChol_grid"][q["finalDcAfterChol"] != 0] == 1) and np.all(q["finalDcAfterChol"][q["finalChol_grid"] == 0] == 0)
    assert np.all(q["finalDc_grid"][q["finalSkipIfDone"] != 0] == 1) and np.all(q["finalSkipIfDone"][q["finalDc_grid"] == 0] == 0)
    assert np.all(q["finalDc_grid"][q["finalChol_grid"] > 0] == 1)   # the Cholesky route alone certifies, it does not fall back
    for name in ("finalChol", "finalDc"):
        assert np.all(d["nk"][q[name + "_grid"] > 0] <= 128), name


def test_exactly_one_of_dense_kernel_copy_pair_nothing(swept):
    d, q = swept
    dense, pair = q["dense_grid"] > 0, q["copyPair"] != 0
    assert not np.any(dense & pair)
    assert np.array_equal(dense, (d["nk"] > 0) & (d["nm"] > 0))
    assert np.array_equal(pair, (d["nk"] > 0) & (d["nm"] == 0))
    assert np.array_equal(~dense & ~pair, d["nk"] == 0)
    for flag in ("denseUseLds", "denseProdLds", "denseTileChol"):
        assert np.all(q[flag][~dense] == 0), flag


# ------------------------------------------------------------------------------------------------ 3. which frames leave
def reference_frames(ids, is_keyframe, num_keyframes, num_imu_frames):
    """Estimator.cpp:499-540 on a std::map walked from its newest entry"""
    order = sorted(range(len(ids)), key=lambda i: ids[i], reverse=True)
    rit = 0
    for _ in range(num_imu_frames):                # :500-506
        rit += 1
        if rit >= len(order):                      # (an empty map: the reference increments rend(), undefined; nothing to do)
            return None
    remove_frames, remove_all_but_pose, all_linearized = [], [], []
    counted = 0
    while rit < len(order):                        # :529-538
        i = order[rit]
        if not is_keyframe[i] or counted >= num_keyframes:
            remove_frames.append(ids[i])
        else:
            counted += 1
        remove_all_but_pose.append(ids[i])
        all_linearized.append(ids[i])
        rit += 1
    return remove_frames, remove_all_but_pose, all_linearized


def test_select_marg_frames(lib):
    cases = 0
    for n in range(0, 9):
        ids = [10 + 3 * k + (k * k) % 3 for k in range(n)]   # ascending, uneven gaps
        for pattern in itertools.product((0, 1), repeat=n):
            for num_keyframes in range(5):
                for num_imu_frames in range(5):
                    want = reference_frames(ids, pattern, num_keyframes, num_imu_frames)
                    got = mpl.select_frames(lib, ids, pattern, num_keyframes, num_imu_frames)
                    if want is None:
                        assert got is None, (ids, pattern, num_keyframes, num_imu_frames)
                    else:
                        assert got == tuple(want), (ids, pattern, num_keyframes, num_imu_frames)
                    cases += 1
    assert cases == 25 * sum(2 ** n for n in range(9))


# ------------------------------------------------------------------------------------------------ 4. under a sanitizer
def test_planner_under_address_and_undefined_behaviour_sanitizers(tmp_path):
    """a stand-alone program (its own main, every function of the header on seeded inputs), run as a child"""
    exe = str(tmp_path / "marg_plan_sanitize")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-Wall", "-Wextra", "-Werror", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                           os.path.join(ROOT, "tests", "csrc", "marg_plan_sanitize.cpp"), "-o", exe])
    run = subprocess.run([exe], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, universal_newlines=True)
    assert run.returncode == 0, run.stdout[-4000:]
