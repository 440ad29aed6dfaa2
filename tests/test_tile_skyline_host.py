"""The tile skyline of the narrow window's reduced system (svin_amd/csrc/pack_plan.hpp planTileSkyline) on the CPU, through
tests/csrc/tile_skyline_shim.cpp.  k_chol_solve_lds<0> leaves every tile below the skyline alone, so a profile that is too low
anywhere is a wrong factorisation: the planner's profile is held against a numpy reference that knows nothing of tiles until
the end -- the boolean entry pattern of S from the same block lists, a dense symbolic Cholesky entry by entry, then each tile
column's last non-zero tile row (tests/helpers/tile_skyline_lib.py).  The planner may never be below the reference; on the
chain windows it must be equal to it, before and after the fill.  The same cases run through a stand-alone program under
AddressSanitizer and UndefinedBehaviorSanitizer (tests/csrc/tile_skyline_sanitize.cpp), whose answers must be the shim's."""
import os
import subprocess

import numpy as np
import pytest

from helpers import tile_skyline_lib as ts

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def lib(tmp_path_factory):
    return ts.build_shim(tmp_path_factory.mktemp("tile_skyline"))


def _cases():
    """name -> (d, dC, cliques, recognised, exact): exact = the planner must EQUAL the reference (the chain windows)"""
    out = {}

    def add(name, w, recognised=True, exact=True):
        out[name] = (w[0], w[1], w[2], recognised, exact)
    for P in (3, 5, 6, 10, 11):
        add("P%d" % P, ts.window(P))
    # 21 and 22 pose blocks in front of a short chain: dC = 126 / 132, a 6-row pose block straddles every other tile edge
    add("dC21", ts.window(21, fixed_sb=range(0, 16)))
    add("dC22", ts.window(22, fixed_sb=range(0, 18)))
    add("fixed_first_pose", ts.window(10, fixed_poses=(0,)))
    add("fixed_sb_mid_chain", ts.window(10, fixed_sb=(4,)))
    add("fixed_pose_and_sb", ts.window(8, fixed_poses=(0, 1), fixed_sb=(0, 5)))
    for k in (1, 3, 8, 12, 14):
        add("prior_first_%d" % k, ts.window(10, prior_first=k), exact=False)
    add("prior_all", ts.window(10, prior_all=True))
    add("edge_p0_s9", ts.window(10, extra=(("p0", "s9"),)))
    add("edge_s0_s9", ts.window(10, extra=(("s0", "s9"),)), exact=False)
    add("ext_per_frame_P6", ts.window(6, ext_per_frame=True))
    add("ext_per_frame_P8", ts.window(8, ext_per_frame=True))
    add("unknown_kind", ts.window(10), recognised=False, exact=False)
    add("one_block", (6, 6, [[(0, 6)]], {}))
    add("empty", (9, 0, [], {}), exact=False)
    return out


CASES = _cases()


@pytest.mark.parametrize("name", sorted(CASES))
def test_profile_against_symbolic_cholesky(lib, name):
    d, dC, cliques, recognised, exact = CASES[name]
    q = ts.plan(lib, d, dC, cliques, recognised)
    pre, hi = ts.reference(d, dC, cliques)
    nT = (d + 15) // 16
    print(name, "d", d, "dC", dC, "planner", q["pre"], q["hi"], "reference", pre, hi)
    assert q["nT"] == nT and len(q["hi"]) == nT
    assert all(a >= b for a, b in zip(q["pre"], pre)), "the build may write below the planner's profile"
    assert all(a >= b for a, b in zip(q["hi"], hi)), "the factor has entries below the planner's skyline"
    assert all(k <= q["pre"][k] <= q["hi"][k] <= nT - 1 for k in range(nT))
    if exact:
        assert q["pre"] == pre and q["hi"] == hi
    if not recognised:
        assert q["hi"] == [nT - 1] * nT and q["cut"] == 0 and q["cutPre"] == 0
    # the words DeviceProblem carries say the same, and 0 is the dense profile
    assert ts.unpack(q["cut"], nT) == q["hi"] and ts.unpack(q["cutPre"], nT) == q["pre"]
    assert [lib.ts_hi_of(q["cut"], nT, k) for k in range(nT)] == q["hi"]
    assert ts.unpack(0, nT) == [nT - 1] * nT


def test_bench_window_and_first_skipped_tile(lib):
    """the profiles worked out by hand: the bench window (P = 10, d = 150) and the smallest window that skips a tile (P = 6)"""
    d, dC, cliques, _ = ts.window(10)
    assert (d, dC) == (150, 60)
    q = ts.plan(lib, d, dC, cliques)
    assert q["pre"][:4] == [5, 7, 8, 9] and q["hi"] == [5, 7, 8, 9, 9, 9, 9, 9, 9, 9]
    # tile products and panel solves inside the skyline (column k: rows k+1 .. hi[k], every pair J <= I of them)
    rows = [h - k for k, h in enumerate(q["hi"])]
    assert [r * (r + 1) // 2 for r in rows[:3]] == [15, 21, 21] and sum(r * (r + 1) // 2 for r in rows) == 113 and sum(rows) == 38
    for P in (3, 5):
        d, dC, cliques, _ = ts.window(P)
        nT = (d + 15) // 16
        assert ts.plan(lib, d, dC, cliques)["hi"] == [nT - 1] * nT, "dense up to P = 5"
    d, dC, cliques, _ = ts.window(6)
    assert d == 90 and ts.plan(lib, d, dC, cliques)["hi"] == [4, 5, 5, 5, 5, 5]
    d, dC, cliques, _ = ts.window(11)
    assert d == 165 and ts.plan(lib, d, dC, cliques)["nT"] == 11


def test_one_far_edge_fills_the_skyline(lib):
    d, dC, cliques, _ = ts.window(10, extra=(("p0", "s9"),))
    assert ts.plan(lib, d, dC, cliques)["hi"] == [9] * 10


def test_dense_fallbacks(lib):
    d, dC, cliques, _ = ts.window(10)
    assert ts.plan(lib, d, dC, cliques, recognised=False)["cut"] == 0
    assert ts.plan(lib, d, dC, ts.window(10, prior_all=True)[2])["cut"] == 0
    # a block outside the system, an inverted CSR: dense, never an access outside the arrays
    assert ts.plan(lib, d, dC, cliques + [[(145, 9)]])["cut"] == 0
    assert ts.plan(lib, d, dC, cliques + [[(-1, 6)]])["cut"] == 0
    # systems beyond the LDS-resident solver's eleven tile rows carry no profile
    big = ts.window(14)
    assert ts.plan(lib, big[0], big[1], big[2])["cut"] == 0 and ts.plan(lib, big[0], big[1], big[2])["nT"] == 14


def test_random_cliques_never_below_the_reference(lib):
    rng = np.random.default_rng(7)
    for _ in range(200):
        nb = int(rng.integers(2, 20))
        sizes = rng.choice([6, 9], nb)
        offs = np.concatenate([[0], np.cumsum(sizes)])
        d = int(offs[-1])
        if d > 176:
            continue
        dC = int(offs[int(rng.integers(0, nb + 1))])
        cliques = []
        for _c in range(int(rng.integers(0, 8))):
            pick = rng.choice(nb, int(rng.integers(1, min(nb, 3) + 1)), replace=False)
            cliques.append([(int(offs[b]), int(sizes[b])) for b in pick])
        q = ts.plan(lib, d, dC, cliques)
        pre, hi = ts.reference(d, dC, cliques)
        assert all(a >= b for a, b in zip(q["pre"], pre)) and all(a >= b for a, b in zip(q["hi"], hi)), (d, dC, cliques)


def test_planner_under_address_and_undefined_behaviour_sanitizers(lib, tmp_path):
    exe, cases = str(tmp_path / "tile_skyline_sanitize"), str(tmp_path / "cases.txt")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-Wall", "-Wextra", "-Werror", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                           os.path.join(ROOT, "tests", "csrc", "tile_skyline_sanitize.cpp"), "-o", exe])
    names = sorted(CASES)
    with open(cases, "w") as f:
        for n in names:
            d, dC, cliques, recognised, _ = CASES[n]
            f.write(ts.case_text(d, dC, cliques, recognised) + "\n")
    out = subprocess.run([exe, cases], stdout=subprocess.PIPE, stderr=subprocess.PIPE, universal_newlines=True)
    assert out.returncode == 0, out.stderr
    lines = out.stdout.strip().split("\n")
    assert len(lines) == len(names)
    for n, line in zip(names, lines):
        d, dC, cliques, recognised, _ = CASES[n]
        q = ts.plan(lib, d, dC, cliques, recognised)
        hi, pre, words = (part.split() for part in line.split("|"))
        assert int(hi[0]) == q["nT"] and [int(v) for v in hi[1:]] == q["hi"] and [int(v) for v in pre] == q["pre"], n
        assert [int(v) for v in words] == [q["cut"], q["cutPre"]], n
