"""The deal of the narrow window's tile rows to the waves of the LDS-resident solver (svin_amd/csrc/pack_plan.hpp planTileDeal) on
the CPU, through tests/csrc/tile_deal_shim.cpp.  A deal moves arithmetic between waves and never changes a value, so what can go
wrong is the synchronisation: a row without an owner, a flag with two writers, a wave that waits for a flag nobody will store.  The
planner's deals are therefore held against the rules it promises (tests/helpers/tile_deal_lib.py check_deal) and each one is
rehearsed on a model of the kernel's flag protocol -- wave 0, the six owners and the quiet wave in the order the kernel issues their
waits and stores -- under many schedules: every wave must terminate, and every pivot, panel solve and tile product must come after
what the right-looking factorisation makes it depend on.  The same cases run through a stand-alone program under AddressSanitizer
and UndefinedBehaviorSanitizer (tests/csrc/tile_deal_sanitize.cpp), whose answers must be the shim's."""
import os
import subprocess

import numpy as np
import pytest

from helpers import tile_deal_lib as td

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

# today's closed form, written out: rows nT-1 .. nT-6 on waves 1, 2, 3, 7, 6, 5; rows 2 .. nT-7 on the quiet wave (4)
CLOSED_FORM = {
    8: {2: 5, 3: 6, 4: 7, 5: 3, 6: 2, 7: 1},
    9: {2: 4, 3: 5, 4: 6, 5: 7, 6: 3, 7: 2, 8: 1},
    10: {2: 4, 3: 4, 4: 5, 5: 6, 6: 7, 7: 3, 8: 2, 9: 1},
    11: {2: 4, 3: 4, 4: 4, 5: 5, 6: 6, 7: 7, 8: 3, 9: 2, 10: 1},
}
BENCH_HI = [5, 7, 8, 9, 9, 9, 9, 9, 9, 9]   # the headline window: 10 keyframes, d = 150
# row 2 (column 0) to the wave of row 8 (first work in column 2), row 3 (columns 0-1) to the wave of row 9 (first work in column 3)
BENCH_DEAL = {2: 2, 3: 1, 4: 5, 5: 6, 6: 7, 7: 3, 8: 2, 9: 1}
BENCH_WORD = (2 << 8) | (1 << 12)


@pytest.fixture(scope="module")
def lib(tmp_path_factory):
    return td.build_shim(tmp_path_factory.mktemp("tile_deal"))


def random_skylines(n=200, seed=11):
    rng = np.random.default_rng(seed)
    out = []
    for _ in range(n):
        nT = int(rng.integers(8, td.MAX_TILES + 1))
        reach = int(rng.integers(1, nT))   # how far below the diagonal a column may start out
        out.append(td.close_fill([min(nT - 1, k + int(rng.integers(0, reach + 1))) for k in range(nT)]))
    return out


def designed_skylines():
    out = [BENCH_HI]
    for nT in range(2, td.MAX_TILES + 1):
        out.append([nT - 1] * nT)                                   # dense
        out.append(list(range(nT)))                                  # diagonal: no row has any work
        out.append([min(nT - 1, k + 1) for k in range(nT)])          # tridiagonal tiles
        out.append(td.close_fill([min(nT - 1, k + 3) for k in range(nT)]))
        out.append(td.close_fill([min(nT - 1, k + 5) for k in range(nT)]))
    out.append(td.close_fill([6, 7, 8, 9, 10, 10, 10, 10, 10, 10, 10]))   # an eleven-row window of the bench's kind
    out.append(td.close_fill([4, 6, 7, 8, 8, 8, 8, 8, 8]))
    out.append(td.close_fill([3, 5, 6, 7, 7, 7, 7, 7]))
    return out


def every_skyline():
    return designed_skylines() + random_skylines()


def test_zero_word_is_the_closed_form(lib):
    for nT, table in CLOSED_FORM.items():
        assert td.decode(lib, 0, nT) == table
        assert {I: lib.td_base_owner(nT, I) for I in range(2, nT)} == table
    # the row masks the kernel starts from are the same closed form, wave by wave, for every size of the solver
    for nT in range(1, td.MAX_TILES + 1):
        for w in range(8):
            rows = [I for I in range(2, nT) if lib.td_base_owner(nT, I) == w]
            assert lib.td_base_rows(nT, w) == sum(1 << I for I in rows), (nT, w)


def test_dense_profile_gives_the_zero_word(lib):
    for nT in range(2, td.MAX_TILES + 1):
        word, owner = td.plan(lib, [nT - 1] * nT)
        assert word == 0
        assert owner == td.decode(lib, 0, nT)
    # systems beyond the solver's eleven tile rows, and none at all, carry no deal
    assert td.plan(lib, [13] * 14)[0] == 0 and td.plan(lib, [])[0] == 0


def test_profiles_of_the_skyline_planner(lib, tmp_path):
    """the deal of the profiles planTileSkyline gives: the P = 10 window is the bench profile; a prior over all of its blocks, or an
    unrecognised window, is dense and keeps the closed form"""
    from helpers import tile_skyline_lib as ts
    sky = ts.build_shim(tmp_path)
    d, dC, cliques, _ = ts.window(10)
    q = ts.plan(sky, d, dC, cliques)
    assert q["hi"] == BENCH_HI and lib.td_plan_cut(q["nT"], q["cut"]) == BENCH_WORD
    dense = ts.plan(sky, d, dC, ts.window(10, prior_all=True)[2])
    assert dense["cut"] == 0 and td.plan(lib, dense["hi"])[0] == 0 and lib.td_plan_cut(10, dense["cut"]) == 0
    unknown = ts.plan(sky, d, dC, cliques, recognised=False)
    assert td.plan(lib, unknown["hi"])[0] == 0


def test_at_most_seven_tile_rows_give_the_zero_word(lib):
    for hi in every_skyline():
        if len(hi) <= 7:
            assert td.plan(lib, hi)[0] == 0


def test_bench_profile_gives_the_expected_deal(lib):
    word, owner = td.plan(lib, BENCH_HI)
    assert owner == BENCH_DEAL and word == BENCH_WORD
    assert td.decode(lib, word, 10) == BENCH_DEAL
    assert lib.td_plan_cut(10, td.pack_cut(BENCH_HI)) == BENCH_WORD
    # the rows the quiet wave held are gone from it
    assert td.QUIET not in owner.values()


def test_every_deal_keeps_the_rules(lib):
    moved = 0
    for hi in every_skyline():
        nT = len(hi)
        assert hi == td.close_fill(hi)
        word, owner = td.plan(lib, hi)
        assert owner == td.decode(lib, word, nT), hi       # what the kernel decodes is what the planner meant
        assert lib.td_plan_cut(nT, td.pack_cut(hi)) == word, hi
        td.check_deal(hi, owner)
        base = td.decode(lib, 0, nT)
        for I in owner:   # only rows of the quiet wave move, and only to an owner; the word names the moved rows alone
            nib = (word >> (4 * I)) & 15
            assert (nib == 0 and owner[I] == base[I]) or (base[I] == td.QUIET and nib == owner[I] and nib in td.OWNERS), (hi, I)
        assert word >> (4 * nT) == 0 and word & 0xff == 0
        moved += word != 0
    assert moved > 50   # (the sample is not all dense)


def test_every_deal_runs_the_flag_protocol_to_the_end(lib):
    rng = np.random.default_rng(5)
    for hi in every_skyline():
        nT = len(hi)
        word, owner = td.plan(lib, hi)
        for deal in ([owner] if word == 0 else [owner, td.decode(lib, 0, nT)]):   # the planned deal, and today's on the same skyline
            td.rehearse(hi, deal, greedy="low")
            td.rehearse(hi, deal, greedy="high")
            for _ in range(3):
                td.rehearse(hi, deal, rng=rng)


def test_the_model_catches_a_row_without_owner(lib):
    """the rehearsal is only worth something if a bad deal fails it"""
    _, owner = td.plan(lib, BENCH_HI)
    orphan = dict(owner)
    orphan[3] = 9   # no such wave: nobody stores the row's flags
    with pytest.raises(AssertionError, match="deadlock"):
        td.rehearse(BENCH_HI, orphan, greedy="low")


def test_planner_under_address_and_undefined_behaviour_sanitizers(lib, tmp_path):
    exe, cases = str(tmp_path / "tile_deal_sanitize"), str(tmp_path / "cases.txt")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-Wall", "-Wextra", "-Werror", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                           os.path.join(ROOT, "tests", "csrc", "tile_deal_sanitize.cpp"), "-o", exe])
    sky = every_skyline()
    with open(cases, "w") as f:
        for hi in sky:
            f.write(" ".join(str(v) for v in [len(hi)] + hi) + "\n")
    out = subprocess.run([exe, cases], stdout=subprocess.PIPE, stderr=subprocess.PIPE, universal_newlines=True)
    assert out.returncode == 0, out.stderr
    lines = out.stdout.strip().split("\n")
    assert len(lines) == len(sky)
    for hi, line in zip(sky, lines):
        word, owner = td.plan(lib, hi)
        got = [int(v) for v in line.split()]
        assert got[0] == word and got[1:] == [owner[I] for I in range(2, len(hi))], hi
