"""The reference of the pose graph's marginal covariances (tests/helpers/pg_cov_reference.py) without a GPU:

  mpmath        on dense40 (4-DoF) the long-double columns agree with the columns of a 40-digit inverse (mpmath Cholesky of the same
                matrix, two column keyframes) within kappa_2(A) n (3n + 1) eps_ld, the solve's own bound in the reference's precision;
  restatement   the float64 restatement of the device's recursion (elimination order of pr.partition, the later keyframe of a pair
                as the column, mirrored diagonal blocks, both-sided unscaling) meets the GPU test's bars on every case graph at its
                initial states: backward error of every column under the ceiling and under 8 max(eta(LAPACK), eps), forward error
                under kappa times that, constant rows exactly zero, (a, b) and (b, a) transposes bit for bit;
  breaks        raises, in the reference and in the restatement;
  defects       damping left in at radius 1e4, the scale on one side only, Sigma_ab transposed, the Huber corrector left off,
                a column taken one keyframe off, a non-zero block for a constant keyframe: each rejected by the check meant for it;
  second graph  the GPU test's second singular input (a second sequence with no loop to the first) has a smallest pivot below
                1e-12 of its diagonal in the reference.
"""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "helpers"))
import pg_cases as pc  # noqa: E402
import pg_cov_reference as cr  # noqa: E402
import pg_reference as pr  # noqa: E402

pytestmark = pytest.mark.skipif(not pr.have_long_double(), reason="np.longdouble is not an extended type on this platform")

CASES = [c for c in pc.build_cases() if c.name != "radius_small"]      # (the graph of pieces60 again)
CASE_DOFS = [(c, six) for c in CASES for six in c.dofs if c.name != "breaks"]
IDS = ["%s-%ddof" % (c.name, 6 if six else 4) for c, six in CASE_DOFS]
BY_NAME = {c.name: c for c in CASES}


def _setup(case, six):
    P = case.problem(six)
    return P, case.partition(P, six)


def test_reference_against_mpmath():
    mp = pytest.importorskip("mpmath")
    case, six = BY_NAME["dense40"], False
    P, _ = _setup(case, six)
    ref = cr.Reference(P, P, six)
    n, D = len(ref.s), ref.D
    mp.mp.dps = 40

    def to_mp(x):   # a long double as the exact sum of two doubles
        hi = float(x)
        return mp.mpf(hi) + mp.mpf(float(x - pr.LD(hi)))
    old = mp.mp.dps
    try:
        M = mp.matrix([[to_mp(x) for x in row] for row in ref.A])
        L = mp.cholesky(M)
        nodes = [int(np.where(ref.off >= 0)[0][0]), len(ref.off) - 1]
        kap = pr.kappa2(ref.A)
        bound = kap * n * (3 * n + 1) * pr.EPS_LD
        # (the same a-priori bound in float64 is three digits wider: the reference is fit to judge a float64 result)
        assert bound * 1000 <= kap * pr.eta_ceiling(n, D)
        for node in nodes:
            got = ref.column_block(node) / (ref.s[:, None] * ref.s[None, ref.off[node]:ref.off[node] + D])
            for j in range(D):
                u = ref.off[node] + j
                z = [mp.mpf(0)] * n
                for i in range(u, n):
                    z[i] = ((1 if i == u else 0) - sum(L[i, k] * z[k] for k in range(u, i))) / L[i, i]
                x = [mp.mpf(0)] * n
                for i in range(n - 1, -1, -1):
                    x[i] = (z[i] - sum(L[k, i] * x[k] for k in range(i + 1, n))) / L[i, i]
                err = mp.sqrt(sum((to_mp(got[i, j]) - x[i]) ** 2 for i in range(n))) / mp.sqrt(sum(v * v for v in x))
                assert float(err) <= bound, (node, j, float(err), bound)
    finally:
        mp.mp.dps = old


@pytest.mark.parametrize("case,six", CASE_DOFS, ids=IDS)
def test_restatement_meets_the_bars(case, six):
    P, part = _setup(case, six)
    case.reach(part, P, six)
    nn = len(P["off"])
    cols = cr.role_columns(part, P)
    pairs = cr.column_pairs(nn, cols)
    blocks = cr.device_blocks(P, P, six, part, pairs)
    A, s = cr.scaled_system(P, P, six, dtype=np.float64)      # what the restatement factorised, before its rounding to float64
    sigma = cr.columns_from_blocks(P, six, cols, blocks)
    cr.check_columns(A, s, P, six, cols, sigma)
    flipped = cr.device_blocks(P, P, six, part, [(b, a) for a, b in pairs])
    cr.check_transposes(blocks, flipped)
    # and against the reference proper (long-double evaluation): the evaluation's rounding is far inside the forward bound
    ref = cr.Reference(P, P, six)
    cr.check_blocks(ref, pairs[::7], blocks[::7])


@pytest.mark.parametrize("six", [False, True])
def test_breaks_raises(six):
    case = BY_NAME["breaks"]
    P, part = _setup(case, six)
    case.reach(part, P, six)
    with pytest.raises(cr.Singular):
        cr.Reference(P, P, six)
    with pytest.raises(cr.Singular):
        cr.device_blocks(P, P, six, part, [(len(P["off"]) - 1, len(P["off"]) - 1)])


def _defect_run(name, six, defect):
    case = BY_NAME[name]
    P, part = _setup(case, six)
    nn = len(P["off"])
    cols = cr.role_columns(part, P)
    pairs = cr.column_pairs(nn, cols)
    return P, part, cols, pairs, cr.device_blocks(P, P, six, part, pairs, defect=defect)


@pytest.mark.parametrize("name,six", [("dense40", False), ("pieces60", True)])
def test_damping_left_in_is_rejected(name, six):
    P, part, cols, pairs, blocks = _defect_run(name, six, "damping")
    A, s = cr.scaled_system(P, P, six, dtype=np.float64)
    with pytest.raises(AssertionError, match="backward error"):
        cr.check_columns(A, s, P, six, cols, cr.columns_from_blocks(P, six, cols, blocks))


@pytest.mark.parametrize("name,six", [("dense40", True), ("pieces60", False)])
def test_one_sided_scale_is_rejected(name, six):
    P, part, cols, pairs, blocks = _defect_run(name, six, "one_sided_scale")
    A, s = cr.scaled_system(P, P, six, dtype=np.float64)
    with pytest.raises(AssertionError, match="backward error"):
        cr.check_columns(A, s, P, six, cols, cr.columns_from_blocks(P, six, cols, blocks))


@pytest.mark.parametrize("name,six", [("pieces60", False), ("pieces60", True)])
def test_transposed_block_is_rejected(name, six):
    P, part, cols, pairs, blocks = _defect_run(name, six, "transposed")
    ref = cr.Reference(P, P, six)
    with pytest.raises(AssertionError, match=r"block \(\d+, \d+\): off by"):
        cr.check_blocks(ref, pairs, blocks)
    # ... and held against the sound (b, a) blocks it is no transpose either
    good_ba = cr.device_blocks(P, P, six, part, [(b, a) for a, b in pairs])
    with pytest.raises(AssertionError, match="bit for bit"):
        cr.check_transposes(blocks, good_ba)


@pytest.mark.parametrize("name,six", [("huber_4", False), ("huber_6", True)])
def test_huber_left_off_is_rejected(name, six):
    P, part, cols, pairs, blocks = _defect_run(name, six, "no_huber")
    ref = cr.Reference(P, P, six)
    with pytest.raises(AssertionError, match=r"block \(\d+, \d+\): off by"):
        cr.check_blocks(ref, pairs, blocks)
    cr.check_blocks(ref, pairs, cr.device_blocks(P, P, six, part, pairs))


@pytest.mark.parametrize("name,six", [("pieces60", False), ("level2_6", True)])
def test_column_one_keyframe_off_is_rejected(name, six):
    P, part, cols, pairs, blocks = _defect_run(name, six, "column_off")
    A, s = cr.scaled_system(P, P, six, dtype=np.float64)
    with pytest.raises(AssertionError, match="backward error"):
        cr.check_columns(A, s, P, six, cols, cr.columns_from_blocks(P, six, cols, blocks))


@pytest.mark.parametrize("name,six", [("dense40", False), ("constant_middle_6", True)])
def test_constant_block_not_zero_is_rejected(name, six):
    P, part, cols, pairs, blocks = _defect_run(name, six, "constant_nonzero")
    with pytest.raises(AssertionError, match="constant keyframe"):
        cr.columns_from_blocks(P, six, cols, blocks)


@pytest.mark.parametrize("six", [False, True])
def test_second_singular_input_has_a_pivot_below_the_rule(six):
    case = cr.second_sequence_case()
    P = case.problem(six)
    A, _ = cr.scaled_system(P, P, six)
    assert np.all(np.diag(A) > 0)
    assert cr.smallest_pivot_ratio(A) < cr.PIVOT_TOL
    with pytest.raises(cr.Singular):
        cr.Reference(P, P, six)
