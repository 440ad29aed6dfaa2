"""The pose-graph kernels stage by stage against the long-double reference (tests/helpers/pg_reference.py), on the case graphs of
tests/helpers/pg_cases.py, through PoseGraph.debug_step(): ONE Levenberg-Marquardt step of svin_pg_optimize's own code whose
intermediates stay in the handle.

Per case and DoF
  partition     the captured index tables equal the Python restatement of the symbolic step, the planned edge was reached,
                cholFail == 0, and the local problem equals the restated construction;
  evaluation    res, Ja, Jb (as stored: robustified) and the cost against edges(), entry by entry within the derived bound;
  node pass     g, colsq, nodeBlk, scale, gradmax against node_quantities() of the device's own res, Ja, Jb;
  solve         eta(y) = |b - A y| / (|A| |y| + |b|) on the reference's A, b under the a-priori ceiling n (3n + 13 + R) eps AND under
                8 max(eta(LAPACK), eps); forward error under kappa_2(A) times that bar;
  model         model cost change, candidate, step^2, x^2, candidate cost against model_and_candidate() of the device's own y;
  determinism   a second debug_step on a fresh handle returns the same bits.
The bounds and their derivation: pg_reference.py.  tests/test_pg_reference_host.py holds the reference, the bounds (on a float64
evaluation by the CPU) and the rejection of planted defects without a GPU.

Measured on an MI355X on 2026-10-20 (`pytest -s` prints the line of every case; ratio = eta(device) / max(eta(LAPACK), eps), the
bar is 8; the full table with ceiling, kappa and forward error is in DESIGN.md section 9).  The whole file: 242 tests in 8 s.
  case                 DoF     n  eta(device) eta(LAPACK)  ratio
  dense40              4    160   1.30e-16    6.94e-17   0.58
  dense40              6    240   1.53e-16    9.98e-17   0.69
  pieces60             4    240   1.02e-16    6.28e-17   0.46
  pieces60             6    360   1.50e-16    8.59e-17   0.68
  short_last_4         4    248   1.01e-16    6.42e-17   0.45
  short_last_6         6    372   1.35e-16    8.40e-17   0.61
  edges127_4           4    252   1.22e-16    8.33e-17   0.55
  edges127_6           6    192   1.47e-16    9.32e-17   0.66
  edges128_4           4    252   1.49e-16    7.41e-17   0.67
  edges128_6           6    192   1.70e-16    7.22e-17   0.77
  edges129_4           4    252   1.25e-16    6.62e-17   0.56
  edges129_6           6    192   1.50e-16    9.27e-17   0.68
  nodes128             4    508   1.34e-16    7.33e-17   0.60
  nodes128             6    762   1.74e-16    9.76e-17   0.78
  nodes129             4    512   1.10e-16    6.68e-17   0.50
  nodes129             6    768   1.56e-16    1.00e-16   0.70
  level2_4             4    640   1.02e-16    7.10e-17   0.46
  level2_control_4     4    640   1.18e-16    7.10e-17   0.53
  level2_6             6    660   1.35e-16    1.07e-16   0.61
  level2_control_6     6    660   1.37e-16    1.07e-16   0.62
  heavy_hi_4           4    700   1.38e-16    6.60e-17   0.62
  heavy_lo_4           4    484   1.13e-16    7.02e-17   0.51
  heavy_6              6   1014   1.71e-16    1.21e-16   0.77
  level2_fallback_6    6   1002   2.93e-16    1.06e-16   1.32
  level2_wide_4        4    748   1.10e-16    7.65e-17   0.49
  level2_wide_6        6   1002   2.01e-16    1.13e-16   0.91
  shared_sep_4         4    240   9.51e-17    6.51e-17   0.43
  shared_band_4        4    240   1.02e-16    6.90e-17   0.46
  shared_coupling_4    4    240   9.59e-17    5.75e-17   0.43
  shared_sep_6         6    360   1.02e-16    9.92e-17   0.46
  shared_band_6        6    360   1.11e-16    7.71e-17   0.50
  shared_coupling_6    6    360   1.08e-16    9.03e-17   0.49
  breaks               4    232   1.07e-16    7.32e-17   0.48
  breaks               6    348   1.14e-16    8.23e-17   0.51
  constant_middle_6    6    312   1.91e-16    8.78e-17   0.86
  huber_4              4    240   9.38e-17    7.50e-17   0.42
  huber_6              6    360   1.19e-16    7.86e-17   0.54
  wrap_4               4    480   9.79e-17    7.76e-17   0.44
  radius_small         4    240   9.33e-17    7.37e-17   0.42
  radius_small         6    360   1.21e-16    1.66e-16   0.55
"""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "helpers"))
import pg_cases as pc  # noqa: E402
import pg_reference as pr  # noqa: E402

from svin_amd import synthetic_pg as spg  # noqa: E402

pytestmark = [pytest.mark.gpu, pytest.mark.skipif(not pr.have_long_double(), reason="np.longdouble is not an extended type on this platform")]

CASES = pc.build_cases()
CASE_DOFS = [(c, six) for c in CASES for six in c.dofs]
IDS = ["%s-%ddof" % (c.name, 6 if six else 4) for c, six in CASE_DOFS]
_CAPTURES = {}


def _step(case, six):
    from svin_amd.posegraph import PoseGraph
    g = PoseGraph(0, six_dof=six)
    case.configure(g)
    spg.feed(g, case.spec)
    before = g.poses()
    cap = g.debug_step(case.earliest, case.cur, case.radius)
    after = g.poses()
    assert cap is not None
    assert np.array_equal(before[0], after[0]) and np.array_equal(before[1], after[1]), "debug_step moved the keyframes"
    g.close()
    return cap


def capture(case, six):
    key = (case.name, six)
    if key not in _CAPTURES:
        _CAPTURES[key] = _step(case, six)
    return _CAPTURES[key]


@pytest.mark.parametrize("case,six", CASE_DOFS, ids=IDS)
def test_partition_and_problem(gpu_lib, case, six):
    cap = capture(case, six)
    P = case.problem(six)
    for key in pc.PROBLEM_KEYS:
        a, b = np.asarray(cap[key]), np.asarray(P[key])
        assert a.shape == b.shape, key
        if a.dtype.kind == "i":
            assert np.array_equal(a, b), key
        else:   # host float64 on both sides, other roundings (atan2, contraction): 64 eps of 180 degrees / of the positions
            assert np.max(np.abs(a - b), initial=0.0) <= 64 * pr.EPS64 * max(180.0, float(np.max(np.abs(b), initial=0.0))), key
    part = case.partition(cap, six)
    pr.check_partition(cap, part)
    assert cap["cholFail"] == 0
    ref = dict(yawC=cap["yawC"])
    case.reach(part, cap, six, ref=ref)
    assert len(cap["y"]) == (6 if six else 4) * int(np.sum(cap["off"] >= 0)) and len(cap["yS"]) == cap["nS"]


@pytest.mark.parametrize("case,six", CASE_DOFS, ids=IDS)
def test_evaluation(gpu_lib, case, six):
    pr.check_evaluation(capture(case, six), six)


@pytest.mark.parametrize("case,six", CASE_DOFS, ids=IDS)
def test_node_pass(gpu_lib, case, six):
    pr.check_node_pass(capture(case, six), six)


@pytest.mark.parametrize("case,six", CASE_DOFS, ids=IDS)
def test_solve(gpu_lib, case, six):
    cap = capture(case, six)
    pr.check_solve(cap, six, case.radius, verbose="eta %s %d-DoF" % (case.name, 6 if six else 4))
    # separators: yS is y in separator order
    D = 6 if six else 4
    for k in np.where(cap["sepOff"] >= 0)[0]:
        assert np.array_equal(cap["yS"][cap["sepOff"][k]:cap["sepOff"][k] + D], cap["y"][cap["off"][k]:cap["off"][k] + D])


@pytest.mark.parametrize("case,six", CASE_DOFS, ids=IDS)
def test_model_and_candidate(gpu_lib, case, six):
    pr.check_model_and_candidate(capture(case, six), six)


@pytest.mark.parametrize("case,six", CASE_DOFS, ids=IDS)
def test_second_step_is_bit_identical(gpu_lib, case, six):
    """fixed accumulation orders and commuting atomics: a fresh handle returns the same bits (the shared-destination cases are
    where two atomic adds meet in one block)"""
    a, b = capture(case, six), _step(case, six)
    for key in ("res", "Ja", "Jb", "g", "scale", "colsq", "nodeBlk", "y", "yS", "yawC", "tC", "qC"):
        assert np.array_equal(a[key].view(np.int64), b[key].view(np.int64)), key
    for key in ("cost", "costC", "gradmax", "model", "step2", "x2", "cholFail"):
        assert np.float64(a[key]).tobytes() == np.float64(b[key]).tobytes(), key


@pytest.mark.parametrize("six", [False, True])
def test_capture_is_the_path_optimize_takes(gpu_lib, six):
    """optimize() with one iteration on a fresh handle ends at the captured candidate: positions bit for bit; rotations through
    the host's write-back (ypr2R / quaternion -> matrix -> quaternion in float64: a few eps), restated here"""
    from svin_amd.posegraph import PoseGraph
    case = next(c for c in CASES if c.name == "pieces60")
    cap = capture(case, six)
    g = PoseGraph(0, six_dof=six, max_iterations=1)
    case.configure(g)
    spg.feed(g, case.spec)
    s = g.optimize(case.earliest, case.cur)
    assert s["iterations"] == 1 and s["successful"] == 1, s
    assert abs(s["initial_cost"] - cap["cost"]) == 0 and abs(s["final_cost"] - cap["costC"]) == 0
    T, Q = g.poses()
    lo = case.earliest
    assert np.array_equal(T[lo:], cap["tC"].reshape(-1, 3))
    if six:
        want = np.array([spg.R2q(spg.q2R(q)) for q in cap["qC"].reshape(-1, 4)])
    else:
        want = np.array([spg.R2q(spg.ypr2R([y, p, r])) for y, p, r in zip(cap["yawC"], cap["pitch"], cap["roll"])])
    sign = np.sign(np.sum(want * Q[lo:], axis=1, keepdims=True))
    assert np.max(np.abs(want * sign - Q[lo:])) <= 16 * pr.EPS64
    g.close()
