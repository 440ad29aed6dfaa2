"""CPU tests of the long-double reference of absolute pose-graph measurements (tests/helpers/pg_prior_reference.py), of the
comparisons tests/test_gpu_posegraph_priors.py judges the device with, and of its case graphs (tests/helpers/pg_prior_cases.py):

  * a plain float64 evaluation of the same expressions stays inside every bound on every case;
  * the reference's cost equals the independent plain-numpy restatement to 1e-10 relative (tests/test_pg_edge_reference_host.py's bar);
  * the Jacobians after the factor agree with central differences through the manifold's Plus;
  * six planted defects are rejected: the yaw row in radians, q_m^-1 q_k for q_k q_m^-1, L for L^T, DEPTH on row 0, the loss on
    |u|^2, a prior given two incidences;
  * every case reaches the edge it was built for, by the restated construction and symbolic step;
  * the dense Levenberg-Marquardt of the helper pulls the depth-drift chain of the GPU's whole-run test tenfold towards the truth.
"""
import functools
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "helpers"))
import pg_prior_cases as qc  # noqa: E402
import pg_prior_reference as rr  # noqa: E402
import pg_reference as pr  # noqa: E402

pytestmark = pytest.mark.skipif(not pr.have_long_double(), reason="np.longdouble is not an extended type on this platform")

CASES = qc.build_cases()
BY_NAME = {c.name: c for c in CASES}
CASE_DOFS = [(c, six) for c in CASES for six in c.dofs]
IDS = ["%s-%ddof" % (c.name, 6 if six else 4) for c, six in CASE_DOFS]


@functools.lru_cache(maxsize=None)
def problem(name, six):
    return BY_NAME[name].problem(six)


def as_capture(P, six, defect=None):
    """a float64 evaluation standing where the device stands: the arrays check_evaluation reads"""
    F = rr.evaluate64(P, P, six, defect)
    cap = dict(P)
    cap.update(res=F["res"].reshape(-1), Ja=F["Ja"].reshape(-1), Jb=F["Jb"].reshape(-1), cost=float(F["cost"]))
    return cap


@pytest.mark.parametrize("case,six", CASE_DOFS, ids=IDS)
def test_cases_reach_their_edges(case, six):
    P = problem(case.name, six)
    case.reach(case.partition(P, six), P, six)
    assert np.sum(P["eloop"] == 3) >= 1 and 20 <= len(P["off"]) <= 300


@pytest.mark.parametrize("case,six", CASE_DOFS, ids=IDS)
def test_float64_evaluation_stays_inside_every_bound(case, six):
    rr.check_evaluation(as_capture(problem(case.name, six), six), six)


@pytest.mark.parametrize("case,six", CASE_DOFS, ids=IDS)
def test_cost_matches_the_numpy_restatement(case, six):
    P = problem(case.name, six)
    c_ref, c_np = float(rr.edges(P, P, six)["cost"].v), rr.numpy_cost(P, P, six)
    assert abs(c_ref - c_np) <= 1e-10 * c_np, (c_ref, c_np)


@pytest.mark.parametrize("name,six", [("losses", False), ("losses", True), ("positions_4", False), ("positions_6", True)])
def test_jacobians_match_central_differences(name, six):
    """r0 = S u against (r0(Plus(x, h e_c)) - r0(Plus(x, -h e_c))) / 2h in float64, h = 1e-6: rounding of the two evaluations moves the
    quotient by about eps |r0| / h <= 1e-9 max(1, |r0|) per unit of |S|, the truncation h^2 |r'''| / 6 is below 1e-12 |S| (the rotation
    rows are sines of the tangent).  Bar: 1e-7 (1 + max |J0| + max |r0|)."""
    P = problem(name, six)
    F = rr.evaluate64(P, P, six)
    for e in np.where(P["eloop"] == 3)[0][:14]:
        num = rr.central_difference_jacobian(P, P, six, int(e))
        ana = F["Ja0"][e]
        bar = 1e-7 * (1.0 + float(np.max(np.abs(ana))) + float(np.max(np.abs(F["r0"][e]))))
        assert np.max(np.abs(num - ana)) <= bar, (int(e), num, ana)
        assert np.all(F["Jb0"][e] == 0.0)


def test_rotation_jacobian_away_from_the_measurement():
    """the rotation rows 2 (e_w I - [e_v]x) where e is far from the identity: a POSE prior sixty degrees off"""
    case = BY_NAME["losses"]
    spec = case.spec
    far = [qc.near(spec, 9, qc.POSE, v=(0.3, -0.2, 0.1), dq_deg=(60.0, -35.0, 20.0), info=qc.pose_info(70, 10.0))]
    P = rr.local_problem(spec, True, 0, case.cur, [], far)
    e = int(np.where(P["eloop"] == 3)[0][0])
    F = rr.evaluate64(P, P, True)
    assert np.linalg.norm(F["r0"][e]) > 0.5
    num = rr.central_difference_jacobian(P, P, True, e)
    assert np.max(np.abs(num - F["Ja0"][e])) <= 1e-7 * (1.0 + float(np.max(np.abs(F["Ja0"][e]))) + float(np.max(np.abs(F["r0"][e]))))


# ---------------------------------------------------------------- planted defects
def _defect_problem(defect, six):
    if defect == "depth_row0" or defect == "two_incidences":
        return problem("left_out", six)
    return problem("losses", six)


# (the yaw row is the 4-DoF residual's, the quaternion product the 6-DoF residual's)
DEFECT_DOFS = [(d, six) for d in rr.DEFECTS for six in (False, True) if not (d == "yaw_radians" and six) and not (d == "q_order" and not six)]


@pytest.mark.parametrize("defect,six", DEFECT_DOFS, ids=["%s-%ddof" % (d, 6 if six else 4) for d, six in DEFECT_DOFS])
def test_planted_defects_are_rejected(defect, six):
    P = _defect_problem(defect, six)
    good, bad = as_capture(P, six), as_capture(P, six, defect)
    rr.check_evaluation(good, six)
    if defect == "two_incidences":
        # the evaluation check refuses a non-zero Jb on a prior; downstream, the keyframe's block counted on both sides is out of the
        # node pass's bound by the block itself
        with pytest.raises(AssertionError, match=r"^Jb: "):
            rr.check_evaluation(bad, six)
        with pr.evaluate_in(np.float64):
            N = pr.node_quantities(good["res"], good["Ja"], good["Jb"], good, six)
        good.update(g=N["g"][0], colsq=N["colsq"][0], nodeBlk=N["blk"][0].reshape(-1), scale=N["scale"][0], gradmax=N["gradmax"][0])
        rr.check_node_pass(good, six)
        _, twice = rr.node_blocks(bad["res"], bad["Ja"], bad["Jb"], bad, six, inc=pr.incident(bad))
        D = 6 if six else 4
        good["nodeBlk"] = np.where(np.tril(np.ones((D, D), bool)), twice, 0).reshape(-1)
        with pytest.raises(AssertionError, match=r"^(colsq|nodeBlk): "):
            rr.check_node_pass(good, six)
        return
    with pytest.raises(AssertionError, match=r"^(res|Ja): "):
        rr.check_evaluation(bad, six)
    # the cost alone sees the defects that touch it, when the stored arrays are the right ones
    good["cost"] = bad["cost"]
    with pytest.raises(AssertionError, match=r"^cost: "):
        rr.check_evaluation(good, six)
    # ... and so does the independent restatement
    c_np = rr.numpy_cost(P, P, six)
    assert abs(bad["cost"] - c_np) > 1e-10 * c_np


# ---------------------------------------------------------------- the dense Levenberg-Marquardt and the depth chain
@pytest.mark.parametrize("six", [False, True])
def test_helper_lm_pulls_the_depth_chain_tenfold(six):
    spec, priors = qc.depth_chain()
    P = rr.local_problem(spec, six, 0, spec.n - 1, [], priors)
    x, cost, its = rr.lm_solve(P, P, six)
    z0 = np.asarray(P["t"]).reshape(-1, 3)[:, 2] - spec.t_true[:, 2]
    z1 = np.asarray(x["t"]).reshape(-1, 3)[:, 2] - spec.t_true[:, 2]
    rms0, rms1 = float(np.sqrt(np.mean(z0 ** 2))), float(np.sqrt(np.mean(z1 ** 2)))
    print("%d-DoF depth chain: helper LM %d iterations, cost %.6g, rms z error %.4g -> %.4g" % (6 if six else 4, its, cost, rms0, rms1))
    assert spec.n <= 40 and rms0 > 0.1 and rms1 <= rms0 / 10.0
    # at the optimum the gradient is gone: no descent direction is left to a first-order test
    F = rr.evaluate64(P, x, six)
    J = np.asarray(pr._dense_jacobian(P, F["Ja"], F["Jb"], 6 if six else 4), np.float64)
    assert np.max(np.abs(J.T @ F["res"].reshape(-1))) <= 1e-6 * max(1.0, float(np.sum(np.abs(J.T) @ np.abs(F["res"].reshape(-1)))))


def test_helper_lm_recovers_a_known_minimum():
    """a free-gauge chain whose poses are the generating ones moved rigidly, POSE prior on one keyframe at the truth: zero cost there"""
    spec, priors = qc.rigid_case(True)
    P = rr.local_problem(spec, True, 0, spec.n - 1, [], priors, gauge=1)
    x, cost, _ = rr.lm_solve(P, P, True)
    assert cost < 1e-18 * max(1.0, float(rr.evaluate64(P, P, True)["cost"])) or cost < 1e-20
    assert np.max(np.abs(np.asarray(x["t"]).reshape(-1, 3) - spec.t_true)) < 1e-8
