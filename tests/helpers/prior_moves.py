"""Designed moves of the blocks of a marginalisation prior away from their linearisation points, shared by
tests/test_prior_reference_host.py (oracle windows) and tests/test_gpu_prior_edges.py / test_gpu_step_edges.py (device windows).
A move goes through the estimator's own setter; what its getter returns afterwards is the data the reference is given.

  at_lin    the control: nothing moves
  tiny      1e-9 m and 1e-9 rad, 1e-9 on speed / bias: q * q_lin^-1 cancels to nine digits
  large     poses 0.5 m and 0.8 rad about a skew axis, extrinsics 0.01 m and 0.05 rad, speed +-1, biases +-0.1
  flipped   0.01 rad (0.01 m), the stored quaternion negated on every other pose / extrinsics block
  constant  `large`; the caller then sets one pose of the prior constant
"""
import numpy as np

MOVES = ("at_lin", "tiny", "large", "flipped", "constant")


def quat_mul(a, b):
    """a * b, quaternions as (x, y, z, w)"""
    return np.array([a[3] * b[0] + a[0] * b[3] + a[1] * b[2] - a[2] * b[1],
                     a[3] * b[1] + a[1] * b[3] + a[2] * b[0] - a[0] * b[2],
                     a[3] * b[2] + a[2] * b[3] + a[0] * b[1] - a[1] * b[0],
                     a[3] * b[3] - a[0] * b[0] - a[1] * b[1] - a[2] * b[2]])


def _axis(k):
    a = np.array([1.0 + 0.3 * k, -2.0 + 0.7 * (k % 3), 3.0 - 0.5 * (k % 5)])   # skew: no coordinate axis, another one per block
    return a / np.linalg.norm(a)


def moved_value(move, kind, k, x):
    """the value of block number k of the prior (kind "p" | "e" | "s") after `move`, from its value x"""
    x = np.array(x, np.float64)
    if move == "at_lin":
        return x
    sign = np.array([1.0, -1.0, 1.0, -1.0, 1.0, -1.0, 1.0, -1.0, 1.0]) * (1.0 if k % 2 == 0 else -1.0)
    if kind == "s":
        step = {"tiny": np.full(9, 1e-9), "flipped": np.full(9, 0.01)}.get(move, np.r_[np.full(3, 1.0), np.full(6, 0.1)])
        return x + sign * step
    pose = kind == "p"
    length, angle = {"tiny": (1e-9, 1e-9), "flipped": (0.01, 0.01)}.get(move, (0.5, 0.8) if pose else (0.01, 0.05))
    ax = _axis(k)
    dq = np.r_[np.sin(0.5 * angle) * ax, np.cos(0.5 * angle)]
    q = quat_mul(dq, x[3:7])
    if move == "flipped" and k % 2 == 1:
        q = -q
    return np.r_[x[:3] + length * _axis(k + 1) * sign[:3], q]


def apply(move, blocks, get, put):
    """blocks: [(kind, id)] of the prior's blocks that have rows; get(id) -> value, put(id, value).  Returns the number of blocks
    whose stored quaternion kept the negative sign it was given (0 unless move == "flipped")."""
    kept = 0
    for k, (kind, bid) in enumerate(blocks):
        want = moved_value(move, kind, k, get(bid))
        if move != "at_lin":
            put(bid, want)
        if move == "flipped" and kind != "s" and k % 2 == 1:
            got = np.asarray(get(bid))
            kept += int(np.sign(got[3:7] @ want[3:7]) > 0)
    return kept
