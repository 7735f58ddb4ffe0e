"""NumPy restatement of the sharpness score of include/hhsr.h ("reference selection"), independent of the kernel.

A frame is [H][W] with H and W even.  Values: a float32 frame's own, float32(count) for integer counts.  Green image at
half resolution: (v_a + v_b) * 0.5f over the two CFA positions that are green (cell order (row & 1) * 2 + (col & 1)), or
((v00 + v01) + (v10 + v11)) * 0.25f without a CFA.  Terms: the squared float32 differences of horizontal and vertical
neighbours of the green image.  Score: their sum — here exactly rounded (math.fsum), which every float64 summation
order approximates to n_terms 2^-52 relative for non-negative terms."""
import math

import numpy as np


def green_image(frame, cfa=None):
    """float32 [H/2, W/2] green image of a frame (float32 values or integer counts)."""
    v = np.asarray(frame)
    if v.ndim != 2 or v.shape[0] % 2 or v.shape[1] % 2 or 0 in v.shape:
        raise ValueError(f"frame must be [H, W] with even sizes, got {v.shape}")
    v = v.astype(np.float32)
    q = [v[0::2, 0::2], v[0::2, 1::2], v[1::2, 0::2], v[1::2, 1::2]]  # cell order
    with np.errstate(all="ignore"):
        if cfa is None:
            return ((q[0] + q[1]) + (q[2] + q[3])) * np.float32(0.25)
        flat = [int(c) for c in np.asarray(cfa).reshape(-1)]
        greens = [k for k, c in enumerate(flat) if c == 1]
        if len(flat) != 4 or len(greens) != 2 or max(flat) > 2:
            raise ValueError(f"cfa {cfa!r}: 2 x 2 with exactly two entries equal to 1 and none above 2")
        return (q[greens[0]] + q[greens[1]]) * np.float32(0.5)


def terms(frame, cfa=None):
    """The h (w - 1) + (h - 1) w float32 terms of a frame, 1-D (dx terms row-major, then dy terms row-major)."""
    g = green_image(frame, cfa)
    with np.errstate(all="ignore"):
        dx = g[:, 1:] - g[:, :-1]
        dy = g[1:, :] - g[:-1, :]
        out = np.concatenate([(dx * dx).reshape(-1), (dy * dy).reshape(-1)])
    assert out.dtype == np.float32
    return out


def n_terms(H, W):
    h, w = H // 2, W // 2
    return h * (w - 1) + (h - 1) * w


def score(frame, cfa=None):
    """The exactly rounded score (NaN / Inf as IEEE addition gives them: fsum refuses them)."""
    t = terms(frame, cfa).astype(np.float64)
    if not np.isfinite(t).all():
        with np.errstate(all="ignore"):
            return float(t.sum())
    return math.fsum(t.tolist())


def select(scores, candidates=None):
    """Index of the largest finite score among the first `candidates`, ties to the lowest index; 0 if none is finite."""
    s = np.asarray(scores, np.float64)
    n = len(s) if candidates is None else min(int(candidates), len(s))
    best, arg = -math.inf, 0
    for i in range(n):
        if math.isfinite(s[i]) and s[i] > best:
            best, arg = float(s[i]), i
    return arg
