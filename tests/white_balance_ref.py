"""NumPy restatement of the white-balance estimator of include/hhsr.h ("white balance"), independent of the kernel and of the
library's fit: the tile histogram (the contract of hhsr_white_balance_hist), the fit (hhsr_white_balance_fit), and a small
"camera" that divides known gains out of a balanced scene and quantises it to counts."""
import math

import numpy as np

BINS = 192
BIN_BASE = (127 - 2) << 5
LOW = np.float32(1.0 / 64.0)


def sat_counts(black_levels, white_level):
    """Per colour the count from which a tile is dropped: ceil(black + 15 / 16 (white - black)) in float64."""
    return [int(math.ceil(float(b) + 15.0 / 16.0 * (float(white_level) - float(b)))) for b in list(black_levels)[:3]]


def tile_bins(counts, cfa, black_levels, white_level):
    """(keep, u, v) per whole 16 x 16 tile of integer counts [H][W]: bool / int64 / int64 [H // 16][W // 16]."""
    p = np.asarray(counts).astype(np.int64)
    if p.ndim != 2 or p.shape[0] % 2 or p.shape[1] % 2:
        raise ValueError("even 2-D frame expected")
    flat = [int(v) for v in np.asarray(cfa).reshape(-1)]
    assert sorted(flat) == [0, 1, 1, 2], "one R, two G, one B"
    nby, nbx = p.shape[0] // 16, p.shape[1] // 16
    S = np.zeros((3, nby, nbx), np.int64)
    clipped = np.zeros((nby, nbx), bool)
    sat = sat_counts(black_levels, white_level)
    for q in range(4):
        plane = p[q >> 1::2, q & 1::2][:8 * nby, :8 * nbx].reshape(nby, 8, nbx, 8)
        S[flat[q]] += plane.sum(axis=(1, 3))
        clipped |= (plane >= sat[flat[q]]).any(axis=(1, 3))
    assert S.max(initial=0) < 1 << 24
    m = []
    for c in range(3):  # every operation float32 op float32 -> float32, one rounding each
        n = np.float32(128 if c == 1 else 64)
        black = np.float32(float(black_levels[c]))
        den = np.float32(float(white_level) - float(black_levels[c]))
        mc = (S[c].astype(np.float32) / n - black) / den
        assert mc.dtype == np.float32
        m.append(mc)
    keep = ~clipped & (m[0] >= LOW) & (m[1] >= LOW) & (m[2] >= LOW)
    with np.errstate(all="ignore"):
        qr, qb = m[1] / m[0], m[1] / m[2]
    assert qr.dtype == np.float32 and qb.dtype == np.float32
    u = (qr.view(np.uint32).astype(np.int64) >> 18) - BIN_BASE
    v = (qb.view(np.uint32).astype(np.int64) >> 18) - BIN_BASE
    keep &= (u >= 0) & (u < BINS) & (v >= 0) & (v < BINS)
    return keep, u, v


def histogram(frames, cfa, black_levels, white_level):
    """uint32 [192][192] of a list of frames of integer counts."""
    hist = np.zeros((BINS, BINS), np.uint32)
    for f in frames:
        keep, u, v = tile_bins(f, cfa, black_levels, white_level)
        np.add.at(hist, (u[keep], v[keep]), 1)
    return hist


def centre(k):
    """Centre of bin k in log2 units."""
    return math.log2(2.0 ** (k // 32 - 2) * (1.0 + ((k % 32) + 0.5) / 32.0))


CENTRES = np.array([centre(k) for k in range(BINS)], np.float64)


def _centroid(h, mask):
    n = int(h[mask].sum())
    if n == 0:
        return 0, None, None
    cu = np.broadcast_to(CENTRES[:, None], h.shape)
    cv = np.broadcast_to(CENTRES[None, :], h.shape)
    return n, float((h[mask] * cu[mask]).sum() / n), float((h[mask] * cv[mask]).sum() / n)


def fit(hist, min_tiles=16, gate=True):
    """{"white_balance": [r, 1.0, b], "tiles": N, "tiles_gated": n}; gate False: the un-gated centroid (tiles_gated = N)."""
    h = np.asarray(hist).reshape(BINS, BINS).astype(np.float64)
    N, u, v = _centroid(h, np.ones(h.shape, bool))
    if N < min_tiles:
        raise ValueError(f"white balance: {N} usable tiles, fewer than min_tiles = {min_tiles}")
    gated = N
    if gate:
        for _ in range(4):
            d2 = (CENTRES[:, None] - u) ** 2 + (CENTRES[None, :] - v) ** 2
            n, gu, gv = _centroid(h, (d2 <= 0.25) & (h > 0))
            gated = n
            if n == 0:
                break
            u, v = gu, gv
    return {"white_balance": [2.0 ** u, 1.0, 2.0 ** v], "tiles": N, "tiles_gated": gated}


def estimate(frames, cfa, black_levels, white_level, min_tiles=16, gate=True):
    return fit(histogram(frames, cfa, black_levels, white_level), min_tiles, gate)


def camera(scene, cfa, gains, black=64, white=1023):
    """Counts a sensor would give for the balanced float scene [H][W] (values in [0, 1], CFA-sampled): the gains divided
    out per colour, scaled to [black, white], rounded; uint16."""
    f = np.asarray(scene, np.float64).copy()
    for q in range(4):
        f[q >> 1::2, q & 1::2] /= gains[int(cfa[q >> 1][q & 1])] / gains[1]
    return np.clip(np.rint(np.clip(f, 0.0, 1.0) * (white - black) + black), 0, 65535).astype(np.uint16)


def paint_block(scene, cfa, rows, rgb=(0.8, 0.15, 0.1)):
    """The scene with a saturated-colour block (balanced values `rgb`) over its top `rows` rows."""
    f = np.asarray(scene, np.float64).copy()
    for q in range(4):
        f[q >> 1:rows:2, q & 1::2] = rgb[int(cfa[q >> 1][q & 1])]
    return f


def gain_error(wb, gains):
    """Largest relative error of the R and B gains."""
    return max(abs(wb[0] / (gains[0] / gains[1]) - 1.0), abs(wb[2] / (gains[2] / gains[1]) - 1.0))
