"""NumPy restatement of the noise-profile estimator of include/hhsr.h ("noise profile"), independent of the kernel and of the
library's fit: the tile histogram (the contract of hhsr_noise_profile_hist) and the line fit (hhsr_noise_profile_fit)."""
import numpy as np

MEAN_BINS, ENERGY_BINS = 64, 1024
ENERGY_BASE = (127 - 32) << 5
COLOURS = ("red", "green", "blue")


def inv_gains(cfa, white_balance):
    """float32 [4]: the float32 reciprocal of wb[cfa[p]] / wb[1] per CFA position; all 1 without a CFA."""
    if cfa is None:
        return np.ones(4, np.float32)
    wb = np.asarray(white_balance, np.float64)
    flat = [int(v) for v in np.asarray(cfa).reshape(-1)]
    return np.array([np.float32(1.0) / np.float32(wb[c] / wb[1]) for c in flat], np.float32)


def _rows_then_columns(a):
    """float64 sum of [..., rows, cols]: each row left to right, then the row sums top to bottom."""
    rs = a[..., 0]
    for k in range(1, a.shape[-1]):
        rs = rs + a[..., k]
    s = rs[..., 0]
    for j in range(1, rs.shape[-1]):
        s = s + rs[..., j]
    return s


def tile_stats(frame, inv_gain):
    """(ok, m, e) per plane and tile: bool / float64 / float32 [4][h // 8][w // 8] (empty for a frame without a tile)."""
    f = np.asarray(frame)
    if f.ndim != 2 or f.shape[0] % 2 or f.shape[1] % 2:
        raise ValueError("even 2-D frame expected")
    f = f.astype(np.float32, copy=False)
    nby, nbx = f.shape[0] // 16, f.shape[1] // 16
    ok = np.zeros((4, nby, nbx), bool)
    m = np.zeros((4, nby, nbx), np.float64)
    e = np.zeros((4, nby, nbx), np.float32)
    if nby == 0 or nbx == 0:
        return ok, m, e
    with np.errstate(all="ignore"):
        for p in range(4):
            plane = f[p >> 1::2, p & 1::2][:8 * nby, :8 * nbx] * np.float32(inv_gain[p])  # float32 product
            t = plane.reshape(nby, 8, nbx, 8).transpose(0, 2, 1, 3)  # [nby][nbx][8][8]
            assert t.dtype == np.float32
            ok[p] = ((t > 0) & (t < 1)).all(axis=(2, 3))
            m[p] = _rows_then_columns(t.astype(np.float64)) / 64.0
            r = t[:, :, 1:7, 1:7] - np.float32(0.25) * ((t[:, :, 1:7, 0:6] + t[:, :, 1:7, 2:8])
                                                         + (t[:, :, 0:6, 1:7] + t[:, :, 2:8, 1:7]))
            rr = r * r
            assert rr.dtype == np.float32
            e[p] = (_rows_then_columns(rr.astype(np.float64)) / 45.0).astype(np.float32)
    return ok, m, e


def bins(m, e):
    """(mean bin, energy bin) of a tile's (float64 m, float32 e)."""
    with np.errstate(all="ignore"):
        b = np.minimum(63, np.nan_to_num(np.asarray(m, np.float64) * 64.0).astype(np.int64))
    bits = np.asarray(e, np.float32).view(np.uint32).astype(np.int64)
    k = np.clip((bits >> 18) - ENERGY_BASE, 0, ENERGY_BINS - 1)
    return b, k


def histogram(frames, cfa=None, white_balance=None, inv_gain=None):
    """uint32 [4][64][1024] of a list of frames of one shape."""
    g = inv_gains(cfa, white_balance) if inv_gain is None else np.asarray(inv_gain, np.float32)
    hist = np.zeros((4, MEAN_BINS, ENERGY_BINS), np.uint32)
    for f in frames:
        ok, m, e = tile_stats(f, g)
        ok = ok & (e != 0)
        b, k = bins(m, e)
        for p in range(4):
            np.add.at(hist[p], (b[p][ok[p]], k[p][ok[p]]), 1)
    return hist


def edge(k):
    """Lower edge of energy bin k as float64 (k = 1024: 1.0)."""
    return float(np.array([(k + ENERGY_BASE) << 18], np.uint32).view(np.float32)[0])


def fit_colour(h, min_tiles=16):
    """(alpha, beta, bins used) of one colour's histogram [64][1024] (integer counts); alpha = beta = None below 2 bins."""
    h = np.asarray(h).astype(np.int64)
    Sw = Swx = Swy = Swxx = Swxy = 0.0
    used = 0
    for b in range(MEAN_BINS):
        n = int(h[b].sum())
        if n == 0 or n < min_tiles:
            continue
        target = 0.5 * float(n)
        cum = np.cumsum(h[b])
        k = int(np.argmax(cum >= target))
        prev = int(cum[k]) - int(h[b, k])
        lo, hi = edge(k), edge(k + 1)
        y = lo + (target - float(prev)) / float(h[b, k]) * (hi - lo)
        x = (b + 0.5) / 64.0
        w = float(n) / (y * y)
        Sw += w
        Swx += w * x
        Swy += w * y
        Swxx += w * x * x
        Swxy += w * x * y
        used += 1
    if used < 2:
        return None, None, used
    det = Sw * Swxx - Swx * Swx
    a, c = (Sw * Swxy - Swx * Swy) / det, (Swxx * Swy - Swx * Swxy) / det
    if c < 0.0:
        a, c = Swxy / Swxx, 0.0
    elif a < 0.0:
        a, c = 0.0, Swy / Sw
    return a, c, used


def fit(hist, cfa=None, min_tiles=16):
    """{"alpha", "beta", "per_colour": [(alpha, beta)] * 3, "bins_used": [3]}; ValueError below 2 usable bins of a colour."""
    hist = np.asarray(hist).reshape(4, MEAN_BINS, ENERGY_BINS).astype(np.int64)
    flat = None if cfa is None else [int(v) for v in np.asarray(cfa).reshape(-1)]
    pairs, used = [], []
    for c in range(3):
        planes = [p for p in range(4) if flat is None or flat[p] == c]
        a, b, n = fit_colour(sum((hist[p] for p in planes), np.zeros((MEAN_BINS, ENERGY_BINS), np.int64)), min_tiles)
        pairs.append((a, b))
        used.append(n)
    for c in range(3):
        if used[c] < 2:
            raise ValueError(f"noise profile: {COLOURS[c]} has {used[c]} usable mean bins, a line needs 2")
    if flat is None:
        alpha, beta = pairs[0]
    else:
        alpha, beta = (pairs[0][0] + pairs[1][0] + pairs[2][0]) / 3.0, (pairs[0][1] + pairs[1][1] + pairs[2][1]) / 3.0
    return {"alpha": alpha, "beta": beta, "per_colour": pairs, "bins_used": used}


def estimate(frames, cfa=None, white_balance=None, min_tiles=16):
    return fit(histogram(frames, cfa, white_balance), cfa, min_tiles)


def smooth_scene(H, W):
    """The texture-free test scene of the accuracy checks, float64 [H][W] in [0.05, 0.95]."""
    y, x = np.mgrid[0:H, 0:W].astype(np.float64)
    return 0.05 + 0.9 * (0.5 * x / W + 0.25 + 0.25 * np.sin(3 * np.pi * y / H))


def noisy(scene, alpha, beta, seed):
    """scene + N(0, alpha scene + beta), clipped to [0, 1], float32."""
    rng = np.random.default_rng(seed)
    return np.clip(scene + rng.standard_normal(scene.shape) * np.sqrt(alpha * scene + beta), 0.0, 1.0).astype(np.float32)


def sigma_error(alpha, beta, alpha0, beta0):
    """Largest relative error of sqrt(alpha x + beta) against (alpha0, beta0) over x = 0.1 .. 0.9."""
    x = np.linspace(0.1, 0.9, 9)
    return float(np.max(np.abs(np.sqrt(alpha * x + beta) / np.sqrt(alpha0 * x + beta0) - 1.0)))
