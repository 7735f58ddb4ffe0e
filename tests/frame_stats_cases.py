"""Inputs, censuses and plain restatements shared by the frame-statistics border tests (tests/test_frame_stats_ref.py on the
CPU, tests/test_frame_stats_edges.py on the GPU): k_frame_stats / k_mono_stats of csrc/hhsr_kernels.hip at degenerate
gradient grids, at the edges of the 32 x 16-quad tile, and on structured images that reach every exact-comparison branch of
Alg. 5 (the census below says which image reaches which branch).  Pure NumPy."""
import functools

import numpy as np

from oracle import kernels as ok
from oracle.grey import decimate_to_grey

F32, F64 = np.float32, np.float64

# raw H x W of a Bayer frame; the same numbers are pixel counts of a monochrome frame
DEGENERATE = [(2, 2), (2, 4), (4, 2), (2, 70), (70, 2), (4, 4)]  # gradient grid empty, one row, one column, one sample
TILE_EDGES = [(32, 64), (34, 66), (66, 130), (34, 450)]  # one tile; one quad past it; 3 x 3 workgroups; 8 x 2 workgroups
SHAPES = DEGENERATE + TILE_EDGES
REF_SHAPES = DEGENERATE + [(34, 66)]  # scalar restatement and golden "frame_stats_edges"
ODD_SHAPE = (35, 67)
LAWS = ["hard_threshold", "linear"]
SNR = 12.0  # tuning of test_cov_random_and_constant (k_detail 0.31, k_denoise 4.5, D_th 0.785, D_tr 1.18)
SWEEP_EXPONENTS = [-60, -20, 20, 60]
A_BAND, MAX_LEFT_OUT = 1e-5, 1e-3  # hard-threshold rule: |A - 1.95| < 1e-5 is left out, at most 0.1 % of a case's quads

# Largest difference between the oracle (reference typing: float32 tensor sums, float32 eigenvectors) and the float64
# computation cov_float64() on the well-conditioned quads of every Bayer case below, relative to the largest entry of the
# quad's covariance.  tests/test_frame_stats_ref.py::test_float64_reference measures it (2.134e-5, "dynamic" at 32 x 64,
# linear law) and asserts that this constant is that figure.  What it measures is the reference's eigenvector formula
# e1 ~ (T00 + T01 - l2, T01 + T11 - l2) — (T - l2 I) applied to (1, 1) — in float32: both components cancel when the
# gradient runs along the anti-diagonal.  The bound of the comparison is 4 x the figure (factor and reasoning of
# tests/test_tonemap.py, comparison 4: the kernel's own float32 roundings are of the size of the oracle's).
F64_SPREAD = 2.14e-5
F64_BOUND = 4 * F64_SPREAD


def frozen(a):
    a.setflags(write=False)
    return a


def config(law="hard_threshold", mode="bayer", beta=None):
    from helpers import base_config

    cfg = base_config(snr=SNR, ts=16, mode=mode)
    cfg.merging.selection_law = law
    if beta is not None:
        cfg.noise_model.beta = float(beta)
    return cfg


ALPHA, BETA = 1.80710882e-4, 3.1937599182128e-6  # helpers.ALPHA, helpers.BETA (asserted by test_frame_stats_ref.py)


def _alpha_beta():
    return ALPHA, BETA


# ---- short-mantissa images ---------------------------------------------------------------------------------------------
def _ordinal(v):
    """float32 -> integer that orders like the value (non-negative values only)."""
    return int(np.array(v, F32).view(np.uint32))


@functools.lru_cache(maxsize=None)
def raw_for_gat(target, alpha, beta):
    """A non-negative raw float32 value whose oracle.kernels.gat is exactly `target` (a float32), found by bisection over
    float32 ordinals (the transform is monotonic).  Around the working point a raw ulp moves the transform by less than
    an ulp of its result, so every float32 in its range is hit; the result is asserted."""
    target = F32(target)
    lo, hi = _ordinal(0.0), _ordinal(4.0)
    g = lambda o: ok.gat(np.array([o], np.uint32).view(F32), alpha, beta)[0]  # noqa: E731
    assert g(lo) <= target <= g(hi), (target, g(lo), g(hi))
    while lo < hi:  # smallest ordinal with gat >= target
        mid = (lo + hi) // 2
        if g(mid) >= target:
            hi = mid
        else:
            lo = mid + 1
    assert g(lo) == target, (float(target), float(g(lo)))
    return np.array([lo], np.uint32).view(F32)[0]


def _from_grey_levels(levels, H, W):
    """Raw frame [H, W] whose stabilised 2 x 2 quad mean is 96 + 2 levels[qy, qx] exactly (all four pixels of a quad carry
    the same raw value; 96 .. 128 lies inside the transform's range 20 .. 150 for raw values in [0, 1]): a slope of one
    level per quad is a gradient of exactly 1, squares and sums are exact in float32, and sqrt(l1) is 1 .. 2.83 — D lies
    in its transition band or on its lower clamp, where the covariance depends on the eigenvectors (at D = 1 it is
    isotropic and a swapped pair of vectors would go unseen)."""
    alpha, beta = _alpha_beta()
    gh, gw = H // 2, W // 2
    lut = {int(k): raw_for_gat(F32(96.0 + 2.0 * int(k)), alpha, beta) for k in np.unique(levels)}
    quad = np.vectorize(lut.__getitem__, otypes=[F32])(levels[:gh, :gw])
    return np.repeat(np.repeat(quad, 2, 0), 2, 1)


def _tri(n, period=8):
    """0 1 .. period .. 1 0 1 ..: slopes of +-1 that keep the levels (and the mantissas) short at any width."""
    k = np.arange(n) % (2 * period)
    return np.where(k <= period, k, 2 * period - k)


def _sm_x(H, W, seed):  # pure x-gradient: T01 = T11 = 0, l2 = 0, a1 == 0
    return _from_grey_levels(np.broadcast_to(_tri(W // 2)[None, :], (H // 2, W // 2)), H, W)


def _sm_y(H, W, seed):  # pure y-gradient: T00 = T01 = 0, l2 = 0, a0 == 0
    return _from_grey_levels(np.broadcast_to(_tri(H // 2)[:, None], (H // 2, W // 2)), H, W)


def _sm_diag(H, W, seed):  # 45 degrees: T00 == T11 == |T01| != 0
    return _from_grey_levels(_tri(H // 2)[:, None] + _tri(W // 2)[None, :], H, W)


def _sm_iso(H, W, seed):
    """x-slope +1 everywhere, y-slope +-1 with a ridge every 2 rows: a quad on a ridge sees the samples (a, a), (a, a),
    (a, -a), (a, -a): T01 == 0, T00 == T11 != 0 (the identity branch with a non-zero tensor)."""
    return _from_grey_levels(_tri(H // 2, 2)[:, None] + _tri(W // 2)[None, :], H, W)


# ---- image families: name -> (function of (H, W, seed), seed) --------------------------------------------------------------
def _yx(H, W):
    return np.arange(H, dtype=np.float64)[:, None], np.arange(W, dtype=np.float64)[None, :]


def _noise(H, W, seed):
    return np.random.default_rng(seed).random((H, W))


def _low_noise(H, W, seed):
    return 0.4 + 0.002 * np.random.default_rng(seed).standard_normal((H, W))


def _ramp_x(H, W, seed):
    y, x = _yx(H, W)
    return x / 256 + 0.1 + 0 * y


def _ramp_y(H, W, seed):
    y, x = _yx(H, W)
    return y / 256 + 0.1 + 0 * x


def _ramp_xy(H, W, seed):
    y, x = _yx(H, W)
    return (x + y) / 512 + 0.1


def _step(mask):
    return np.where(mask, 0.7, 0.2)


def _step_v(H, W, seed):
    y, x = _yx(H, W)
    return _step(x + 0 * y >= 2 * (W // 4))


def _step_h(H, W, seed):
    y, x = _yx(H, W)
    return _step(y + 0 * x >= 2 * (H // 4))


def _step_d1(H, W, seed):
    y, x = _yx(H, W)
    return _step(x // 2 + y // 2 >= (H + W) // 4)


def _step_d2(H, W, seed):
    y, x = _yx(H, W)
    return _step(x // 2 - y // 2 >= (W - H) // 4)


def _step_noise(H, W, seed):
    return _step_v(H, W, seed) + 0.003 * np.random.default_rng(seed).standard_normal((H, W))


def _checker(H, W, seed):
    y, x = _yx(H, W)
    return np.where((y // 4 + x // 4) % 2 == 0, 0.25, 0.6)


def _const(v):
    return lambda H, W, seed: np.full((H, W), v)


def _dynamic(H, W, seed):
    rng = np.random.default_rng(seed)
    return rng.random((H, W)).astype(F32) * np.exp2(-rng.integers(0, 29, (H, W)).astype(np.float64))


def _sweep(e):
    return lambda H, W, seed: _noise(H, W, seed).astype(F32) * np.exp2(float(e))


def _nan_inner(H, W, seed):
    img = _noise(H, W, seed)
    img[H // 2, W // 2] = np.nan  # (away from the border wherever the frame has an interior)
    return img


def _nan_corner(H, W, seed):
    img = _noise(H, W, seed)
    img[0, 0] = np.nan
    return img


FAMILIES = {
    "noise": (_noise, 101), "low_noise": (_low_noise, 102), "ramp_x": (_ramp_x, 0), "ramp_y": (_ramp_y, 0),
    "ramp_xy": (_ramp_xy, 0), "step_v": (_step_v, 0), "step_h": (_step_h, 0), "step_d1": (_step_d1, 0),
    "step_d2": (_step_d2, 0), "step_noise": (_step_noise, 113), "checker": (_checker, 0), "flat": (_const(0.3), 0),
    "zeros": (_const(0.0), 0), "negative": (_const(-0.1), 0), "neg_beta": (_noise, 104), "dynamic": (_dynamic, 105),
    "nan_inner": (_nan_inner, 106), "nan_corner": (_nan_corner, 107),
    "sm_x": (_sm_x, 0), "sm_y": (_sm_y, 0), "sm_diag": (_sm_diag, 0), "sm_iso": (_sm_iso, 0),
}
SWEEPS = {f"sweep{e:+d}": (_sweep(e), 110 + i) for i, e in enumerate(SWEEP_EXPONENTS)}  # the statistics only
COV_FAMILIES = list(FAMILIES)
STAT_FAMILIES = list(FAMILIES) + list(SWEEPS)
NAN_FAMILIES = ["nan_inner", "nan_corner"]


@functools.lru_cache(maxsize=None)
def image(family, H, W):
    """The raw float32 frame [H, W] of a family (read-only, shared)."""
    fn, seed = {**FAMILIES, **SWEEPS}[family]
    return frozen(np.ascontiguousarray(fn(H, W, seed), dtype=F32))


def beta_of(family):
    """The noise model's beta of a family: the default one, except for "neg_beta", where alpha v + 3/8 alpha^2 + beta <= 0
    for v <= 0.5 — about half of the samples of noise in [0, 1]."""
    alpha, beta = _alpha_beta()
    return -(0.5 * alpha + 3 / 8 * alpha * alpha) if family == "neg_beta" else beta


def family_config(family, law, mode="bayer"):
    return config(law, mode, beta_of(family))


# ---- the oracle's intermediates and the branch census -----------------------------------------------------------------------
def intermediates(raw, cfg):
    """The oracle's own intermediates of estimate_kernels (same functions, same order): dict of [gh, gw] arrays."""
    t = cfg.merging.tuning
    alpha, beta = cfg.noise_model.alpha, cfg.noise_model.beta
    arg = F64(alpha) * np.asarray(raw, F32).astype(F64) + 3 / 8 * F64(alpha) * F64(alpha) + F64(beta)
    vst = ok.gat(raw, alpha, beta)
    grey = decimate_to_grey(vst) if cfg.mode == "bayer" else vst
    gh, gw = grey.shape
    gx, gy = ok._gradients(grey)
    pgx, pgy = np.zeros((gh + 1, gw + 1), F32), np.zeros((gh + 1, gw + 1), F32)
    pgx[1:gh, 1:gw], pgy[1:gh, 1:gw] = gx, gy
    T00, T01, T11 = np.zeros((gh, gw), F32), np.zeros((gh, gw), F32), np.zeros((gh, gw), F32)
    for i in range(2):
        for j in range(2):
            ax, ay = pgx[i:i + gh, j:j + gw], pgy[i:i + gh, j:j + gw]
            T00 += ax * ax
            T01 += ax * ay
            T11 += ay * ay
    l1, l2, *_ = ok.eigen_2x2(T00, T01, T01, T11)
    with np.errstate(all="ignore"):
        b = -(T00 + T11)
        c = T00 * T11 - T01 * T01
        delta = (b * b).astype(F32).astype(F64) - 4 * c.astype(F64)
        sq = np.sqrt(np.where(delta > 0, delta, 0.0))
        r1, r2 = (-b.astype(F64) + sq) / 2, (-b.astype(F64) - sq) / 2
        A = 1 + np.sqrt(((l1 - l2) / (l1 + l2)).astype(F32)).astype(F32).astype(F64)
        D = 1 - np.sqrt(l1).astype(F32).astype(F64) / F64(t.D_tr) + F64(t.D_th)  # before the clamps
        ratio = (l1.astype(F64) - l2) / (l1.astype(F64) + l2)
    ident = (T01 == 0) & (T00 == T11)
    return dict(arg=arg, grey=grey, T00=T00, T01=T01, T11=T11, l1=l1, l2=l2, r1=r1, r2=r2, A=A, D=D, ratio=ratio,
                ident=ident, a0=(T00 + T01 - l2).astype(F32), a1=(T01 + T11 - l2).astype(F32))


CENSUS_KEYS = ["D<=0", "D band", "D>=1 finite", "A==2", "l2<0", "A NaN", "a0==0", "a1==0", "a0==a1==0", "ident T!=0",
               "T01==0 T00!=T11", "gat arg<=0", "|r1|<|r2|", "near 1.95"]


def census(raw, cfg, covs):
    """Quads (pixels of the raw frame for "gat arg<=0") of one case per branch of quad_cov; `covs`: the oracle's result."""
    m = intermediates(raw, cfg)
    fin = np.isfinite(covs).all((-1, -2))
    with np.errstate(all="ignore"):
        out = {
            "D<=0": m["D"] <= 0, "D band": (m["D"] > 0) & (m["D"] < 1), "D>=1 finite": (m["D"] >= 1) & fin,
            "A==2": m["A"] == 2, "l2<0": m["l2"] < 0, "A NaN": np.isnan(m["A"]),
            "a0==0": ~m["ident"] & (m["a0"] == 0), "a1==0": ~m["ident"] & (m["a1"] == 0),
            "a0==a1==0": ~m["ident"] & (m["a0"] == 0) & (m["a1"] == 0),
            "ident T!=0": m["ident"] & (m["T00"] != 0), "T01==0 T00!=T11": (m["T01"] == 0) & (m["T00"] != m["T11"]),
            "gat arg<=0": m["arg"] <= 0, "|r1|<|r2|": np.abs(m["r1"]) < np.abs(m["r2"]),
            "near 1.95": np.abs(m["A"] - 1.95) < A_BAND,
        }
    return {k: int(v.sum()) for k, v in out.items()}


def compared(raw, cfg):
    """Boolean [gh, gw]: the quads whose covariance is compared — all of them under the linear law; under the hard
    threshold those whose oracle A is not within A_BAND of the discontinuity at 1.95."""
    A = intermediates(raw, cfg)["A"]
    if cfg.merging.selection_law != "hard_threshold":
        return np.ones(A.shape, bool)
    with np.errstate(all="ignore"):
        return ~(np.abs(A - 1.95) < A_BAND)


def well_conditioned(raw, cfg):
    """Boolean [gh, gw]: finite A, (l1 - l2) / (l1 + l2) > 0.05 and D strictly inside (0, 1), away from the threshold —
    except the quads where the reference does not compute an eigen-decomposition at all: outside the identity case
    a0 == a1 == 0 (a gradient exactly along the anti-diagonal, SURVEY.md D19: e1 = (0, 1) for the true (1, -1) / sqrt 2;
    oracle, kernel and the reference's own run agree there bit for bit, float64 differs by 0.91 of the largest entry)."""
    m = intermediates(raw, cfg)
    with np.errstate(all="ignore"):
        d19 = ~m["ident"] & (m["a0"] == 0) & (m["a1"] == 0)
        return np.isfinite(m["A"]) & (m["ratio"] > 0.05) & (m["D"] > 0) & (m["D"] < 1) & compared(raw, cfg) & ~d19


def cov_float64(raw, cfg):
    """Alg. 5 in plain float64 from the stabilised float32 grey image on (the image both sides store in float32): the two
    gradient filters, the 2 x 2-window structure tensor, numpy.linalg.eigh, k1 / k2 by the same formulas, the covariance
    k1^2 e1 e1^T + k2^2 e2 e2^T.  float64 [gh, gw, 2, 2]."""
    t = cfg.merging.tuning
    vst = ok.gat(raw, cfg.noise_model.alpha, cfg.noise_model.beta)
    g = (decimate_to_grey(vst) if cfg.mode == "bayer" else vst).astype(F64)
    gh, gw = g.shape
    gx = (g[:-1, 1:] - g[:-1, :-1] + g[1:, 1:] - g[1:, :-1]) / 4
    gy = (g[1:, :-1] - g[:-1, :-1] + g[1:, 1:] - g[:-1, 1:]) / 4
    px, py = np.zeros((gh + 1, gw + 1)), np.zeros((gh + 1, gw + 1))
    px[1:gh, 1:gw], py[1:gh, 1:gw] = gx, gy
    T = np.zeros((gh, gw, 2, 2))
    for i in range(2):
        for j in range(2):
            ax, ay = px[i:i + gh, j:j + gw], py[i:i + gh, j:j + gw]
            T[..., 0, 0] += ax * ax
            T[..., 0, 1] += ax * ay
            T[..., 1, 1] += ay * ay
    T[..., 1, 0] = T[..., 0, 1]
    w, vec = np.linalg.eigh(T)  # ascending
    l1, l2, e1, e2 = w[..., 1], w[..., 0], vec[..., :, 1], vec[..., :, 0]
    with np.errstate(all="ignore"):
        A = 1 + np.sqrt((l1 - l2) / (l1 + l2))
        D = np.clip(1 - np.sqrt(l1) / t.D_tr + t.D_th, 0, 1)
        if cfg.merging.selection_law == "hard_threshold":
            k1, k2 = np.where(A > 1.95, 1 / t.k_shrink, 1.0), np.where(A > 1.95, float(t.k_stretch), 1.0)
        else:
            k1, k2 = 1 + A / 2 * (1 / t.k_shrink - 1), 1 + A / 2 * (t.k_stretch - 1)
        k1 = t.k_detail * ((1 - D) * k1 + D * t.k_denoise)
        k2 = t.k_detail * ((1 - D) * k2 + D * t.k_denoise)
        return (k1 * k1)[..., None, None] * e1[..., :, None] * e1[..., None, :] + \
            (k2 * k2)[..., None, None] * e2[..., :, None] * e2[..., None, :]


def f64_spread(covs, raw, cfg):
    """(largest |covs - cov_float64| over the well-conditioned quads relative to the quad's largest entry, their number)."""
    sel = well_conditioned(raw, cfg)
    if not sel.any():
        return 0.0, 0
    want = cov_float64(raw, cfg)[sel]
    d = np.abs(np.asarray(covs, F64)[sel] - want).max((-1, -2)) / np.abs(want).max((-1, -2))
    return float(d.max()), int(sel.sum())


# ---- scalar restatements: one quad at a time, the reference's typing statement by statement ---------------------------------
def guide_scalar(raw, cfa, wb):
    """robustness.py:207-226 per quad: x = raw / wb[c] in float64 (float32 / float64), g an integer 0 that the first green
    turns into a float64, the other colours stored float32, green g / 2 stored float32."""
    raw = np.asarray(raw, F32)
    h, w = raw.shape[0] // 2, raw.shape[1] // 2
    guide = np.zeros((3, h, w), F32)
    with np.errstate(all="ignore"):
        for ty in range(h):
            for tx in range(w):
                g = 0
                for i in range(2):
                    for j in range(2):
                        c = int(cfa[i][j])
                        x = F64(raw[2 * ty + i, 2 * tx + j]) / F64(wb[c])
                        if c == 1:
                            g = g + x
                        else:
                            guide[c, ty, tx] = F32(x)
                guide[1, ty, tx] = F32(g / 2)
    return guide


def local_stats_scalar(guide):
    """robustness.py:269-294 per position: two float32 running sums over the clamped 3 x 3 window in (i, j) order, the
    mean and the variance from float64 quotients by 9, stored float32."""
    guide = np.asarray(guide, F32)
    nc, h, w = guide.shape
    mean, var = np.zeros_like(guide), np.zeros_like(guide)
    with np.errstate(all="ignore"):
        for ch in range(nc):
            for idy in range(h):
                for idx in range(w):
                    s0, s1 = F32(0), F32(0)
                    for i in range(-1, 2):
                        for j in range(-1, 2):
                            v = guide[ch, min(max(idy + i, 0), h - 1), min(max(idx + j, 0), w - 1)]
                            s0 = F32(s0 + v)
                            s1 = F32(s1 + F32(v * v))
                    m = F64(s0) / 9
                    mean[ch, idy, idx] = F32(m)
                    var[ch, idy, idx] = F32(F64(s1) / 9 - m * m)
    return mean, var


def _pymax0(v):
    return v if v > 0 else F64(0)  # max(v, 0) with a NaN v: 0


def cov_scalar(raw, cfg):
    """kernels.py:29-243 and linalg.py:87-185 per quad on np.float32 / np.float64 scalars: float32 [gh, gw, 2, 2]."""
    t = cfg.merging.tuning
    law = cfg.merging.selection_law
    kd, kn, D_th, D_tr = F64(t.k_detail), F64(t.k_denoise), F64(t.D_th), F64(t.D_tr)
    k_stretch, k_shrink = F64(t.k_stretch), F64(t.k_shrink)
    alpha, beta = F64(cfg.noise_model.alpha), F64(cfg.noise_model.beta)
    raw = np.asarray(raw, F32)
    H, W = raw.shape
    h5, m5 = F32(0.5), F32(-0.5)
    with np.errstate(all="ignore"):
        # utils_image.py:157-170 per pixel, :346-357 per quad
        vst = np.empty((H, W), F32)
        for y in range(H):
            for x in range(W):
                v = alpha * F64(raw[y, x]) + 3 / 8 * alpha * alpha + beta
                vst[y, x] = F32(2 / alpha * np.sqrt(_pymax0(v)))
        if cfg.mode == "bayer":
            gh, gw = H // 2, W // 2
            grey = np.empty((gh, gw), F32)
            for y in range(gh):
                for x in range(gw):
                    c = 0
                    for i in range(2):
                        for j in range(2):
                            c = c + F64(vst[2 * y + i, 2 * x + j])
                    grey[y, x] = F32(c / 4)
        else:
            gh, gw, grey = H, W, vst
        covs = np.empty((gh, gw, 2, 2), F32)
        for y in range(gh):
            for x in range(gw):
                T00 = T01 = T11 = F32(0)
                for i in range(2):
                    for j in range(2):
                        sy, sx = y - 1 + i, x - 1 + j
                        if 0 <= sy < gh - 1 and 0 <= sx < gw - 1:
                            g00, g01, g10, g11 = grey[sy, sx], grey[sy, sx + 1], grey[sy + 1, sx], grey[sy + 1, sx + 1]
                            t0a, t0b = F32(m5 * g00 + h5 * g01), F32(m5 * g10 + h5 * g11)
                            t1a, t1b = F32(h5 * g00 + h5 * g01), F32(h5 * g10 + h5 * g11)
                            vx, vy = F32(h5 * t0a + h5 * t0b), F32(m5 * t1a + h5 * t1b)
                            T00 = F32(T00 + F32(vx * vx))
                            T01 = F32(T01 + F32(vx * vy))
                            T11 = F32(T11 + F32(vy * vy))
                # linalg.py:113-130
                b = F32(-F32(T00 + T11))
                c = F32(F32(T00 * T11) - F32(T01 * T01))
                delta = _pymax0(F64(F32(b * b)) - 4 * F64(c))
                r1, r2 = (-F64(b) + np.sqrt(delta)) / 2, (-F64(b) - np.sqrt(delta)) / 2
                l1, l2 = (F32(r1), F32(r2)) if abs(r1) >= abs(r2) else (F32(r2), F32(r1))
                # linalg.py:154-179
                if T01 == 0 and T00 == T11:
                    e1, e2 = [F32(1), F32(0)], [F32(0), F32(1)]
                else:
                    e1 = [F32(F32(T00 + T01) - l2), F32(F32(T01 + T11) - l2)]
                    if e1[0] == 0:
                        e1[1] = F32(1)
                        e2 = [F32(1), F32(0)]
                    elif e1[1] == 0:
                        e1[0] = F32(1)
                        e2 = [F32(0), F32(1)]
                    else:
                        n = F32(np.sqrt(F32(F32(e1[0] * e1[0]) + F32(e1[1] * e1[1]))))
                        e1 = [F32(e1[0] / n), F32(e1[1] / n)]
                        e2 = [F32(-e1[1] * F32(np.copysign(F32(1), e1[0]))), F32(abs(e1[0]))]
                # kernels.py:218-243
                A = 1 + F64(F32(np.sqrt(F32(F32(l1 - l2) / F32(l1 + l2)))))
                D = 1 - F64(F32(np.sqrt(l1))) / D_tr + D_th
                D = D if D > 0 else F64(0)
                D = D if D < 1 else F64(1)
                if law == "hard_threshold":
                    k1, k2 = (1 / k_shrink, k_stretch) if A > 1.95 else (F64(1), F64(1))
                else:
                    k1, k2 = 1 + A / 2 * (1 / k_shrink - 1), 1 + A / 2 * (k_stretch - 1)
                k1, k2 = F32(kd * ((1 - D) * k1 + D * kn)), F32(kd * ((1 - D) * k2 + D * kn))
                k1s, k2s = F32(k1 * k1), F32(k2 * k2)
                c01 = F32(F32(F32(k1s * e1[0]) * e1[1]) + F32(F32(k2s * e2[0]) * e2[1]))
                covs[y, x, 0, 0] = F32(F32(F32(k1s * e1[0]) * e1[0]) + F32(F32(k2s * e2[0]) * e2[0]))
                covs[y, x, 0, 1] = covs[y, x, 1, 0] = c01
                covs[y, x, 1, 1] = F32(F32(F32(k1s * e1[1]) * e1[1]) + F32(F32(k2s * e2[1]) * e2[1]))
    return covs


# ---- the golden "frame_stats_edges" (tools/refsim/make_goldens.py, stage frame_stats_edges) ---------------------------------
GOLDEN_CFA, GOLDEN_WB = [[0, 1], [1, 2]], [1.9, 1.0, 1.6]


def golden_key(family, H, W):
    return f"{family}_{H}x{W}"
