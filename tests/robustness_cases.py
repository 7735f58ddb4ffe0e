"""Inputs and censuses shared by the robustness border tests (tests/test_robustness_ref.py on the CPU,
tests/test_robustness_edges.py on the GPU): the kernels of csrc/hhsr_robustness.hip at flow ties, image borders, invalid
flows and the thresholds of S, sigma^2 and the local minimum.  Pure NumPy; every array handed out is read-only.

The fast kernels (k_rob_frames_row4<VEC>, k_mono_rob_frame4) replace the reference's float64 position
    l = (p + f + 0.5) / 2 - 0.5                                                    (robustness.py:380-383)
by n = p + floor(f) and predicates on ff = f - floor(f).  The flow fields below are WRITTEN tile by tile from named special
values, so that each of those decisions is taken by stored pixels; census() counts them from the float64 expression alone
(never from the kernel's integers).  Census key -> branch of the kernel:

    tie up / tie down      frac(l) == 0.5 inside the image, round-half-even goes up (floor(l) odd) / down (floor(l) even):
                           rob_centre's `!a.eq || (m & 1)`, both values of it
    l == 0                 `n == 0 && !lt` at equality (accepted: ff == 0.5)
    n == 0 in / out        0 < l < 0.25 (accepted) / -0.25 <= l < 0 (rejected): the two sides of `n == 0 && !lt`
    l == len               `n == 2 len && lt` at equality (rejected: ff == 0.5)
    n == 2len in / out     len - 0.25 <= l < len (accepted) / len < l < len + 0.25 (rejected)
    low / high tap         inside, rint(l) - 1 < 0 / rint(l) + 1 > len - 1: dodgson3's clamped tap with the centre's weight
    shared / per pixel     pixels x and x + 2 (x % 4 < 2) that take rob_row4's shared-phase path (both axes inside,
                           1 <= rint(lx), rint(lx) + 2 <= len - 1) / that take the per-pixel path although inside
    shared, other way      shared-phase pixels whose partner x + 2 rounds to rint(lx) + 2, not rint(lx) + 1 (a tie with an
                           even centre); "at border": the partner's high tap is clamped there (rint(lx) + 3 > len - 1), where
                           the two tap sets no longer weigh alike
    clamped origin         pixels of 16 x 16 sub-tiles whose first pixel has rint(l) < -4 or > len + 4 on an axis, with a
                           finite |f| < 1e9 (the LDS window origin clamp of k_rob_frames_row4; the clamp moves the window
                           of sub-tiles that lie wholly outside or reach in by less than 4 guide pixels, and a tap is
                           only read for a pixel inside, 0 .. 8 rows from the origin either way: these cases run it, but
                           no result depends on it)
    !ok                    pixels of tiles with a NaN, infinite or |f| >= 1e9 flow component (RobAxis::ok false)
    outside / inside       the reference's `0 <= l < len` on both axes
"""
import collections
import functools

import numpy as np

F32, F64 = np.float32, np.float64

Geometry = collections.namedtuple("Geometry", "name mode H W ts kernel")
# the smallest frames that reach every launch form (rule of hhsr_rob_frame / hhsr_mono_rob_frame: ts % 16, W % 4)
GEOMETRIES = (
    Geometry("80x112_ts16", "bayer", 80, 112, 16, "k_rob_frames_row4"),       # 3 x 4 workgroups, the last ones ragged
    Geometry("80x114_ts32", "bayer", 80, 114, 32, "k_rob_frames_row4_dword"),
    Geometry("80x112_ts64", "bayer", 80, 112, 64, "k_rob_frames_row4"),       # 4 sub-tiles of a workgroup in one flow tile
    Geometry("80x112_ts8", "bayer", 80, 112, 8, "k_rob_frame"),
    Geometry("18x20_ts16", "bayer", 18, 20, 16, "k_rob_frames_row4"),         # guide image smaller than the 11 x 11 window
    Geometry("4x6_ts16", "bayer", 4, 6, 16, "k_rob_frames_row4_dword"),
    Geometry("grey_48x64_ts16", "grey", 48, 64, 16, "k_mono_rob_frame4"),
    Geometry("grey_48x66_ts16", "grey", 48, 66, 16, "k_mono_rob_frame"),
)
FIELDS = ("ties", "edges", "invalid")
CFA = ((1, 0), (2, 1))  # GRBG
WB = (1.8, 1.0, 1.4)
SNR = 18.0
# content seeds of the two frames with a handful of pixels, chosen so that some of them lie in the transition band of R
SEEDS = {"18x20_ts16": 1, "4x6_ts16": 20}


def kernel_of(g):
    """The kernel the library chooses for aligned planes (csrc/hhsr_robustness.hip: rob_grouped, rob_frames_launch,
    hhsr_mono_rob_frame)."""
    if g.mode == "grey":
        return "k_mono_rob_frame4" if g.W % 4 == 0 and g.ts % 4 == 0 else "k_mono_rob_frame"
    if g.ts % 16:
        return "k_rob_frame"
    return "k_rob_frames_row4" if g.W % 4 == 0 else "k_rob_frames_row4_dword"


def frozen(a):
    a.setflags(write=False)
    return a


def cdiv(a, b):
    return -(-a // b)


def grid(g):
    return cdiv(g.H, g.ts), cdiv(g.W, g.ts)


def lens(g):
    """(lh, lw) of the statistics map the positions are tested against: the guide image; the frame itself in grey mode
    (robustness.py:337-343)."""
    return (g.H // 2, g.W // 2) if g.mode == "bayer" else (g.H, g.W)


def _na(v, to):
    return np.nextafter(F32(v), F32(to))


# every combination of these over x and y is cycled over the tiles of `ties`
TIE_VALUES = frozen(np.array(
    [0.0, -0.0, 0.5, -0.5, 1.5, -1.5, 2.5, 1.0, -1.0, 2.0, 0.25, 0.75, _na(0.5, 0), _na(-0.5, 0), _na(0.5, np.inf),
     _na(-0.5, -np.inf), 1e-30, -1e-30], F32))
HALVES = frozen(np.array([1.5, -0.5, 0.5, -1.5, 2.5], F32))  # the last tile row / column of `ties` cycle through these
INVALID_VALUES = frozen(np.array([_na(1e9, 0), np.nan, np.inf, -np.inf, 1e9, -1e10], F32))


def _ties(g):
    ny, nx = grid(g)
    n = len(TIE_VALUES)
    rot = 7 * GEOMETRIES.index(g)  # the small grids start at different combinations
    flow = np.empty((ny, nx, 2), F32)
    for ty in range(ny):
        for tx in range(nx):
            t = ty * nx + tx + rot  # t -> (t % n, (t // n + 5 t) % n) walks through all n^2 pairs
            flow[ty, tx] = TIE_VALUES[t % n], TIE_VALUES[(t // n + 5 * t) % n]
    if nx > 1:  # the half-integer ties next to the right / lower border, where pixel x + 2's clamped tap matters
        flow[:, -1, 0] = HALVES[np.arange(ny) % 5]
    if ny > 1:
        flow[-1, :, 1] = HALVES[(np.arange(nx) + 1) % 5]
    return flow


def _low_recipes(N):
    """Flows of the first tile of an axis of N pixels."""
    pa = min(3, max(1, N // 4))
    eq3, eq4 = F32(0.5 - pa), F32(0.5 - (pa + 1))  # l(pa) == 0 / l(pa + 1) == 0 exactly: f = 0.5 - p
    push = [F32(-2 * k + 0.25) for k in (1, 5, 9, 40)]  # the tile's first centre is -k: k guide pixels outside
    return [eq3, push[3], eq4, push[1], _na(eq3, np.inf), push[2], _na(eq4, -np.inf), push[0], _na(eq3, -np.inf),
            _na(eq4, np.inf)]


def _high_recipes(p0, N, L):
    """Flows of the last tile of an axis (origin p0, the axis has N pixels, the map L)."""
    pa = max(p0, N - 1 - min(2, N // 4))
    pb = max(p0, min(pa + 1, N - 1))
    eqa, eqb = F32(2 * L + 0.5 - pa), F32(2 * L + 0.5 - pb)  # l(pa) == L exactly: f = 2 L + 0.5 - p
    push = [F32(2 * L + 2 * k - N - 0.25) for k in (1, 5, 9, 40)]  # the last pixel's centre is L - 1 + k
    return [eqa, push[3], eqb, push[1], _na(eqa, -np.inf), push[2], _na(eqb, np.inf), push[0], _na(eqa, np.inf),
            _na(eqb, -np.inf)]


def _edges(g):
    ny, nx = grid(g)
    lh, lw = lens(g)
    flow = np.array(_ties(g))
    for tx in range(nx):  # y flows of the first and the last tile row (a single row: the low side)
        flow[0, tx, 1] = _low_recipes(g.H)[tx % 10]
        if ny > 1:
            flow[-1, tx, 1] = _high_recipes((ny - 1) * g.ts, g.H, lh)[(tx + 2) % 10]
    for ty in range(ny):  # x flows of the first and the last tile column (a single column: the high side)
        if nx > 1:
            flow[ty, 0, 0] = _low_recipes(g.W)[(ty + 2) % 10]
        flow[ty, -1, 0] = _high_recipes((nx - 1) * g.ts, g.W, lw)[ty % 10]
    return flow


def _invalid(g):
    ny, nx = grid(g)
    flow = np.array(_ties(g))
    modes = ("x", "y", "xy")
    k = 0
    for ty in range(ny):
        for tx in range(nx):
            if (ty + tx) % 2 or k >= 24:  # checkerboard: valid tiles between them; the corner tile (0, 0) is one
                continue
            v, m = INVALID_VALUES[k % 6], modes[(k // 6) % 3]
            if "x" in m:
                flow[ty, tx, 0] = v
            if "y" in m:
                flow[ty, tx, 1] = v
            k += 1
    return flow


@functools.lru_cache(maxsize=None)
def field(g, name):
    """Flow field [ny, nx, 2] float32 of geometry g."""
    return frozen({"ties": _ties, "edges": _edges, "invalid": _invalid}[name](g))


def config(g):
    from helpers import base_config

    return base_config(ts=g.ts, snr=SNR, mode=g.mode)


def noise_curves():
    from helpers import ALPHA, BETA
    from handheld_super_resolution import synthetic as synth

    return synth.noise_curves(ALPHA, BETA)


@functools.lru_cache(maxsize=None)
def content(g):
    """(ref [H, W], comp [3, H, W]) float32: one smooth random scene (tests/helpers.smooth), shallow enough that a
    displacement by a guide pixel moves the local means by about the noise level, and per frame a smooth difference whose
    amplitude ramps over the image plus sensor-like noise: exp(-d^2 / sigma^2) takes every value between 0 and 1 at either
    value of S (asserted by tests/test_robustness_ref.py::test_transition_band).  Frame k goes with FIELDS[k]."""
    from helpers import smooth

    rng = np.random.default_rng(SEEDS.get(g.name, 1000 + GEOMETRIES.index(g)))
    H, W = g.H, g.W
    chans = 3 if g.mode == "bayer" else 1
    scene = [0.3 + 0.35 * smooth(rng, H + 8, W + 8, 7.0)[4:4 + H, 4:4 + W].astype(F64) for _ in range(chans)]
    yy, xx = np.mgrid[0:H, 0:W]
    ramp = (yy / max(H - 1, 1) + xx / max(W - 1, 1)) / 2  # 0 in the first corner, 1 in the last

    def mosaic(planes, noise):
        out = np.empty((H, W), F64)
        if chans == 1:
            out[:] = planes[0]
        else:
            for i in range(2):
                for j in range(2):
                    out[i::2, j::2] = planes[CFA[i][j]][i::2, j::2]
        out = np.clip(out + noise * rng.standard_normal((H, W)), 0.0, 1.0)
        if chans == 3:
            for i in range(2):
                for j in range(2):
                    out[i::2, j::2] *= WB[CFA[i][j]] / WB[1]
        return out.astype(F32)

    ref = mosaic(scene, 0.004)
    gain = 2.0 if grid(g) == (1, 1) else 1.0  # one tile: S = s2 = 12 everywhere, the band of R lies at larger distances
    comp = []
    for k in range(len(FIELDS)):
        amp = gain * 0.004 * 40.0 ** (ramp if k % 2 == 0 else 1 - ramp)  # 0.004 .. 0.16: from R = 1 to R = 0
        diff = [amp * (smooth(rng, H + 8, W + 8, 3.0)[4:4 + H, 4:4 + W] - 0.5) for _ in range(chans)]
        comp.append(mosaic([s + d for s, d in zip(scene, diff)], 0.004))
    return frozen(ref), frozen(np.stack(comp))


# ---- the branch census (float64 expression only) ---------------------------------------------------------------------------
CENSUS_KEYS = ("inside", "outside", "tie up", "tie down", "l == 0", "n == 0 in", "n == 0 out", "l == len", "n == 2len in",
               "n == 2len out", "low tap", "high tap", "shared", "per pixel", "shared, other way", "other way at border",
               "clamped origin", "!ok")


def positions(g, flow):
    """(ly, lx) float64 [H, W] by the reference's statement; non-finite where the flow is."""
    y = np.arange(g.H)[:, None]
    x = np.arange(g.W)[None, :]
    fl = np.asarray(flow, F32)
    fx = fl[y // g.ts, x // g.ts, 0].astype(F64)
    fy = fl[y // g.ts, x // g.ts, 1].astype(F64)
    with np.errstate(all="ignore"):
        return (y + fy + 0.5) / 2 - 0.5, (x + fx + 0.5) / 2 - 0.5


def census(g, flow):
    """{key: stored pixels} (an axis event on either axis counts the pixel once per axis)."""
    lh, lw = lens(g)
    ly, lx = positions(g, flow)
    fl = np.asarray(flow, F32)
    y = np.arange(g.H)[:, None]
    x = np.arange(g.W)[None, :]
    tile_f = fl[y // g.ts, x // g.ts].astype(F64)  # [H, W, 2]
    with np.errstate(all="ignore"):
        ok = np.isfinite(tile_f).all(-1) & (np.abs(tile_f) < 1e9).all(-1)
        iny, inx = (ly >= 0) & (ly < lh), (lx >= 0) & (lx < lw)
        inside = iny & inx
        out = dict.fromkeys(CENSUS_KEYS, 0)
        out["inside"], out["outside"] = int(inside.sum()), int((~inside).sum())
        out["!ok"] = int((~ok).sum())
        for l, L, ina in ((ly, lh, iny), (lx, lw, inx)):
            fin = np.isfinite(l)
            lf = np.where(fin, l, 0.0)
            fl_ = np.floor(lf)
            tie = fin & ina & (lf - fl_ == 0.5)
            out["tie up"] += int((tie & (fl_ % 2 == 1)).sum())
            out["tie down"] += int((tie & (fl_ % 2 == 0)).sum())
            out["l == 0"] += int((fin & (lf == 0)).sum())
            out["n == 0 in"] += int((fin & (lf > 0) & (lf < 0.25)).sum())
            out["n == 0 out"] += int((fin & (lf >= -0.25) & (lf < 0)).sum())
            out["l == len"] += int((fin & (lf == L)).sum())
            out["n == 2len in"] += int((fin & (lf >= L - 0.25) & (lf < L)).sum())
            out["n == 2len out"] += int((fin & (lf > L) & (lf < L + 0.25)).sum())
            c = np.rint(lf)
            out["low tap"] += int((inside & (c - 1 < 0)).sum())
            out["high tap"] += int((inside & (c + 1 > L - 1)).sum())
        # the shared-phase path of the 4-pixel kernels: pixel x (x % 4 < 2) decides for itself and for x + 2
        cx = np.rint(np.where(np.isfinite(lx), lx, 0.0))
        lead = (x % 4 < 2) & (x + 2 < g.W)
        sh = lead & inside & (cx >= 1) & (cx + 2 <= lw - 1)
        cx2 = np.zeros_like(cx)
        cx2[:, :-2] = cx[:, 2:]
        in2 = np.zeros_like(inside)
        in2[:, :-2] = inside[:, 2:]
        out["shared"] = 2 * int(sh.sum())
        out["per pixel"] = int((inside & ~sh & ~np.roll(sh, 2, axis=1)).sum())
        other = sh & (cx2 != cx + 1)
        out["shared, other way"] = int(other.sum())
        out["other way at border"] = int((other & in2 & (cx + 3 > lw - 1)).sum())
        # the LDS window origin of a 16 x 16 sub-tile: centre of its first pixel
        y0, x0 = (y // 16) * 16, (x // 16) * 16
        cy0 = np.rint((y0 + tile_f[..., 1] + 0.5) / 2 - 0.5)
        cx0 = np.rint((x0 + tile_f[..., 0] + 0.5) / 2 - 0.5)
        out["clamped origin"] = int((ok & ((cy0 < -4) | (cy0 > lh + 4) | (cx0 < -4) | (cx0 > lw + 4))).sum())
    return out


# ---- flow-irregularity cases S ----------------------------------------------------------------------------------------------
S_SIZES = ((1, 1), (1, 5), (5, 1), (3, 4))
S1, S2 = 2.0, 12.0
# float32 spreads (d0, d1) with fl32(fl32(d0 d0) + fl32(d1 d1)) equal to 0.25 = 0.5^2, one float32 below it, one above it
# (asserted by tests/test_robustness_ref.py; the last two are exact sums before the one rounding, so a fused multiply-add
# gives the same)
S_SPREADS = {"equal": (0.5, 0.0), "equal_34": (0.3, 0.4), "below": (0.5 - 2.0 ** -25, 2.0 ** -13), "above": (0.5, 1.5 * 2.0 ** -13)}


def _s_grid(ny, nx, spread, at, base=(0.25, -0.75)):
    """A constant field with one tile displaced by `spread`: every 3 x 3 neighbourhood that holds it has that spread."""
    f = np.empty((ny, nx, 2), F32)
    f[...] = base
    f[at] = (F32(base[0]) + F32(spread[0]), F32(base[1]) - F32(spread[1]))
    return f


@functools.lru_cache(maxsize=None)
def s_cases():
    """{name: (flow [ny, nx, 2], Mt)}"""
    rng = np.random.default_rng(5)
    cases = {}
    for ny, nx in S_SIZES:
        tag = f"{ny}x{nx}"
        at = (ny // 2, nx // 2)
        for name, sp in S_SPREADS.items():
            cases[f"{tag}_{name}"] = (_s_grid(ny, nx, sp, at, base=(0.0, 0.0)), 0.5)
        cases[f"{tag}_default"] = (rng.uniform(-0.45, 0.45, (ny, nx, 2)).astype(F32), 0.8)
        corner = _s_grid(ny, nx, (0.8, 0.0), (ny - 1, nx - 1), base=(0.0, 0.0))
        cases[f"{tag}_default_08"] = (corner, 0.8)
    for ny, nx in ((3, 4), (1, 5)):
        tag = f"{ny}x{nx}"
        f = rng.uniform(-0.2, 0.2, (ny, nx, 2)).astype(F32)
        f[ny // 2, 1] = (np.nan, 0.1)
        cases[f"{tag}_nan"] = (f, 0.8)
        f = rng.uniform(-0.2, 0.2, (ny, nx, 2)).astype(F32)
        f[ny // 2, 2] = (0.1, -np.inf)
        cases[f"{tag}_inf"] = (f, 0.8)
        f = np.full((ny, nx, 2), np.nan, F32)  # only NaN neighbours: the running extremes stay at -inf / +inf
        f[0, 0] = (0.0, 0.0)
        cases[f"{tag}_all_nan"] = (f, 0.8)
    return {k: (frozen(f), mt) for k, (f, mt) in cases.items()}


def s_statement(flow, Mt, s1=S1, s2=S2):
    """robustness.py:570-612 per tile on scalars; max / min of two float32 in a Numba CUDA kernel lower to libdevice's
    fmaxf / fminf: the operand that is a number wins over a NaN."""
    def fmax(a, b):
        return b if (a != a) else a if (b != b) else (a if a > b else b)

    def fmin(a, b):
        return b if (a != a) else a if (b != b) else (a if a < b else b)

    flow = np.asarray(flow, F32)
    ny, nx = flow.shape[:2]
    S = np.empty((ny, nx), F32)
    with np.errstate(all="ignore"):
        for ty in range(ny):
            for tx in range(nx):
                mx = [F32(-np.inf), F32(-np.inf)]
                mn = [F32(np.inf), F32(np.inf)]
                for i in (-1, 0, 1):
                    for j in (-1, 0, 1):
                        y, x = ty + i, tx + j
                        if 0 <= x < nx and 0 <= y < ny:
                            for c in range(2):
                                mx[c] = fmax(mx[c], flow[y, x, c])
                                mn[c] = fmin(mn[c], flow[y, x, c])
                d0, d1 = F32(mx[0] - mn[0]), F32(mx[1] - mn[1])
                m = F32(F32(d0 * d0) + F32(d1 * d1))
                S[ty, tx] = s1 if F64(m) > F64(Mt) * F64(Mt) else s2
    return S


# ---- noise-model cases (sigma^2 and the packed curve index) ----------------------------------------------------------------
SIGMA_SPECIALS = frozen(np.array([-0.5, -0.0, 0.0, 0.0625, 0.1875, 0.9995, 1.0, 1.0235, 7.0, np.inf, np.nan], F32))
SIGMA_SHAPE = (10, 52)  # 520 pixels: three workgroups, the last one ragged
NCURVES = (1, 1001, 1024)


@functools.lru_cache(maxsize=None)
def sigma_case(ncurve):
    """(means [3, H, W], variances [3, H, W], std_curve [ncurve], diff_curve [ncurve]): the specials in every channel, each
    at a variance below and above the curve's, random values elsewhere."""
    rng = np.random.default_rng(40 + ncurve)
    H, W = SIGMA_SHAPE
    b = np.linspace(0.0, (ncurve - 1) / 1000.0, ncurve)
    std = 0.9139 * np.sqrt(1.8e-4 * b + 3.2e-6)
    dif = 0.3761 * np.sqrt(1.8e-4 * b + 3.2e-6)
    means = rng.uniform(0.0, 1.05, (3, H, W)).astype(F32)
    n = len(SIGMA_SPECIALS)
    for c in range(3):
        flat = means[c].reshape(-1)
        for rep in range(2):  # twice: once per side of the variance comparison
            flat[40 * c + rep * n: 40 * c + (rep + 1) * n] = np.roll(SIGMA_SPECIALS, c)
    with np.errstate(all="ignore"):
        idx = sigma_index(means, ncurve)
    st2 = (std * std)[idx]
    side = (np.arange(H * W).reshape(H, W) // n) % 2 == 0
    vars_ = np.where(side[None], 0.5 * st2, 3.0 * st2 + 1e-7).astype(F32)
    return frozen(means), frozen(vars_), frozen(std), frozen(dif)


def sigma_index(means, ncurve):
    """clip(rint(1000 b), 0, ncurve - 1) in float64 (robustness.py:517), 0 where b is not finite."""
    b = np.asarray(means, F32).astype(F64)
    with np.errstate(all="ignore"):
        idx = np.where(np.isfinite(b), np.rint(1000 * b), 0)
    return np.clip(idx, 0, ncurve - 1).astype(np.int64)


# ---- local-minimum cases -----------------------------------------------------------------------------------------------------
LOCAL_MIN_SHAPES = ((1, 1), (3, 70), (17, 65), (4, 4), (33, 129))


@functools.lru_cache(maxsize=None)
def local_min_case(shape):
    """R float32 [H, W] in [0, 1]: random values in [0.3, 0.9], patches of exact 0 and exact 1, and one isolated minimum
    in each corner (four different values, so a corner read from the wrong side shows)."""
    H, W = shape
    rng = np.random.default_rng(H * 1000 + W)
    R = rng.uniform(0.3, 0.9, (H, W)).astype(F32)
    if H * W > 1:
        R[H // 2, W // 3: W // 3 + 2] = 0.0
        R[H // 3: H // 3 + 6, (2 * W) // 3: (2 * W) // 3 + 7] = 1.0
        R[0, 0], R[0, -1], R[-1, 0], R[-1, -1] = 0.125, 0.15625, 0.1875, 0.21875
    return frozen(R)


def local_min_loops(R):
    """robustness.py:670-686 as a direct 25-tap loop with clamped indices."""
    H, W = R.shape
    out = np.empty_like(R)
    for y in range(H):
        for x in range(W):
            m = np.inf
            for i in range(-2, 3):
                for j in range(-2, 3):
                    v = R[min(max(y + i, 0), H - 1), min(max(x + j, 0), W - 1)]
                    m = v if v < m else m
            out[y, x] = m
    return out


# ---- the oracle's maps of a (geometry, field), computed once and shared ---------------------------------------------------
@functools.lru_cache(maxsize=None)
def ref_maps(g):
    """(config, (std_curve, diff_curve), oracle ref means, oracle ref variances) of geometry g."""
    import oracle

    cfg = config(g)
    ref, _ = content(g)
    om, ov = oracle.init_robustness(ref, [list(r) for r in CFA], list(WB), cfg)
    return cfg, noise_curves(), frozen(om), frozen(ov)


@functools.lru_cache(maxsize=None)
def oracle_maps(g, name):
    """The oracle on frame FIELDS.index(name) of content(g) under field(g, name): dict with the frame's guide means `cm`
    [nc, lh, lw] and comp_means_up, d_sq, sigma_sq, S, R, r (oracle.compute_robustness's debug maps)."""
    import oracle

    cfg, curves, om, ov = ref_maps(g)
    comp = content(g)[1][FIELDS.index(name)]
    cfa, wb = [list(r) for r in CFA], list(WB)
    dbg = {}
    r = oracle.compute_robustness(comp, om, ov, field(g, name), cfa, wb, curves, cfg, debug=dbg)
    cm, _ = oracle.local_stats(oracle.robustness._guide(comp, cfa, wb, cfg))
    dbg.update(r=r, cm=cm)
    return {k: frozen(np.asarray(v)) for k, v in dbg.items()}
