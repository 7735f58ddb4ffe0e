"""k_frame_stats (csrc/hhsr_kernels.hip) at the edges of its tile of 24 x 32 quads (FS_TY x FS_TX; three quads per thread, the
gradient samples formed once into an LDS tile of 25 x 33): grids gh x gw of one quad, 1 x 35, 23 x 33 (a tile minus one /
plus one), 24 x 32 (exactly one tile), 25 x 33, 25 x 65 and 49 x 31 (two tiles plus one in either direction).

Every family of tests/frame_stats_cases.py, both threshold laws, the three template forms and a batch of MAX_BATCH + 1
frames, under the bounds and the bitwise checks of tests/test_frame_stats_edges.py (covariances rtol 1e-4 / atol 1e-6, means
1e-6 / 1e-7, variances 1e-5 / 1e-7 against the oracle, NaN masks equal; under the hard threshold the quads within 1e-5 of
A = 1.95 are left out).  Two checks are this file's own: the bits of the kernel before the re-tiling
(tests/golden/frame_stats_parent.npz, written by tools/frame_stats_parent_golden.py), and images whose only gradients lie in
the last sample row and column of a tile."""
import ctypes
import functools

import numpy as np
import pytest
import torch

import frame_stats_cases as fc
import oracle
from helpers import assert_close

pytestmark = pytest.mark.gpu

from handheld_super_resolution import _lib, kernels, robustness  # noqa: E402

TILE_Y, TILE_X = 24, 32  # quads: FS_TY, FS_TX
SHAPES = [(2, 2), (2, 70), (46, 66), (48, 64), (50, 66), (50, 130), (98, 62)]  # raw H x W
PARENT_CASES = [("noise", "hard_threshold"), ("dynamic", "linear")]  # tools/frame_stats_parent_golden.py: CASES
CFA, WB = fc.GOLDEN_CFA, fc.GOLDEN_WB
COV_TOL, MEAN_TOL, VAR_TOL = (1e-4, 1e-6), (1e-6, 1e-7), (1e-5, 1e-7)
ids = dict(ids=lambda s: f"{s[0]}x{s[1]}")


def T(a):
    return torch.as_tensor(np.array(a), dtype=torch.float32).cuda()  # (a copy: the shared cases are read-only)


def N(t):
    return t.cpu().numpy()


def bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def same_nan(got, want, what):
    assert np.array_equal(np.isnan(got), np.isnan(want)), \
        f"{what}: NaN masks differ ({int(np.isnan(got).sum())} vs {int(np.isnan(want).sum())})"


def same_bits(got, want, what):
    got, want = np.asarray(got), np.asarray(want)
    assert got.shape == want.shape, f"{what}: shape {got.shape} vs {want.shape}"
    same_nan(got, want, what)
    ok = np.isnan(want) | (bits(got) == bits(want))
    assert ok.all(), f"{what}: {int((~ok).sum())} of {ok.size} values differ in their bits"


@functools.lru_cache(maxsize=None)
def want_stats(raw_key, cfa, wb):
    """Oracle (means, variances) of the Bayer guide image; raw_key = (family, H, W), or ("edge", H, W) for edge_image."""
    raw = image(raw_key)
    with np.errstate(all="ignore"):
        m, v = oracle.local_stats(oracle.guide_image(raw, [list(r) for r in cfa], list(wb)))
    return fc.frozen(m), fc.frozen(v)


@functools.lru_cache(maxsize=None)
def want_cov(raw_key, cfg_key):
    return fc.frozen(oracle.estimate_kernels(image(raw_key), config(cfg_key)))


def image(raw_key):
    return edge_image(*raw_key[1:]) if raw_key[0] == "edge" else fc.image(*raw_key)


def config(cfg_key):
    family, law = cfg_key
    return fc.family_config(family, law)


def key(cfa):
    return tuple(tuple(r) for r in cfa)


def check_stats(m, v, want, what):
    wm, wv = want
    same_nan(m, wm, what + " means")
    assert_close(m, wm, *MEAN_TOL, f"frame stats tiles: means vs {what}")
    if v is not None:
        same_nan(v, wv, what + " variances")
        assert_close(v, wv, *VAR_TOL, f"frame stats tiles: variances vs {what}")


def check_cov(got, raw_key, cfg_key):
    raw, cfg = image(raw_key), config(cfg_key)
    want = want_cov(raw_key, cfg_key)
    same_nan(got, want, f"{cfg_key[1]} covariances vs oracle")
    sel = fc.compared(raw, cfg)
    if (~sel).sum() > fc.MAX_LEFT_OUT * sel.size:  # a grid too small for the 0.1 % to cover one quad: nothing is left out
        sel = np.ones_like(sel)
    assert_close(got[sel], want[sel], *COV_TOL, f"frame stats tiles: covariances vs oracle, {cfg_key[1]}")


# ------------------------------------------------------------------------------------------ every (shape, family), both laws
@pytest.mark.parametrize("family", fc.STAT_FAMILIES)
@pytest.mark.parametrize("shape", SHAPES, **ids)
def test_bayer_vs_oracle(shape, family):
    """The three template forms against the oracle and against each other: hhsr_rob_stats (<STATS>), hhsr_cov_from_raw
    (<COV>) and hhsr_frame_stats (<STATS, COV>), the latter with and without variances; both laws.  The exponent sweeps
    are compared for their statistics only."""
    raw_key = (family, *shape)
    raw = T(fc.image(*raw_key))
    m, v = robustness.compute_local_stats_from_raw(raw, CFA, WB)
    check_stats(N(m), N(v), want_stats(raw_key, key(CFA), tuple(WB)), "oracle")
    m1, none = robustness.compute_local_stats_from_raw(raw, CFA, WB, want_vars=False)
    assert none is None
    same_bits(N(m1), N(m), "statistics-only means without variances")
    for law in fc.LAWS if family in fc.COV_FAMILIES else []:
        cfg = fc.family_config(family, law)
        m2, v2, c = kernels.frame_stats(raw, CFA, WB, cfg, want_vars=True)
        same_bits(N(m2), N(m), "fused means")
        same_bits(N(v2), N(v), "fused variances")
        m3, none, c3 = kernels.frame_stats(raw, CFA, WB, cfg)
        assert none is None
        same_bits(N(m3), N(m), "fused means without variances")
        same_bits(N(c3), N(c), "fused covariances without variances")
        same_bits(N(kernels.estimate_kernels(raw, cfg)), N(c), "covariances of the two entry points")
        c = N(c)
        assert np.array_equal(bits(c[..., 0, 1]), bits(c[..., 1, 0]))
        check_cov(c, raw_key, (family, law))


@pytest.mark.parametrize("wb", [(1.0, 1.0, 1.0), (2.0, 1.0, 0.5)], ids=["unit", "pow2"])
@pytest.mark.parametrize("shape", SHAPES, **ids)
def test_means_are_the_oracles_bits(shape, wb):
    """Samples times 2^-60 .. 2^60 and the 28-binade image (every 3 x 3 sum far above 2^-100): the means are the oracle's
    bits, with the unit white balance (the float32 shortcut) and with (2, 1, 1/2) (the float64 route, exact reciprocals)."""
    for family in list(fc.SWEEPS) + ["dynamic"]:
        m, _, _ = kernels.frame_stats(T(fc.image(family, *shape)), CFA, list(wb), fc.config())
        same_bits(N(m), want_stats((family, *shape), key(CFA), wb)[0], f"means {family} wb {wb}")


BATCH_FAMILIES = ["noise", "ramp_x", "sm_iso", "step_d1", "nan_corner", "low_noise", "dynamic", "checker", "sm_y"]


@pytest.mark.parametrize("shape", SHAPES, **ids)
def test_batch_equals_single_frames(shape):
    """frame_stats_batch of HHSR_MAX_BATCH + 1 frames (a second launch of one frame), each of another family, equals the
    per-frame calls bit for bit."""
    assert len(BATCH_FAMILIES) == _lib.MAX_BATCH + 1
    cfg = fc.config("linear")
    frames = [T(fc.image(f, *shape)) for f in BATCH_FAMILIES]
    got = kernels.frame_stats_batch(frames, CFA, WB, cfg)
    assert len(got) == len(frames)
    for f, frame, (m, v, c) in zip(BATCH_FAMILIES, frames, got):
        m1, _, c1 = kernels.frame_stats(frame, CFA, WB, cfg)
        assert v is None
        same_bits(N(m), N(m1), f"batch, {f}: means")
        same_bits(N(c), N(c1), f"batch, {f}: covariances")
        check_cov(N(c), (f, *shape), (f, "linear"))


# ------------------------------------------------------------------------------------------ the kernel before the re-tiling
@pytest.mark.parametrize("case", PARENT_CASES, ids=lambda c: c[0])
@pytest.mark.parametrize("shape", SHAPES, **ids)
def test_bits_of_the_parent_kernel(golden, shape, case):
    """Means, variances and covariances are the bits the kernel with the 16 x 32 tile (every thread forming its four gradient samples
    itself) computed on an MI355X, NaNs in the same places — in all three template forms."""
    family, law = case
    g, gk = golden("frame_stats_parent"), fc.golden_key(family, *shape)
    raw, cfg = T(fc.image(family, *shape)), fc.family_config(family, law)
    m, v, c = (N(t) for t in kernels.frame_stats(raw, CFA, WB, cfg, want_vars=True))
    same_bits(m, g[gk + "_means"], "means vs parent")
    same_bits(v, g[gk + "_vars"], "variances vs parent")
    same_bits(np.stack([c[..., 0, 0], c[..., 0, 1], c[..., 1, 1]], -1), g[gk + "_cov"], "covariances vs parent")
    assert np.array_equal(bits(c[..., 0, 1]), bits(c[..., 1, 0]))
    m1, v1 = robustness.compute_local_stats_from_raw(raw, CFA, WB)
    same_bits(N(m1), g[gk + "_means"], "hhsr_rob_stats means vs parent")
    same_bits(N(v1), g[gk + "_vars"], "hhsr_rob_stats variances vs parent")
    c1 = N(kernels.estimate_kernels(raw, cfg))
    same_bits(np.stack([c1[..., 0, 0], c1[..., 0, 1], c1[..., 1, 1]], -1), g[gk + "_cov"], "hhsr_cov_from_raw vs parent")


# ------------------------------------------------------------------------------------------ the sample tile's last row and column
EDGE_SHAPES = [(48, 64), (50, 66), (52, 68), (50, 130), (98, 66), (100, 132)]  # gh - 1 = 23, 24, 25, 48, 49; gw - 1 = 31, 32, 33, 64, 65


@functools.lru_cache(maxsize=None)
def edge_image(H, W):
    """Flat but for one step of one grey level between the quad rows 24 k - 1 and 24 k and one of two levels between the
    quad columns 32 k - 1 and 32 k: the only non-zero gradient samples are the rows 24 k - 1 and the columns 32 k - 1 of the
    sample grid — the LAST row and column of a workgroup's 25 x 33 sample tile (the ones no quad of the tile is the top-left
    of), which are the first row and column of the next workgroup's.  Exact levels (fc._from_grey_levels): a y-gradient
    of 1 (D in its transition band) and an x-gradient of 2 (D on its lower clamp), the flat quads at D = 1."""
    qy, qx = np.arange(H // 2)[:, None], np.arange(W // 2)[None, :]
    return fc.frozen(fc._from_grey_levels((qy // TILE_Y) % 2 + 2 * ((qx // TILE_X) % 2), H, W))


@pytest.mark.parametrize("law", fc.LAWS)
@pytest.mark.parametrize("shape", EDGE_SHAPES, **ids)
def test_sample_tile_edges(shape, law):
    """A sample of the tile's last row or column that is missing, stale or taken from the wrong place changes the quads on
    both sides of the tile boundary: they are compared with the oracle, and they must differ from the flat quads' value.
    gh - 1 or gw - 1 on the boundary (50 x 66: the grid's last sample row and column ARE the tile's extra ones), one short
    of it (48 x 64: the extra ones lie outside the grid and count as nothing) and one past it (52 x 68)."""
    raw_key, cfg_key = ("edge", *shape), ("noise", law)
    raw = image(raw_key)
    c = N(kernels.estimate_kernels(T(raw), config(cfg_key)))
    check_cov(c, raw_key, cfg_key)
    gh, gw = shape[0] // 2, shape[1] // 2
    flat = c[min(8, gh - 1), min(8, gw - 1)]
    for k in range(TILE_Y, gh, TILE_Y):  # quads on either side of a horizontal boundary, away from the vertical ones
        for row in (k - 1, k):
            assert not np.array_equal(bits(c[row, 8]), bits(flat)), f"quad row {row} does not see the step at {k}"
    for k in range(TILE_X, gw, TILE_X):
        for col in (k - 1, k):
            assert not np.array_equal(bits(c[8, col]), bits(flat)), f"quad column {col} does not see the step at {k}"
    m, v, c2 = kernels.frame_stats(T(raw), CFA, WB, config(cfg_key), want_vars=True)
    same_bits(N(c2), c, "fused covariances")
    check_stats(N(m), N(v), want_stats(raw_key, key(CFA), tuple(WB)), "oracle, edge image")


# ------------------------------------------------------------------------------------------ guard bands, unwritten outputs
FILL = 0x7FC5A5A5  # a NaN no arithmetic produces: an element that still holds it was not written
GUARD = 64         # floats (256 bytes) on either side of every output


class Guarded:
    """n floats of device memory between two guard bands, everything pre-filled with FILL."""

    def __init__(self, n):
        self.n = int(n)
        self.buf = torch.full((2 * GUARD + self.n,), FILL, dtype=torch.int32, device="cuda")
        self.ptr = ctypes.c_void_p(self.buf.data_ptr() + 4 * GUARD)

    def read(self, shape):
        got = self.buf.cpu().numpy()
        assert (got[:GUARD] == FILL).all() and (got[GUARD + self.n:] == FILL).all(), "a guard band was written"
        got = got[GUARD:GUARD + self.n]
        assert (got != FILL).all(), f"{int((got == FILL).sum())} of {self.n} outputs were not written"
        return got.view(np.float32).reshape(shape).copy()


@pytest.mark.parametrize("shape", SHAPES, **ids)
def test_outputs_written_once_and_only_inside(shape):
    """The three entry points with their outputs between guard bands, pre-filled with a NaN pattern: every element comes
    back written, the bands untouched (at 2 x 2 and 2 x 70 most of the workgroup's four quads per thread lie outside)."""
    H, W = shape
    gh, gw = H // 2, W // 2
    cfa, wb, st = _lib.cfa_bytes(CFA), _lib.doubles(WB), _lib.stream()
    cfg = fc.family_config("noise", "hard_threshold")
    params = kernels._kernel_params(cfg)
    raw = T(fc.image("noise", H, W))
    m0, v0, c0 = (N(t) for t in kernels.frame_stats(raw, CFA, WB, cfg, want_vars=True))
    m, v, c = Guarded(3 * gh * gw), Guarded(3 * gh * gw), Guarded(4 * gh * gw)
    _lib.call("hhsr_frame_stats", _lib.ptr(raw), H, W, W, cfa, wb, m.ptr, v.ptr, c.ptr, *params, st)
    same_bits(m.read(m0.shape), m0, "hhsr_frame_stats means")
    same_bits(v.read(v0.shape), v0, "hhsr_frame_stats variances")
    same_bits(c.read(c0.shape), c0, "hhsr_frame_stats covariances")
    m, v, c = Guarded(3 * gh * gw), Guarded(3 * gh * gw), Guarded(4 * gh * gw)
    _lib.call("hhsr_rob_stats", _lib.ptr(raw), H, W, W, cfa, wb, m.ptr, v.ptr, st)
    _lib.call("hhsr_cov_from_raw", _lib.ptr(raw), H, W, W, c.ptr, *params, st)
    same_bits(m.read(m0.shape), m0, "hhsr_rob_stats means")
    same_bits(v.read(v0.shape), v0, "hhsr_rob_stats variances")
    same_bits(c.read(c0.shape), c0, "hhsr_cov_from_raw")
