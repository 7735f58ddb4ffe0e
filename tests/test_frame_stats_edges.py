"""k_frame_stats / k_mono_stats (csrc/hhsr_kernels.hip) through all their entry points at the cases of
tests/frame_stats_cases.py: gradient grids of 0 or 1 samples, one tile, one quad past the tile, 9 and 16 workgroups, and images
that reach every exact-comparison branch of quad_cov (census: tests/test_frame_stats_ref.py).  Expected values: the oracle
(held on the CPU by test_frame_stats_ref.py), the reference's own outputs where it can be stepped (golden
"frame_stats_edges") and, on the well-conditioned quads, Alg. 5 in float64 under the bound derived on the CPU.

Bounds (the project's for these quantities): covariances rtol 1e-4 / atol 1e-6, means 1e-6 / 1e-7, variances 1e-5 / 1e-7;
NaN masks equal.  Under the hard threshold the quads whose oracle anisotropy lies within 1e-5 of the discontinuity
A = 1.95 are left out of the covariance comparison (at most 0.1 % of a case: asserted on the CPU)."""
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

CFA, WB = fc.GOLDEN_CFA, fc.GOLDEN_WB
PATTERNS = {"rggb": [[0, 1], [1, 2]], "bggr": [[2, 1], [1, 0]], "grbg": [[1, 0], [2, 1]], "gbrg": [[1, 2], [0, 1]]}
NON_BAYER = [[0, 1], [2, 1]]  # the run-time colour loop of k_frame_stats
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
    same_nan(got, want, what)
    ok = np.isnan(want) | (bits(got) == bits(want))
    assert ok.all(), f"{what}: {int((~ok).sum())} of {ok.size} values differ in their bits"


@functools.lru_cache(maxsize=None)
def want_cov(family, shape, law, mode="bayer"):
    return fc.frozen(oracle.estimate_kernels(fc.image(family, *shape), fc.family_config(family, law, mode)))


@functools.lru_cache(maxsize=None)
def want_stats(family, shape, cfa=None, wb=None):
    """Oracle (means, variances): Bayer guide image with `cfa` / `wb`, or (cfa None) the frame as its own guide."""
    raw = fc.image(family, *shape)
    guide = np.asarray(raw)[None] if cfa is None else oracle.guide_image(raw, [list(r) for r in cfa], list(wb))
    with np.errstate(all="ignore"):
        m, v = oracle.local_stats(guide)
    return fc.frozen(m), fc.frozen(v)


def key(cfa):
    return tuple(tuple(r) for r in cfa)


def check_stats(m, v, want, what):
    wm, wv = want
    same_nan(m, wm, what + " means")
    assert_close(m, wm, *MEAN_TOL, f"frame stats edges: means vs {what}")
    if v is not None:
        same_nan(v, wv, what + " variances")
        assert_close(v, wv, *VAR_TOL, f"frame stats edges: variances vs {what}")


def check_cov(got, family, shape, law, mode="bayer", want=None, what="oracle"):
    raw, cfg = fc.image(family, *shape), fc.family_config(family, law, mode)
    want = want_cov(family, shape, law, mode) if want is None else want
    same_nan(got, want, f"{mode} {law} covariances vs {what}")
    sel = fc.compared(raw, cfg)
    assert (~sel).sum() <= fc.MAX_LEFT_OUT * sel.size
    assert_close(got[sel], want[sel], *COV_TOL, f"frame stats edges: {mode} covariances vs {what}, {law}")


def check_cov_f64(got, family, shape, law):
    """The kernel against Alg. 5 in float64 on the well-conditioned quads: within 4 x the oracle's own distance."""
    raw, cfg = fc.image(family, *shape), fc.family_config(family, law)
    sel = fc.well_conditioned(raw, cfg)
    if not sel.any():
        return
    want = fc.cov_float64(raw, cfg)[sel]
    scale = np.abs(want).max((-1, -2), keepdims=True)
    assert_close(got[sel] / scale, want / scale, 0, fc.F64_BOUND, f"frame stats edges: covariances vs float64 Alg. 5, {law}")


# ------------------------------------------------------------------------------------------ every (shape, family), both laws
@pytest.mark.parametrize("family", fc.STAT_FAMILIES)
@pytest.mark.parametrize("shape", fc.SHAPES, **ids)
def test_bayer_vs_oracle(golden, shape, family):
    """kernels.frame_stats(want_vars=True), kernels.estimate_kernels and robustness.compute_local_stats_from_raw against the
    oracle, the golden (where the reference ran) and float64; the NaN frames are two of the families: no NaN outside the
    oracle's mask, none missing.  The exponent sweeps are compared for their statistics only."""
    raw = T(fc.image(family, *shape))
    want = want_stats(family, shape, key(CFA), tuple(WB))
    m, v = robustness.compute_local_stats_from_raw(raw, CFA, WB)
    check_stats(N(m), N(v), want, "oracle")
    g = golden("frame_stats_edges") if shape in fc.REF_SHAPES else None
    if g is not None:
        gk = fc.golden_key(family, *shape)
        check_stats(N(m), N(v), (g[gk + "_means"], g[gk + "_vars"]), "the reference's kernels")
    for law in fc.LAWS if family in fc.COV_FAMILIES else []:
        cfg = fc.family_config(family, law)
        m2, v2, c = kernels.frame_stats(raw, CFA, WB, cfg, want_vars=True)
        same_bits(N(m2), N(m), "fused means")
        same_bits(N(v2), N(v), "fused variances")
        c1 = kernels.estimate_kernels(raw, cfg)
        same_bits(N(c1), N(c), "covariances of the two entry points")
        c = N(c)
        assert np.array_equal(bits(c[..., 0, 1]), bits(c[..., 1, 0]))
        check_cov(c, family, shape, law)
        check_cov_f64(c, family, shape, law)
        if g is not None and f"{shape[0]}x{shape[1]}_bayer" in g["cov_ran"]:
            w = g[f"{gk}_bayer_{law}"]
            check_cov(c, family, shape, law, want=np.stack([w[..., 0], w[..., 1], w[..., 1], w[..., 2]], -1).reshape(c.shape),
                      what="the reference's kernel")


def test_odd_size_is_refused():
    """An odd raw size has no quad grid: every wrapper refuses it (the oracle would drop the last row and column)."""
    raw = T(fc.image("noise", *fc.ODD_SHAPE))
    cfg = fc.config()
    for call in (lambda: kernels.estimate_kernels(raw, cfg), lambda: kernels.frame_stats(raw, CFA, WB, cfg),
                 lambda: kernels.frame_stats_batch([raw], CFA, WB, cfg),
                 lambda: robustness.compute_local_stats_from_raw(raw, CFA, WB)):
        with pytest.raises(ValueError, match="even dimensions"):
            call()


# ------------------------------------------------------------------------------------------ the means' quotient, unit white balance
@pytest.mark.parametrize("wb", [(1.0, 1.0, 1.0), (2.0, 1.0, 0.5)], ids=["unit", "pow2"])
@pytest.mark.parametrize("family", list(fc.SWEEPS) + ["dynamic"])
@pytest.mark.parametrize("shape", [(2, 2), (2, 70), (34, 66), (66, 130)], **ids)
def test_in_contract_means_bit_for_bit(shape, family, wb):
    """Samples times 2^-60 .. 2^60 and the 28-binade image: every 3 x 3 sum is far above 2^-100, where the comment at the
    float32 `/9` quotient claims the correctly rounded float32 of the float64 quotient — the oracle's bits.  With the unit
    white balance the guide takes the float32 shortcut, with (2, 1, 1/2) the float64 route (exact reciprocals)."""
    m, _, _ = kernels.frame_stats(T(fc.image(family, *shape)), CFA, list(wb), fc.config())
    same_bits(N(m), want_stats(family, shape, key(CFA), wb)[0], f"means {family} wb {wb}")
    if wb[0] == 1.0:
        mm = kernels.mono_frame_stats(T(fc.image(family, *shape)), fc.config(mode="grey"), covs=False)[0]
        same_bits(N(mm), want_stats(family, shape)[0], f"monochrome means {family}")


@pytest.mark.parametrize("pattern", list(PATTERNS))
@pytest.mark.parametrize("shape", [(2, 70), (34, 66), (66, 130)], **ids)
def test_unit_white_balance_shortcut(shape, pattern):
    """White balance (1, 1, 1) takes the float32 shortcut for the guide image, (1, 1, 1 + 2^-52) the float64 route (its
    reciprocal is 1 - 2^-52, and a float32 times it rounds back to itself): the same bits on the 28-binade image, for the
    means and the variances, and the oracle's bits for the means."""
    cfa = PATTERNS[pattern]
    raw = T(fc.image("dynamic", *shape))
    m1, v1 = robustness.compute_local_stats_from_raw(raw, cfa, [1.0, 1.0, 1.0])
    m2, v2 = robustness.compute_local_stats_from_raw(raw, cfa, [1.0, 1.0, 1.0 + 2.0 ** -52])
    same_bits(N(m1), N(m2), "means, shortcut vs float64 route")
    same_bits(N(v1), N(v2), "variances, shortcut vs float64 route")
    want = want_stats("dynamic", shape, key(cfa), (1.0, 1.0, 1.0))
    same_bits(N(m1), want[0], "means vs oracle")
    check_stats(N(m1), N(v1), want, "oracle, unit white balance")


def test_unit_white_balance_exact_at_the_smallest_values():
    """A flat frame of 3 x 2^-149: the green mean (3 + 3) / 2, the sum of nine and the quotient 27 / 9 are all exact, in
    float32 as in float64, so no rounding rule is involved and the means are the oracle's bits although the values lie far
    below the range in which an inexact quotient is guaranteed (halving each green before the sum would round 1.5 to 2)."""
    u = np.float32(2.0 ** -149)
    for shape in [(2, 2), (34, 66)]:
        raw = np.full(shape, 3 * u, np.float32)
        m, _ = robustness.compute_local_stats_from_raw(T(raw), CFA, [1.0, 1.0, 1.0], want_vars=False)
        with np.errstate(all="ignore"):
            want, _ = oracle.local_stats(oracle.guide_image(raw, CFA, [1.0, 1.0, 1.0]))
        assert (want == 3 * u).all()
        same_bits(N(m), want, "means of a flat sub-normal frame")


# ------------------------------------------------------------------------------------------ CFA patterns, white balance
@pytest.mark.parametrize("pattern", list(PATTERNS) + ["rgbg"])
@pytest.mark.parametrize("shape", [(2, 2), (2, 70), (34, 66)], **ids)
def test_cfa_patterns_and_white_balance(shape, pattern):
    """The four Bayer patterns (compile-time channel routing) and [[0, 1], [2, 1]] (the run-time loop: one green per quad,
    halved) with a non-unit white balance and with the unit one, on noise and on the 28-binade image."""
    cfa = PATTERNS.get(pattern, NON_BAYER)
    for family in ("noise", "dynamic", "nan_corner"):
        raw = T(fc.image(family, *shape))
        for wb in (tuple(WB), (1.0, 1.0, 1.0)):
            m, v, c = kernels.frame_stats(raw, cfa, list(wb), fc.config(), want_vars=True)
            check_stats(N(m), N(v), want_stats(family, shape, key(cfa), wb), "oracle, CFA patterns")
            check_cov(N(c), family, shape, "hard_threshold")  # (the covariances do not depend on the pattern)


# ------------------------------------------------------------------------------------------ template forms
@pytest.mark.parametrize("shape", fc.SHAPES, **ids)
def test_template_forms_agree(shape):
    """hhsr_frame_stats (<STATS, COV>) == hhsr_rob_stats (<STATS>) + hhsr_cov_from_raw (<COV>), bit for bit, with and
    without variances."""
    for family, law in (("noise", "linear"), ("sm_diag", "hard_threshold"), ("nan_inner", "linear"), ("dynamic", "linear")):
        raw, cfg = T(fc.image(family, *shape)), fc.family_config(family, law)
        m, v, c = kernels.frame_stats(raw, CFA, WB, cfg, want_vars=True)
        m0, v0, c0 = kernels.frame_stats(raw, CFA, WB, cfg)
        m1, v1 = robustness.compute_local_stats_from_raw(raw, CFA, WB)
        m2, v2 = robustness.compute_local_stats_from_raw(raw, CFA, WB, want_vars=False)
        c1 = kernels.estimate_kernels(raw, cfg)
        assert v0 is None and v2 is None
        for a, b, what in ((m, m1, "means"), (v, v1, "variances"), (c, c1, "covariances"), (m0, m1, "means without variances"),
                           (m2, m1, "statistics-only means without variances"), (c0, c1, "covariances without variances")):
            same_bits(N(a), N(b), f"{family} {what}")


BATCH_FAMILIES = ["noise", "ramp_x", "sm_iso", "step_d1", "nan_corner", "low_noise", "dynamic", "checker", "sm_y"]


@pytest.mark.parametrize("n", [1, _lib.MAX_BATCH, _lib.MAX_BATCH + 1])
@pytest.mark.parametrize("shape", [(2, 70), (34, 66)], **ids)
def test_batch_equals_single_frames(shape, n):
    """frame_stats_batch == per-frame calls for 1, HHSR_MAX_BATCH and HHSR_MAX_BATCH + 1 (a second launch of one frame)
    frames, each of another family."""
    assert len(BATCH_FAMILIES) == _lib.MAX_BATCH + 1
    cfg = fc.config("linear")
    frames = [T(fc.image(f, *shape)) for f in BATCH_FAMILIES[:n]]
    got = kernels.frame_stats_batch(frames, CFA, WB, cfg)
    assert len(got) == n
    for f, frame, (m, v, c) in zip(BATCH_FAMILIES, frames, got):
        m1, _, c1 = kernels.frame_stats(frame, CFA, WB, cfg)
        assert v is None
        same_bits(N(m), N(m1), f"batch of {n}, {f}: means")
        same_bits(N(c), N(c1), f"batch of {n}, {f}: covariances")
        check_cov(N(c), f, shape, "linear")


# ------------------------------------------------------------------------------------------ guard bands, unwritten outputs
FILL = 0x7FC5A5A5  # a NaN no arithmetic produces: an element that still holds it was not written
GUARD = 64         # floats (256 bytes) on either side of every output


class Guarded:
    """n floats of device memory between two guard bands, everything pre-filled with FILL."""

    def __init__(self, n):
        self.n = int(n)
        self.buf = torch.full((2 * GUARD + self.n,), FILL, dtype=torch.int32, device="cuda")
        assert self.buf.data_ptr() % 256 == 0
        self.ptr = ctypes.c_void_p(self.buf.data_ptr() + 4 * GUARD)

    def raw(self):
        got = self.buf.cpu().numpy()
        assert (got[:GUARD] == FILL).all() and (got[GUARD + self.n:] == FILL).all(), "a guard band was written"
        return got[GUARD:GUARD + self.n]

    def read(self, shape):
        """The n floats, after checking that the bands still hold FILL and that no element does."""
        got = self.raw()
        assert (got != FILL).all(), f"{int((got == FILL).sum())} of {self.n} outputs were not written"
        return got.view(np.float32).reshape(shape).copy()


@pytest.mark.parametrize("shape", fc.SHAPES, **ids)
def test_outputs_written_once_and_only_inside(shape):
    """Every entry point with its outputs between guard bands and pre-filled with a NaN pattern: all elements come back
    written, the bands untouched (at 2 x 2 and 2 x 70 most of a workgroup lies outside the image), and the values are the
    wrappers' bits.  `negative` makes NaN-free zero tensors, `noise` generic values."""
    H, W = shape
    gh, gw = H // 2, W // 2
    cfa, wb, st = _lib.cfa_bytes(CFA), _lib.doubles(WB), _lib.stream()
    for family, law in (("noise", "hard_threshold"), ("negative", "linear")):
        cfg = fc.family_config(family, law)
        params = kernels._kernel_params(cfg)
        raw = T(fc.image(family, H, W))
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
        m, v = Guarded(3 * gh * gw), Guarded(3 * gh * gw)
        _lib.call("hhsr_rob_stats", _lib.ptr(raw), H, W, W, cfa, wb, m.ptr, None, st)
        same_bits(m.read(m0.shape), m0, "hhsr_rob_stats means alone")
        ms = [Guarded(3 * gh * gw) for _ in range(2)]
        cs = [Guarded(4 * gh * gw) for _ in range(2)]
        arr = lambda gs: (ctypes.c_void_p * len(gs))(*[g.ptr.value for g in gs])  # noqa: E731
        _lib.call("hhsr_frame_stats_batch", _lib.ptr_array([raw, raw]), 2, H, W, W, cfa, wb, arr(ms), arr(cs), *params, st)
        for mg, cg in zip(ms, cs):
            same_bits(mg.read(m0.shape), m0, "hhsr_frame_stats_batch means")
            same_bits(cg.read(c0.shape), c0, "hhsr_frame_stats_batch covariances")
        # no frames: returns without a launch, nothing is written
        m, c = Guarded(3 * gh * gw), Guarded(4 * gh * gw)
        _lib.call("hhsr_frame_stats_batch", _lib.ptr_array([raw]), 0, H, W, W, cfa, wb, arr([m]), arr([c]), *params, st)
        torch.cuda.synchronize()
        assert (m.raw() == FILL).all() and (c.raw() == FILL).all(), "a batch of no frames wrote"
        # monochrome: H x W pixels
        gcfg = fc.family_config(family, law, "grey")
        gparams = kernels._kernel_params(gcfg)
        mm0, mv0, mc0 = (N(t) for t in kernels.mono_frame_stats(raw, gcfg, want_vars=True))
        m, v, c = Guarded(H * W), Guarded(H * W), Guarded(4 * H * W)
        _lib.call("hhsr_mono_frame_stats", _lib.ptr(raw), H, W, W, m.ptr, v.ptr, c.ptr, *gparams, st)
        same_bits(m.read(mm0.shape), mm0, "hhsr_mono_frame_stats means")
        same_bits(v.read(mv0.shape), mv0, "hhsr_mono_frame_stats variances")
        same_bits(c.read(mc0.shape), mc0, "hhsr_mono_frame_stats covariances")
        m, c = Guarded(H * W), Guarded(4 * H * W)
        _lib.call("hhsr_mono_frame_stats", _lib.ptr(raw), H, W, W, m.ptr, None, None, *gparams, st)
        _lib.call("hhsr_mono_frame_stats", _lib.ptr(raw), H, W, W, None, None, c.ptr, *gparams, st)
        same_bits(m.read(mm0.shape), mm0, "hhsr_mono_frame_stats, statistics only")
        same_bits(c.read(mc0.shape), mc0, "hhsr_mono_frame_stats, covariances only")


# ------------------------------------------------------------------------------------------ monochrome twin
@pytest.mark.parametrize("family", fc.STAT_FAMILIES)
@pytest.mark.parametrize("shape", fc.SHAPES, **ids)
def test_mono_vs_oracle(golden, shape, family):
    """kernels.mono_frame_stats in its three forms (statistics, covariances, both) on the same shapes read as pixels:
    against oracle.local_stats(raw[None]) and oracle.estimate_kernels in grey mode (and the golden where the reference
    ran); the forms agree bit for bit.  (No float64 comparison here: per pixel the stabilised noise images have gradients
    along the anti-diagonal often enough that the reference's own eigenvector formula is off by more than the values.)"""
    raw = T(fc.image(family, *shape))
    cfg0 = fc.config(mode="grey")
    m, v, none = kernels.mono_frame_stats(raw, cfg0, covs=False, want_vars=True)
    assert none is None
    check_stats(N(m), N(v), want_stats(family, shape), "oracle, monochrome")
    m1 = kernels.mono_frame_stats(raw, cfg0, covs=False)[0]
    same_bits(N(m1), N(m), "monochrome means without variances")
    g = golden("frame_stats_edges")
    for law in fc.LAWS if family in fc.COV_FAMILIES else []:
        cfg = fc.family_config(family, law, "grey")
        m2, v2, c = kernels.mono_frame_stats(raw, cfg, want_vars=True)
        c1 = kernels.mono_frame_stats(raw, cfg, stats=False)[2]
        c2 = kernels.estimate_kernels(raw, cfg)
        same_bits(N(m2), N(m), "monochrome means, both")
        same_bits(N(v2), N(v), "monochrome variances, both")
        same_bits(N(c1), N(c), "monochrome covariances, covariances only")
        same_bits(N(c2), N(c), "monochrome covariances, estimate_kernels")
        c = N(c)
        check_cov(c, family, shape, law, "grey")
        if f"{shape[0]}x{shape[1]}_grey" in g["cov_ran"]:
            w = g[f"{fc.golden_key(family, *shape)}_grey_{law}"]
            check_cov(c, family, shape, law, "grey", what="the reference's kernel",
                      want=np.stack([w[..., 0], w[..., 1], w[..., 1], w[..., 2]], -1).reshape(c.shape))
