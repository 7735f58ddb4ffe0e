"""The oracle of the post path (oracle/post.py) against plain restatements, on the CPU: the gauss frame-count denoiser
against a per-pixel loop (NaN samples stay inside their own window), and the reflect-mode Gaussian of the unsharp mask
against scipy at images smaller than the filter."""
import numpy as np
import pytest

import post_cases as pc
from oracle import post


def test_gauss_denoiser_nan_stays_in_its_own_window():
    """One NaN sample, integer accumulated robustness, sigma_max 2 at 17 x 23: the oracle equals the per-pixel loop bit for
    bit and has NaN exactly where the loop has — a tap outside a pixel's own window contributes nothing (not 0 * NaN,
    which made every pixel within the LARGEST window of the image NaN: 156 instead of 56 outputs here)."""
    H, W = 17, 23
    rng = np.random.default_rng(11)
    img = rng.random((H, W, 3)).astype(np.float32)
    img[8, 11, 1] = np.nan
    racc = pc.integer_racc(*pc.acc_reach(H, W, 2, True), seed=3)
    read = pc.acc_read(racc, H, W, 2, True)
    assert len(np.unique(read)) >= 5 and (read == 0).any() and (read >= 8).any()  # windows from 13 x 13 down to 1 x 1
    cfg = {"sigma_max": 2, "max_frame_count": 8}
    got = post.frame_count_denoising_gauss(img, racc, cfg, 2)
    want = pc.gauss_denoiser_loop(img, racc, 2, 8, 2)
    assert np.array_equal(np.isnan(got), np.isnan(want)), (int(np.isnan(got).sum()), int(np.isnan(want).sum()))
    assert 1 < np.isnan(want).sum() < 13 * 13
    assert np.array_equal(got, want, equal_nan=True), float(np.nanmax(np.abs(got - want)))


@pytest.mark.parametrize("mode", list(pc.INDEX_MODES))
def test_gauss_denoiser_loop_index_modes(mode):
    """The same equality without NaN under the three index rules, scale 1.5, a robustness map smaller than the indices
    reach (clamped) and sigma_max 4 (3 sigma = 3 exactly at r = 6)."""
    H, W = 9, 14
    img = pc.unit_image(H, W, seed=5)
    racc = pc.integer_racc(3, 4, seed=1)
    half = pc.INDEX_MODES[mode]
    got = post.frame_count_denoising_gauss(img, racc, {"sigma_max": 4, "max_frame_count": 8}, 1.5, half)
    assert np.array_equal(got, pc.gauss_denoiser_loop(img, racc, 4, 8, 1.5, half))


@pytest.mark.parametrize("sigma", [0.5, 3, 16])
@pytest.mark.parametrize("shape", [(1, 7), (2, 9), (5, 70), (7, 1), (1, 1)])
def test_reflect_gaussian_restatement_equals_scipy(shape, sigma):
    """scipy.ndimage.gaussian_filter(mode="reflect") — what the oracle's unsharp mask rests on — against the index rule
    ((i % 2n) + 2n) % 2n, mirrored above n, rows first, float32 intermediate: images smaller than the 2 / 12 / 64 taps,
    up to more than six reflection periods.  The two must be equal, bit for bit (so they are with scipy 1.15.3).  The
    float64 sums of the two sides differ by their association only (scipy adds the two samples of a symmetric tap pair
    first), so a scipy that sums otherwise could move a float32 rounding by one ulp: this test would then fail, and the
    restatement, not the bound, is what to look at."""
    from scipy.ndimage import gaussian_filter

    plane = np.ascontiguousarray(pc.unit_image(*shape, seed=7)[..., 0])
    got = pc.reflect_gaussian(plane, sigma)
    want = gaussian_filter(plane, sigma=sigma, mode="reflect")
    assert got.dtype == want.dtype == np.float32
    d = float(np.abs(got.astype(np.float64) - want).max())
    print(f"reflect restatement vs scipy {shape} sigma {sigma}: {d:.3e}")
    assert np.array_equal(got, want), d
    # and through the oracle's unsharp mask, image + (image - blurred) * amount in float32: were the blurred images to
    # differ by 2^-23, that times the amount 1.5, plus the roundings of the difference (2^-24), the product (2^-24) and
    # the sum (2^-23 below 4) should one of them fall on the other side: < 4 x 2^-23
    img = pc.unit_image(*shape, seed=7)
    mine = np.stack([img[..., c] + (img[..., c] - pc.reflect_gaussian(img[..., c], sigma)) * np.float32(1.5) for c in range(3)], -1)
    assert np.abs(post.unsharp_mask(img, sigma, 1.5).astype(np.float64) - mine).max() <= 4 * pc.ULP1


def test_reflect_index_periods():
    """The index rule itself at n = 1, 2, 5 over several periods on both sides, against an explicitly mirrored line."""
    for n in (1, 2, 5):
        line = np.arange(n)
        tiled = np.concatenate([np.concatenate([line, line[::-1]])] * 16)  # (a b c | c b a) ...: index 0 = start of a period
        i = np.arange(-8 * 2 * n, 8 * 2 * n)
        assert np.array_equal(pc.reflect_index(i, n), tiled[i + 8 * 2 * n])
