"""Inputs and plain restatements shared by the post-path border tests (tests/test_post_ref.py on the CPU,
tests/test_post_edges.py on the GPU): the kernels of csrc/hhsr_post.hip at one row, one column, one pixel, fewer rows than
taps, windows wider than the image, tied and NaN samples, integer accumulated robustness."""
import functools
import math
import os

import numpy as np

from oracle import post

F32 = np.float32
ULP1 = 2.0 ** -23  # one float32 ulp just below 1

# 64 x 4 pixels per workgroup: one pixel, one row, one column, two rows, fewer rows than a 12-tap blur, a generic odd
# shape (several workgroups), three workgroups across with remainders on both axes
SHAPES = [(1, 1), (1, 7), (7, 1), (2, 9), (5, 70), (37, 53), (9, 131)]
with np.load(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "post.npz")) as _g:
    XYZ2CAM = _g["pp_xyz2cam"]  # the colour matrix of the golden "post"
INDEX_MODES = {"half": True, "nearest": False, "grey": 2}  # name -> half_index of oracle.post


# the runs of the golden "post_edges" (tools/refsim/make_goldens.py, stage post_edges: the reference's own functions)
GOLDEN_MEDIANS = ["med_r7_bayer", "med_r7_grey", "med_s15", "med_tie", "med_row", "med_col"]
GOLDEN_POST_SHAPES = [(1, 7), (7, 1), (1, 1), (2, 9), (5, 70)]


def golden_median_case(g, tag):
    """(image, accumulated robustness, config, scale, half_index, expected) of one median run of the golden "post_edges"."""
    radius_max, mfc, scale, grey = g[f"{tag}_par"]
    img = g["med_row_in"] if tag == "med_row" else g["med_col_in"] if tag == "med_col" else g["med_in"]
    scale = int(scale) if scale == int(scale) else float(scale)
    return (img, g[f"{tag}_racc"], {"radius_max": int(radius_max), "max_frame_count": int(mfc)}, scale,
            2 if grey else True, g[f"{tag}_out"])


def frozen(a):
    a.setflags(write=False)
    return a


def acc_reach(H, W, scale, half_index):
    """(rows, columns) of the accumulated-robustness map that an H x W image reaches: 1 + the largest unclamped index."""
    return int(post._acc_index(H, scale, half_index).max()) + 1, int(post._acc_index(W, scale, half_index).max()) + 1


def acc_read(racc, H, W, scale, half_index):
    """[H, W]: the accumulated robustness each pixel reads (index clamped to the map, as the kernels do)."""
    yi = np.minimum(post._acc_index(H, scale, half_index), racc.shape[0] - 1)
    xi = np.minimum(post._acc_index(W, scale, half_index), racc.shape[1] - 1)
    return np.asarray(racc, np.float64)[np.ix_(yi, xi)]


@functools.lru_cache(maxsize=None)
def quantised_image(H, W, seed=0):
    """float32 [H, W, 3] on 6 levels of 1/8 (ties in every window) with a NaN sample at a corner and, where the image has
    an interior, one there (another channel)."""
    rng = np.random.default_rng(1000 + seed)
    img = (rng.integers(0, 6, (H, W, 3)) / 8.0).astype(F32)
    img[0, 0, 0] = np.nan
    if H > 2 and W > 2:
        img[H // 2, W // 2, 1] = np.nan
    return frozen(img)


@functools.lru_cache(maxsize=None)
def integer_racc(ah, aw, seed=0):
    """float64 [ah, aw] accumulated robustness of a burst whose frames are all fully robust: integers 0 .. 9.  The first
    cells are 6, 9, 0, 4, 8, so that the smallest images already read 6 (a quarter of the strength at max_frame_count 8)
    and a value >= max_frame_count (no denoising); the rest is random."""
    rng = np.random.default_rng(2000 + seed)
    r = rng.integers(0, 10, ah * aw).astype(np.float64)
    head = np.array([6, 9, 0, 4, 8], np.float64)[:ah * aw]
    r[:len(head)] = head
    return frozen(r.reshape(ah, aw))


@functools.lru_cache(maxsize=None)
def unit_image(H, W, seed=0, nans=0):
    """float32 [H, W, 3] in [0, 1]; `nans` NaN pixels (all channels): the first at a corner, the second inside."""
    rng = np.random.default_rng(3000 + seed)
    img = rng.random((H, W, 3)).astype(F32)
    if nans >= 1:
        img[0, W - 1] = np.nan
    if nans >= 2:
        img[H // 2, W // 3] = np.nan
    return frozen(img)


@functools.lru_cache(maxsize=None)
def post_image(H, W, seed=0, nan=True):
    """float32 [H, W, 3] in [-0.05, 1.05] with a block of exact 0.0 (top left), a block of exact 1.0 (bottom right) and,
    with `nan` and more than one pixel, one NaN pixel (channel 1) between them."""
    rng = np.random.default_rng(4000 + seed)
    img = (rng.random((H, W, 3)) * 1.1 - 0.05).astype(F32)
    bh, bw = max(1, H // 3), max(1, W // 4)
    img[:bh, :bw] = 0.0
    img[H - bh:, W - bw:] = 1.0
    if nan and H * W > 1:
        img[H // 2, W // 2, 1] = np.nan
    return frozen(img)


# ---- plain restatements ---------------------------------------------------------------------------------------------------
def gauss_denoiser_loop(image, r_acc, sigma_max, mfc, scale, half_index=True):
    """The gauss frame-count denoiser pixel by pixel, as oracle.post.frame_count_denoising_gauss states it:
    t = ceil(3 sigma), w = exp(-(i^2 + j^2) / (2 sigma^2)) (w = [i == j == 0] at sigma = 0), float64 sums, float32 result.
    A pixel sees the samples of its own window and nothing else."""
    image = np.asarray(image, F32)
    H, W, C = image.shape
    r = acc_read(r_acc, H, W, scale, half_index)
    out = np.empty_like(image)
    for y in range(H):
        for x in range(W):
            sigma = sigma_max * (mfc - min(r[y, x], mfc)) / mfc
            t = int(math.ceil(3 * sigma))
            num, den = np.zeros(C, np.float64), 0.0
            for i in range(-t, t + 1):
                for j in range(-t, t + 1):
                    if not (0 <= y + i < H and 0 <= x + j < W):
                        continue
                    w = float(i == 0 and j == 0) if sigma == 0 else float(np.exp(-(j * j + i * i) / (2 * sigma * sigma)))
                    num += w * image[y + i, x + j].astype(np.float64)
                    den += w
            with np.errstate(all="ignore"):
                out[y, x] = (num / den).astype(F32)
    return out


def gaussian_taps(sigma, truncate=4.0):
    """scipy.ndimage's normalised 1-D Gaussian: radius int(truncate sigma + 0.5), float64."""
    radius = int(truncate * float(sigma) + 0.5)
    x = np.arange(-radius, radius + 1, dtype=np.float64)
    phi = np.exp(-0.5 / (float(sigma) * float(sigma)) * x ** 2)
    return phi / phi.sum(), radius


def reflect_index(i, n):
    """scipy.ndimage mode "reflect" (d c b a | a b c d | d c b a) for any i: period 2 n, mirrored above n."""
    p = 2 * n
    i = ((i % p) + p) % p
    return np.where(i < n, i, p - 1 - i)


def reflect_gaussian(plane, sigma):
    """scipy.ndimage.gaussian_filter(float32 [H, W], sigma, mode="reflect") restated: rows (axis 0) first, float64 sums,
    float32 intermediate and result."""
    plane = np.asarray(plane, F32)
    taps, radius = gaussian_taps(sigma)
    for axis in (0, 1):
        n = plane.shape[axis]
        acc = np.zeros(plane.shape, np.float64)
        for k in range(-radius, radius + 1):
            acc += taps[k + radius] * np.take(plane, reflect_index(np.arange(n) + k, n), axis=axis).astype(np.float64)
        plane = acc.astype(F32)
    return plane
