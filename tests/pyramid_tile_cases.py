"""Shapes and images of tests/test_pyramid_tiles.py, shared with tools/pyramid_parent_golden.py (which records what the
kernel before the re-tiling computed for them).  NumPy only.

k_gauss_decimate<F> (csrc/hhsr_pyramid.hip) works on tiles of TILE[f] = (TY, TX) outputs: 16 x 120 at factor 2, 8 x 60 at
factor 4.  A source of H x W pixels gives (H - 4 f) // f x (W - 4 f) // f outputs."""
import functools

import numpy as np

TILE = {2: (16, 120), 4: (8, 60)}  # GdTile<F>::TY, TX
N_IMAGES = 3                       # images per shape: the frames of the batches are these, cyclically


def source_shape(f, h2, w2, ey=0, ex=0):
    """H x W with h2 x w2 outputs and ey, ex (< f) surplus rows and columns that no output reads."""
    assert 0 <= ey < f and 0 <= ex < f
    return f * h2 + 4 * f + ey, f * w2 + 4 * f + ex


def shapes(f):
    """name -> (H, W).  One output pixel (H = W = 4 f + 1 + (f - 1)); exactly one tile; a tile minus one / plus one in
    each direction; three tiles plus one in each direction and two tiles plus two columns (interior and clamped workgroups
    meet); widths with W % 4 of 0, 1 and 2."""
    ty, tx = TILE[f]
    out = {
        "one_pixel": source_shape(f, 1, 1),
        "one_tile": source_shape(f, ty, tx),                      # W % 4 == 0
        "minus_plus": source_shape(f, ty - 1, tx + 1, 0, f - 1),  # f = 2: 2 * 121 + 9, W % 4 == 3; f = 4: W % 4 == 3
        "plus_minus": source_shape(f, ty + 1, tx - 1, f - 1, 0),  # f = 2: 2 * 119 + 8, W % 4 == 2; f = 4: W % 4 == 0
        "three_plus": source_shape(f, 3 * ty + 1, 3 * tx + 1, 0, 0 if f == 2 else 2),  # W % 4 == 2
        "two_w1": source_shape(f, ty + 1, 2 * tx + 2, 0, 1),      # W % 4 == 1
        "two_w0": source_shape(f, ty + 1, 2 * tx + 2, 0, 0),      # W % 4 == 0: 16-byte loads on the two interior tiles
    }
    assert out["one_pixel"] == (5 * f, 5 * f)
    assert {W % 4 for _, W in out.values()} >= {0, 1, 2}
    return out


def frozen(a):
    a.setflags(write=False)
    return a


@functools.lru_cache(maxsize=None)
def image(f, name, k):
    """Image k of a shape: a permutation of H W equally spaced values in (0, 1) — no value twice in the image, so that an
    element taken from the wrong place shows."""
    H, W = shapes(f)[name]
    rng = np.random.default_rng([f, sorted(shapes(f)).index(name), k])
    return frozen(((rng.permutation(H * W) + 0.5) / (H * W)).astype(np.float32).reshape(H, W))


@functools.lru_cache(maxsize=None)
def special_image(f):
    """three_plus-shaped: -0.0 everywhere (an output there is +0.0 only through the sums' leading 0.f +), with blocks of
    denormals, of +-1e30 and of ordinary values, each larger than a footprint of taps, and single such values sprinkled in."""
    H, W = shapes(f)["three_plus"]
    rng = np.random.default_rng(100 + f)
    a = np.full((H, W), -0.0, np.float32)
    pool = np.array([1e-40, -3e-42, 1e30, -1e30, 1.0, -0.37, 2.5e-38, 0.0], np.float32)
    a[H // 3:2 * H // 3, :W // 4] = rng.choice(pool[:2], (2 * H // 3 - H // 3, W // 4))
    a[:H // 3, W // 2:] = rng.choice(pool[2:4], (H // 3, W - W // 2))
    a[2 * H // 3:, W // 3:2 * W // 3] = rng.random((H - 2 * H // 3, 2 * W // 3 - W // 3), dtype=np.float32)
    ys, xs = rng.integers(0, H, 200), rng.integers(0, W, 200)
    a[ys, xs] = rng.choice(pool, 200)
    return frozen(a)


def golden_key(f, name, k):
    return f"f{f}_{name}_{k}"
