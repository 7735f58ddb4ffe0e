"""Inputs and shared reference results of the tone-mapping tests (tests/test_tonemap_ref.py, tests/test_tonemap.py)."""
import functools
import json
import os

import numpy as np

import mertens_ref as ref

F32 = np.float32
EPS32 = float(np.finfo(np.float32).eps)

# the smallest shapes that reach every border rule of the pyramids (32 x 8 tiles of the down / up kernels, 64 x 4 of the
# weight kernel): odd -> odd chains; plain; top level 1 x 1 and pyrUp from n = 1; fewer rows than taps (repeated
# reflection); L = 1; L = 0; several workgroups per axis at level 0 and no multiple of any tile
SHAPES = [(37, 53), (64, 48), (16, 16), (5, 70), (2, 9), (1, 7), (131, 259)]


def image(H, W, seed=0, lo=0.0, hi=1.0):
    """float32 [H][W][3] in [lo, hi]: blocky coloured noise with fine texture; the top-left quadrant is an exactly grey
    (r = g = b) textured region, the bottom-left quadrant a flat colour."""
    rng = np.random.default_rng(seed)
    blocks = rng.random((-(-H // 4), -(-W // 4), 3))
    img = np.repeat(np.repeat(blocks, 4, 0), 4, 1)[:H, :W] * 0.8 + 0.1
    img = np.clip(img + 0.04 * rng.standard_normal((H, W, 3)), 0, 1)
    gy, gx = H // 2, W // 2
    img[:gy, :gx] = np.clip(0.5 + 0.2 * rng.standard_normal((gy, gx, 1)), 0, 1)
    img[gy:, :gx] = (0.6, 0.3, 0.2)
    return (lo + (hi - lo) * img).astype(F32)


def regions(H, W):
    """(grey, flat) boolean masks [H][W] of `image`."""
    grey, flat = np.zeros((H, W), bool), np.zeros((H, W), bool)
    grey[:H // 2, :W // 2] = True
    flat[H // 2:, :W // 2] = True
    return grey, flat


def blend_bound(L):
    """Float32 rounding of a fused value in [0, 1]: each of the L + 1 levels adds a pyrUp sample (8 rounded operations)
    to a weighted Laplacian (n products, n - 1 sums); in the worst case the errors add: 8 (L + 1) eps."""
    return 8 * (L + 1) * EPS32


@functools.lru_cache(maxsize=None)
def case(shape, seed=0):
    """Everything the tests of one shape share, computed once: exposures of `image`, the normalised weights, the float32
    and float64 blends and their spread (max-abs difference), without and with the smoothstep curve."""
    H, W = shape
    img = image(H, W, seed)
    expo = ref.exposures(img)
    I = ref.to_float(expo)
    wn = ref.normalise(ref.weight_maps(I))
    r32, r64 = ref.blend(I, wn, F32), ref.blend(I, wn, np.float64)
    s32, s64 = ref.smoothstep(r32), ref.smoothstep(r64)
    out = dict(img=img, expo=expo, I=I, wn=wn, r32=r32, r64=r64, s32=s32, s64=s64,
               spread=float(np.abs(r32 - r64).max()), spread_smooth=float(np.abs(s32 - s64).max()))
    for v in out.values():
        if isinstance(v, np.ndarray):
            v.setflags(write=False)
    return out


def log_figure(what, value, bound, n=1, scale=1.0):
    """A measured figure next to its bound, printed and appended to the parity log (HHSR_PARITY_LOG) in the record
    format of helpers.assert_close, which tools/parity_report.py reads."""
    rec = {"test": os.environ.get("PYTEST_CURRENT_TEST", "").split(" ")[0], "what": what, "n": int(n),
           "max_abs": float(value), "p999_abs": float(value), "rtol": 0, "atol": float(bound), "outliers": 0,
           "allowed_frac": 0.0, "scale": float(scale)}
    print(f"{what}: {value:.3e} (bound {bound:.3e})")
    log = os.environ.get("HHSR_PARITY_LOG")
    if log:
        with open(log, "a") as f:
            f.write(json.dumps(rec) + "\n")
