"""Record what the library in use computes for the tile-edge cases of tests/test_frame_stats_tiles.py:

    HHSR_LIB=<library built from the parent commit> python tools/frame_stats_parent_golden.py [out.npz]

Means, variances and covariances of kernels.frame_stats(want_vars=True) on an MI355X, for the families and laws of CASES
at SHAPES, as float32 arrays under "<family>_<H>x<W>_{means,vars,cov}" (cov: the entries xx, xy, yy; the test checks that
yx holds xy's bits).  tests/golden/frame_stats_parent.npz was written by this tool with the library of the commit before
k_frame_stats went to its tile of 24 x 32 quads with the gradient-sample tile: the test asks the present kernel for the same bits.
Run once; a later change of the kernel is compared against the same file, not against a new recording."""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "handheld-multi-frame-super-resolution_amd"), os.path.join(ROOT, "tests")):
    if p not in sys.path:
        sys.path.insert(0, p)

# raw H x W: gh x gw = one quad, 1 x 35, 23 x 33, 24 x 32, 25 x 33, 25 x 65, 49 x 31 around the tile of 24 x 32 quads
SHAPES = [(2, 2), (2, 70), (46, 66), (48, 64), (50, 66), (50, 130), (98, 62)]
CASES = [("noise", "hard_threshold"), ("dynamic", "linear")]


def record():
    import torch

    import frame_stats_cases as fc
    from handheld_super_resolution import _lib, kernels

    out = {}
    for family, law in CASES:
        cfg = fc.family_config(family, law)
        for H, W in SHAPES:
            raw = torch.as_tensor(np.array(fc.image(family, H, W)), dtype=torch.float32).cuda()
            m, v, c = (t.cpu().numpy() for t in kernels.frame_stats(raw, fc.GOLDEN_CFA, fc.GOLDEN_WB, cfg, want_vars=True))
            key = fc.golden_key(family, H, W)
            out[key + "_means"], out[key + "_vars"] = m, v
            out[key + "_cov"] = np.stack([c[..., 0, 0], c[..., 0, 1], c[..., 1, 1]], -1)
    return out, _lib.LIB_PATH


if __name__ == "__main__":
    path = sys.argv[1] if len(sys.argv) > 1 else os.path.join(ROOT, "tests", "golden", "frame_stats_parent.npz")
    arrays, lib = record()
    np.savez_compressed(path, **arrays)
    print(f"{path}: {len(arrays)} arrays, {os.path.getsize(path)} bytes, computed by {lib}")
