"""Record what the library in use computes for the cases of tests/test_pyramid_tiles.py:

    HHSR_LIB=<library built from the parent commit> python tools/pyramid_parent_golden.py [out.npz]

hhsr_gauss_decimate on an MI355X, factors 2 and 4, of the images of tests/pyramid_tile_cases.py (compact buffers), as float32
arrays under "f<factor>_<shape>_<k>" and "f<factor>_special".  tests/golden/pyramid_parent.npz was written by this tool with
the library of the commit before k_gauss_decimate<F> went to its tiles of a wave per group of rows: the test asks the present
kernel for the same bits.  Run once; a later change of the kernel is compared against the same file, not against a new
recording."""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "handheld-multi-frame-super-resolution_amd"), os.path.join(ROOT, "tests")):
    if p not in sys.path:
        sys.path.insert(0, p)


def decimate(img, f):
    import torch

    from handheld_super_resolution import _lib, utils_image

    H, W = img.shape
    src = torch.as_tensor(np.array(img), dtype=torch.float32).cuda()
    dst = torch.empty(((H - 4 * f) // f, (W - 4 * f) // f), dtype=torch.float32, device="cuda")
    taps, ntaps = utils_image._taps_for_launch(f)
    _lib.call("hhsr_gauss_decimate", _lib.ptr(src), H, W, W, _lib.ptr(dst), dst.shape[1], f, taps, ntaps, _lib.stream())
    return dst.cpu().numpy()


def record():
    import pyramid_tile_cases as pc
    from handheld_super_resolution import _lib

    out = {}
    for f in (2, 4):
        for name in pc.shapes(f):
            for k in range(pc.N_IMAGES):
                out[pc.golden_key(f, name, k)] = decimate(pc.image(f, name, k), f)
        out[f"f{f}_special"] = decimate(pc.special_image(f), f)
    return out, _lib.LIB_PATH


if __name__ == "__main__":
    path = sys.argv[1] if len(sys.argv) > 1 else os.path.join(ROOT, "tests", "golden", "pyramid_parent.npz")
    arrays, lib = record()
    np.savez_compressed(path, **arrays)
    print(f"{path}: {len(arrays)} arrays, {os.path.getsize(path)} bytes, computed by {lib}")
