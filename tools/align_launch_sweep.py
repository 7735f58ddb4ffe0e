"""us per hhsr_align_level_batch launch (4 and 3 frames, zero incoming flow) over the tile count, for the instantiations of
k_align_wave that have a frame loop.  The library is the one HHSR_LIB names (A/B builds: tools/build_variant.sh
<name> hhsr_align "-DHHSR_ALIGN_LOOP_MIN_TILES=<0 | 1073741824>" = loop at every size | never), else the built one.

    HHSR_LIB=$PWD/variants_loop0.so python tools/align_launch_sweep.py
"""
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "handheld-multi-frame-super-resolution_amd")]
import numpy as np  # noqa: E402
import torch  # noqa: E402
from handheld_super_resolution import ICA, _lib  # noqa: E402

SMALL = [(8, 8), (16, 16), (23, 31), (32, 32), (32, 64), (64, 64), (64, 128), (93, 125)]
SWEEP = [  # (ts, r, metric code, tile grids)
    (16, 1, 1, SMALL + [(128, 128), (128, 160), (128, 192), (128, 224), (128, 256), (160, 256), (187, 250)]),
    (16, 2, 0, [(64, 64), (128, 128), (128, 192), (128, 256)]),
    (8, 1, 0, [(128, 128), (128, 192), (128, 256), (256, 256)]),
    (32, 1, 1, [(32, 32), (64, 64), (93, 125), (128, 128), (128, 192)]),
]

print("lib", _lib.LIB_PATH)
torch.manual_seed(0)
for ts, r, metric, grids in SWEEP:
    for ny, nx in grids:
        h, w = ny * ts, nx * ts
        base = torch.nn.functional.avg_pool2d(torch.rand(1, 1, h + 8, w + 8, device="cuda"), 5, 1, 2)[0, 0]
        ref = base[4:4 + h, 4:4 + w].contiguous()
        movs = [(base[4 + k % 3:4 + k % 3 + h, 3 + k:3 + k + w] + 0.01 * torch.rand(h, w, device="cuda")).contiguous()
                for k in range(4)]
        hess = ICA.init_ica(ref, ts)[2]
        flows = [torch.zeros(ny, nx, 2, device="cuda") for _ in range(4)]
        res = []
        for nf in (4, 3):
            def launch():
                _lib.call("hhsr_align_level_batch", _lib.ptr(ref), h, w, w, _lib.ptr(hess), _lib.ptr_array(movs[:nf]), nf,
                          h, w, w, _lib.ptr_array(flows[:nf]), ny, nx, ts, r, metric, 3, None, 0, 0, -1, 1.0, _lib.stream())

            for _ in range(5):
                launch()
            torch.cuda.synchronize()
            t = []
            for _ in range(5):  # 5 blocks of 20 back-to-back launches between two events
                a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                a.record()
                for _ in range(20):
                    launch()
                b.record()
                torch.cuda.synchronize()
                t.append(a.elapsed_time(b) * 1000 / 20)
            res.append(f"nf={nf}: median {np.median(t):7.1f} us (min {min(t):.1f} max {max(t):.1f})")
        print(f"tiles {ny * nx:6d} ({ny}x{nx}) ts={ts} r={r}  " + "   ".join(res), flush=True)
