"""Time of the tone mapping on one MI355X: hhsr_post_expose, hhsr_mertens and the whole
raw2rgb.postprocess(do_tonemapping=True), per image size.

    python tools/tonemap_time.py [--shapes 6000x8000,3000x4000] [--blocks 7] [--calls 5] [--cpu-shape 3000x4000]

HIP events around blocks of `calls` back-to-back calls after a warm-up; the figure is the median block / calls.  Bytes
are counted from the shapes, twice: by the traffic model of the algorithm (exposures 9 B/px, weights 12 B/px, pyramids
4/3 x 48 B/px, output 12 B/px = 97 B/px, what a fully fused implementation of MergeMertens would move) and by what
these kernels read and write (143 B/px at 3 exposures: the weight pass, one decimation and one collapse per level; halo
re-reads, served by the caches, not counted).  Share of HBM peak = model bytes / time / 8 TB/s.  The NumPy restatement
(tests/mertens_ref.py) is timed once on the CPU as context.  The script ends itself after --timeout seconds."""
import argparse
import ctypes
import os
import signal
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (os.path.join(ROOT, "tests"), os.path.join(ROOT, "handheld-multi-frame-super-resolution_amd")):
    sys.path.insert(0, p)

HBM_PEAK = 8.0e12       # B/s, specification
HBM_MEASURED = 6.29e12  # B/s, float4 copy
MODEL_BPP = 9 + 12 + 48 * 4 / 3 + 12


def kernel_bytes_per_pixel(n):
    """What the kernels of hhsr_mertens read + write per level-0 pixel (geometric sums over the levels, halos not counted)."""
    e, w, g, gc, r = 3 * n, 4 * n, 16 * n, 12 * n, 12  # uint8 exposures, wn, G_l (4 planes), its 3 colours, out_l
    weights = e + w
    down0 = e + w + g / 4
    down = g / 3 + g / 12
    up = g / 3 + (gc + r) / 12 + r / 3
    up0 = e + w + (gc + r) / 4 + r
    return weights + down0 + down + up + up0


def gpu_ms(fn, blocks, calls):
    import torch

    for _ in range(3):
        fn()
    torch.cuda.synchronize()
    ms = []
    for _ in range(blocks):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        for _ in range(calls):
            fn()
        b.record()
        b.synchronize()
        ms.append(a.elapsed_time(b) / calls)
    ms.sort()
    return ms[len(ms) // 2], ms[0], ms[-1]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--shapes", default="6000x8000,3000x4000")
    ap.add_argument("--blocks", type=int, default=7)
    ap.add_argument("--calls", type=int, default=5)
    ap.add_argument("--cpu-shape", default="3000x4000", help="size of the one CPU run of the restatement ('' = skip)")
    ap.add_argument("--timeout", type=int, default=540)
    args = ap.parse_args()
    signal.alarm(args.timeout)  # a hang ends here, not at somebody else's limit

    import numpy as np
    import torch

    from handheld_super_resolution import _lib, raw2rgb

    assert torch.cuda.is_available(), "tonemap_time.py measures on the GPU: no device, no number"
    dev = torch.device("cuda", 0)
    n = len(raw2rgb.TONEMAP_TIMES)
    print(f"# tone mapping, n = {n} exposures, median of {args.blocks} blocks of {args.calls} calls (min - max); "
          f"model {MODEL_BPP:.0f} B/px, kernels {kernel_bytes_per_pixel(n):.0f} B/px")
    print(f"# device: {torch.cuda.get_device_name(0)}")
    for shape in args.shapes.split(","):
        H, W = (int(v) for v in shape.split("x"))
        g = torch.Generator(device=dev).manual_seed(H * 7 + W)
        img = torch.rand((H, W, 3), generator=g, device=dev) * 1.3 - 0.1
        nbytes, levels = ctypes.c_size_t(), ctypes.c_int()
        _lib.call("hhsr_tonemap_workspace", H, W, n, nbytes, levels)
        expo = torch.empty((n, H, W, 3), dtype=torch.uint8, device=dev)
        work = torch.empty(nbytes.value, dtype=torch.uint8, device=dev)
        out = torch.empty_like(img)
        times = _lib.doubles(raw2rgb.TONEMAP_TIMES)
        s = _lib.stream(dev)

        def expose():
            _lib.call("hhsr_post_expose", _lib.ptr(img), _lib.ptr(None), H, W, None, 0, 0.0, _lib.ptr(None), 0, 0, times, n,
                      _lib.ptr(expo), s)

        def mertens():
            _lib.call("hhsr_mertens", _lib.ptr(expo), n, H, W, _lib.ptr(work), nbytes.value, _lib.ptr(None), _lib.ptr(out), 1, s)

        def whole():
            raw2rgb.postprocess(None, img, False, True, True, None, False, restated_tonemapping=True)

        px = H * W
        print(f"{H} x {W} ({px / 1e6:.0f} MP), {levels.value} levels, workspace {nbytes.value / 2**20:.0f} MiB")
        for name, fn, model, kern in (("hhsr_post_expose", expose, 12 + 3 * n, 12 + 3 * n),
                                      ("hhsr_mertens", mertens, MODEL_BPP, kernel_bytes_per_pixel(n)),
                                      ("postprocess(do_tonemapping=True), allocations included", whole, None, None)):
            med, lo, hi = gpu_ms(fn, args.blocks, args.calls)
            line = f"  {name}: {med:.3f} ms ({lo:.3f} - {hi:.3f})"
            if model:
                line += (f" | model {model * px / 1e9:.2f} GB -> {model * px / med / 1e9:.2f} TB/s = "
                         f"{100 * model * px / (med * 1e-3) / HBM_PEAK:.1f} % of the 8 TB/s peak "
                         f"({100 * model * px / (med * 1e-3) / HBM_MEASURED:.1f} % of the 6.29 TB/s copy rate)"
                         f" | kernels' own traffic {kern * px / 1e9:.2f} GB -> {kern * px / med / 1e9:.2f} TB/s")
            print(line, flush=True)
        del img, expo, work, out
        torch.cuda.empty_cache()
    if args.cpu_shape:
        import mertens_ref as ref

        H, W = (int(v) for v in args.cpu_shape.split("x"))
        img = (np.random.default_rng(0).random((H, W, 3), dtype=np.float32) * 1.3 - 0.1).astype(np.float32)
        t0 = time.perf_counter()
        ref.tonemap(img)
        print(f"CPU, NumPy restatement (float32), {H} x {W}: {time.perf_counter() - t0:.1f} s (context only)")


if __name__ == "__main__":
    main()
