"""Time of the integer output on one MI355X: the encode kernel, the tail device image -> host ndarray, and the
post-processing as one line of context.

    python tools/output_time.py [--shapes 6000x8000,3000x4000] [--blocks 7] [--calls 5]

(a) hhsr_encode_image, 8 and 16 bits, HIP events around blocks of `calls` back-to-back calls after a warm-up; the figure
    is the median block / calls (min - max).  Bytes from the shapes: 12 B/px read + 3 or 6 B/px written, as a share of the
    8 TB/s specification and of the 6.29 TB/s a float4 copy reaches.  The kernel does nothing but move these bytes: it is
    bandwidth-bound.  Baseline: the expression a user would write with torch today,
    (x.nan_to_num().clamp(0, 1) * M).round().to(dtype), its blocks alternating with the kernel's in the same process.
(b) the tail: device float32 image -> host ndarray, wall clock around a synchronised call, three legs whose blocks
    alternate: float32 as process() returns it today (x.cpu().numpy()), uint8 and uint16 with the encode included
    (encode_image(x, dtype).cpu().numpy()).  Pageable destination, as process() has it; for information the same with a
    page-locked destination allocated once outside the timed region (copy_ into a pinned tensor).
(c) raw2rgb.postprocess with the defaults (gamma + unsharp mask) at the first shape.

The script ends itself after --timeout seconds, fails without a device, and exits non-zero — after printing everything —
when the kernel is slower than the torch expression or the uint8 tail is not shorter than the float32 tail by more than
the blocks' spread."""
import argparse
import os
import signal
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (os.path.join(ROOT, "tests"), os.path.join(ROOT, "handheld-multi-frame-super-resolution_amd")):
    sys.path.insert(0, p)

HBM_PEAK = 8.0e12       # B/s, specification
HBM_MEASURED = 6.29e12  # B/s, float4 copy
LINK_SPEC = 63e9        # B/s, the host link's specification


def stats(ms):
    ms = sorted(ms)
    return ms[len(ms) // 2], ms[0], ms[-1]


def gpu_blocks(fns, blocks, calls):
    """Median (min, max) ms per call of each fn: HIP events around blocks of `calls` calls, the fns' blocks alternating."""
    import torch

    for fn in fns:
        for _ in range(3):
            fn()
    torch.cuda.synchronize()
    ms = [[] for _ in fns]
    for _ in range(blocks):
        for i, fn in enumerate(fns):
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            for _ in range(calls):
                fn()
            b.record()
            b.synchronize()
            ms[i].append(a.elapsed_time(b) / calls)
    return [stats(m) for m in ms]


def wall_blocks(fns, blocks, calls):
    """The same with the wall clock around synchronised host-visible work (each fn returns when its result is on the host)."""
    import torch

    for fn in fns:
        fn()
    ms = [[] for _ in fns]
    for _ in range(blocks):
        for i, fn in enumerate(fns):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            for _ in range(calls):
                fn()
            torch.cuda.synchronize()
            ms[i].append((time.perf_counter() - t0) * 1e3 / calls)
    return [stats(m) for m in ms]


def fmt(s):
    return f"{s[0]:.3f} ms ({s[1]:.3f} - {s[2]:.3f})"


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--shapes", default="6000x8000,3000x4000")
    ap.add_argument("--blocks", type=int, default=7)
    ap.add_argument("--calls", type=int, default=5)
    ap.add_argument("--tail-calls", type=int, default=2)
    ap.add_argument("--timeout", type=int, default=540)
    args = ap.parse_args()
    assert args.blocks >= 5
    signal.alarm(args.timeout)  # a hang ends here, not at somebody else's limit

    import torch

    from handheld_super_resolution import _lib, raw2rgb
    from handheld_super_resolution.config import Config
    from handheld_super_resolution.utils_image import encode_image

    assert torch.cuda.is_available(), "output_time.py measures on the GPU: no device, no number"
    dev = torch.device("cuda", 0)
    print(f"# integer output: median of {args.blocks} blocks (min - max), legs alternating in one process; "
          f"kernel blocks of {args.calls} calls, tail blocks of {args.tail_calls}")
    print(f"# device: {torch.cuda.get_device_name(0)}")
    shapes = [tuple(int(v) for v in s.split("x")) for s in args.shapes.split(",")]
    failed = 0  # verdicts that went the wrong way: the profile is still printed whole, the exit status tells
    for H, W in shapes:
        g = torch.Generator(device=dev).manual_seed(H * 7 + W)
        img = torch.rand((H, W, 3), generator=g, device=dev) * 1.5 - 0.2
        img[::97, ::89] = float("nan")
        px = H * W
        s = _lib.stream(dev)
        print(f"{H} x {W} x 3 ({px / 1e6:.0f} MP)")

        print("  (a) encode on the device — bandwidth-bound: 12 B/px read + 3 or 6 B/px written, nothing else")
        for bits, name in ((8, "uint8"), (16, "uint16")):
            dt = getattr(torch, name)
            out = torch.empty((H, W, 3), dtype=dt, device=dev)
            M = float(2 ** bits - 1)

            def kernel():
                _lib.call("hhsr_encode_image", _lib.ptr(img), H, W, 3, 3, _lib.ptr(out), bits, W * 3 * bits // 8, s)

            def torch_expr():
                return (img.nan_to_num().clamp(0, 1) * M).round().to(dt)

            kernel()
            assert torch.equal(out, torch_expr()), "the kernel and the torch expression disagree"
            (k, t) = gpu_blocks([kernel, torch_expr], args.blocks, args.calls)
            nbytes = (12 + 3 * bits // 8) * px
            slower = k[0] > t[0] + (t[2] - t[0]) + (k[2] - k[0])
            failed += slower
            verdict = "SLOWER than the baseline beyond the spread" if slower else "not slower"
            print(f"    hhsr_encode_image {name}: {fmt(k)} | {nbytes / 1e9:.2f} GB -> {nbytes / k[0] / 1e9:.2f} TB/s = "
                  f"{100 * nbytes / (k[0] * 1e-3) / HBM_PEAK:.1f} % of the 8 TB/s peak "
                  f"({100 * nbytes / (k[0] * 1e-3) / HBM_MEASURED:.1f} % of the 6.29 TB/s copy rate)")
            print(f"    torch expression  {name}: {fmt(t)} | kernel / torch = {k[0] / t[0]:.2f} ({verdict})", flush=True)
            del out

        print("  (b) tail: device float32 image -> host ndarray, wall clock (encode included in the integer legs)")
        legs = [("float32 (today)", lambda: img.cpu().numpy(), 12),
                ("uint8", lambda: encode_image(img, "uint8").cpu().numpy(), 3),
                ("uint16", lambda: encode_image(img, "uint16").cpu().numpy(), 6)]
        res = wall_blocks([f for _, f, _ in legs], args.blocks, args.tail_calls)
        for (name, _, bpp), r in zip(legs, res):
            print(f"    pageable    {name:16s}: {fmt(r)} | {bpp * px / 1e6:.0f} MB -> {bpp * px / r[0] / 1e6:.1f} GB/s "
                  f"(floor at the link's 63 GB/s: {bpp * px / LINK_SPEC * 1e3:.1f} ms)")
        f32, u8 = res[0], res[1]
        gap, spread = f32[0] - u8[0], max(f32[2] - f32[0], f32[0] - f32[1], u8[2] - u8[0], u8[0] - u8[1])
        failed += not gap > spread
        print(f"    uint8 is {gap:.3f} ms shorter than float32; largest distance of a block from its median {spread:.3f} ms: "
              f"{'shorter by more than the spread' if gap > spread else 'NOT shorter by more than the spread'}", flush=True)
        pinned = {n: torch.empty((H, W, 3), dtype=d).pin_memory() for n, d in
                  (("float32", torch.float32), ("uint8", torch.uint8), ("uint16", torch.uint16))}
        legs = [("float32", lambda: pinned["float32"].copy_(img), 12),
                ("uint8", lambda: pinned["uint8"].copy_(encode_image(img, "uint8")), 3),
                ("uint16", lambda: pinned["uint16"].copy_(encode_image(img, "uint16")), 6)]
        res = wall_blocks([f for _, f, _ in legs], args.blocks, args.tail_calls)
        for (name, _, bpp), r in zip(legs, res):
            print(f"    page-locked {name:16s}: {fmt(r)} | {bpp * px / r[0] / 1e6:.1f} GB/s (information: staging is not built)")
        del pinned
        if (H, W) == shapes[0]:
            sharpen = Config({"enabled": True, "amount": 1.5, "radius": 3})
            (p,) = gpu_blocks([lambda: raw2rgb.postprocess(None, img, False, False, True, sharpen, False)], args.blocks, args.calls)
            print(f"  (c) raw2rgb.postprocess, defaults (unsharp mask + gamma), allocations included: {fmt(p)}", flush=True)
        del img
        torch.cuda.empty_cache()
    if failed:
        sys.exit(f"output_time.py: {failed} verdict(s) above went the wrong way (kernel slower than the torch expression, or "
                 "the uint8 tail not shorter than the float32 tail, beyond the blocks' spread)")


if __name__ == "__main__":
    main()
