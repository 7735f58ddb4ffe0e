"""Size and time of the JPEG options on one MI355X: {4:4:4, 4:2:0} x {standard, optimised tables} (method of tools/jpeg_time.py,
whose photograph-like image this uses).

    python tools/jpeg_subsampling_time.py [--shape 6000x8000] [--blocks 7] [--calls 3] [--restarts 8,16,64,256,1024,4096]
                                          [--parent-lib path/to/libhhsr_hip.so]

(1) per combination: the file's bytes, the tail device float32 image -> host bytes (encode_jpeg, wall clock around
    synchronised calls, the four legs alternating in one process, median (min - max) of the blocks) and every device stage
    on its own (HIP events around blocks of back-to-back calls): the transform, the histogram, the entropy coder;
(2) for 4:2:0 with the standard tables, the restart sweep: scan bytes and coder time per interval;
(3) with --parent-lib (a build of the parent commit): the 4:4:4 / standard route of this build against the parent's, the same
    calls through both libraries, blocks alternating: both stages on the device and the tail.  This build's median must lie
    within the range of the parent's blocks; the script exits non-zero, after printing everything, when it does not.

The script ends itself after --timeout seconds and fails without a device."""
import argparse
import ctypes
import os
import signal
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (os.path.join(ROOT, "tests"), os.path.join(ROOT, "handheld-multi-frame-super-resolution_amd"),
          os.path.dirname(os.path.abspath(__file__))):
    sys.path.insert(0, p)

from jpeg_time import photo_like  # noqa: E402
from output_time import fmt, gpu_blocks, wall_blocks  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--shape", default="6000x8000")
    ap.add_argument("--blocks", type=int, default=7)
    ap.add_argument("--calls", type=int, default=3)
    ap.add_argument("--tail-calls", type=int, default=2)
    ap.add_argument("--quality", type=int, default=90)
    ap.add_argument("--restarts", default="8,16,64,256,1024,4096")
    ap.add_argument("--parent-lib", default=None)
    ap.add_argument("--timeout", type=int, default=540)
    args = ap.parse_args()
    assert args.blocks >= 5
    signal.alarm(args.timeout)  # a hang ends here, not at somebody else's limit

    import numpy as np
    import torch

    from handheld_super_resolution import _lib, utils_image

    assert torch.cuda.is_available(), "jpeg_subsampling_time.py measures on the GPU: no device, no number"
    dev = torch.device("cuda", 0)
    H, W = (int(v) for v in args.shape.split("x"))
    px, q, ri = H * W, args.quality, utils_image.JPEG_RESTART_MCUS
    img = photo_like(H, W, dev, 7)
    s = _lib.stream(dev)
    print(f"# JPEG options at quality {q}, Ri {ri}: median of {args.blocks} blocks (min - max), legs alternating in one process; "
          f"kernel blocks of {args.calls} calls, tail blocks of {args.tail_calls}")
    print(f"# device: {torch.cuda.get_device_name(0)}; {H} x {W} x 3 ({px / 1e6:.0f} MP), photograph-like")

    length = torch.empty(1, dtype=torch.int64, device=dev)
    scan = torch.empty(2 * px * 3, dtype=torch.uint8, device=dev)
    counts = torch.empty((4, 256), dtype=torch.int64, device=dev)
    combos = [("444", "standard"), ("444", "optimized"), ("420", "standard"), ("420", "optimized")]
    print("  (1) the four combinations")
    tails = wall_blocks([lambda a=a, b=b: utils_image.encode_jpeg(img, quality=q, subsampling=a, huffman=b) for a, b in combos],
                        args.blocks, args.tail_calls)
    sizes = {}
    for (a, b), t in zip(combos, tails):
        data = utils_image.encode_jpeg(img, quality=q, subsampling=a, huffman=b)
        sizes[a, b] = data.size
        print(f"    {a} / {b:9s}: file {data.size / 1e6:7.3f} MB = {100 * data.size / sizes['444', 'standard']:5.1f} % of 444 / standard"
              f" | device image -> host bytes {fmt(t)}", flush=True)
    for sub_name, sub in (("444", 0), ("420", 1)):
        coef_bytes, scratch_bytes, _ = utils_image.jpeg_workspace_ex(H, W, 3, ri, sub)
        coef = torch.empty(coef_bytes // 2, dtype=torch.int16, device=dev)
        scratch = torch.empty((scratch_bytes + 7) // 8, dtype=torch.int64, device=dev)

        def dct():
            _lib.call("hhsr_jpeg_dct_ex", _lib.ptr(img), H, W, 3, 3, q, sub, _lib.ptr(coef), coef_bytes, s)

        def hist():
            _lib.call("hhsr_jpeg_histogram", _lib.ptr(coef), H, W, 3, sub, ri, _lib.ptr(counts), _lib.ptr(scratch),
                      scratch.numel() * 8, s)

        def entropy(spec=None, interval=ri):
            _lib.call("hhsr_jpeg_entropy_ex", _lib.ptr(coef), H, W, 3, interval, sub, utils_image._jpeg_spec(spec, 4),
                      _lib.ptr(scratch), scratch.numel() * 8, _lib.ptr(scan), scan.numel(), _lib.ptr(length), s)

        dct()
        hist()
        spec = utils_image.jpeg_huffman(counts.cpu().numpy().view(np.uint64))
        d, h, e_std, e_opt = gpu_blocks([dct, hist, entropy, lambda: entropy(spec)], args.blocks, args.calls)
        print(f"    {sub_name}: hhsr_jpeg_dct_ex {fmt(d)} | {(12 * px + coef_bytes) / 1e9:.2f} GB -> "
              f"{(12 * px + coef_bytes) / d[0] / 1e9:.2f} TB/s")
        print(f"    {sub_name}: hhsr_jpeg_histogram {fmt(h)} | coefficients read once, {coef_bytes / h[0] / 1e9:.2f} TB/s")
        print(f"    {sub_name}: hhsr_jpeg_entropy_ex, standard tables {fmt(e_std)}; optimised tables {fmt(e_opt)}", flush=True)
        if sub:
            print("  (2) 4:2:0, standard tables: the restart sweep (an MCU is 16 x 16 pixels)")
            rows = []
            for interval in (int(v) for v in args.restarts.split(",")):
                _, need, _ = utils_image.jpeg_workspace_ex(H, W, 3, interval, sub)
                big = torch.empty((need + 7) // 8, dtype=torch.int64, device=dev)

                def sweep():
                    _lib.call("hhsr_jpeg_entropy_ex", _lib.ptr(coef), H, W, 3, interval, sub, None, _lib.ptr(big), big.numel() * 8,
                              _lib.ptr(scan), scan.numel(), _lib.ptr(length), s)

                (e,) = gpu_blocks([sweep], args.blocks, args.calls)
                rows.append((interval, e, int(length.item())))
            smallest = min(n for _, _, n in rows)
            for interval, e, n in rows:
                print(f"      Ri {interval:5d}: {fmt(e)} | scan {n / 1e6:.3f} MB, +{100 * (n / smallest - 1):.2f} % over the smallest",
                      flush=True)
        del coef, scratch

    failed = 0
    if args.parent_lib:
        print("  (3) 4:4:4 / standard: this build against the library built from the parent commit")
        parent = ctypes.CDLL(args.parent_lib)
        ours = _lib.load()
        for name in ("hhsr_jpeg_dct", "hhsr_jpeg_entropy"):
            getattr(parent, name).argtypes = _lib._SIGS[name]
        coef_bytes, scratch_bytes, _ = utils_image.jpeg_workspace(H, W, 3, ri)
        coef = torch.empty(coef_bytes // 2, dtype=torch.int16, device=dev)
        scratch = torch.empty((scratch_bytes + 7) // 8, dtype=torch.int64, device=dev)

        def dct(lib):
            assert lib.hhsr_jpeg_dct(_lib.ptr(img), H, W, 3, 3, q, _lib.ptr(coef), coef_bytes, s) == 0

        def entropy(lib):
            assert lib.hhsr_jpeg_entropy(_lib.ptr(coef), H, W, 3, ri, _lib.ptr(scratch), scratch.numel() * 8, _lib.ptr(scan),
                                         scan.numel(), _lib.ptr(length), s) == 0

        def tail(lib):  # the default route of encode_jpeg, call for call
            dct(lib)
            entropy(lib)
            n = int(length.item())
            return scan[:n].cpu().numpy()

        rows = gpu_blocks([lambda: dct(parent), lambda: dct(ours), lambda: entropy(parent), lambda: entropy(ours)],
                          args.blocks, args.calls)
        rows += wall_blocks([lambda: tail(parent), lambda: tail(ours)], args.blocks, args.tail_calls)
        for what, (a, b) in zip(("hhsr_jpeg_dct", "hhsr_jpeg_entropy", "dct + entropy + length word + copy of the scan"),
                                zip(rows[0::2], rows[1::2])):
            ok = b[0] <= a[2]  # (faster than every block of the parent is no regression)
            inside = a[1] <= b[0] <= a[2]
            failed += not ok
            print(f"    {what}: parent {fmt(a)} | this build {fmt(b)} | this build's median is "
                  f"{'inside' if inside else ('below' if ok else 'ABOVE')} the range of the parent's blocks", flush=True)
    if failed:
        sys.exit("jpeg_subsampling_time.py: the 4:4:4 / standard route is slower than every block of the parent's")


if __name__ == "__main__":
    main()
