"""Time and size of the PNG output on one MI355X against the host path it replaces (method of tools/jpeg_time.py).

    python tools/png_time.py [--shape 6000x8000] [--bits 8,16] [--blocks 7] [--calls 3] [--intervals 4096,...,262144]
                             [--parent-lib path/to/libhhsr_hip.so] [--skip a,d]

The photograph-like image of tools/jpeg_time.py (photo_like, seed 7), made on the device.  Per bit depth:
(a) device float32 image -> file bytes on the host, wall clock around synchronised calls, legs alternating in one process:
    the parent commit's path — encode_image, .cpu(), utils_image.save_png into a memory file (filter 0, zlib level 1 on the
    host) — against encode_png (adaptive filters, the default interval); both file sizes;
(b) the stages of encode_png: HIP events around blocks of `calls` calls of hhsr_png_filter (with its share of the 6.29 TB/s
    copy rate: 12 B/px read + the stream written) and of hhsr_png_deflate (size pass, offsets scan, write pass, checksums),
    and the wall clock of the two synchronisations (counts -> host code; result words and the file's bytes -> host);
(c) the interval sweep: time of hhsr_png_deflate and size of the file per interval; the default is the fastest interval
    whose file is within 1 % of the largest interval's file — chosen value and runner-up are printed;
(d) the file against zlib on the same filtered stream: Z_HUFFMAN_ONLY and level 6, as sizes;
(e) once, with --parent-lib: hhsr_encode_image (uint8) and hhsr_jpeg_dct + hhsr_jpeg_entropy (4:4:4, quality 90) through
    this build and through the parent's library, blocks alternating in one process — nothing of theirs moved.

The script ends itself after --timeout seconds and fails without a device."""
import argparse
import ctypes
import os
import signal
import sys
import tempfile
import time
import zlib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (os.path.join(ROOT, "tests"), os.path.join(ROOT, "handheld-multi-frame-super-resolution_amd")):
    sys.path.insert(0, p)

from jpeg_time import HBM_MEASURED, photo_like  # noqa: E402  (the same image)
from output_time import fmt, gpu_blocks, stats, wall_blocks  # noqa: E402  (the same block statistics)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--shape", default="6000x8000")
    ap.add_argument("--bits", default="8,16")
    ap.add_argument("--blocks", type=int, default=7)
    ap.add_argument("--calls", type=int, default=3)
    ap.add_argument("--intervals", default="4096,8192,16384,32768,65536,131072,262144")
    ap.add_argument("--parent-lib", default=None)
    ap.add_argument("--skip", default="")
    ap.add_argument("--timeout", type=int, default=1100)
    args = ap.parse_args()
    assert args.blocks >= 5
    signal.alarm(args.timeout)  # a hang ends here, not at somebody else's limit

    import numpy as np
    import torch

    from handheld_super_resolution import _lib, utils_image

    assert torch.cuda.is_available(), "png_time.py measures on the GPU: no device, no number"
    dev = torch.device("cuda", 0)
    H, W = (int(v) for v in args.shape.split("x"))
    px = H * W
    skip = set(args.skip.split(",")) - {""}
    intervals = [int(v) for v in args.intervals.split(",")]
    default_i = utils_image.PNG_INTERVAL_BYTES
    s = _lib.stream(dev)
    img = photo_like(H, W, dev, 7)
    print(f"# PNG output: median of {args.blocks} blocks (min - max), legs alternating in one process; kernel blocks of "
          f"{args.calls} calls")
    print(f"# device: {torch.cuda.get_device_name(0)}; {H} x {W} x 3 ({px / 1e6:.0f} MP), photograph-like; default interval "
          f"{default_i} bytes", flush=True)
    memdir = "/dev/shm" if os.path.isdir("/dev/shm") else None
    for bits in (int(v) for v in args.bits.split(",")):
        dtype = "uint8" if bits == 8 else "uint16"
        n, scratch_bytes, bound = utils_image.png_workspace(H, W, 3, bits, min(intervals + [default_i]))
        print(f"{bits} bits: filtered stream {n / 1e6:.2f} MB")
        filtered = torch.empty(n, dtype=torch.uint8, device=dev)
        scratch = torch.empty((scratch_bytes + 7) // 8, dtype=torch.int64, device=dev)
        counts = torch.empty(256, dtype=torch.int64, device=dev)
        result = torch.empty(3, dtype=torch.int64, device=dev)
        out = torch.empty(bound, dtype=torch.uint8, device=dev)

        def run_filter():
            _lib.call("hhsr_png_filter", _lib.ptr(img), H, W, 3, 3, bits, 5, _lib.ptr(filtered), n, _lib.ptr(counts),
                      _lib.ptr(scratch), scratch.numel() * 8, s)

        def spec_for(interval):
            c = np.empty(257, np.uint64)
            c[:256] = counts.cpu().numpy().view(np.uint64)
            c[256] = -(-n // interval)
            return utils_image.png_huffman(c)

        def deflate_call(interval, spec):
            p = spec.ctypes.data_as(ctypes.POINTER(ctypes.c_uint8))
            return lambda: _lib.call("hhsr_png_deflate", _lib.ptr(filtered), n, interval, p, _lib.ptr(scratch),
                                     scratch.numel() * 8, _lib.ptr(out), bound, _lib.ptr(result), s)

        run_filter()
        if "a" not in skip:
            def parent_path():
                host = utils_image.encode_image(img, dtype).cpu().numpy()
                with tempfile.NamedTemporaryFile(dir=memdir, suffix=".png") as f:
                    utils_image.save_png(host, f.name)
                    return os.path.getsize(f.name)

            def png_path():
                return utils_image.encode_png(img, bits=bits).size

            a, b = wall_blocks([parent_path, png_path], args.blocks, 1)
            na, nb = parent_path(), png_path()
            print(f"  (a) parent: encode_image, .cpu(), save_png (filter 0, zlib 1, host): {fmt(a)} | {na / 1e6:.2f} MB")
            print(f"      encode_png (adaptive, interval {default_i})                     : {fmt(b)} | {nb / 1e6:.2f} MB, "
                  f"{100 * (1 - nb / na):.1f} % smaller, {a[0] / b[0]:.0f} x shorter", flush=True)

        (f,) = gpu_blocks([run_filter], args.blocks, args.calls)
        moved = 12 * px + n
        print(f"  (b) hhsr_png_filter (adaptive): {fmt(f)} | {moved / 1e9:.2f} GB -> {moved / f[0] / 1e9:.2f} TB/s = "
              f"{100 * moved / (f[0] * 1e-3) / HBM_MEASURED:.1f} % of the 6.29 TB/s copy rate")
        (d,) = gpu_blocks([deflate_call(default_i, spec_for(default_i))], args.blocks, args.calls)
        print(f"      hhsr_png_deflate, interval {default_i} (sizes, scan, write, checksums): {fmt(d)}")
        t_counts, t_code, t_words, t_bytes = [], [], [], []
        for _ in range(args.blocks):  # the two synchronisations of encode_png, wall clock, the device idle before each
            run_filter()
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            host_counts = counts.cpu().numpy()
            t1 = time.perf_counter()
            spec = spec_for(default_i)
            t2 = time.perf_counter()
            deflate_call(default_i, spec)()
            torch.cuda.synchronize()
            t3 = time.perf_counter()
            length = int(result.cpu().numpy()[0])
            t4 = time.perf_counter()
            data = out[:length].cpu().numpy()
            t5 = time.perf_counter()
            t_counts.append((t1 - t0) * 1e3), t_code.append((t2 - t1) * 1e3), t_words.append((t4 - t3) * 1e3), t_bytes.append((t5 - t4) * 1e3)
            del host_counts, data
        print(f"      sync 1: counts -> host {fmt(stats(t_counts))}, the code on the host (with a second copy of the counts) "
              f"{fmt(stats(t_code))}")
        print(f"      sync 2: result words -> host {fmt(stats(t_words))}, {length / 1e6:.2f} MB of file bytes -> host (pageable) "
              f"{fmt(stats(t_bytes))}", flush=True)

        rows = []
        for interval in intervals:
            (e,) = gpu_blocks([deflate_call(interval, spec_for(interval))], args.blocks, args.calls)
            rows.append((interval, e, int(result.cpu().numpy()[0]) + 63))
        largest = rows[-1][2]
        ok = sorted((r for r in rows if r[2] <= 1.01 * largest), key=lambda r: r[1][0])
        print("  (c) interval sweep (hhsr_png_deflate; file = stream + 63 bytes)")
        for interval, e, size in rows:
            print(f"      {interval:7d} B: {fmt(e)} | file {size / 1e6:.3f} MB, +{100 * (size / largest - 1):.2f} % over the "
                  f"largest interval's")
        print(f"      fastest within 1 % of the largest interval's file: {ok[0][0]} B; runner-up: "
              f"{ok[1][0] if len(ok) > 1 else 'none'} B", flush=True)

        if "d" not in skip:
            deflate_call(default_i, spec_for(default_i))()
            ours = int(result.cpu().numpy()[0])
            host = filtered.cpu().numpy().tobytes()
            sizes = {}
            for name, level, strategy in (("Z_HUFFMAN_ONLY", 6, zlib.Z_HUFFMAN_ONLY), ("level 6", 6, zlib.Z_DEFAULT_STRATEGY)):
                c = zlib.compressobj(level, zlib.DEFLATED, 15, 9, strategy)
                t0 = time.perf_counter()
                sizes[name] = len(c.compress(host)) + len(c.flush())
                print(f"  (d) zlib {name} on the same filtered stream: {sizes[name] / 1e6:.3f} MB ({time.perf_counter() - t0:.1f} s "
                      f"on the host, one run); this coder: {(ours + 6) / 1e6:.3f} MB = {100 * ((ours + 6) / sizes[name] - 1):+.2f} %",
                      flush=True)
            del host
        del filtered, scratch, out
        torch.cuda.empty_cache()

    if args.parent_lib:
        parent = ctypes.CDLL(args.parent_lib)
        this = _lib.load()
        for name in ("hhsr_encode_image", "hhsr_jpeg_dct", "hhsr_jpeg_entropy"):
            getattr(parent, name).argtypes = _lib._SIGS[name]
        u8 = torch.empty((H, W, 3), dtype=torch.uint8, device=dev)
        coef_bytes, jscratch_bytes, _ = utils_image.jpeg_workspace(H, W, 3, utils_image.JPEG_RESTART_MCUS)
        coef = torch.empty(coef_bytes // 2, dtype=torch.int16, device=dev)
        jscratch = torch.empty((jscratch_bytes + 7) // 8, dtype=torch.int64, device=dev)
        scan = torch.empty(2 * px * 3, dtype=torch.uint8, device=dev)
        length = torch.empty(1, dtype=torch.int64, device=dev)

        def encode(lib):
            def call():
                assert lib.hhsr_encode_image(_lib.ptr(img), H, W, 3, 3, _lib.ptr(u8), 8, W * 3, s) == 0
            return call

        def jpeg(lib):
            def call():
                assert lib.hhsr_jpeg_dct(_lib.ptr(img), H, W, 3, 3, 90, _lib.ptr(coef), coef_bytes, s) == 0
                assert lib.hhsr_jpeg_entropy(_lib.ptr(coef), H, W, 3, utils_image.JPEG_RESTART_MCUS, _lib.ptr(jscratch),
                                             jscratch.numel() * 8, _lib.ptr(scan), scan.numel(), _lib.ptr(length), s) == 0
            return call

        print("  (e) the parent's routes, this build | the parent's library, blocks alternating")
        for name, make in (("hhsr_encode_image uint8", encode), ("hhsr_jpeg_dct + hhsr_jpeg_entropy 4:4:4 q90", jpeg)):
            a, b = gpu_blocks([make(this), make(parent)], args.blocks, args.calls)
            print(f"      {name}: {fmt(a)} | {fmt(b)}", flush=True)


if __name__ == "__main__":
    main()
