"""Time of the JPEG output on one MI355X against the uint8 output it competes with (method of tools/output_time.py).

    python tools/jpeg_time.py [--shape 6000x8000] [--blocks 7] [--calls 3] [--restarts 8,16,64,256,1024,4096]
                              [--parent-lib path/to/libhhsr_hip.so]

Two images of the shape, both made on the device from a seed: a photograph-like one (smooth shading, a few hard edges, fine
texture, sensor-like noise of sigma 0.02 = 5 levels, which puts its file at a tenth of its samples) and uniform noise.  For each:
(1) the two stages on the device, HIP events around blocks of `calls` back-to-back calls after a warm-up, median (min - max):
    hhsr_jpeg_dct (12 B/px read + 6 B/px written) and hhsr_jpeg_entropy (its five launches; 6 B/px read twice + the scan
    written) for every restart interval of --restarts, with the size of the file next to the time;
(2) the tail device float32 image -> host bytes, wall clock around synchronised calls, legs alternating in one process:
    (a) the uint8 path of the parent commit — hhsr_encode_image, from --parent-lib when given (a build of the parent commit;
        this commit does not touch that kernel), plus the copy into a pageable ndarray — and
    (b) encode_jpeg end to end at quality 90 with the default interval: both stages, the length word, the copy of exactly
        that many bytes, the assembly of the file;
(3) for information, Pillow's (libjpeg's) encode of the same uint8 samples on the CPU, 4:4:4, same quality, one run.

The script ends itself after --timeout seconds, fails without a device, and exits non-zero — after printing everything —
when (b) is not shorter than (a) by more than the blocks' spread on the photograph-like image; the stage times above it
say where the time went."""
import argparse
import ctypes
import io
import os
import signal
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (os.path.join(ROOT, "tests"), os.path.join(ROOT, "handheld-multi-frame-super-resolution_amd")):
    sys.path.insert(0, p)

from output_time import fmt, gpu_blocks, wall_blocks  # noqa: E402  (the same block statistics)

HBM_MEASURED = 6.29e12  # B/s, float4 copy (profiles/output_encode.txt)
LINK_PAGEABLE = 6.9e9   # B/s, the pageable copy of the uint8 image (profiles/output_encode.txt)


def photo_like(H, W, dev, seed):
    import torch

    g = torch.Generator(device=dev).manual_seed(seed)
    y = torch.linspace(0, 1, H, device=dev)[:, None]
    x = torch.linspace(0, 1, W, device=dev)[None, :]
    shade = 0.5 + 0.3 * torch.sin(3.1 * x + 1.7 * y) * torch.cos(2.3 * y - 0.9 * x)
    edges = 0.15 * ((x * 7).floor() % 2) * ((y * 5).floor() % 2) - 0.1 * ((x + y) > 1.1)
    texture = 0.03 * torch.sin(900 * x) * torch.sin(700 * y) * (y > 0.5)
    base = shade + edges + texture
    img = torch.stack([base, 0.85 * base + 0.1 * x, 0.9 * base + 0.1 * (1 - y)], dim=-1)
    return (img + 0.02 * torch.randn((H, W, 3), generator=g, device=dev)).clamp_(0, 1).contiguous()


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

    assert torch.cuda.is_available(), "jpeg_time.py measures on the GPU: no device, no number"
    dev = torch.device("cuda", 0)
    H, W = (int(v) for v in args.shape.split("x"))
    px, q = H * W, args.quality
    restarts = [int(v) for v in args.restarts.split(",")]
    default_ri = utils_image.JPEG_RESTART_MCUS
    parent = ctypes.CDLL(args.parent_lib) if args.parent_lib else None
    if parent is not None:
        parent.hhsr_encode_image.argtypes = _lib._SIGS["hhsr_encode_image"]
    print(f"# JPEG output at quality {q}: median of {args.blocks} blocks (min - max), legs alternating in one process; "
          f"kernel blocks of {args.calls} calls, tail blocks of {args.tail_calls}")
    print(f"# device: {torch.cuda.get_device_name(0)}; uint8 path (a): "
          f"{'the library built from the parent commit' if parent is not None else 'this build (the kernel is not touched by this commit)'}")
    print(f"# default restart interval: {default_ri} MCUs")
    failed = 0
    for name, img in (("photograph-like", photo_like(H, W, dev, 7)),
                      ("uniform noise", torch.rand((H, W, 3), generator=torch.Generator(device=dev).manual_seed(8), device=dev))):
        s = _lib.stream(dev)
        print(f"{H} x {W} x 3 ({px / 1e6:.0f} MP), {name}")
        coef_bytes, _, _ = utils_image.jpeg_workspace(H, W, 3, 1)
        coef = torch.empty(coef_bytes // 2, dtype=torch.int16, device=dev)
        length = torch.empty(1, dtype=torch.int64, device=dev)
        scan = torch.empty(2 * px * 3, dtype=torch.uint8, device=dev)

        def dct():
            _lib.call("hhsr_jpeg_dct", _lib.ptr(img), H, W, 3, 3, q, _lib.ptr(coef), coef_bytes, s)

        (d,) = gpu_blocks([dct], args.blocks, args.calls)
        nbytes = 18 * px
        print(f"  (1) hhsr_jpeg_dct: {fmt(d)} | {nbytes / 1e9:.2f} GB -> {nbytes / d[0] / 1e9:.2f} TB/s = "
              f"{100 * nbytes / (d[0] * 1e-3) / HBM_MEASURED:.1f} % of the 6.29 TB/s copy rate", flush=True)
        rows = []
        for ri in restarts:
            _, scratch_bytes, _ = utils_image.jpeg_workspace(H, W, 3, ri)
            scratch = torch.empty((scratch_bytes + 7) // 8, dtype=torch.int64, device=dev)

            def entropy():
                _lib.call("hhsr_jpeg_entropy", _lib.ptr(coef), H, W, 3, ri, _lib.ptr(scratch), scratch.numel() * 8,
                          _lib.ptr(scan), scan.numel(), _lib.ptr(length), s)

            (e,) = gpu_blocks([entropy], args.blocks, args.calls)
            n = int(length.item())
            assert n <= scan.numel()
            rows.append((ri, e, n))
            del scratch
        smallest = min(n for _, _, n in rows)
        for ri, e, n in rows:  # (read 6 B/px twice, write the scan)
            moved = 12 * px + n
            print(f"      hhsr_jpeg_entropy Ri {ri:5d}: {fmt(e)} | scan {n / 1e6:.3f} MB = {n / (3 * px):.4f} B/sample, "
                  f"+{100 * (n / smallest - 1):.2f} % over the smallest | {moved / 1e9:.2f} GB -> {moved / e[0] / 1e9:.3f} TB/s | "
                  f"its copy at the 6.9 GB/s pageable rate: {n / LINK_PAGEABLE * 1e3:.2f} ms", flush=True)
        del coef, scan

        print("  (2) tail: device float32 image -> host bytes, wall clock")
        u8 = torch.empty((H, W, 3), dtype=torch.uint8, device=dev)

        def uint8_path():
            if parent is not None:
                rc = parent.hhsr_encode_image(_lib.ptr(img), H, W, 3, 3, _lib.ptr(u8), 8, W * 3, s)
                assert rc == 0
                return u8.cpu().numpy()
            return utils_image.encode_image(img, "uint8").cpu().numpy()

        def jpeg_path():
            return utils_image.encode_jpeg(img, quality=q)

        a, b = wall_blocks([uint8_path, jpeg_path], args.blocks, args.tail_calls)
        data = jpeg_path()
        print(f"    (a) uint8 samples, pageable ndarray : {fmt(a)} | {3 * px / 1e6:.0f} MB")
        print(f"    (b) encode_jpeg, Ri {default_ri}            : {fmt(b)} | {data.size / 1e6:.3f} MB, {3 * px / data.size:.1f} x smaller")
        gap, spread = a[0] - b[0], max(a[2] - a[0], a[0] - a[1], b[2] - b[0], b[0] - b[1])
        ok = gap > spread
        print(f"    (b) is {gap:.3f} ms shorter than (a); largest distance of a block from its median {spread:.3f} ms: "
              f"{'shorter by more than the spread' if ok else 'NOT shorter by more than the spread'}", flush=True)
        if name == "photograph-like":
            failed += not ok
        try:
            from PIL import Image

            host = uint8_path()
            t0 = time.perf_counter()
            buf = io.BytesIO()
            Image.fromarray(host).save(buf, "JPEG", quality=q, subsampling=0)
            print(f"  (3) Pillow on the CPU, same samples, 4:4:4, quality {q}: {(time.perf_counter() - t0) * 1e3:.0f} ms, "
                  f"{buf.tell() / 1e6:.3f} MB (one run; information)", flush=True)
            back = np.asarray(Image.open(io.BytesIO(data.tobytes())))
            print(f"      Pillow opens the file of (b): {back.shape}, mean |decoded - samples| = "
                  f"{np.abs(back.astype(np.int16) - host).mean():.3f} levels")
        except ImportError:
            print("  (3) Pillow is not installed: no CPU figure")
        del img, u8
        torch.cuda.empty_cache()
    if failed:
        sys.exit("jpeg_time.py: encode_jpeg is not shorter than the uint8 path on the photograph-like image beyond the "
                 "blocks' spread; the stage times under (1) say where the time went")


if __name__ == "__main__":
    main()
