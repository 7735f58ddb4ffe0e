"""Time and size of the DNG output on one MI355X against the 16-bit route it replaces (method of tools/png_time.py).

    python tools/dng_time.py [--shape 6000x8000] [--blocks 7] [--calls 3] [--tiles 128,256,512] [--skip a,d]
                             [--out profiles/dng_encode.txt]

Everything printed also goes to --out (the record profiles/dng_encode.txt; the two bench.py lines are added to it by hand).

The photograph-like image of tools/jpeg_time.py (photo_like, seed 7), made on the device, as uint16 RGB:
(a) device float32 image -> file bytes on the host, wall clock around synchronised calls, legs alternating in one process:
    the parent commit's nearest route — encode_image(uint16), the pageable .cpu() copy, utils_dng.save_as_tiff into a
    memory file — against utils_dng.encode_dng at the default tile; both file sizes against the uncompressed samples;
(b) the stages of encode_dng: HIP events around blocks of `calls` calls of hhsr_ljpeg_histogram and of hhsr_ljpeg_encode
    (size pass, offsets scan, write pass), and the wall clock of the two synchronisations (counts -> host tables; the
    record and the file's bytes -> host);
(c) the tile sweep: time of hhsr_ljpeg_histogram + hhsr_ljpeg_encode and size of the streams per square tile; the default
    is the fastest tile whose file is within 1 % of the smallest of them — chosen value and runner-up are printed;
(d) the size of the streams for predictors 1 .. 7 at the default tile (the default predictor stays 1).

The script ends itself after --timeout seconds and fails without a device."""
import argparse
import ctypes
import os
import signal
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (os.path.join(ROOT, "tests"), os.path.join(ROOT, "handheld-multi-frame-super-resolution_amd")):
    sys.path.insert(0, p)

from jpeg_time import photo_like  # noqa: E402  (the same image)
from output_time import fmt, gpu_blocks, stats, wall_blocks  # noqa: E402  (the same block statistics)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--shape", default="6000x8000")
    ap.add_argument("--blocks", type=int, default=7)
    ap.add_argument("--calls", type=int, default=3)
    ap.add_argument("--tiles", default="128,256,512")
    ap.add_argument("--skip", default="")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "dng_encode.txt"))
    ap.add_argument("--timeout", type=int, default=500)
    args = ap.parse_args()
    assert args.blocks >= 5
    signal.alarm(args.timeout)  # a hang ends here, not at somebody else's limit

    import numpy as np
    import torch

    from handheld_super_resolution import _lib, utils_dng, utils_image

    assert torch.cuda.is_available(), "dng_time.py measures on the GPU: no device, no number"
    record = open(args.out, "w")

    def print(*a, flush=False):  # noqa: A001  (the record holds what the terminal shows)
        line = " ".join(str(v) for v in a)
        sys.stdout.write(line + "\n")
        record.write(line + "\n")
        if flush:
            sys.stdout.flush()
            record.flush()
    dev = torch.device("cuda", 0)
    H, W = (int(v) for v in args.shape.split("x"))
    px = H * W
    raw_bytes = px * 3 * 2
    skip = set(args.skip.split(",")) - {""}
    tiles = [int(v) for v in args.tiles.split(",")]
    default_t = utils_dng.DNG_TILE
    s = _lib.stream(dev)
    img = photo_like(H, W, dev, 7)
    print(f"# DNG output: median of {args.blocks} blocks (min - max), legs alternating in one process; kernel blocks of "
          f"{args.calls} calls")
    print(f"# device: {torch.cuda.get_device_name(0)}; {H} x {W} x 3 ({px / 1e6:.0f} MP), photograph-like; uncompressed uint16 "
          f"samples {raw_bytes / 1e6:.1f} MB; default tile {default_t}, predictor {utils_dng.DNG_PREDICTOR}", flush=True)
    memdir = "/dev/shm" if os.path.isdir("/dev/shm") else None
    samples = utils_image.encode_image(img, "uint16")

    class Coder:
        """The buffers and calls of encode_dng for one tile size and predictor."""

        def __init__(self, tile, predictor=1):
            self.tile, self.predictor = tile, predictor
            self.n_tiles = (-(-H // tile)) * (-(-W // tile))
            scratch_bytes, _ = utils_dng.ljpeg_encode_workspace(H, W, 3, tile, tile)
            self.scratch = torch.empty((scratch_bytes + 7) // 8, dtype=torch.int64, device=dev)
            self.counts = torch.empty(3 * 17 + 1, dtype=torch.int64, device=dev)
            self.record = torch.empty(self.n_tiles + 2 + (self.n_tiles + 1) // 2, dtype=torch.int64, device=dev)
            self.cap = raw_bytes + 256 * self.n_tiles
            self.out = torch.empty(self.cap, dtype=torch.uint8, device=dev)
            self.args = (_lib.ptr(samples), H, W, 3, W * 3, 16, predictor, tile, tile)
            self.bits = self.values = None

        def histogram(self):
            _lib.call("hhsr_ljpeg_histogram", *self.args, _lib.ptr(self.counts),
                      ctypes.c_void_p(self.counts.data_ptr() + 8 * 51), _lib.ptr(self.scratch), self.scratch.numel() * 8, s)

        def tables(self):
            self.bits, self.values = utils_dng.ljpeg_huffman(self.counts.cpu().numpy().view(np.uint64)[:51].reshape(3, 17))

        def encode(self):
            p = self.record.data_ptr()
            n = self.n_tiles
            _lib.call("hhsr_ljpeg_encode", *self.args, self.bits.ctypes.data, self.values.ctypes.data, _lib.ptr(self.scratch),
                      self.scratch.numel() * 8, _lib.ptr(self.out), self.cap, ctypes.c_void_p(p),
                      ctypes.c_void_p(p + 8 * (n + 2)), ctypes.c_void_p(p + 8 * (n + 1)), s)

        def length(self):
            v = int(self.record[self.n_tiles + 1].item())
            assert 0 < v <= self.cap, v
            return v

    if "a" not in skip:
        def parent_path():
            host = utils_image.encode_image(img, "uint16").cpu().numpy()
            with tempfile.NamedTemporaryFile(dir=memdir, suffix=".tif") as f:
                utils_dng.save_as_tiff(host, f.name)
                return os.path.getsize(f.name)

        def parent_copy_only():
            return utils_image.encode_image(img, "uint16").cpu().numpy().nbytes

        def dng_path():
            return utils_dng.encode_dng(img).size

        a, c, b = wall_blocks([parent_path, parent_copy_only, dng_path], args.blocks, 1)
        na, nb = parent_path(), dng_path()
        print(f"  (a) parent: encode_image(uint16), pageable .cpu(), save_as_tiff: {fmt(a)} | {na / 1e6:.2f} MB")
        print(f"      parent without the file: encode_image(uint16), pageable .cpu() : {fmt(c)}")
        print(f"      encode_dng (tile {default_t}, predictor 1)                          : {fmt(b)} | {nb / 1e6:.2f} MB = "
              f"{100 * nb / raw_bytes:.1f} % of the uncompressed samples, {a[0] / b[0]:.1f} x shorter than the TIFF route, "
              f"{c[0] / b[0]:.1f} x than the copy alone", flush=True)

    k = Coder(default_t)
    k.histogram()
    k.tables()
    hist, enc = gpu_blocks([k.histogram, k.encode], args.blocks, args.calls)
    probe = torch.zeros(4, dtype=torch.int64, device=dev)  # the shader clock next to one more histogram + encode
    with torch.cuda.stream(torch.cuda.Stream()):
        _lib.call("hhsr_clock_probe", _lib.ptr(probe), int(0.6 * (hist[0] + enc[0]) * 1e5), _lib.stream())
    k.histogram()
    k.encode()
    torch.cuda.synchronize()
    c0, r0, c1, r1 = (int(v) for v in probe.cpu().tolist())
    mhz = (c1 - c0) / (r1 - r0) * 100.0 if r1 > r0 else float("nan")
    print(f"  (b) shader clock next to one histogram + encode: {mhz:.0f} MHz")
    print(f"      hhsr_ljpeg_histogram: {fmt(hist)} | {raw_bytes / hist[0] / 1e9:.2f} TB/s of samples read")
    print(f"      hhsr_ljpeg_encode (sizes, scan, write), tile {default_t}: {fmt(enc)} | {raw_bytes / enc[0] / 1e6:.1f} GB/s of "
          f"samples coded")
    t_counts, t_code, t_rec, t_bytes = [], [], [], []
    for _ in range(args.blocks):  # the two synchronisations of encode_dng, wall clock, the device idle before each
        k.histogram()
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        host_counts = k.counts.cpu().numpy()
        t1 = time.perf_counter()
        k.tables()
        t2 = time.perf_counter()
        k.encode()
        torch.cuda.synchronize()
        t3 = time.perf_counter()
        rec = k.record.cpu().numpy()
        t4 = time.perf_counter()
        length = int(rec[k.n_tiles + 1])
        data = np.empty(length, np.uint8)
        torch.from_numpy(data).copy_(k.out[:length])
        t5 = time.perf_counter()
        t_counts.append((t1 - t0) * 1e3), t_code.append((t2 - t1) * 1e3), t_rec.append((t4 - t3) * 1e3), t_bytes.append((t5 - t4) * 1e3)
        del host_counts, data
    print(f"      sync 1: counts -> host {fmt(stats(t_counts))}, the tables on the host (with a second copy of the counts) "
          f"{fmt(stats(t_code))}")
    print(f"      sync 2: offsets, byte counts, length -> host {fmt(stats(t_rec))}, {length / 1e6:.2f} MB of streams -> host "
          f"(pageable) {fmt(stats(t_bytes))}", flush=True)
    del k
    torch.cuda.empty_cache()

    rows = []
    for tile in tiles:
        k = Coder(tile)
        k.histogram()
        k.tables()

        def both(k=k):
            k.histogram()
            k.encode()

        (e,) = gpu_blocks([both], args.blocks, args.calls)
        rows.append((tile, e, k.length(), k.n_tiles))
        del k
        torch.cuda.empty_cache()
    smallest = min(r[2] for r in rows)
    ok = sorted((r for r in rows if r[2] <= 1.01 * smallest), key=lambda r: r[1][0])
    print("  (c) tile sweep (hhsr_ljpeg_histogram + hhsr_ljpeg_encode; the streams without the container)")
    for tile, e, size, n in rows:
        print(f"      {tile:4d} x {tile:<4d} ({n:5d} tiles): {fmt(e)} | {size / 1e6:.3f} MB, +{100 * (size / smallest - 1):.2f} % over "
              f"the smallest")
    print(f"      fastest within 1 % of the smallest: {ok[0][0]}; runner-up: {ok[1][0] if len(ok) > 1 else 'none'}", flush=True)

    if "d" not in skip:
        print(f"  (d) predictors at tile {default_t}: size of the streams")
        sizes = {}
        for predictor in range(1, 8):
            k = Coder(default_t, predictor)
            k.histogram()
            k.tables()
            k.encode()
            sizes[predictor] = k.length()
            del k
            torch.cuda.empty_cache()
        for predictor, size in sizes.items():
            print(f"      predictor {predictor}: {size / 1e6:.3f} MB = {100 * size / raw_bytes:.1f} % of the samples, "
                  f"{100 * (size / sizes[1] - 1):+.2f} % against predictor 1", flush=True)
    record.close()


if __name__ == "__main__":
    main()
