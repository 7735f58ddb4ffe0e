"""Time of the lossless-JPEG DNG front end on one MI355X, written to profiles/dng_read.txt.

    python tools/dng_read_time.py [--shape 3000x4000] [--frames 8,20] [--bits 10,14] [--blocks 7] [--out FILE]

Per precision and burst length, per frame, medians of `blocks` blocks that alternate the legs in one process (min - max):
(a) pageable upload of the compressed blob + hhsr_ljpeg_decode, host clock around work that ends in a synchronise;
(b) hhsr_ljpeg_decode alone on the resident blob, HIP events;
(c) pageable upload of the same frames as uint16 counts: what any host decoder still pays;
(d) hhsr_ljpeg_decode_host on one thread (one frame's streams per block);
(e) libjpeg-turbo through Pillow on an 8-bit lossless stream of the same sample count, tiling and predictor, one core (one
    frame's streams per block): the outside yardstick; it is 8-bit (the counts' high bits) and one component, which
    flatters the CPU.
The counts are synthetic.make_burst scaled to the precision — `--distinct` rendered frames repeated to the burst's length —
in 256 x 256 tiles coded as X = 128, Nf = 2, predictor 1 with one K.2 table per component (tests/ljpeg_ref.py).  The decoded
counts are compared with the input at the timed size first.  The shader clock is read by hhsr_clock_probe next to one
more (untimed) decode.  The last line applies the rule for the default decoder: "gpu" while (a) < (c) + (d) / 16.
The script ends itself after --timeout seconds."""
import argparse
import ctypes
import io
import os
import signal
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "handheld-multi-frame-super-resolution_amd"))
sys.path.insert(0, os.path.join(ROOT, "tests"))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--shape", default="3000x4000")
    ap.add_argument("--frames", default="8,20")
    ap.add_argument("--bits", default="10,14")
    ap.add_argument("--blocks", type=int, default=7)
    ap.add_argument("--distinct", type=int, default=2)
    ap.add_argument("--tile", type=int, default=256)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "dng_read.txt"))
    ap.add_argument("--timeout", type=int, default=1100)
    args = ap.parse_args()
    signal.alarm(args.timeout)  # a hang ends here, not at somebody else's limit

    import numpy as np
    import torch
    from PIL import Image

    import ljpeg_cases as cases
    import ljpeg_ref
    from handheld_super_resolution import _lib, synthetic as synth

    assert torch.cuda.is_available(), "dng_read_time.py measures on the GPU: no device, no number"
    dev = torch.device("cuda", 0)
    H, W = (int(v) for v in args.shape.split("x"))
    T = args.tile
    lines = []

    def say(s):
        print(s, flush=True)
        lines.append(s)

    def med(v):
        v = sorted(v)
        m = v[len(v) // 2] if len(v) % 2 else 0.5 * (v[len(v) // 2 - 1] + v[len(v) // 2])
        return m, v[0], v[-1]

    def fmt(v, unit="ms"):
        m, lo, hi = med(v)
        return f"{m:.3f} {unit} ({lo:.3f} - {hi:.3f})"

    say(f"# DNG lossless-JPEG front end, {H} x {W}, {T} x {T} tiles as X = {T // 2}, Nf = 2, predictor 1; device: "
        f"{torch.cuda.get_device_name(0)}; medians of {args.blocks} alternating blocks (min - max), per frame")
    ref, comp, _ = synth.make_burst(H, W, args.distinct, seed=7, max_shift=2.0)
    rendered = np.concatenate([ref[None], comp])
    verdicts = []
    for bits in (int(b) for b in args.bits.split(",")):
        white = (1 << bits) - 1
        distinct = np.clip(np.rint(rendered * white), 0, white).astype(np.int64)
        t0 = time.perf_counter()
        per_frame = [cases.segment_streams(distinct[i:i + 1], bits, "tiles", (T, T), Nf=2, predictor=1, tables="k2")
                     for i in range(args.distinct)]
        # (e)'s streams: the same tiles, 8 bits, one component
        eight = [[ljpeg_ref.encode((np.pad(distinct[i, y0:y0 + T, x0:x0 + T], ((0, T - min(T, H - y0)), (0, T - min(T, W - x0))),
                                           mode="edge") >> (bits - 8))[:, :, None], 8, 1)
                  for y0 in range(0, H, T) for x0 in range(0, W, T)] for i in range(1)]
        say(f"# {bits}-bit counts: {args.distinct} rendered frames encoded on the host in {time.perf_counter() - t0:.1f} s")
        for n in (int(v) for v in args.frames.split(",")):
            items = [(st, f, x0, y0, w, h) for f in range(n) for (st, _, x0, y0, w, h) in per_frame[f % args.distinct]]
            plan = cases.plan_from_streams(items, n, H, W)
            counts = np.ascontiguousarray(np.stack([distinct[f % args.distinct] for f in range(n)]).astype(np.uint16))
            nseg, ntab = len(plan.segments), len(plan.tables)
            segs_d = torch.as_tensor(np.frombuffer(plan.segments, np.uint8).copy()).to(dev)
            tabs_d = torch.as_tensor(np.frombuffer(plan.tables, np.uint8).copy()).to(dev)
            work = torch.zeros(max(1, plan.workspace_elems), dtype=torch.uint16, device=dev)
            out = torch.zeros((n, H, W), dtype=torch.uint16, device=dev)
            status = torch.zeros(nseg, dtype=torch.int32, device=dev)
            blob_h = torch.as_tensor(plan.blob)  # pageable
            counts_h = torch.as_tensor(counts)   # pageable

            def decode(blob_d):
                _lib.call("hhsr_ljpeg_decode", _lib.ptr(blob_d), blob_d.numel(), _lib.ptr(segs_d), nseg, _lib.ptr(tabs_d), ntab,
                          _lib.ptr(work), work.numel() * 2, _lib.ptr(out), n, H, W, W, H * W, _lib.ptr(status), _lib.stream())

            blob_d = blob_h.to(dev)
            decode(blob_d)
            torch.cuda.synchronize()
            same = bool((out.cpu().numpy() == counts).all()) and not bool(status.any())
            # one frame's streams for the host legs
            one = cases.plan_from_streams(per_frame[0], 1, H, W)
            h_out, h_work = np.zeros((1, H, W), np.uint16), np.zeros(max(1, one.workspace_elems), np.uint16)
            h_st = np.zeros(len(one.segments), np.int32)

            def host_decode():
                _lib.call("hhsr_ljpeg_decode_host", one.blob.ctypes.data, one.blob.size, ctypes.addressof(one.segments),
                          len(one.segments), ctypes.addressof(one.tables), len(one.tables), h_work.ctypes.data,
                          h_work.size * 2, h_out.ctypes.data, 1, H, W, W, H * W, h_st.ctypes.data)

            host_decode()
            same_host = bool((h_out[0] == counts[0]).all()) and not h_st.any()
            ta, tb, tc, td, te = [], [], [], [], []
            for _ in range(args.blocks + 1):  # (the first block is the warm-up)
                torch.cuda.synchronize()
                t = time.perf_counter()
                bd = blob_h.to(dev)
                decode(bd)
                torch.cuda.synchronize()
                ta.append((time.perf_counter() - t) * 1e3 / n)
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record()
                decode(blob_d)
                e1.record()
                torch.cuda.synchronize()
                tb.append(e0.elapsed_time(e1) / n)
                t = time.perf_counter()
                cd = counts_h.to(dev)
                torch.cuda.synchronize()
                tc.append((time.perf_counter() - t) * 1e3 / n)
                del cd, bd
                t = time.perf_counter()
                host_decode()
                td.append((time.perf_counter() - t) * 1e3)
                t = time.perf_counter()
                for st in eight[0]:
                    Image.open(io.BytesIO(st)).load()
                te.append((time.perf_counter() - t) * 1e3)
            ta, tb, tc, td, te = (v[1:] for v in (ta, tb, tc, td, te))
            # the shader clock next to one more decode
            probe = torch.zeros(4, dtype=torch.int64, device=dev)
            side = torch.cuda.Stream()
            with torch.cuda.stream(side):
                _lib.call("hhsr_clock_probe", _lib.ptr(probe), int(0.6 * med(tb)[0] * n * 1e5), _lib.stream())
            decode(blob_d)
            torch.cuda.synchronize()
            c0, r0, c1, r1 = (int(v) for v in probe.cpu().tolist())
            mhz = (c1 - c0) / (r1 - r0) * 100.0 if r1 > r0 else float("nan")
            comp_b, raw_b = plan.blob.size / n, 2.0 * H * W
            say(f"{bits}-bit, {n} frames: {nseg} streams, {ntab} tables, {comp_b / 1e6:.2f} MB compressed per frame = "
                f"{100 * comp_b / raw_b:.1f} % of {raw_b / 1e6:.1f} MB (2 bytes per sample); GPU == counts: {same}, host == "
                f"counts: {same_host}; shader clock {mhz:.0f} MHz")
            say(f"  (a) upload blob + hhsr_ljpeg_decode : {fmt(ta)}")
            say(f"  (b) hhsr_ljpeg_decode alone         : {fmt(tb)}  [one lane per stream, {max(1, -(-nseg // 2048))} per wave]")
            say(f"  (c) upload uint16 counts            : {fmt(tc)}")
            say(f"  (d) hhsr_ljpeg_decode_host, 1 thread: {fmt(td)}")
            say(f"  (e) Pillow / libjpeg-turbo, 8-bit   : {fmt(te)}")
            a, c, d = med(ta)[0], med(tc)[0], med(td)[0]
            verdicts.append(a < c + d / 16)
            say(f"  rule: (a) {a:.3f} ms {'<' if a < c + d / 16 else '>='} (c) + (d) / 16 = {c + d / 16:.3f} ms")
            del out, work, blob_d
    say(f"# default decoder by the rule, all cases: {'gpu' if all(verdicts) else 'host'}")
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as f:
        f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
