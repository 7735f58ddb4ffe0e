"""Time of hhsr_linearize_raw_u16 on one MI355X next to hhsr_normalize_raw_u16, written to profiles/dng_linearize.txt.

    python tools/dng_linearize_time.py [--shape 3000x4000] [--pool 24] [--blocks 9] [--frames-per-block 96] [--out FILE]

Per frame of uint16 counts, in calls of 1 and of 8 frames: the sibling kernel, then the new entry with nothing to apply, with
a LinearizationTable of 1024, 16384 and 65536 entries, with both black deltas, with four 13 x 17 gain maps, and with
everything on (table 16384 + deltas + maps).  All variants run on the same frames in one process: HIP events around blocks
of back-to-back calls that add up to `frames-per-block` frames, the variants alternating block by block, median of `blocks`
blocks (min - max).  The calls walk a pool of `pool` distinct frames and outputs (1.7 GB at 12 MP: nothing of a call is
still in the 256 MB Infinity Cache when its frame comes round again).  Two kinds of counts: "scene" — a smooth picture with
1 % noise, whose neighbouring counts are close, as a sensor's are — and "random" — uniform over the table, the worst case of
the table lookup.  The script ends itself after --timeout seconds."""
import argparse
import ctypes
import os
import signal
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "handheld-multi-frame-super-resolution_amd"))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--shape", default="3000x4000")
    ap.add_argument("--pool", type=int, default=24)
    ap.add_argument("--blocks", type=int, default=9)
    ap.add_argument("--frames-per-block", type=int, default=96)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "dng_linearize.txt"))
    ap.add_argument("--timeout", type=int, default=300)
    args = ap.parse_args()
    signal.alarm(args.timeout)  # a hang ends here, not at somebody else's limit

    import numpy as np
    import torch

    from handheld_super_resolution import _lib

    assert torch.cuda.is_available(), "dng_linearize_time.py measures on the GPU: no device, no number"
    dev = torch.device("cuda", 0)
    H, W = (int(v) for v in args.shape.split("x"))
    P = args.pool - args.pool % 8
    assert P >= 8
    lines = []

    def say(s):
        print(s, flush=True)
        lines.append(s)

    def median(v):
        v = sorted(v)
        return v[len(v) // 2] if len(v) % 2 else 0.5 * (v[len(v) // 2 - 1] + v[len(v) // 2])

    g = torch.Generator(device=dev).manual_seed(50712)
    yy = torch.linspace(0, 1, H, device=dev)[:, None]
    xx = torch.linspace(0, 1, W, device=dev)[None, :]
    scene = 0.45 + 0.25 * torch.sin(9 * xx + 4 * yy) * torch.cos(7 * yy - 2 * xx) + 0.15 * xx * yy

    def pool(kind, top):
        frames = torch.empty((P, H, W), dtype=torch.int16, device=dev)  # (uint16 bits)
        for i in range(P):
            if kind == "scene":
                v = (scene + 0.01 * torch.randn((H, W), device=dev, generator=g)).clamp_(0, 1) * (top - 1)
            else:
                v = torch.rand((H, W), device=dev, generator=g) * (top - 1)
            frames[i] = v.to(torch.int32).to(torch.uint16).view(torch.int16)
        return frames

    out = torch.empty((P, H, W), dtype=torch.float32, device=dev)
    s = _lib.stream(dev)
    cfa, bl, wb = _lib.cfa_bytes([[0, 1], [1, 2]]), _lib.doubles([64.0, 65.0, 63.0]), _lib.doubles([1.9, 1.0, 1.6])
    rng = np.random.default_rng(1)
    tables = {n: torch.from_numpy(np.sort(rng.integers(0, 1 << 16, n)).astype(np.uint16).view(np.int16)).to(dev)
              for n in (1024, 16384, 65536)}
    dh = torch.from_numpy(rng.standard_normal(W).astype(np.float32)).to(dev)
    dv = torch.from_numpy(rng.standard_normal(H).astype(np.float32)).to(dev)
    yv, xv = np.meshgrid(np.linspace(-1, 1, 13), np.linspace(-1, 1, 17), indexing="ij")
    gains = torch.from_numpy(np.stack([1 + (0.3 + 0.05 * k) * (yv * yv + xv * xv) for k in range(4)]).astype(np.float32)).to(dev)
    descs = (_lib.GainMapDesc * 4)(*[_lib.GainMapDesc(k // 2, k % 2, 2, 2, 13, 17, 1 / 12, 1 / 16, 0.0, 0.0, k * 13 * 17)
                                      for k in range(4)])

    def linearize(frames, white, table=None, deltas=False, maps=False):
        def fn(first, n):
            _lib.call("hhsr_linearize_raw_u16", ctypes.c_void_p(frames.data_ptr() + first * H * W * 2), n, H, W, W, cfa, bl, white,
                      wb, _lib.ptr(table), 0 if table is None else table.numel(), _lib.ptr(dh if deltas else None),
                      _lib.ptr(dv if deltas else None), ctypes.addressof(descs) if maps else None, 4 if maps else 0,
                      _lib.ptr(gains if maps else None), gains.numel() if maps else 0,
                      ctypes.c_void_p(out.data_ptr() + first * H * W * 4), s)
        return fn

    def normalize(frames, white):
        def fn(first, n):
            _lib.call("hhsr_normalize_raw_u16", ctypes.c_void_p(frames.data_ptr() + first * H * W * 2), n, H, W, W, cfa, bl, white,
                      wb, ctypes.c_void_p(out.data_ptr() + first * H * W * 4), s)
        return fn

    def measure(variants, per_call):
        """{name: (median, min, max) us per frame}: blocks of frames-per-block frames, the variants alternating."""
        calls = max(1, args.frames_per_block // per_call)
        at = {k: 0 for k in variants}

        def block(k):
            for _ in range(calls):
                variants[k](at[k], per_call)
                at[k] = (at[k] + per_call) % P
        for k in variants:
            block(k)
        torch.cuda.synchronize()
        us = {k: [] for k in variants}
        for _ in range(args.blocks):
            for k in variants:
                a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                a.record()
                block(k)
                b.record()
                b.synchronize()
                us[k].append(a.elapsed_time(b) * 1e3 / (calls * per_call))
        return {k: (median(v), min(v), max(v)) for k, v in us.items()}

    say(f"# DNG linearization, {H} x {W} ({H * W / 1e6:.0f} MP) uint16 frames, device: {torch.cuda.get_device_name(0)}")
    say(f"# us per frame: median of {args.blocks} alternating blocks of {args.frames_per_block} frames (min - max), a pool of {P} "
        f"frames; 6 B per pixel = {6 * H * W / 1e6:.0f} MB per frame")
    for kind, top in ((k, t) for t in (1024, 16384, 65536) for k in ("scene", "random")):  # (counts over the whole table)
        frames, white = pool(kind, top), float(top - 1)
        variants = {"hhsr_normalize_raw_u16": normalize(frames, white), "nothing to apply": linearize(frames, white),
                    f"table {top}": linearize(frames, white, tables[top])}
        if top == 16384:
            variants.update({"deltas h + v": linearize(frames, white, deltas=True),
                             "four 13 x 17 maps": linearize(frames, white, maps=True),
                             "everything (table 16384, deltas, maps)": linearize(frames, white, tables[16384], True, True)})
        # the link between the two contracts, at the timed size
        variants["hhsr_normalize_raw_u16"](0, 8)
        want = out[:8].clone()
        out[:8].zero_()
        variants["nothing to apply"](0, 8)
        same = bool(torch.equal(out[:8].view(torch.int32), want.view(torch.int32)))
        say(f"{kind} counts below {top}; nothing to apply == hhsr_normalize_raw_u16, bit for bit: {same}")
        for per_call in (1, 8):
            res = measure(variants, per_call)
            base = res["hhsr_normalize_raw_u16"][0]
            for k, (med, lo, hi) in res.items():
                say(f"  {per_call} frame{'s' if per_call > 1 else ' '} per call | {k:40s}: {med:6.1f} us ({lo:.1f} - {hi:.1f}) | "
                    f"{med / base:.2f} x the sibling | {6 * H * W / med / 1e6:.2f} TB/s")
        del frames
    with open(args.out, "w") as f:
        f.write("\n".join(lines) + "\n")
    print("written", args.out)


if __name__ == "__main__":
    main()
