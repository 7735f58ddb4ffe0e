"""Time of the packed-raw front end on one MI355X, written to profiles/packed_raw.txt.

    python tools/packed_raw_time.py [--shape 3000x4000] [--frames 20] [--blocks 5] [--calls 10] [--steps 10] [--out FILE]

(a) hhsr_normalize_raw_packed per layout next to hhsr_normalize_raw_u16 on the same counts, in the same run: HIP events
    around blocks of `calls` back-to-back calls of `frames` frames each (one frame's 72 MB would stay in the 256 MB
    Infinity Cache from call to call; 20 frames do not), median block / calls / frames (min - max).  Bytes are counted
    from the shapes: B/8 or 2 bytes in + 4 out per pixel.  Every packed result is compared with the uint16 result at the
    timed size first (bit equality); the frames are one packed frame repeated.
(b) the host-resident burst (scale 2, `frames` frames, distributed.HipEngine -> graph.HostBurstRunner like bench.py's
    legs) with pinned mipi10 frames against pinned uint16 counts of the same image: blocks of `steps` bursts, the two
    legs alternating block by block in one process, median of `blocks` blocks each (min - max).
The script ends itself after --timeout seconds."""
import argparse
import os
import signal
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "handheld-multi-frame-super-resolution_amd"))

HBM_MEASURED = 6.29e12  # B/s, float4 copy


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--shape", default="3000x4000")
    ap.add_argument("--frames", type=int, default=20)
    ap.add_argument("--blocks", type=int, default=5)
    ap.add_argument("--calls", type=int, default=10)
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--skip-burst", action="store_true")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "packed_raw.txt"))
    ap.add_argument("--timeout", type=int, default=540)
    args = ap.parse_args()
    signal.alarm(args.timeout)  # a hang ends here, not at somebody else's limit

    import numpy as np
    import torch

    import handheld_super_resolution as hsr
    from handheld_super_resolution import _lib, utils_dng, synthetic as synth, distributed as hdist

    assert torch.cuda.is_available(), "packed_raw_time.py measures on the GPU: no device, no number"
    dev = torch.device("cuda", 0)
    H, W = (int(v) for v in args.shape.split("x"))
    NF = args.frames
    lines = []

    def say(s):
        print(s, flush=True)
        lines.append(s)

    def median(v):
        v = sorted(v)
        return v[len(v) // 2] if len(v) % 2 else 0.5 * (v[len(v) // 2 - 1] + v[len(v) // 2])

    def gpu_ms(fn):
        for _ in range(3):
            fn()
        torch.cuda.synchronize()
        ms = []
        for _ in range(args.blocks):
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            for _ in range(args.calls):
                fn()
            b.record()
            b.synchronize()
            ms.append(a.elapsed_time(b) / args.calls / NF)
        return median(ms), min(ms), max(ms)

    say(f"# packed raw front end, {H} x {W} ({H * W / 1e6:.0f} MP), device: {torch.cuda.get_device_name(0)}")
    say(f"# (a) kernels: {NF} frames per call, median of {args.blocks} blocks of {args.calls} calls (min - max), per frame")
    cfa, bl, wb = [[0, 1], [1, 2]], [64.0, 64.0, 64.0], [1.9, 1.0, 1.6]
    out = torch.empty((NF, H, W), dtype=torch.float32, device=dev)
    s = _lib.stream(dev)
    rng = np.random.default_rng(5)
    for bits in (10, 12, 14):
        wl = float((1 << bits) - 1)
        counts = rng.integers(0, 1 << bits, (H, W), dtype=np.uint16)
        c16 = torch.from_numpy(counts).to(dev)[None].expand(NF, H, W).contiguous()
        args16 = (_lib.ptr(c16), NF, H, W, W, _lib.cfa_bytes(cfa), _lib.doubles(bl), wl, _lib.doubles(wb), _lib.ptr(out), s)
        _lib.call("hhsr_normalize_raw_u16", *args16)
        want = out[0].clone()
        med, lo, hi = gpu_ms(lambda: _lib.call("hhsr_normalize_raw_u16", *args16))
        byt = 6.0 * H * W
        say(f"{bits}-bit counts | hhsr_normalize_raw_u16 (k_normalize_u16): {1e3 * med:.1f} us ({1e3 * lo:.1f} - {1e3 * hi:.1f}) | "
            f"{byt / 1e6:.0f} MB -> {byt / med / 1e9:.2f} TB/s = {100 * byt / (med * 1e-3) / HBM_MEASURED:.0f} % of the 6.29 TB/s copy rate")
        for name in (f"mipi{bits}", f"be{bits}"):
            rb = utils_dng.packed_row_bytes(W, name)
            one = np.concatenate([utils_dng.pack_raw(counts[a:a + 250], name) for a in range(0, H, 250)])  # (slabs: memory)
            pk = torch.from_numpy(one).to(dev)[None].expand(NF, H, rb).contiguous()
            argsp = (_lib.ptr(pk), NF, H, W, rb, H * rb, utils_dng.PACKINGS[name], _lib.cfa_bytes(cfa), _lib.doubles(bl), wl,
                     _lib.doubles(wb), _lib.ptr(out), s)
            out.zero_()
            _lib.call("hhsr_normalize_raw_packed", *argsp)
            same = bool(torch.equal(out[0], want) and torch.equal(out[NF - 1], want))
            med, lo, hi = gpu_ms(lambda: _lib.call("hhsr_normalize_raw_packed", *argsp))
            byt = (rb / W + 4.0) * H * W
            say(f"  {name:7s} hhsr_normalize_raw_packed: {1e3 * med:.1f} us ({1e3 * lo:.1f} - {1e3 * hi:.1f}) | {byt / 1e6:.0f} MB -> "
                f"{byt / med / 1e9:.2f} TB/s = {100 * byt / (med * 1e-3) / HBM_MEASURED:.0f} % | == uint16 result: {same}")
            del pk
        del c16
    del out
    torch.cuda.empty_cache()

    if not args.skip_burst:
        black, white = 64.0, 1023.0
        ref, comp, _ = synth.make_burst_torch(H, W, NF, dev, seed=1234)
        to_counts = lambda t: np.clip(np.rint(t.cpu().numpy() * (white - black) + black), 0, white).astype(np.uint16)  # noqa: E731
        frames16 = [to_counts(ref)] + [to_counts(comp[i]) for i in range(NF - 1)]
        mean = float(ref.mean())
        del ref, comp
        torch.cuda.empty_cache()
        pin = lambda a: torch.from_numpy(a).pin_memory()  # noqa: E731
        legs = {"uint16": [pin(f) for f in frames16],
                "mipi10": [pin(np.concatenate([utils_dng.pack_raw(f[a:a + 250], "mipi10") for a in range(0, H, 250)]))
                           for f in frames16]}

        def config(**keys):
            cfg = hsr.default_config()
            cfg.verbose = 0
            cfg.scale = 2
            cfg.hip = {"raw_norm": dict({"black_levels": [black] * 3, "white_level": white}, **keys)}
            hsr.prepare_config(cfg, np.full((H, W), mean, np.float32), synth.ALPHA_ISO100, synth.BETA_ISO100, [[0, 1], [1, 2]],
                               [1.0, 1.0, 1.0])
            return cfg

        cfgs = {"uint16": config(), "mipi10": config(packing="mipi10", width=W)}
        engines = {k: hdist.HipEngine(c) for k, c in cfgs.items()}
        run = lambda k: hdist.main_sharded(legs[k][0], legs[k][1:], cfgs[k], engine=engines[k])[0]  # noqa: E731
        outs = {}
        for k in legs:  # eager, capture, replays until the copy path is at speed (bench.py: host_leg)
            for _ in range(10):
                outs[k] = run(k)
            torch.cuda.synchronize()
            outs[k] = outs[k].clone()
        same = bool(torch.equal(outs["uint16"].view(torch.int32), outs["mipi10"].view(torch.int32)))
        graphs = {k: bool(not e._host.disabled and any(st != "seen" for st in e._host.states.values())) for k, e in engines.items()}
        blocks = {k: [] for k in legs}
        for _ in range(args.blocks):
            for k in legs:  # alternating
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                for _ in range(args.steps):
                    run(k)
                torch.cuda.synchronize()
                blocks[k].append((time.perf_counter() - t0) / args.steps * 1e3)
        say(f"# (b) host-resident burst, {NF} frames x2, pinned frames, HostBurstRunner graphs {graphs}: median of {args.blocks} "
            f"alternating blocks of {args.steps} bursts (min - max); results bit-identical: {same}")
        for k, v in blocks.items():
            mb = sum(f.numel() * f.element_size() for f in legs[k]) / 1e6
            say(f"  {k}: {median(v):.2f} ms per burst ({min(v):.2f} - {max(v):.2f}) | {mb:.0f} MB uploaded per burst")
    with open(args.out, "w") as f:
        f.write("\n".join(lines) + "\n")
    print("written", args.out)


if __name__ == "__main__":
    main()
