"""Time of the reference selection on one MI355X, written to profiles/ref_select.txt.

    python tools/ref_select_time.py [--shape 3000x4000] [--frames 20] [--blocks 7] [--calls 20] [--steps 3] [--out FILE]

(a) hhsr_frame_sharpness per frame for float32, uint16, mipi10 and be12 frames of the same counts: HIP events around
    blocks of `calls` back-to-back calls of 3 frames (the default number of candidates) and of HHSR_MAX_BATCH frames, the
    formats alternating block by block in one process, median block / calls / frames (min - max).  The calls walk through
    a pool of frame copies of at least 512 MB per format, so that no frame is still in the 256 MB Infinity Cache when
    its turn comes again.  Bytes are counted from the shapes: the frames' rows, read once.  Every format's score is
    compared with the uint16 score at the timed size first (bit equality).
(b) the torch statement of the same score on normalised float32 device frames (what a caller would write today), per
    frame, in the same process and the same alternation.  The normalisation that produces those frames is NOT timed.
(c) process() on a host-resident burst of uint16 counts (pageable NumPy arrays, noise curves given, scale 2) with
    config.reference.select first and sharpest: blocks of `steps` calls, alternating, median of `blocks` blocks each.
The script ends itself after --timeout seconds."""
import argparse
import os
import signal
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "handheld-multi-frame-super-resolution_amd"))

HBM_MEASURED = 6.29e12  # B/s, float4 copy (profiles/output_encode.txt)
POOL_BYTES = 512e6


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--shape", default="3000x4000")
    ap.add_argument("--frames", type=int, default=20)
    ap.add_argument("--blocks", type=int, default=7)
    ap.add_argument("--calls", type=int, default=20)
    ap.add_argument("--steps", type=int, default=3)
    ap.add_argument("--skip-burst", action="store_true")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "ref_select.txt"))
    ap.add_argument("--timeout", type=int, default=540)
    args = ap.parse_args()
    signal.alarm(args.timeout)  # a hang ends here, not at somebody else's limit

    import numpy as np
    import torch

    import handheld_super_resolution as hsr
    from handheld_super_resolution import _lib, utils_dng, utils_image, synthetic as synth

    assert torch.cuda.is_available(), "ref_select_time.py measures on the GPU: no device, no number"
    dev = torch.device("cuda", 0)
    H, W = (int(v) for v in args.shape.split("x"))
    NF = args.frames
    cfa = [[0, 1], [1, 2]]
    lines = []

    def say(s):
        print(s, flush=True)
        lines.append(s)

    def median(v):
        v = sorted(v)
        return v[len(v) // 2] if len(v) % 2 else 0.5 * (v[len(v) // 2 - 1] + v[len(v) // 2])

    say(f"# reference selection, {H} x {W} ({H * W / 1e6:.0f} MP), device: {torch.cuda.get_device_name(0)}")
    rng = np.random.default_rng(5)
    counts = rng.integers(0, 1024, (H, W), dtype=np.uint16)
    slabs = lambda name: np.concatenate([utils_dng.pack_raw(counts[a:a + 250], name) for a in range(0, H, 250)])  # noqa: E731
    forms = {"float32": (torch.from_numpy(counts.astype(np.float32)), 0, None),
             "uint16": (torch.from_numpy(counts), -1, None),
             "mipi10": (torch.from_numpy(slabs("mipi10")), 1, "mipi10"),
             "be12": (torch.from_numpy(slabs("be12")), 5, "be12")}
    stream = _lib.stream(dev)
    cfa_b = _lib.cfa_bytes(cfa)
    work = torch.empty(utils_image.sharpness_workspace_bytes(H, W, _lib.MAX_BATCH) // 8, dtype=torch.float64, device=dev)
    out = torch.empty(_lib.MAX_BATCH, dtype=torch.float64, device=dev)
    want = utils_image.frame_sharpness([forms["uint16"][0].to(dev)], cfa).cpu().numpy()

    legs = {}  # name -> (callable making one call, frames per call, bytes per frame)
    pools = {}
    for name, (host, fmt, packing) in forms.items():
        one = host.to(dev)
        frame_bytes = one.numel() * one.element_size()
        got = utils_image.frame_sharpness([one], cfa, packing=packing, width=W).cpu().numpy()
        same = bool(got.view(np.uint64)[0] == want.view(np.uint64)[0])
        n_pool = -(-int(POOL_BYTES // frame_bytes + 1) // _lib.MAX_BATCH) * _lib.MAX_BATCH
        pools[name] = [one.clone() for _ in range(n_pool)]
        say(f"# {name}: {frame_bytes / 1e6:.1f} MB per frame, pool of {n_pool} copies, score == uint16 score: {same}")
        row_bytes = one.stride(0) * one.element_size()
        for per_call in (3, _lib.MAX_BATCH):
            tables = [_lib.ptr_array(pools[name][i:i + per_call]) for i in range(0, n_pool - per_call + 1, per_call)]
            state = {"i": 0}

            def call(tables=tables, state=state, per_call=per_call, row_bytes=row_bytes, fmt=fmt):
                _lib.call("hhsr_frame_sharpness", tables[state["i"] % len(tables)], per_call, H, W, row_bytes, fmt, cfa_b,
                          _lib.ptr(work), work.numel() * 8, _lib.ptr(out), stream)
                state["i"] += 1

            legs[f"{name} x{per_call}"] = (call, per_call, frame_bytes)
    # (b) the torch statement on normalised float32 frames
    norm = [(p.to(torch.float32) - 64.0) / (1023.0 - 64.0) for p in pools["uint16"][:len(pools["float32"])]]
    tstate = {"i": 0}

    def torch_score(f):
        g = (f[0::2, 1::2] + f[1::2, 0::2]) * 0.5
        dx, dy = g[:, 1:] - g[:, :-1], g[1:] - g[:-1]
        return (dx * dx).sum(dtype=torch.float64) + (dy * dy).sum(dtype=torch.float64)

    def torch_call():
        for k in range(3):
            torch_score(norm[(tstate["i"] + k) % len(norm)])
        tstate["i"] += 3

    legs["torch statement x3"] = (torch_call, 3, 4.0 * H * W)
    t_got = float(torch_score(pools["float32"][0]).cpu())
    say(f"# torch statement on the float32 counts: {t_got!r}, kernel {float(want[0])!r} (relative difference "
        f"{abs(t_got - want[0]) / want[0]:.1e}: another summation order)")

    for fn, _, _ in legs.values():  # warm-up of every leg
        for _ in range(3):
            fn()
    torch.cuda.synchronize()
    times = {k: [] for k in legs}
    for _ in range(args.blocks):
        for k, (fn, per_call, _) in legs.items():  # alternating
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            for _ in range(args.calls):
                fn()
            b.record()
            b.synchronize()
            times[k].append(a.elapsed_time(b) / args.calls / per_call)
    say(f"# (a), (b): median of {args.blocks} alternating blocks of {args.calls} calls (min - max), per frame; the rate counts "
        f"the frame's bytes once")
    for k, v in times.items():
        byt = legs[k][2]
        med = median(v)
        say(f"  {k:20s} {1e3 * med:7.1f} us ({1e3 * min(v):.1f} - {1e3 * max(v):.1f}) | {byt / 1e6:.0f} MB -> "
            f"{byt / med / 1e9:.2f} TB/s = {100 * byt / (med * 1e-3) / HBM_MEASURED:.0f} % of the 6.29 TB/s copy rate")
    say("# a call's time as fixed part + frames x per-frame part, from the two call sizes (the per-frame part is what the "
        "kernel's loads sustain; the fixed part is two dependent launches plus the grid's ramp-up and tail):")
    for name in forms:
        t3, t8 = 3 * median(times[f"{name} x3"]), _lib.MAX_BATCH * median(times[f"{name} x{_lib.MAX_BATCH}"])
        per = (t8 - t3) / (_lib.MAX_BATCH - 3)
        byt = legs[f"{name} x3"][2]
        say(f"  {name:8s} {1e3 * (t3 - 3 * per):5.1f} us per call + {1e3 * per:.2f} us per frame ({byt / per / 1e9:.2f} TB/s = "
            f"{100 * byt / (per * 1e-3) / HBM_MEASURED:.0f} % of the copy rate)")
    del pools, norm, legs
    torch.cuda.empty_cache()

    if not args.skip_burst:
        black, white = 64.0, 1023.0
        ref, comp, _ = synth.make_burst_torch(H, W, NF, dev, seed=1234)
        to_counts = lambda t: np.clip(np.rint(t.cpu().numpy() * (white - black) + black), 0, white).astype(np.uint16)  # noqa: E731
        frames16 = [to_counts(ref)] + [to_counts(comp[i]) for i in range(NF - 1)]
        del ref, comp
        torch.cuda.empty_cache()
        std, diff = synth.noise_curves(synth.ALPHA_ISO100, synth.BETA_ISO100)
        burst = dict(ref=frames16[0], comp=np.stack(frames16[1:]), cfa_pattern=cfa, white_balance=[1.0, 1.0, 1.0],
                     black_levels=[black] * 3, white_level=white, alpha=synth.ALPHA_ISO100, beta=synth.BETA_ISO100,
                     std_curve=std, diff_curve=diff)

        def run(select):
            cfg = hsr.default_config()
            cfg.verbose = 0
            cfg.scale = 2
            cfg.reference = {"select": select, "candidates": 3}
            return hsr.process(burst, cfg)

        picked = run("sharpest")[1]["reference index"]
        run("first")
        blocks = {"first": [], "sharpest": []}
        for _ in range(args.blocks):
            for k in blocks:  # alternating
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                for _ in range(args.steps):
                    run(k)
                torch.cuda.synchronize()
                blocks[k].append((time.perf_counter() - t0) / args.steps * 1e3)
        say(f"# (c) process(), host-resident burst of {NF} uint16 frames (pageable), x2, float32 result copied back: median of "
            f"{args.blocks} alternating blocks of {args.steps} calls (min - max); sharpest picked frame {picked}")
        for k, v in blocks.items():
            say(f"  select {k:9s} {median(v):8.1f} ms per call ({min(v):.1f} - {max(v):.1f})")
        say(f"  difference of the medians: {median(blocks['sharpest']) - median(blocks['first']):+.1f} ms "
            f"(3 candidates = {3 * 2 * H * W / 1e6:.0f} MB uploaded a second time, one kernel call, one synchronisation)")
    with open(args.out, "w") as f:
        f.write("\n".join(lines) + "\n")
    print("written", args.out)


if __name__ == "__main__":
    main()
