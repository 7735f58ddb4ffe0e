"""Time of the noise-profile estimator on one MI355X, written to profiles/noise_profile.txt.

    python tools/noise_profile_time.py [--shape 3000x4000] [--frames 20] [--blocks 7] [--calls 20] [--steps 3] [--out FILE]

(a) hhsr_noise_profile_hist per frame on normalised float32 frames, in calls of 1 frame (what process() does by default) and
    of HHSR_MAX_BATCH frames, next to hhsr_frame_sharpness on the same frames in the same call sizes (both read a frame
    once): HIP events around blocks of `calls` back-to-back calls, the legs alternating block by block in one process,
    median block / calls / frames (min - max).  The calls walk through a pool of frame copies of at least 512 MB, so that
    no frame is still in the 256 MB Infinity Cache when its turn comes again.  Bytes are counted from the shape: the
    frame's rows, read once; the ratio to the time the box's measured copy rate gives for those bytes is reported, not
    asserted.  The kernel's histogram is compared with the torch statement's at the timed size first.
(b) the torch statement of the same tile statistics (what a caller would write today), per frame, in the same alternation.
(c) process() on a host-resident burst of uint16 counts (pageable NumPy arrays, noise curves given, scale 2) with the
    profile given and with noise_model.source = estimate: blocks of `steps` calls, alternating, median of `blocks` each.
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
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "noise_profile.txt"))
    ap.add_argument("--timeout", type=int, default=540)
    args = ap.parse_args()
    signal.alarm(args.timeout)  # a hang ends here, not at somebody else's limit

    import numpy as np
    import torch

    import handheld_super_resolution as hsr
    from handheld_super_resolution import _lib, noise_profile as npf, utils_image, synthetic as synth

    assert torch.cuda.is_available(), "noise_profile_time.py measures on the GPU: no device, no number"
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

    say(f"# noise profile, {H} x {W} ({H * W / 1e6:.0f} MP), device: {torch.cuda.get_device_name(0)}")
    # a smooth ramp with the ISO-100 profile's noise: the tiles spread over the mean bins like a photograph's
    g = torch.Generator(device=dev).manual_seed(5)
    scene = (0.05 + 0.9 * torch.linspace(0, 1, W, device=dev))[None, :].expand(H, W)
    one = (scene + torch.randn((H, W), device=dev, generator=g) * torch.sqrt(synth.ALPHA_ISO100 * scene + synth.BETA_ISO100))
    one = one.clamp_(0, 1).to(torch.float32).contiguous()
    frame_bytes = 4 * H * W
    n_pool = -(-int(POOL_BYTES // frame_bytes + 1) // _lib.MAX_BATCH) * _lib.MAX_BATCH
    pool = [one.clone() for _ in range(n_pool)]
    stream = _lib.stream(dev)
    cfa_b = _lib.cfa_bytes(cfa)
    gains = _lib.floats([1.0] * 4)
    hist = torch.empty(npf.HIST_SHAPE, dtype=torch.int32, device=dev)
    work = torch.empty(utils_image.sharpness_workspace_bytes(H, W, _lib.MAX_BATCH) // 8, dtype=torch.float64, device=dev)
    scores = torch.empty(_lib.MAX_BATCH, dtype=torch.float64, device=dev)

    def torch_hist(f):
        """The tile statistics in torch (float32 residuals, float64 sums in torch's own order) -> int64 [4 * 64 * 1024]."""
        nby, nbx = H // 16, W // 16
        out = torch.zeros(4 * 64 * 1024, dtype=torch.int64, device=dev)
        for p in range(4):
            t = f[p >> 1::2, p & 1::2][:8 * nby, :8 * nbx].reshape(nby, 8, nbx, 8).permute(0, 2, 1, 3)
            ok = ((t > 0) & (t < 1)).all(dim=3).all(dim=2)
            m = t.sum(dim=(2, 3), dtype=torch.float64) / 64.0
            r = t[:, :, 1:7, 1:7] - 0.25 * ((t[:, :, 1:7, 0:6] + t[:, :, 1:7, 2:8]) + (t[:, :, 0:6, 1:7] + t[:, :, 2:8, 1:7]))
            e = ((r * r).sum(dim=(2, 3), dtype=torch.float64) / 45.0).to(torch.float32)
            ok &= e != 0
            b = (m * 64.0).to(torch.int64).clamp_(max=63)
            k = ((e.view(torch.int32).to(torch.int64) >> 18) - ((127 - 32) << 5)).clamp_(0, 1023)
            out += torch.bincount(((p * 64 + b) * 1024 + k)[ok], minlength=4 * 64 * 1024)
        return out

    legs = {}  # name -> (callable making one call, frames per call)
    for per_call in (1, _lib.MAX_BATCH):
        tables = [_lib.ptr_array(pool[i:i + per_call]) for i in range(0, n_pool - per_call + 1, per_call)]

        def hist_call(tables=tables, state={"i": 0}, per_call=per_call):
            _lib.call("hhsr_noise_profile_hist", tables[state["i"] % len(tables)], per_call, H, W, 4 * W, cfa_b, gains,
                      _lib.ptr(hist), stream)
            state["i"] += 1

        def sharp_call(tables=tables, state={"i": 0}, per_call=per_call):
            _lib.call("hhsr_frame_sharpness", tables[state["i"] % len(tables)], per_call, H, W, 4 * W, 0, cfa_b,
                      _lib.ptr(work), work.numel() * 8, _lib.ptr(scores), stream)
            state["i"] += 1

        legs[f"noise_profile_hist x{per_call}"] = (hist_call, per_call)
        legs[f"frame_sharpness x{per_call}"] = (sharp_call, per_call)

    def torch_call(state={"i": 0}):
        torch_hist(pool[state["i"] % n_pool])
        state["i"] += 1

    legs["torch statement x1"] = (torch_call, 1)
    got = npf.noise_histogram([one], cfa, [1.0, 1.0, 1.0]).to(torch.int64).reshape(-1)
    want = torch_hist(one)
    say(f"# {frame_bytes / 1e6:.1f} MB per frame, pool of {n_pool} copies; kernel histogram: {int(got.sum())} tiles in "
        f"{int((got > 0).sum())} bins; the torch statement's differs in {int((got != want).sum())} bins (another summation "
        "order)")
    prof = npf.fit_profile(got.to(torch.int32).reshape(npf.HIST_SHAPE), cfa)
    say(f"# fitted alpha {prof['alpha']:.4e} beta {prof['beta']:.4e} (simulated {synth.ALPHA_ISO100:.4e}, "
        f"{synth.BETA_ISO100:.4e}), bins used {prof['bins_used']}")

    for fn, _ in legs.values():  # warm-up of every leg
        for _ in range(3):
            fn()
    torch.cuda.synchronize()
    times = {k: [] for k in legs}
    for _ in range(args.blocks):
        for k, (fn, per_call) in legs.items():  # alternating
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            for _ in range(args.calls):
                fn()
            b.record()
            b.synchronize()
            times[k].append(a.elapsed_time(b) / args.calls / per_call)
    say(f"# (a), (b): median of {args.blocks} alternating blocks of {args.calls} calls (min - max), per frame; the rate counts "
        f"the frame's bytes once; {frame_bytes / HBM_MEASURED * 1e6:.1f} us is the frame at the 6.29 TB/s copy rate")
    for k, v in times.items():
        med = median(v)
        say(f"  {k:26s} {1e3 * med:7.1f} us ({1e3 * min(v):.1f} - {1e3 * max(v):.1f}) | {frame_bytes / med / 1e9:.2f} TB/s = "
            f"{100 * frame_bytes / (med * 1e-3) / HBM_MEASURED:.0f} % of the copy rate")
    for per_call in (1, _lib.MAX_BATCH):
        h, s = median(times[f"noise_profile_hist x{per_call}"]), median(times[f"frame_sharpness x{per_call}"])
        say(f"  calls of {per_call}: noise_profile_hist / frame_sharpness = {h / s:.2f}, / the frame at the copy rate = "
            f"{h * 1e-3 / (frame_bytes / HBM_MEASURED):.2f}")
    say(f"  torch statement / noise_profile_hist x1 = "
        f"{median(times['torch statement x1']) / median(times['noise_profile_hist x1']):.0f}")
    del pool, legs
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

        def run(source):
            cfg = hsr.default_config()
            cfg.verbose = 0
            cfg.scale = 2
            cfg.noise_model.source = source
            return hsr.process(burst, cfg)

        est = run("estimate")[1]["noise profile"]
        run("given")
        blocks = {"given": [], "estimate": []}
        for _ in range(args.blocks):
            for k in blocks:  # alternating
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                for _ in range(args.steps):
                    run(k)
                torch.cuda.synchronize()
                blocks[k].append((time.perf_counter() - t0) / args.steps * 1e3)
        say(f"# (c) process(), host-resident burst of {NF} uint16 frames (pageable), x2, float32 result copied back, noise "
            f"curves given: median of {args.blocks} alternating blocks of {args.steps} calls (min - max).  The scene is "
            f"synthetic.make_burst's textured one, on which the estimate is an upper bound: alpha {est['alpha']:.3e} beta "
            f"{est['beta']:.3e}, so the SNR-based parameters of the two legs differ")
        for k, v in blocks.items():
            say(f"  source {k:9s} {median(v):8.1f} ms per call ({min(v):.1f} - {max(v):.1f})")
        say(f"  difference of the medians: {median(blocks['estimate']) - median(blocks['given']):+.1f} ms "
            "(one kernel call, 1 MiB copied back, one synchronisation, the fit on the host)")
    with open(args.out, "w") as f:
        f.write("\n".join(lines) + "\n")
    print("written", args.out)


if __name__ == "__main__":
    main()
