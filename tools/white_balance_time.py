"""Time of the white-balance statistic on one MI355X, written to profiles/white_balance.txt.

    python tools/white_balance_time.py [--shape 3000x4000] [--blocks 7] [--calls 20] [--out FILE]

(a) hhsr_white_balance_hist per frame on uint16 counts and on mipi10 rows, in calls of 1 frame (what process() does by
    default) and of HHSR_MAX_BATCH frames, on a textured synthetic frame (synthetic.make_burst_torch, the gains (2, 1, 1.5)
    divided out, 10-bit counts) and on a uniform grey frame, whose tiles all add to ONE histogram address; next to
    hhsr_frame_sharpness on the same textured frames in the same call sizes (it reads the same bytes once): HIP events around
    blocks of `calls` back-to-back calls, the legs alternating block by block in one process, median block / calls / frames
    (min - max).  The calls walk through a pool of frame copies of at least 512 MB, so that no frame is still in the 256 MB
    Infinity Cache when its turn comes again.  Bytes are counted from the shape: the frame's rows, read once.  The kernel's
    histogram is compared with the torch statement's at the timed size first.
(b) the torch statement of the same tile means and bins on the uint16 frame (what a caller would write today), per frame, in
    the same alternation.
The script ends itself after --timeout seconds."""
import argparse
import os
import signal
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "handheld-multi-frame-super-resolution_amd"))

HBM_MEASURED = 6.29e12  # B/s, float4 copy (profiles/output_encode.txt)
POOL_BYTES = 512e6
GAINS = (2.0, 1.0, 1.5)
BLACK, WHITE = 64.0, 1023.0


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--shape", default="3000x4000")
    ap.add_argument("--blocks", type=int, default=7)
    ap.add_argument("--calls", type=int, default=20)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "white_balance.txt"))
    ap.add_argument("--timeout", type=int, default=540)
    args = ap.parse_args()
    signal.alarm(args.timeout)  # a hang ends here, not at somebody else's limit

    import numpy as np
    import torch

    from handheld_super_resolution import _lib, utils_dng, utils_image, synthetic as synth, white_balance as wbm

    assert torch.cuda.is_available(), "white_balance_time.py measures on the GPU: no device, no number"
    dev = torch.device("cuda", 0)
    H, W = (int(v) for v in args.shape.split("x"))
    cfa = [[0, 1], [1, 2]]
    lines = []

    def say(s):
        print(s, flush=True)
        lines.append(s)

    def median(v):
        v = sorted(v)
        return v[len(v) // 2] if len(v) % 2 else 0.5 * (v[len(v) // 2 - 1] + v[len(v) // 2])

    say(f"# white balance, {H} x {W} ({H * W / 1e6:.0f} MP), device: {torch.cuda.get_device_name(0)}")
    ref, _, _ = synth.make_burst_torch(H, W, 1, dev, seed=1234)
    scene = ref.cpu().numpy().astype(np.float64)
    for q in range(4):
        scene[q >> 1::2, q & 1::2] /= GAINS[cfa[q >> 1][q & 1]] / GAINS[1]
    counts = {"textured": np.clip(np.rint(np.clip(scene, 0, 1) * (WHITE - BLACK) + BLACK), 0, WHITE).astype(np.uint16),
              "uniform": np.full((H, W), 512, np.uint16)}
    del ref, scene
    stream = _lib.stream(dev)
    cfa_b, black_b = _lib.cfa_bytes(cfa), _lib.doubles([BLACK] * 3)
    hist = torch.empty(wbm.HIST_SHAPE, dtype=torch.int32, device=dev)
    work = torch.empty(utils_image.sharpness_workspace_bytes(H, W, _lib.MAX_BATCH) // 8, dtype=torch.float64, device=dev)
    scores = torch.empty(_lib.MAX_BATCH, dtype=torch.float64, device=dev)
    formats = {"uint16": (-1, 2 * W), "mipi10": (utils_dng.PACKINGS["mipi10"], utils_dng.packed_row_bytes(W, "mipi10"))}

    def torch_hist(f):
        """The tile rule in torch on int16 bits [H][W] -> int64 [192 * 192] (float32 operations in torch's own rounding)."""
        nby, nbx = H // 16, W // 16
        c = f.to(torch.int32) & 0xFFFF
        S = [torch.zeros((nby, nbx), dtype=torch.int32, device=dev) for _ in range(3)]
        clipped = torch.zeros((nby, nbx), dtype=torch.bool, device=dev)
        sat = int(np.ceil(BLACK + 15.0 / 16.0 * (WHITE - BLACK)))
        for q in range(4):
            t = c[q >> 1::2, q & 1::2][:8 * nby, :8 * nbx].reshape(nby, 8, nbx, 8)
            S[cfa[q >> 1][q & 1]] += t.sum(dim=(1, 3), dtype=torch.int32)
            clipped |= (t >= sat).any(dim=3).any(dim=1)
        m = [(S[k].to(torch.float32) / (128.0 if k == 1 else 64.0) - BLACK) / (WHITE - BLACK) for k in range(3)]
        ok = ~clipped & (m[0] >= 1 / 64) & (m[1] >= 1 / 64) & (m[2] >= 1 / 64)
        u = ((m[1] / m[0]).view(torch.int32).to(torch.int64) >> 18) - ((127 - 2) << 5)
        v = ((m[1] / m[2]).view(torch.int32).to(torch.int64) >> 18) - ((127 - 2) << 5)
        ok &= (u >= 0) & (u < 192) & (v >= 0) & (v < 192)
        return torch.bincount((u * 192 + v)[ok], minlength=192 * 192)

    legs = {}  # name -> (callable making one call, frames per call, bytes per frame)
    pools = {}
    for content, c in counts.items():
        for fmt, (fid, row_bytes) in formats.items():
            one = torch.from_numpy(c.view(np.int16) if fmt == "uint16" else utils_dng.pack_raw(c, fmt)).to(dev)
            frame_bytes = H * row_bytes
            n_pool = -(-int(POOL_BYTES // frame_bytes + 1) // _lib.MAX_BATCH) * _lib.MAX_BATCH
            pool = pools[content, fmt] = [one.clone() for _ in range(n_pool)]
            packing = None if fmt == "uint16" else fmt
            got = wbm.white_balance_histogram([one], cfa, [BLACK] * 3, WHITE, packing, W).to(torch.int64).reshape(-1)
            fit = wbm.fit_white_balance(got.to(torch.int32).reshape(wbm.HIST_SHAPE))
            note = ""
            if fmt == "uint16":
                want = torch_hist(one)
                note = f"; the torch statement's histogram differs in {int((got != want).sum())} bins"
            say(f"# {content} {fmt}: {frame_bytes / 1e6:.1f} MB per frame, pool of {n_pool} copies; {int(got.sum())} tiles in "
                f"{int((got > 0).sum())} bins, largest {int(got.max())}; gains {fit['white_balance'][0]:.4f}, "
                f"{fit['white_balance'][2]:.4f} (simulated {GAINS[0]}, {GAINS[2]} on the textured frame){note}")
            for per_call in (1, _lib.MAX_BATCH):
                tables = [_lib.ptr_array(pool[i:i + per_call]) for i in range(0, n_pool - per_call + 1, per_call)]

                def wb_call(tables=tables, state={"i": 0}, per_call=per_call, fid=fid, row_bytes=row_bytes):
                    _lib.call("hhsr_white_balance_hist", tables[state["i"] % len(tables)], per_call, H, W, row_bytes, fid,
                              cfa_b, black_b, WHITE, _lib.ptr(hist), stream)
                    state["i"] += 1

                def sharp_call(tables=tables, state={"i": 0}, per_call=per_call, fid=fid, row_bytes=row_bytes):
                    _lib.call("hhsr_frame_sharpness", tables[state["i"] % len(tables)], per_call, H, W, row_bytes, fid, cfa_b,
                              _lib.ptr(work), work.numel() * 8, _lib.ptr(scores), stream)
                    state["i"] += 1

                legs[f"white_balance_hist {content} {fmt} x{per_call}"] = (wb_call, per_call, frame_bytes)
                if content == "textured":
                    legs[f"frame_sharpness {content} {fmt} x{per_call}"] = (sharp_call, per_call, frame_bytes)

    def torch_call(state={"i": 0}):
        pool = pools["textured", "uint16"]
        torch_hist(pool[state["i"] % len(pool)])
        state["i"] += 1

    legs["torch statement textured uint16 x1"] = (torch_call, 1, 2 * H * W)

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
        "the frame's bytes once, against the 6.29 TB/s copy rate")
    for k, v in times.items():
        med, nbytes = median(v), legs[k][2]
        say(f"  {k:44s} {1e3 * med:7.1f} us ({1e3 * min(v):.1f} - {1e3 * max(v):.1f}) | {nbytes / med / 1e9:.2f} TB/s = "
            f"{100 * nbytes / (med * 1e-3) / HBM_MEASURED:.0f} % of the copy rate")
    for fmt in formats:
        for per_call in (1, _lib.MAX_BATCH):
            t = median(times[f"white_balance_hist textured {fmt} x{per_call}"])
            u = median(times[f"white_balance_hist uniform {fmt} x{per_call}"])
            s = median(times[f"frame_sharpness textured {fmt} x{per_call}"])
            say(f"  {fmt}, calls of {per_call}: white_balance_hist / frame_sharpness = {t / s:.2f}, uniform / textured = {u / t:.2f}")
    say(f"  torch statement / white_balance_hist textured uint16 x1 = "
        f"{median(times['torch statement textured uint16 x1']) / median(times['white_balance_hist textured uint16 x1']):.0f}")
    with open(args.out, "w") as f:
        f.write("\n".join(lines) + "\n")
    print("written", args.out)


if __name__ == "__main__":
    main()
