"""Time of the noise-curve estimators on one MI355X: run_fast_MC(engine="torch") against run_fast_MC(engine="hip"),
and hhsr_noise_mc alone.

    python tools/noise_curves_time.py [--blocks 7] [--calls 3] [--out profiles/noise_curves.txt]

Per profile (synthetic.ALPHA_ISO100 x {1, 16} and the fallback profile that simulates all 1001 levels), after a warm-up
of both engines: `blocks` alternating blocks — `calls` calls of one engine, then of the other — in one process; the
figure is the median over the blocks of block time / calls (min - max).  A call ends in its device-to-host copy, so the
host clock around it measures the whole call: launches, kernels, copy, and for "hip" the host-side fill.
hhsr_noise_mc alone: HIP events around blocks of back-to-back launches on buffers allocated once.  Next to it the VALU
wave-instructions of the launch — VALU_PER_PAIR x patch pairs / 64, VALU_PER_PAIR counted statically in the gfx950
ISA of k_noise_mc's loop body without the large-argument branch of sincosf, which theta < 2 pi never takes — over the
VALU issue peak VERDICT.md uses (256 CU x 4 SIMD x 2.4 GHz / 2 cycles).  The script ends itself after --timeout seconds."""
import argparse
import ctypes
import os
import signal
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "handheld-multi-frame-super-resolution_amd"))

VALU_PEAK = 256 * 4 * 2.4e9 / 2  # wave-instructions / s
VALU_PER_PAIR = 1008             # static: 1868 VALU instructions in the loop body - 10 x 86 in the branch never taken


def median(v):
    v = sorted(v)
    return v[len(v) // 2], v[0], v[-1]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--blocks", type=int, default=7)
    ap.add_argument("--calls", type=int, default=3)
    ap.add_argument("--kernel-calls", type=int, default=20)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "noise_curves.txt"))
    ap.add_argument("--timeout", type=int, default=540)
    args = ap.parse_args()
    signal.alarm(args.timeout)  # a hang ends here, not at somebody else's limit

    import numpy as np
    import torch

    from handheld_super_resolution import _lib, fast_monte_carlo as mc, synthetic as synth

    assert torch.cuda.is_available(), "noise_curves_time.py measures on the GPU: no device, no number"
    dev = torch.device("cuda", 0)
    lines = []

    def say(s):
        print(s, flush=True)
        lines.append(s)

    n = mc.N_PATCHES
    say(f"# noise curves, n_patches = {n}: median of {args.blocks} alternating blocks of {args.calls} calls (min - max), "
        f"one process, after warm-up")
    say(f"# device: {torch.cuda.get_device_name(0)}")
    profiles = [("ALPHA_ISO100 x 1", synth.ALPHA_ISO100, synth.BETA_ISO100),
                ("ALPHA_ISO100 x 16", synth.ALPHA_ISO100 * 16, synth.BETA_ISO100 * 16), ("fallback (0.05, 0.01)", 0.05, 0.01)]
    for name, a, b in profiles:
        levels = np.empty(1001, np.int32)
        n_lv = ctypes.c_int32(0)
        _lib.call("hhsr_noise_mc_levels", a, b, levels.ctypes.data_as(_lib.I32P), 1001, ctypes.byref(n_lv))
        n_lv = n_lv.value
        engines = {e: (lambda e=e: mc.run_fast_MC(a, b, seed=0, device=dev, engine=e)) for e in ("torch", "hip")}
        for fn in engines.values():  # warm-up: code objects, torch's allocator
            fn()
        torch.cuda.synchronize()
        ms = {e: [] for e in engines}
        for _ in range(args.blocks):
            for e, fn in engines.items():
                t0 = time.perf_counter()
                for _ in range(args.calls):
                    fn()
                ms[e].append((time.perf_counter() - t0) * 1e3 / args.calls)
        say(f"{name}: {n_lv} simulated levels")
        med = {}
        for e in engines:
            med[e], lo, hi = median(ms[e])
            say(f"  run_fast_MC(engine=\"{e}\"): {med[e]:.3f} ms per call ({lo:.3f} - {hi:.3f})")
        say(f"  torch / hip = {med['torch'] / med['hip']:.1f}")

        lv = torch.from_numpy(levels[:n_lv].copy()).to(dev)
        nbytes = ctypes.c_size_t(0)
        _lib.call("hhsr_noise_mc_workspace", n_lv, n, ctypes.byref(nbytes))
        ws = torch.empty(nbytes.value // 8, dtype=torch.float64, device=dev)
        out = torch.empty((2, n_lv), dtype=torch.float64, device=dev)
        s = _lib.stream(dev)

        def kernel():
            _lib.call("hhsr_noise_mc", _lib.ptr(lv), n_lv, a, b, n, 0, _lib.ptr(out[0]), _lib.ptr(out[1]), _lib.ptr(ws), nbytes,
                      s)

        for _ in range(3):
            kernel()
        torch.cuda.synchronize()
        ev = []
        for _ in range(args.blocks):
            t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            t0.record()
            for _ in range(args.kernel_calls):
                kernel()
            t1.record()
            t1.synchronize()
            ev.append(t0.elapsed_time(t1) / args.kernel_calls)
        k_med, lo, hi = median(ev)
        valu = VALU_PER_PAIR * n_lv * n / 64
        say(f"  hhsr_noise_mc alone (HIP events, blocks of {args.kernel_calls} launches): {k_med:.3f} ms ({lo:.3f} - {hi:.3f}) | "
            f"{valu:.3e} VALU wave-instructions (static estimate) -> {valu / (k_med * 1e-3):.3e} / s = "
            f"{100 * valu / (k_med * 1e-3) / VALU_PEAK:.1f} % of the {VALU_PEAK:.3e} / s issue peak")
    with open(args.out, "w") as f:
        f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
