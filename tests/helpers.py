"""Shared test helpers (config construction mirrors tools/refsim/make_goldens.py)."""
import contextlib
import ctypes
import os

import numpy as np

from handheld_super_resolution.config import default_config
from handheld_super_resolution import synthetic as synth
import oracle

ALPHA, BETA = synth.ALPHA_ISO100, synth.BETA_ISO100


def base_config(ts=16, scale=2, snr=30.0, metrics=("L2", "L2", "L2", "L2"), **kw):
    cfg = default_config()
    cfg.scale = scale
    cfg.verbose = 0
    cfg.block_matching.tuning.tile_size = ts
    cfg.block_matching.tuning.metrics = list(metrics)
    cfg.noise_model.alpha = ALPHA
    cfg.noise_model.beta = BETA
    oracle.update_snr_config(cfg, snr)
    std, diff = synth.noise_curves(ALPHA, BETA)
    cfg.noise_model.update({"std_curve": std.tolist(), "diff_curve": diff.tolist()})
    cfg.exif = {"cfa_pattern": [[0, 1], [1, 2]], "iso": 100, "white_balance": [1.0, 1.0, 1.0]}
    cfg.accumulated_robustness_denoiser.enabled = False
    for k, v in kw.items():
        cfg[k] = v
    return cfg


# n_frames argument (position behind the name) of the batch entry points; their single forms carry one frame
FRAMES_ARG = {"hhsr_grey_lowpass_batch": 3, "hhsr_gauss_decimate_batch": 1, "hhsr_align_level_batch": 6,
              "hhsr_frame_stats_batch": 1}


@contextlib.contextmanager
def recorded_calls():
    """Records the library calls that enqueue work while they are made (tests/test_front_end_calls.py): yields the list
    that receives one [entry, frames, stream] per call — the entry point without a trailing `_batch`, the frames of the
    launch (only for the entry points of FRAMES_ARG and their single forms), the ordinal of the stream handle in order of
    first appearance.  Calls without a stream (plan creation and queries: they depend on what ran before) are left out."""
    from handheld_super_resolution import _lib

    real, records, streams = _lib.call, [], {}

    def call(name, *args):
        if args and isinstance(args[-1], ctypes.c_void_p):
            entry = name[:-len("_batch")] if name.endswith("_batch") else name
            frames = [int(args[FRAMES_ARG[name]])] if name in FRAMES_ARG else [1] if entry + "_batch" in FRAMES_ARG else []
            records.append([entry, *frames, streams.setdefault(args[-1].value, len(streams))])
        return real(name, *args)

    _lib.call = call
    try:
        yield records
    finally:
        _lib.call = real


# the bursts of tests/golden/e2e_scales.npz (tools/refsim/make_goldens.py, stage e2e_scales: the reference's own main())
E2E_SCALES = {  # name: (H, W, frames, seed, scale, cfa, white balance, kernel, tile size)
    "s15": (128, 160, 3, 5, 1.5, ((1, 0), (2, 1)), (2.1, 1.0, 1.4), "steerable", 16),
    "s3": (128, 128, 4, 9, 3, ((0, 1), (1, 2)), (1.0, 1.0, 1.0), "steerable", 16),
    "s2iso": (128, 144, 3, 21, 2, ((1, 2), (0, 1)), (1.7, 1.0, 2.2), "iso", 16),
    "ts32": (192, 256, 3, 33, 2, ((2, 1), (1, 0)), (1.0, 1.0, 1.0), "steerable", 32),
}


def e2e_scales_case(tag):
    """(ref, comp, shifts, config factory) of one burst of the e2e_scales golden."""
    H, W, n, seed, scale, cfa, wb, kernel, ts = E2E_SCALES[tag]
    ref, comp, shifts = synth.make_burst(H, W, n, seed=seed, max_shift=2.0, occluder=True, cfa=cfa, wb=wb)

    def cfg_fn():
        cfg = base_config(ts=ts, scale=scale)
        cfg.block_matching.tuning.factors = [1, 2, 2, 2]
        cfg.exif = {"cfa_pattern": [list(r) for r in cfa], "iso": 100, "white_balance": list(wb)}
        cfg.merging.kernel = kernel
        return cfg

    return ref, comp, shifts, cfg_fn


def acc_pattern(oh, ow, phase):
    """Same deterministic accumulator content the golden generator used."""
    i = np.arange(oh)[:, None, None]
    j = np.arange(ow)[None, :, None]
    c = np.arange(3)[None, None, :]
    return (((i * 7 + j * 13 + c * 3 + phase) % 17) / 17.0 + 0.25).astype(np.float32)


def smooth(rng, h, w, sigma=2.0):
    """A smooth random field in [0, 1] (float32 [h, w])."""
    from scipy.ndimage import gaussian_filter

    f = gaussian_filter(rng.standard_normal((h + 16, w + 16)), sigma)[8:8 + h, 8:8 + w]
    return ((f - f.min()) / (f.max() - f.min())).astype(np.float32)


def bm_inputs(rng, ts, r, ny, nx, shift):
    """(reference level [ny ts, nx ts], moving level 3 rows / 5 columns smaller and shifted by `shift`, incoming flow
    [ny, nx, 2] with half-integer ties and a few tiles whose search windows leave the moving level)."""
    h, w = ny * ts, nx * ts
    big = smooth(rng, h + 32, w + 32, 1.5)
    ref = big[16:16 + h, 16:16 + w].copy()
    sy, sx = shift
    mov = big[16 + sy:16 + sy + h - 3, 16 + sx:16 + sx + w - 5].copy()
    mov += 0.01 * rng.standard_normal(mov.shape).astype(np.float32)
    flow = rng.uniform(-1.6, 1.6, (ny, nx, 2)).astype(np.float32)
    flow[0, 0] = (0.5, -0.5)
    flow[0, 1] = (1.5, 2.5)
    flow[1, 0] = (-1.5, -2.5)
    flow[-1, -1] = (6.0, 5.0)
    flow[0, -1] = (-7.0, -6.0)
    return ref, mov, flow


def check_bm(got, want, cost, what, atol=0.0, max_ties=1):
    """Integer block-matching result: equal to the oracle's, except on tiles whose two best costs are tied within 1e-4
    relative (the kernel sums float32 FMAs per lane in a fixed order, the oracle float64) — at most `max_ties` of them."""
    diff = np.abs(got - want).max(-1) > atol
    for ty, tx in zip(*np.nonzero(diff)):
        c = np.sort(cost[ty, tx].ravel())
        assert (c[1] - c[0]) <= 1e-4 * max(1.0, abs(c[0])), (what, ty, tx, c[:3], got[ty, tx], want[ty, tx])
    assert diff.sum() <= max_ties, (what, int(diff.sum()))


def merge_frames(H, W, n, ts, seed, cfg):
    """(ref, [(comp, flow, covs, r)] * n): merge inputs with random flows in [-2, 2] and robustness in [0, 1]."""
    ref, comp, _ = synth.make_burst(H, W, n + 1, seed=seed, max_shift=1.5)
    rng = np.random.default_rng(seed)
    fr = []
    for k in range(n):
        flow = rng.uniform(-2, 2, ((H + ts - 1) // ts, (W + ts - 1) // ts, 2)).astype(np.float32)
        r = rng.random((H, W), dtype=np.float32)
        covs = oracle.estimate_kernels(comp[k], cfg)
        fr.append((comp[k], flow, covs, r))
    return ref, fr


def assert_close(a, b, rtol, atol, what="", max_bad_frac=0.0):
    """allclose with NaN == NaN and inf == inf; optionally tolerate a fraction of outliers."""
    a = np.asarray(a, dtype=np.float64)
    b = np.asarray(b, dtype=np.float64)
    assert a.shape == b.shape, f"{what}: shape {a.shape} vs {b.shape}"
    both_nan = np.isnan(a) & np.isnan(b)
    same_inf = np.isinf(a) & np.isinf(b) & (np.sign(a) == np.sign(b))
    with np.errstate(all="ignore"):
        ok = np.abs(a - b) <= atol + rtol * np.abs(b)
    ok = ok | both_nan | same_inf
    bad = (~ok).sum()
    log = os.environ.get("HHSR_PARITY_LOG")
    if log:  # tools/parity_report.py: measured errors next to the tolerances, one JSON line per comparison
        import json

        with np.errstate(all="ignore"):
            d = np.abs(a - b)
            d[both_nan | same_inf] = 0
            fin = np.isfinite(d)
            p99 = float(np.percentile(d[fin], 99.9)) if fin.any() else 0.0
            rec = {"test": os.environ.get("PYTEST_CURRENT_TEST", "").split(" ")[0], "what": what, "n": int(ok.size),
                   "max_abs": float(np.nanmax(np.where(fin, d, 0))) if d.size else 0.0, "p999_abs": p99,
                   "rtol": rtol, "atol": atol, "outliers": int(bad), "allowed_frac": max_bad_frac,
                   "scale": float(np.nanmax(np.abs(np.where(np.isfinite(b), b, 0)))) if b.size else 0.0}
        with open(log, "a") as f:
            f.write(json.dumps(rec) + "\n")
    if bad > max_bad_frac * ok.size:
        with np.errstate(all="ignore"):
            err = np.where(ok, 0, np.abs(a - b))
        k = np.unravel_index(np.nanargmax(err), err.shape)
        raise AssertionError(f"{what}: {bad}/{ok.size} mismatches; worst at {k}: {a[k]} vs {b[k]}")


def flipped_tiles(gflows, oflows, thresh=0.05):
    """Boolean [n, ny, nx]: tiles whose flow differs from the oracle's by more than ICA noise — one of the (up to 4)
    block-matching decisions on the way down the pyramid took the other side of a float32 near-tie (the direct-SSD
    kernel and the oracle's FFT correlation associate their sums differently)."""
    g, o = np.asarray(gflows, np.float64), np.asarray(oflows, np.float64)
    return np.abs(g - o).max(-1) > thresh


def footprint(flipped, ts, shape, scale=1.0, grow=3):
    """Pixels of a [round(scale H), round(scale W)] map that a tile's flow can influence: the tile itself (merge:
    HR pixels whose LR position lies in the tile; robustness: the tile's pixels) grown by `grow` LR pixels (5x5
    minimum of the robustness, bilinear covariance cell, rounding of (h + 0.5) / scale)."""
    H, W = shape
    any_f = np.asarray(flipped).any(0) if np.asarray(flipped).ndim == 3 else np.asarray(flipped)
    lr = np.zeros((H, W), bool)
    for ty, tx in zip(*np.nonzero(any_f)):
        lr[max(0, ty * ts - grow): (ty + 1) * ts + grow, max(0, tx * ts - grow): (tx + 1) * ts + grow] = True
    sH, sW = round(scale * H), round(scale * W)
    yi = np.minimum((((np.arange(sH) + 0.5) / scale)).astype(int), H - 1)
    xi = np.minimum((((np.arange(sW) + 0.5) / scale)).astype(int), W - 1)
    return lr[np.ix_(yi, xi)]


def assert_explained(got, want, atol, flipped, ts, shape, scale, what, max_flipped, per_frame=False, grow=None,
                     stray=(0, 0.0)):
    """|got - want| <= atol everywhere except inside the footprint of flipped tiles; the number of flipped tiles
    (over all frames) is itself bounded by `max_flipped` (the measured count, PARITY.md).  NaN == NaN.
    `grow`: LR pixels the footprint extends beyond the tile; default ts + 3 — a tile's flow enters the flow-irregularity
    weight S of its 8 NEIGHBOUR tiles (robustness.py:587-612), so a flipped decision can switch their S between s1 and
    s2 and with it their robustness and merged pixels.
    `stray` = (count, cap): that many values outside the footprint may exceed atol, each by at most cap (isolated
    flow-sensitive pixels, tests/test_fuzz_parity.py: the measured count goes here, not a blanket allowance)."""
    grow = ts + 3 if grow is None else grow
    got, want = np.asarray(got, np.float64), np.asarray(want, np.float64)
    assert got.shape == want.shape, f"{what}: shape {got.shape} vs {want.shape}"
    nf = int(np.asarray(flipped).sum())
    with np.errstate(all="ignore"):
        bad = ~((np.abs(got - want) <= atol) | (np.isnan(got) & np.isnan(want)))
    if bad.ndim == 3 and bad.shape[-1] == 3 and not per_frame:      # [sH, sW, 3] image
        mask = footprint(flipped, ts, shape, scale, grow)[..., None]
    elif per_frame:                                                  # [n, H, W] per-frame maps
        mask = np.stack([footprint(f, ts, shape, scale, grow) for f in np.asarray(flipped)])
    else:
        mask = footprint(flipped, ts, shape, scale, grow)
    unexplained = bad & ~mask
    log = os.environ.get("HHSR_PARITY_LOG")
    if log:
        import json

        with np.errstate(all="ignore"):
            d = np.where(np.isfinite(got - want), np.abs(got - want), 0)
        with open(log, "a") as f:
            f.write(json.dumps({"test": os.environ.get("PYTEST_CURRENT_TEST", "").split(" ")[0], "what": what,
                                "n": int(bad.size), "max_abs": float(d.max()), "max_abs_outside_footprint": float(np.where(mask, 0, d).max()),
                                "atol": atol, "rtol": 0, "outliers": int(bad.sum()), "unexplained": int(unexplained.sum()),
                                "flipped_tiles": nf, "allowed_flipped": max_flipped}) + "\n")
    assert nf <= max_flipped, f"{what}: {nf} flipped tiles (allowed {max_flipped})"
    if unexplained.any():
        with np.errstate(all="ignore"):
            err = np.where(unexplained, np.abs(got - want), 0)
        if int(unexplained.sum()) <= stray[0] and float(np.nanmax(err)) <= stray[1]:
            return
        k = np.unravel_index(np.nanargmax(err), err.shape)
        raise AssertionError(f"{what}: {int(unexplained.sum())} differences above {atol} outside the footprint of the "
                             f"{nf} flipped tiles; worst at {k}: {got[k]} vs {want[k]}")


# ---- the per-case rules of tests/test_fuzz_parity.py (pure NumPy: unit-tested on the CPU in test_host_logic.py) -------------
FLIP_PX = 1e-3          # flow difference that marks a tile as following another block-matching decision
MAX_ICA_TILES = 16      # tiles per case with a flow difference between 1e-4 and FLIP_PX (measured: <= 10, in 3 of 768 cases)
CLUSTER = 8             # tiles per side of the finest-level tiles under one level-2 tile of the default pyramid
MAX_FLIP_TILES = 16     # finest-level tiles per case under the ONE flipped decision (measured: 1, or a 2 x 2 block)
ACC_TOL = 1e-6          # the accumulated robustness HIP reports (a float32 map) against the float64 sum of ITS OWN maps
# ---- Round 5: the contract is STAGE BY STAGE ON IDENTICAL INPUTS, in both directions.  Round 4's rules
# compared HIP's own-flow image with the oracle's own-flow image and excused "flow-sensitive" values (agree once the oracle's
# flows are injected into HIP) up to a cap, MAX_SENS = 0.15 — violated at 0.177, 0.187 and 0.671 on held-out seeds.  Now
#   alignment     HIP's flows vs the oracle's flows                                            (<= 1e-4 px off flipped tiles)
#   robustness    on IDENTICAL flows (HIP's: side H; the oracle's: side O): r                  (<= 1e-4)
#   merge         on IDENTICAL flows AND IDENTICAL robustness maps (HIP's r injected into the oracle, oracle.main(rob=...)):
#                 image <= 1e-4 EVERYWHERE, identical NaN pattern                              (no region, count, size or
#                 small-weight excuse: measured <= 3.4e-5 over 2560 cases incl. the value whose accumulated weight is 3.4e-7).
#                 The oracle sums HIP's maps in float64 like the reference (super_resolution.py:116-117) — and so does HIP
#                 wherever the sum DECIDES something (robustness.RobustnessSum) since the sweep found case 4300.15: the
#                 denoiser's `acc_rob < max_frame_count` at 1 + 1 + 0.99999994, which is 3 in float32 (6 values, 0.038).  The
#                 map HIP reports is asserted against the float64 sum of its maps: <= ACC_TOL
#   whole chain   on identical flows (o vs want_h, oi vs want): <= 1e-4 wherever every frame is accepted; where a frame is
#                 being rejected a value may exceed 1e-4 only if the merge comparison above shows it to be the effect of the
#                 <= 1e-4 by which r differs (it agrees once HIP's r is injected) — round 4's count / magnitude caps
#                 (MAX_OUTLIERS, MAX_OUTLIER, two raw pixels' worth) are gone with MAX_SENS: nothing is excused by magnitude.


def same_flow_side(shape, scale, out, want, r_hip, r_or, den, want_m=None, den_m=None):
    """HIP image `out` against the oracle image `want` computed from the SAME flow fields (either HIP's or the oracle's),
    and against `want_m`: the oracle's MERGE ALONE on the same flows and HIP's own robustness maps `r_hip` (None with the
    robustness off: then want_m is want).  Robustness maps [n, H, W].  Returns the numbers of the side:
      nan_mis, dr                       NaN pattern out vs want, max |r_hip - r_or|
      n, max, outside, unexplained      values > 1e-4 vs want; those where every frame is fully accepted (r = 1 in the 5 x 5
                                        raw-pixel neighbourhood on both sides: nothing may differ there); those where a frame
                                        is being rejected that do NOT agree once HIP's r is injected
      m_nan, m_n, m_max                 merge alone: NaN mismatches, values > 1e-4 (none allowed), the largest difference"""
    H, W = shape
    if want_m is None:
        want_m, den_m = want, den
    nan_mis = int((np.isnan(out) != np.isnan(want)).sum())
    dr = float(np.abs(r_hip - r_or).max()) if r_or is not None else 0.0
    with np.errstate(all="ignore"):  # NaN == NaN (the pattern is compared above), inf == inf; inf vs finite stays inf
        d = np.where(np.isnan(want) | (out == want), 0.0, np.abs(out.astype(np.float64) - want))
        dm = np.where(np.isnan(want_m) | (out == want_m), 0.0, np.abs(out.astype(np.float64) - want_m))
    rej = np.zeros(out.shape[:2], bool)
    if r_or is not None:
        from scipy.ndimage import minimum_filter

        low = minimum_filter(np.minimum(r_or.min(0), r_hip.min(0)), size=5, mode="nearest") < 0.999
        yy = np.minimum(((np.arange(out.shape[0]) + 0.5) / scale).astype(int), H - 1)
        xx = np.minimum(((np.arange(out.shape[1]) + 0.5) / scale).astype(int), W - 1)
        rej = low[np.ix_(yy, xx)]
    bad, bad_m = d > 1e-4, dm > 1e-4
    return dict(nan_mis=nan_mis, dr=dr, n=int(bad.sum()), max=float(d.max()), outside=int((bad & ~rej[..., None]).sum()),
                unexplained=int((bad & rej[..., None] & bad_m).sum()),
                m_nan=int((np.isnan(out) != np.isnan(want_m)).sum()), m_n=int(bad_m.sum()), m_max=float(dm.max()))


def side_failures(tag, s):
    failed = []
    if not s.get("acc", 0.0) <= ACC_TOL:
        failed.append(f"{tag}: accumulated robustness differs from the sum of HIP's own maps by {s['acc']:.2e}")
    if s["nan_mis"] or s["m_nan"]:
        failed.append(f"{tag}: {s['nan_mis']} / {s['m_nan']} NaN mismatches (whole chain / merge alone)")
    if not s["dr"] <= 1e-4:
        failed.append(f"{tag}: r {s['dr']:.2e}")
    if s["m_n"]:
        failed.append(f"{tag}, merge on identical flows and robustness: {s['m_n']} values above 1e-4 (max {s['m_max']:.2e})")
    if s["outside"] or s["unexplained"]:
        failed.append(f"{tag}: {s['n']} values above 1e-4 (max {s['max']:.2e}): {s['outside']} where every frame is accepted, "
                      f"{s['unexplained']} where a frame is being rejected that HIP's robustness does not explain")
    return failed


def alignment_part(gflow, oflow):
    """The flow fields of the two alignments against each other: (numbers, mask of every tile whose flow deviates)."""
    gflow = np.asarray(gflow)
    big = flipped_tiles(gflow, oflow, FLIP_PX)
    flipped = flipped_tiles(gflow, oflow, 1e-4)  # every tile whose flow deviates
    nflip, n_ica = int(big.sum()), int((flipped & ~big).sum())
    one_cluster = True
    if nflip:
        fn, fy, fx = np.nonzero(big)
        one_cluster = len(set(fn.tolist())) == 1 and np.ptp(fy) < CLUSTER and np.ptp(fx) < CLUSTER
    dflow = float(np.abs(gflow - oflow).max(-1)[~flipped].max()) if (~flipped).any() else 0.0
    return dict(nflip=nflip, one_cluster=one_cluster, n_ica=n_ica, dflow=dflow), flipped


def informational_part(shape, ts, scale, flipped, o, want, want_h):
    """Reported, not asserted: own flows against own flows outside the footprint of deviating tiles, and how far the
    ORACLE's own image moves there when it is given HIP's flows."""
    out_fp = ~footprint(flipped, ts, shape, scale, ts + 3)[..., None]
    with np.errstate(all="ignore"):
        d_own = np.where(np.isnan(want) | (o == want) | ~out_fp, 0.0, np.abs(o.astype(np.float64) - want))
        d_orc = np.where(np.isnan(want) | (want_h == want) | ~out_fp, 0.0, np.abs(want_h.astype(np.float64) - want))
    d_own, d_orc = np.nan_to_num(d_own, nan=np.inf), np.nan_to_num(d_orc, nan=np.inf)
    return dict(n_own=int((d_own > 1e-4).sum()), own_max=float(d_own.max()), n_orc=int((d_orc > 1e-4).sum()),
                orc_max=float(d_orc.max()))


def combine_verdict(scale, al, sh, so, info):
    """(numbers, failed rules) from the parts: alignment, side H (HIP's flows), side O (the oracle's flows)."""
    failed = []  # the assertions of the case (report mode lists them next to the numbers instead of stopping)
    if not (al["one_cluster"] and al["nflip"] <= MAX_FLIP_TILES and al["n_ica"] <= MAX_ICA_TILES):
        failed.append(f"{al['nflip']} flipped tiles (one cluster: {al['one_cluster']}), {al['n_ica']} tiles between 1e-4 and "
                      f"{FLIP_PX:g} px")
    if not al["dflow"] <= 1e-4:
        failed.append(f"flow {al['dflow']:.2e} px")
    failed += side_failures("HIP's flows", sh) + side_failures("oracle's flows", so)
    return dict(al, side_h=sh, side_o=so, **info), failed


def fuzz_verdict(shape, ts, scale, o, oi, want, want_h, gflow, oflow, hr, hr_i, o_r, o_r_h, den_o, den_h, want_hm=None,
                 den_hm=None, want_om=None, den_om=None):
    """One case of the fuzz sweep, judged.  HIP outputs with its own flows `o` / with the oracle's flows injected `oi`;
    oracle outputs with its own flows `want` / with HIP's flows injected `want_h`; flows [n, ny, nx, 2]; robustness maps
    [n, H, W] of the two HIP runs (`hr`, `hr_i`) and of the two oracle runs (`o_r`: own flows, `o_r_h`: HIP's flows), None with
    the robustness off; accumulated weights of the two oracle runs (`den_o`, `den_h`); `want_hm` / `want_om` (+ weights): the
    oracle's merge alone on HIP's flows + `hr` / on its own flows + `hr_i` (None: robustness off, the runs above).
    Returns (numbers, failed rules) — the rules are spelled out above the constants and in the docstring of
    tests/test_fuzz_parity.py:
      alignment   gflow vs oflow
      side H      o  vs want_h, hr   vs o_r_h, o  vs want_hm   (everything downstream of the alignment on HIP's flows)
      side O      oi vs want,   hr_i vs o_r,   oi vs want_om   (the same on the oracle's flows)
    and, reported but NOT asserted (it is implied by the three): o vs want, next to |want_h - want| — how far the ORACLE's
    own image moves under the flow difference.  (The sweep evaluates the parts in its worker processes: same functions.)"""
    al, flipped = alignment_part(gflow, oflow)
    sh = same_flow_side(shape, scale, o, want_h, hr, o_r_h, den_h, want_hm, den_hm)
    so = same_flow_side(shape, scale, oi, want, hr_i, o_r, den_o, want_om, den_om)
    return combine_verdict(scale, al, sh, so, informational_part(shape, ts, scale, flipped, o, want, want_h))
