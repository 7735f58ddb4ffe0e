"""GPU parity of the kernel variants that the dispatchers pick by scale, sensor, tile size or image size, each against
the oracle on identical inputs, on grids that give the XCD-aware workgroup remaps a remainder:

  merge        x1 / x4 / x8 (GEOM_P2 tile kernel), x1.5 / x2.5 (GEOM_F64 generic kernel), x2 / x3 (controls), on RGGB,
               GBRG and `mode: grey`, steerable and iso kernels; the generic, tile, float64-weight, per-frame, frame-split,
               accumulated-robustness and chained (> HHSR_MAX_FRAMES) launch forms; adversarial flows on the GEOM_P2 carry
               thresholds, small negative flows, a frame pushed out of the image, robustness patches of exactly 0
  alignment    every k_align_wave<ts, r, L1> instantiation through hhsr_align_level_batch (a partial second batch, the
               coarser level's flow read in place) and the ts = 64 block-matching + ICA kernels
  grey         the rocFFT fallback plans (plain, pruned, transposed) at sensor sizes with prime factors 17 / 19 / 31
  robustness   k_rob_frames_row4<VEC> (16-byte and dword instantiation) and k_rob_frame; the entry points against each other

Tolerances are the ones of tests/test_hip_parity.py for the same stages (merge rtol 2e-5 / atol 1e-6, flows 2e-4 px
with the block-matching near-tie rule, grey 3e-6, robustness 1e-4)."""
import itertools

import numpy as np
import pytest
import torch

import oracle
from oracle import cfast
from oracle.parallel import available_cores
from helpers import assert_close, base_config, bm_inputs, check_bm, merge_frames, smooth

pytestmark = pytest.mark.gpu

from handheld_super_resolution import (utils_image, alignment, ICA, robustness, merge, utils, _lib,  # noqa: E402
                                       synthetic as synth)

DEV = "cuda"
THREADS = available_cores()


def T(a, dtype=torch.float32):
    return torch.as_tensor(np.ascontiguousarray(a), dtype=dtype, device=DEV)


def N(t):
    return t.detach().cpu().numpy()


def cdiv(a, b):
    return -(-a // b)


# ------------------------------------------------------------------------------------------ merge
SENSORS = {"rggb": ((0, 1), (1, 2)), "gbrg": ((1, 2), (0, 1)), "grey": ((1, 1), (1, 1))}  # grey: the scene's green plane
# LR (H, W, ts) per scale: neither side a multiple of the tile size; at the integer scales the 16 x 16 HR tile kernel's
# grid (cdiv(sW, 16) x cdiv(sH, 16)) has more than 64 workgroups and nblk % 8 != 0 (checked in _merge_inputs)
SHAPES = {1: (150, 200, 32), 2: (70, 102, 16), 3: (54, 76, 16), 4: (58, 90, 16), 8: (70, 90, 16),
          1.5: (100, 150, 32), 2.5: (52, 70, 16)}
SCALES = list(SHAPES)
_INPUTS, _ORACLE = {}, {}


def _carry_thresholds(s):
    """Fractions 1 - frac((h + 0.5) / s) at which the GEOM_P2 carry fl >= floor(fl) + (1 - frac(lr)) flips, plus 0 and
    one half (the float64 window-centre rule of merge.py:319-345)."""
    return sorted({(2 * s - 2 * rem - 1) / (2 * s) for rem in range(s)} | {0.0, 0.5})


def _threshold_flows(rng, scale, ny, nx):
    """Flows whose fractional parts are the carry thresholds of the scale (x4 for the non-integer scales) and their float32
    neighbours, every one of them on both axes, integer parts -3 .. 2."""
    s = int(scale) if float(scale).is_integer() else 4
    base = [(t, d) for t in _carry_thresholds(s) for d in (-1, 0, 1)]
    assert ny * nx >= len(base), "grid too small to carry every threshold on both axes"
    out = np.empty((ny * nx, 2), np.float32)
    for c in range(2):
        for slot, b in enumerate(rng.permutation(ny * nx) % len(base)):
            t, d = base[b]
            f = np.float32(rng.choice([-3.0, -1.0, 0.0, 2.0]) + t)
            out[slot, c] = np.nextafter(f, np.float32(10 * d)) if d else f
    return out.reshape(ny, nx, 2)


def _cfg(scale, sensor, kern="steerable", **hip):
    H, W, ts = SHAPES[scale]
    cfg = base_config(ts=ts, scale=scale, mode="grey" if sensor == "grey" else "bayer")
    cfg.exif = {"cfa_pattern": [list(r) for r in SENSORS[sensor]], "iso": 100, "white_balance": [1.0, 1.0, 1.0]}
    cfg.merging.kernel = kern
    if hip:
        cfg.hip = hip
    return cfg


def _merge_inputs(scale, sensor):
    """(ref, ref covariances, [(raw, flow, covs, r)] x 4) of one (scale, sensor): random flows; flows on the carry
    thresholds; small negative flows (-1e-3, -0.1: flow - floor(flow) is inexact in float32); a frame pushed partly out of
    the image (+9.5).  Frames 0 and 2 have a patch of robustness exactly 0.  Built once per input set."""
    key = (scale, sensor)
    if key not in _INPUTS:
        H, W, ts = SHAPES[scale]
        if float(scale).is_integer():
            sH, sW = int(scale) * H, int(scale) * W
            nblk = cdiv(sW, 16) * cdiv(sH, 16)
            assert nblk > 64 and nblk % 8 != 0, (scale, nblk)
        seed = int(10 * scale) + 7 * len(sensor) + ord(sensor[0])
        ref, comp, _ = synth.make_burst(H, W, 5, seed=seed, max_shift=1.5, cfa=SENSORS[sensor])
        rng = np.random.default_rng(seed)
        ny, nx = cdiv(H, ts), cdiv(W, ts)
        flows = [rng.uniform(-2, 2, (ny, nx, 2)), _threshold_flows(rng, scale, ny, nx),
                 np.where(rng.random((ny, nx, 2)) < 0.5, -1e-3, -0.1), rng.uniform(-2, 2, (ny, nx, 2)) + 9.5]
        cfg = _cfg(scale, sensor)
        frames = []
        for k in range(4):
            r = rng.random((H, W), dtype=np.float32)
            if k in (0, 2):
                r[H // 4:H // 4 + 12, W // 3:W // 3 + 20] = 0.0
            frames.append((comp[k], flows[k].astype(np.float32), oracle.estimate_kernels(comp[k], cfg), r))
        _INPUTS[key] = (ref, oracle.estimate_kernels(ref, cfg), frames)
    return _INPUTS[key]


def _oracle_merge(scale, sensor, kern):
    """The oracle's accumulators after the comp frames (num_c, den_c) and after the reference frame (num, den), and the
    float64 normalised image; once per (inputs, kernel)."""
    key = (scale, sensor, kern)
    if key not in _ORACLE:
        ref, ref_covs, frames = _merge_inputs(scale, sensor)
        H, W, _ = SHAPES[scale]
        cfg = _cfg(scale, sensor, kern)
        cfa = SENSORS[sensor]
        num = np.zeros((round(scale * H), round(scale * W), 3), np.float32)
        den = np.zeros_like(num)
        for f in frames:
            cfast.merge(*f, num, den, cfa, cfg, threads=THREADS)
        num_c, den_c = num.copy(), den.copy()
        cfast.merge_ref(ref, ref_covs, num, den, cfa, cfg, threads=THREADS)
        with np.errstate(all="ignore"):
            out = num.astype(np.float64) / den
        _ORACLE[key] = dict(num_c=num_c, den_c=den_c, num=num, den=den, out=out)
    return _ORACLE[key]


def _acc_want(frames):
    return np.sum([f[3].astype(np.float64) for f in frames], axis=0)


def _burst(scale, sensor, kern, frames=None, acc=True, **hip):
    """merge_burst on the input set: (normalised image, accumulated robustness or None)."""
    ref, ref_covs, fr = _merge_inputs(scale, sensor)
    fr = fr if frames is None else frames
    H, W, _ = SHAPES[scale]
    tf = [tuple(T(a) for a in f) for f in fr]
    out = torch.empty(round(scale * H), round(scale * W), 3, device=DEV)
    acc_r = torch.zeros(H, W, device=DEV) if acc and float(scale).is_integer() and not hip.get("weight_fp64") else None
    merge.merge_burst(tf, T(ref), T(ref_covs), out, None, SENSORS[sensor], _cfg(scale, sensor, kern, **hip), acc_r=acc_r)
    return N(out), (None if acc_r is None else N(acc_r))


TOL = (2e-5, 1e-6)  # the merge tolerance of tests/test_hip_parity.py::test_merge_golden


def _assert_sums(got, want, scale, what):
    """Un-normalised sums: TOL, except within 3 s output rows / columns of the top-left border.  There the flows of the
    threshold frame (integer parts down to -3) put lr + flow just before the first raw row or column, where D11
    extrapolates the covariance to a nearly singular matrix that amplifies the float32 rounding of the weight chain —
    the case of test_hip_parity.py::test_merge_integer_scale_geometry_decisions.  Measured: one value in 1e5 - 1e6 at
    4.8e-5 relative (x3 row 2, x4 row 9, x8 column 18), and on the 2-frame partial den at x3 3.8e-6 absolute on a weight
    sum of 1.4e-3.  The band keeps that test's 1e-3 relative with 1e-5 absolute; the normalised images keep TOL
    everywhere."""
    b = 3 * int(np.ceil(scale))
    assert_close(got[b:, b:], want[b:, b:], *TOL, what)
    assert_close(got, want, 1e-3, 1e-5, what + ", top-left D11 band")


@pytest.mark.parametrize("kern", ["steerable", "iso"])
@pytest.mark.parametrize("sensor", list(SENSORS))
@pytest.mark.parametrize("scale", SCALES)
def test_merge_auto_vs_oracle(scale, sensor, kern):
    """merge_burst with the kernel hhsr_merge_burst picks (x1 / x4 / x8 Bayer: k_merge_burst_tile<GEOM_P2>; grey at every
    scale but x2: k_merge_burst; x1.5 / x2.5: k_merge_burst<float, GEOM_F64>) against the oracle: the normalised image,
    the raw sums num / den (do_ref, no divide), and at the integer scales the accumulated robustness."""
    o = _oracle_merge(scale, sensor, kern)
    ref, ref_covs, frames = _merge_inputs(scale, sensor)
    what = f"x{scale} {sensor} {kern}"
    out, acc = _burst(scale, sensor, kern)
    assert_close(out, o["out"], *TOL, what + " image")
    if acc is not None:
        assert_close(acc, _acc_want(frames), 1e-6, 1e-6, what + " accumulated robustness")
    H, W, _ = SHAPES[scale]
    num = torch.empty(round(scale * H), round(scale * W), 3, device=DEV)
    den = torch.empty_like(num)
    merge.merge_burst([tuple(T(a) for a in f) for f in frames], T(ref), T(ref_covs), num, den, SENSORS[sensor],
                      _cfg(scale, sensor, kern), divide=False, store_den=True)
    _assert_sums(N(num), o["num"], scale, what + " num")
    _assert_sums(N(den), o["den"], scale, what + " den")


FORM_CASES = [(s, "rggb", "steerable") for s in SCALES] + [(1, "grey", "steerable"), (4, "grey", "iso"),
                                                            (8, "gbrg", "iso"), (4, "gbrg", "steerable")]


@pytest.mark.parametrize("scale,sensor,kern", FORM_CASES)
def test_merge_launch_forms_vs_oracle(scale, sensor, kern):
    """The other launch forms on the same inputs, against the same oracle result: merge_kernel generic (k_merge_burst
    <float, GEOM_P2 / GEOM_F64>) and tile; the float64 weight chain; per-frame merge (k_accumulate) + merge_ref + divide;
    a frame split through store_den / load_acc at the integer scales; the accumulated-robustness denoiser's merge_ref at
    x1 and x4."""
    o = _oracle_merge(scale, sensor, kern)
    ref, ref_covs, frames = _merge_inputs(scale, sensor)
    H, W, _ = SHAPES[scale]
    cfa = SENSORS[sensor]
    what = f"x{scale} {sensor} {kern}"
    integer = float(scale).is_integer()
    acc_want = _acc_want(frames)
    for which in (["generic", "tile"] if integer else ["generic"]):
        out, acc = _burst(scale, sensor, kern, merge_kernel=which)
        assert_close(out, o["out"], *TOL, f"{what} merge_kernel={which}")
        if acc is not None:
            assert_close(acc, acc_want, 1e-6, 1e-6, f"{what} merge_kernel={which} accumulated robustness")
    out, _ = _burst(scale, sensor, kern, weight_fp64=True)
    assert_close(out, o["out"], *TOL, what + " weight_fp64")
    # per-frame operators
    cfg = _cfg(scale, sensor, kern)
    sH, sW = round(scale * H), round(scale * W)
    num, den = torch.zeros(sH, sW, 3, device=DEV), torch.zeros(sH, sW, 3, device=DEV)
    for f in frames:
        merge.merge(*(T(a) for a in f), num, den, cfa, cfg)
    _assert_sums(N(num), o["num_c"], scale, what + " per-frame num")
    _assert_sums(N(den), o["den_c"], scale, what + " per-frame den")
    merge.merge_ref(T(ref), T(ref_covs), num, den, cfa, cfg)
    _assert_sums(N(num), o["num"], scale, what + " per-frame + merge_ref num")
    _assert_sums(N(den), o["den"], scale, what + " per-frame + merge_ref den")
    utils.divide(num, den)
    assert_close(N(num), o["out"], *TOL, what + " per-frame + merge_ref + divide")
    if integer:  # frames 0-1 stored as raw sums, frames 2-3 + the reference frame loaded onto them
        tf = [tuple(T(a) for a in f) for f in frames]
        pn, pd = torch.empty(sH, sW, 3, device=DEV), torch.empty(sH, sW, 3, device=DEV)
        acc = torch.zeros(H, W, device=DEV)
        merge.merge_burst(tf[:2], None, None, pn, pd, cfa, cfg, do_ref=False, divide=False, store_den=True, acc_r=acc)
        want_n, want_d = _partial(scale, sensor, kern, 2)
        _assert_sums(N(pn), want_n, scale, what + " split num (2 frames)")
        _assert_sums(N(pd), want_d, scale, what + " split den (2 frames)")
        merge.merge_burst(tf[2:], T(ref), T(ref_covs), pn, pd, cfa, cfg, load_acc=True, acc_r=acc)
        single, _ = _burst(scale, sensor, kern)
        assert_close(N(pn), o["out"], *TOL, what + " split image")
        assert_close(N(pn), single, *TOL, what + " split image vs one launch")
        assert_close(N(acc), acc_want, 1e-6, 1e-6, what + " split accumulated robustness")
    if scale in (1, 4):
        cfg_d = _cfg(scale, sensor, kern)
        cfg_d.accumulated_robustness_denoiser.enabled = True
        cfg_d.accumulated_robustness_denoiser.merge.enabled = True
        acc32 = acc_want.astype(np.float32)  # the same values on both sides (the float32 map HIP accumulates)
        assert 0.05 < (acc32 < cfg_d.accumulated_robustness_denoiser.merge.max_frame_count).mean() < 0.95
        num, den = T(o["num_c"]), T(o["den_c"])
        merge.merge_ref(T(ref), T(ref_covs), num, den, cfa, cfg_d, T(acc32))
        onum, oden = o["num_c"].copy(), o["den_c"].copy()
        cfast.merge_ref(ref, ref_covs, onum, oden, cfa, cfg_d, acc_rob=acc32.astype(np.float64), threads=THREADS)
        assert_close(N(num), onum, *TOL, what + " denoiser merge_ref num")
        assert_close(N(den), oden, *TOL, what + " denoiser merge_ref den")


def _partial(scale, sensor, kern, n):
    """The oracle's raw sums of the first n comp frames (num, den)."""
    ref, ref_covs, frames = _merge_inputs(scale, sensor)
    H, W, _ = SHAPES[scale]
    num = np.zeros((round(scale * H), round(scale * W), 3), np.float32)
    den = np.zeros_like(num)
    for f in frames[:n]:
        cfast.merge(*f, num, den, SENSORS[sensor], _cfg(scale, sensor, kern), threads=THREADS)
    return num, den


def test_merge_x4_more_frames_than_one_launch_holds():
    """x4, 70 frames > HHSR_MAX_FRAMES (64): merge_burst chains a second launch of the tile kernel onto the raw sums of the
    first; image and accumulated robustness against the oracle's 70 frames."""
    H, W, ts, n = 34, 50, 16, 70
    cfg = base_config(ts=ts, scale=4)
    ref, comp, _ = synth.make_burst(H, W, 4, seed=14)
    rng = np.random.default_rng(14)
    covs = [oracle.estimate_kernels(c, cfg) for c in comp]
    frames = [(comp[k % 3], rng.uniform(-1.5, 1.5, (cdiv(H, ts), cdiv(W, ts), 2)).astype(np.float32), covs[k % 3],
               rng.random((H, W), dtype=np.float32)) for k in range(n)]
    assert n > _lib.MAX_FRAMES
    cfa = ((0, 1), (1, 2))
    ref_covs = oracle.estimate_kernels(ref, cfg)
    out, acc = torch.empty(4 * H, 4 * W, 3, device=DEV), torch.zeros(H, W, device=DEV)
    merge.merge_burst([tuple(T(a) for a in f) for f in frames], T(ref), T(ref_covs), out, None, cfa, cfg, acc_r=acc)
    num, den = np.zeros((4 * H, 4 * W, 3), np.float32), np.zeros((4 * H, 4 * W, 3), np.float32)
    for f in frames:
        cfast.merge(*f, num, den, cfa, cfg, threads=THREADS)
    cfast.merge_ref(ref, ref_covs, num, den, cfa, cfg, threads=THREADS)
    with np.errstate(all="ignore"):
        assert_close(N(out), num.astype(np.float64) / den, *TOL, "x4 70-frame burst")
    assert_close(N(acc), _acc_want(frames), 1e-6, 1e-6, "x4 70-frame accumulated robustness")


PLAN_CFAS = {"rggb": [[0, 1], [1, 2]], "bggr": [[2, 1], [1, 0]], "grbg": [[1, 0], [2, 1]], "rbgg": [[0, 2], [1, 1]], "grey": None}
PLAN_SLABS = {1.5: [None], 2: [None, (32, 32), (16, 32)], 3: [None, (48, 48)], 4: [None]}  # of 64 (x2) / 96 (x3) output rows


@pytest.mark.parametrize("W,ts", [(32, 16), (34, 16), (32, 8), (34, 8)])
def test_merge_plan_matches_launch(W, ts):
    """The record of hhsr_merge_plan_query against what the launch does with the same arguments, on real buffers of
    the right sizes: 32 x W raw pixels (two flow tiles per axis at ts 16; W = 34: W % 4 == 2 takes x3 off the x3 kernel),
    2 comp frames, scales 1.5 / 2 / 3 / 4, three Bayer layouts, a non-Bayer one and `mode: grey`, every merge_kernel, the
    whole image and row slabs on and off the x2 / x3 workgroup grids.  A launch with HHSR_MERGE_LOCAL_MIN returns 0 exactly
    where the record's local_min field is 1 and -3 exactly where it is 0 (refusals return before any HIP call); where it
    runs, its image equals robustness.local_min followed by the plain launch, bit for bit.  The first link of
    hhsr_merge_burst_chain likewise against the chain field — with one difference the entry point's own argument check
    makes: for a monochrome sensor or a forced kernel it refuses with -1 ("invalid argument") before it reaches the plan."""
    import ctypes

    H = 32
    lib = _lib.load()
    inputs = {}
    for mode in ("bayer", "grey"):
        cfg = base_config(ts=ts, scale=2, mode=mode)
        ref, fr = merge_frames(H, W, 2, ts, 91, cfg)
        tf = [tuple(T(a) for a in f) for f in fr]
        inputs[mode] = (T(ref), T(oracle.estimate_kernels(ref, cfg)), tf,
                        [(f[0], f[1], f[2], robustness.local_min(f[3])) for f in tf])
    cls = merge.chain_buffer((H, W), torch.device(DEV))
    seen = {"min": set(), "chain": set()}
    for scale, (sensor, cfa), kernel in itertools.product(PLAN_SLABS, PLAN_CFAS.items(), ("auto", "generic", "tile", "x2_v1")):
        mode = "grey" if sensor == "grey" else "bayer"
        cfg = base_config(ts=ts, scale=scale, mode=mode, hip={"merge_kernel": kernel})
        cfa = cfa or [[1, 1], [1, 1]]
        cfg.exif.cfa_pattern = cfa
        ref, ref_covs, tf, tf_min = inputs[mode]
        sH, sW = round(scale * H), round(scale * W)
        fscale, kflags = merge._common(cfg)

        def record(rows, flags):
            rec = (ctypes.c_int32 * _lib.MERGE_PLAN_LEN)()
            assert lib.hhsr_merge_plan_query(2, H, W, ts, _lib.cfa_bytes(cfa), fscale, kflags, flags, sH, sW, *rows, 16, 16,
                                             rec, _lib.MERGE_PLAN_LEN) == 0
            return list(rec)

        for rows in PLAN_SLABS[scale]:
            what = (scale, sensor, kernel, rows)
            row0, nrows = rows or (0, sH)
            rec = record((row0, nrows), _lib.MERGE_DO_REF | _lib.MERGE_DIVIDE)
            assert rec[7] == 0 and row0 % rec[4] == 0, (what, rec)
            assert record((row0, nrows), _lib.MERGE_DO_REF | _lib.MERGE_DIVIDE | _lib.MERGE_LOCAL_MIN)[7] == (0 if rec[2] else -3)
            kw = dict(rows=rows, out_height=sH) if rows else {}
            got = torch.full((nrows, sW, 3), -7.0, device=DEV)
            assert got.data_ptr() % 16 == 0
            seen["min"].add(rec[2])
            if rec[2]:
                merge.merge_burst(tf, ref, ref_covs, got, None, cfa, cfg, local_min=True, **kw)
                want = torch.full_like(got, -7.0)
                merge.merge_burst(tf_min, ref, ref_covs, want, None, cfa, cfg, **kw)
                assert torch.equal(torch.nan_to_num(got, nan=-1.0), torch.nan_to_num(want, nan=-1.0)), what
                assert not (got == -7.0).any(), what
            else:
                with pytest.raises(RuntimeError, match=r"code -3\).*HHSR_MERGE_LOCAL_MIN needs"):
                    merge.merge_burst(tf, ref, ref_covs, got, None, cfa, cfg, local_min=True, **kw)
            if rows is None:
                seen["chain"].add(rec[3])
                assert record((0, sH), _lib.MERGE_STORE_CLASSES)[7] == (0 if rec[3] else -3)
                if rec[3]:
                    merge.merge_burst_chain(tf[:1], 0, None, None, got, cfa, cfg, cls, False)
                else:
                    code = -1 if (mode == "grey" or kernel != "auto") else -3
                    with pytest.raises(RuntimeError, match=rf"code {code}\)"):
                        merge.merge_burst_chain(tf[:1], 0, None, None, got, cfa, cfg, cls, False)
    torch.cuda.synchronize()
    assert seen["min"] == ({0, 1} if ts == 16 else {0}) and seen["chain"] == ({0, 1} if ts == 16 else {0})


# ------------------------------------------------------------------------------------------ alignment
NY, NX = 23, 37  # 851 tiles: 213 workgroups of 4 tiles, 213 % 8 = 5
ALIGN_CASES = ([(ts, r, "L2") for ts in (8, 16, 32) for r in (1, 2, 4)] + [(ts, r, "L1") for ts in (16, 32) for r in (1, 2, 4)]
               + [(16, 1, "L1_ref_effective")])
METRIC_CODE = {"L2": 0, "L1": 1, "L1_ref_effective": 2}


def _align_inputs(ts, r, n_distinct, seed):
    """One reference level of NY x NX tiles and n_distinct moving levels (3 rows / 5 columns smaller, shifted by up to
    3 px) with their incoming flows (bm_inputs' special tiles: half-integer ties, windows leaving the level)."""
    rng = np.random.default_rng(seed)
    h, w = NY * ts, NX * ts
    big = smooth(rng, h + 32, w + 32, 1.5)
    ref = big[16:16 + h, 16:16 + w].copy()
    movs, flows = [], []
    for k in range(n_distinct):
        sy, sx = (int(v) for v in rng.integers(-3, 4, 2))
        mov = big[16 + sy:16 + sy + h - 3, 16 + sx:16 + sx + w - 5].copy()
        mov += 0.01 * rng.standard_normal(mov.shape).astype(np.float32)
        movs.append(mov)
        flow = bm_inputs(rng, ts, r, NY, NX, (0, 0))[2]
        # three search windows entirely outside the moving level: every candidate of a column (L2, clamp to edge) or
        # every candidate (L1, zero outside) costs exactly the same — the first minimum in row-major order must win
        flow[3, 0], flow[9, 0], flow[0, 6] = (-(ts + 20), 0.3), (-(ts + 24), -0.2), (0.2, -(ts + 20))
        flows.append(flow)
    return ref, movs, flows


def _align_oracle(ref, ica_state, mov, flow, ts, r, metric, cfg):
    """oracle.align_lvl of one frame, and the block-matching costs for the near-tie rule (None: no search)."""
    gx, gy, hess = ica_state
    if metric == "L2":
        fbm, cost = oracle.bm_l2(ref, mov, flow, ts, r, return_cost=True)
    elif metric == "L1":
        fbm, cost = oracle.bm_l1(ref, mov, flow, ts, r, return_cost=True)
    else:
        fbm, cost = oracle.bm_l1(ref, mov, flow, ts, r, effective=True), None
    want = oracle.ica(ref, gx, gy, hess, mov, fbm, ts, cfg.ica.tuning.n_iter, ica64_row_bug=cfg.compat.ica64_row_bug)
    return want, cost


def _judge(got, want, cost, what, min_ties=0):
    """Flows within 2e-4 px of the oracle's; a tile beyond that only where its block-matching step sat on a near-tie of
    the two best costs (check_bm: at most one per frame)."""
    if cost is None:  # (no search: nothing can tie)
        assert_close(got, want, 0, 2e-4, what)
        return
    same = np.abs(got - want).max(-1) <= 2e-4
    assert_close(got[same], want[same], 0, 2e-4, what)
    check_bm(got, want, cost, what, atol=2e-4)
    ties = np.sort(cost.reshape(cost.shape[:2] + (-1,)), -1)
    assert (ties[..., 1] == ties[..., 0]).sum() >= min_ties, "the exact ties of the windows outside the level are missing"


def _align_batch(ref, hess, movs, flows_in, ts, r, metric, n_iter, coarse=None):
    """hhsr_align_level_batch over the frames; `coarse` = (coarse flows, rep, mult) or None (incoming flow in place)."""
    rh, rw = ref.shape
    mh, mw = movs[0].shape
    tref, tm = T(ref), [T(m) for m in movs]
    flows = [T(f) for f in flows_in]
    if coarse is None:
        cptr, cny, cnx, rep, mult, tc = None, 0, 0, 0, 1.0, None
    else:
        cf, rep, mult = coarse
        tc = [T(c) for c in cf]
        cptr, (cny, cnx) = _lib.ptr_array(tc), cf[0].shape[:2]
    _lib.call("hhsr_align_level_batch", _lib.ptr(tref), rh, rw, rw, _lib.ptr(hess), _lib.ptr_array(tm), len(tm), mh, mw, mw,
              _lib.ptr_array(flows), NY, NX, ts, r, METRIC_CODE[metric], int(n_iter), cptr, int(cny), int(cnx), int(rep),
              float(mult), _lib.stream())
    return [N(f) for f in flows]


@pytest.mark.parametrize("ts,r,metric", ALIGN_CASES)
def test_align_wave_instantiations_vs_oracle(ts, r, metric):
    """Every k_align_wave<ts, r, L1> instantiation on a 37 x 23 tile grid, 11 moving frames per launch sequence (a full
    batch of HHSR_MAX_BATCH = 8 and a partial one of 3; position 9 repeats frame 0 and must give bit-identical flows); then 3
    frames whose incoming flow is the coarser level's flow read in place (rep 2 and rep 4, a coarse grid that does not
    cover the fine one: zero past it) against oracle.upscale_lvl (nearest) + oracle.align_lvl."""
    cfg = base_config(ts=ts, metrics=(metric,) * 4)
    cfg.block_matching.tuning.tile_sizes = [ts] * 4
    cfg.block_matching.tuning.search_radii = [r] * 4
    n_iter = cfg.ica.tuning.n_iter
    ref, movs, flows = _align_inputs(ts, r, 10, 1000 + 10 * ts + r + METRIC_CODE[metric])
    gx, gy, hess = ICA.init_ica(T(ref), ts)
    ica_state = oracle.init_ica(ref, ts)
    order = list(range(9)) + [0, 9]  # 11 frames, frame 0 again at position 9
    got = _align_batch(ref, hess, [movs[k] for k in order], [flows[k] for k in order], ts, r, metric, n_iter)
    assert np.array_equal(got[0], got[9]), "the same frame in the first and in the partial batch"
    for pos, k in enumerate(order):
        if pos == 9:
            continue
        want, cost = _align_oracle(ref, ica_state, movs[k], flows[k], ts, r, metric, cfg)
        _judge(got[pos], want, cost, f"ts={ts} r={r} {metric} frame {pos}", min_ties=3)
    for rep in (2, 4):
        rng = np.random.default_rng(rep)
        cny, cnx = (NY - 1) // rep, (NX - 1) // rep  # cny * rep < NY: the last tile rows / columns start from zero
        coarse = [rng.uniform(-1.2, 1.2, (cny, cnx, 2)).astype(np.float32) / rep for _ in range(3)]
        cfg_up = base_config(ts=ts, metrics=(metric,) * 4)
        cfg_up.block_matching.tuning.tile_sizes = [ts] * 4
        cfg_up.block_matching.tuning.factors = [1, rep, 2, 2]
        cfg_up.block_matching.tuning.flow_upscale_mode = "nearest"
        got = _align_batch(ref, hess, movs[:3], [np.full((NY, NX, 2), np.nan, np.float32)] * 3, ts, r, metric, n_iter,
                           coarse=(coarse, rep, float(rep)))
        for k in range(3):
            fin = oracle.upscale_lvl(coarse[k], (NY, NX), 0, cfg_up)
            assert (fin[cny * rep:] == 0).all() and np.abs(fin[:cny * rep, :cnx * rep]).max() > 0.4
            want, cost = _align_oracle(ref, ica_state, movs[k], fin, ts, r, metric, cfg)
            _judge(got[k], want, cost, f"ts={ts} r={r} {metric} coarse rep={rep} frame {k}")


@pytest.mark.parametrize("metric", ["L2", "L1"])
def test_align_ts64_separate_kernels_vs_oracle(metric):
    """ts = 64 (no fused kernel): hhsr_bm_* + hhsr_ica through alignment.align_lvl on the same 37 x 23 tile grid."""
    ts, r = 64, 2
    cfg = base_config(ts=ts, metrics=(metric,) * 4)
    cfg.block_matching.tuning.tile_sizes = [ts] * 4
    cfg.block_matching.tuning.search_radii = [r] * 4
    assert alignment._fused_level(0, cfg) is None
    ref, movs, flows = _align_inputs(ts, r, 2 if metric == "L2" else 1, 64 + METRIC_CODE[metric])
    gx, gy, hess = ICA.init_ica(T(ref), ts)
    ica_state = oracle.init_ica(ref, ts)
    for k, (mov, flow) in enumerate(zip(movs, flows)):
        f = T(flow)
        alignment.align_lvl(T(ref), None, None, gx, gy, hess, T(mov), f, 0, cfg)
        want, cost = _align_oracle(ref, ica_state, mov, flow, ts, r, metric, cfg)
        _judge(N(f), want, cost, f"ts=64 {metric} frame {k}", min_ties=3)


# ------------------------------------------------------------------------------------------ grey
# (H, W): the fused FFT kernels decline (a prime factor above 7 in H or W / 2) and the rocFFT plans run
GREY_SIZES = [(3072, 4080), (3648, 5472), (3472, 4624), (323, 646), (342, 476)]
GREY_ALL_PLANS = {(3072, 4080), (323, 646)}  # also the pruned (1) and transposed (2) library plans


@pytest.mark.parametrize("shape", GREY_SIZES)
def test_grey_library_plans_at_non_smooth_sizes(shape, monkeypatch):
    """compute_grey_images (FFT, FFT_torch, FFT_c2c) and compute_grey_images_batch (3 frames) against the float64 oracle at
    sizes whose lengths carry 17, 19 or 31: the default (fused kernels, which decline here) and HHSR_GREY_PLAN 0, and on
    one large and one small size 1 (k_lowpass_scale_pruned) and 2 (k_lowpass_scale_t)."""
    rng = np.random.default_rng(shape[0] + shape[1])
    imgs = [rng.random(shape, dtype=np.float32) for _ in range(3)]
    want = [oracle.grey_fft(i) for i in imgs]
    ti = [T(i) for i in imgs]
    what = f"{shape[0]}x{shape[1]}"
    assert_close(N(utils_image.compute_grey_images(ti[0], "FFT_torch")), want[0], 0, 3e-6, what + " FFT_torch")
    assert_close(N(utils_image.compute_grey_images(ti[0], "FFT_c2c")), want[0], 0, 3e-6, what + " FFT_c2c")
    modes = [None, "0"] + (["1", "2"] if shape in GREY_ALL_PLANS else [])
    for mode in modes:
        if mode is None:
            monkeypatch.delenv("HHSR_GREY_PLAN", raising=False)
        else:
            monkeypatch.setenv("HHSR_GREY_PLAN", mode)
        utils_image._grey_plans.clear()
        tag = f"{what} plan {mode or 'default'}"
        assert_close(N(utils_image.compute_grey_images(ti[0], "FFT")), want[0], 0, 3e-6, tag)
        outs = utils_image.compute_grey_images_batch(ti, "FFT")
        for k in range(3):
            assert_close(N(outs[k]), want[k], 0, 3e-6, f"{tag} batch frame {k}")
    monkeypatch.delenv("HHSR_GREY_PLAN", raising=False)
    utils_image._grey_plans.clear()


# ------------------------------------------------------------------------------------------ robustness
_ROB_CASES = {}


def _rob_case(H, W, ts, seed):
    """One robustness case with its oracle maps, built once per (H, W, ts, seed) and left unchanged by its users."""
    key = (H, W, ts, seed)
    if key not in _ROB_CASES:
        _ROB_CASES[key] = _make_rob_case(H, W, ts, seed)
    return _ROB_CASES[key]


def _make_rob_case(H, W, ts, seed):
    wb = [1.8, 1.0, 1.4]
    cfa = [[1, 0], [2, 1]]
    ref, comp, _ = synth.make_burst(H, W, 3, seed=seed, wb=wb, occluder=True, max_shift=1.5, cfa=((1, 0), (2, 1)))
    cfg = base_config(ts=ts, snr=18.0)
    rng = np.random.default_rng(seed)
    flows = [rng.uniform(-2, 2, (cdiv(H, ts), cdiv(W, ts), 2)).astype(np.float32) for _ in comp]
    std, dif = synth.noise_curves(synth.ALPHA_ISO100, synth.BETA_ISO100)
    om, ov = oracle.init_robustness(ref, cfa, wb, cfg)
    want = [oracle.compute_robustness(c, om, ov, f, cfa, wb, (std, dif), cfg) for c, f in zip(comp, flows)]
    rm, rv = robustness.init_robustness(T(ref), cfa, wb, cfg)
    curves = robustness.noise_curves_to_device(std, dif, DEV)
    return cfg, cfa, wb, comp, flows, want, rm, rv, curves


@pytest.mark.parametrize("H,W,ts,kernel", [(200, 328, 16, "k_rob_frames_row4"), (200, 330, 32, "k_rob_frames_row4_dword"),
                                            (200, 330, 8, "k_rob_frame")])
def test_robustness_kernels_vs_oracle(H, W, ts, kernel):
    """hhsr_rob_frame (one frame) and hhsr_rob_frames choose k_rob_frames_row4<VEC> where ts % 16 == 0 — its 16-byte
    instantiation with W % 4 == 0, the dword one with W = 2 mod 4 — and k_rob_frame everywhere else; each against
    oracle.compute_robustness on a grid with nblk % 8 != 0 (32 x 32-pixel workgroups: 11 x 7 = 77; k_rob_frame's 64 x 4:
    6 x 50 = 300).  k_rob_frame is reached through ts = 8.  A noise curve of more than 1024 entries is not an input the
    Python API accepts (the curves have 1001 entries); the other route to it (no packed curve index) and the other route to
    the dword instantiation (planes that are not 16-byte aligned) are not inputs the Python API produces (torch allocations
    are aligned), but a C client produces them with one pointer offset:
    tests/test_pitched_buffers.py::test_rob_frame_kernels_chosen_by_pointer reaches them through the C ABI."""
    cfg, cfa, wb, comp, flows, want, rm, rv, curves = _rob_case(H, W, ts, 40 + ts)
    assert (ts % 16 == 0) == kernel.startswith("k_rob_frames_row4")
    assert (ts % 16 == 0 and W % 4 != 0) == kernel.endswith("_dword")
    for k, (c, f) in enumerate(zip(comp, flows)):
        r = robustness.compute_robustness(T(c), rm, rv, T(f), cfa, wb, curves, cfg)
        assert_close(N(r), want[k], 0, 1e-4, f"{kernel} (compute_robustness) frame {k}")
    if ts % 16 == 0:  # the grouped entry point, the weights S evaluated inside the kernel in either instantiation
        sig = robustness.noise_sigma_sq(rm, rv, curves[0])
        cms = [robustness.compute_local_stats_from_raw(T(c), cfa, wb, want_vars=False)[0] for c in comp]
        rs = robustness.compute_robustness_group([T(c) for c in comp], rm, [T(f) for f in flows], curves, cfg, sig, cms)
        for k, r in enumerate(rs):
            assert_close(N(r), want[k], 0, 1e-4, f"{kernel} (compute_robustness_group) frame {k}")
    lo = np.mean([(w < 0.5).mean() for w in want])
    assert 0.01 < lo < 0.9, f"inputs do not exercise the robustness ({lo})"


def _bits(a):
    return N(a).view(np.int32)


def test_robustness_entry_points_same_bits():
    """The two promises of include/hhsr.h on the vector route (200 x 328, ts = 16, aligned planes), as equal bits and not
    as a tolerance: hhsr_rob_frames with S given is per frame hhsr_rob_frame, and hhsr_rob_frames with S = NULL (the
    weights evaluated inside the kernel) is hhsr_rob_frames with the maps of hhsr_rob_s."""
    H, W, ts = 200, 328, 16
    cfg, cfa, wb, comp, flows, want, rm, rv, curves = _rob_case(H, W, ts, 56)
    sig2, idx = robustness.noise_sigma_sq(rm, rv, curves[0])
    assert idx is not None
    cms = [robustness.compute_local_stats_from_raw(T(c), cfa, wb, want_vars=False)[0] for c in comp]
    tf = [T(f) for f in flows]
    ny, nx = flows[0].shape[:2]
    t = cfg.robustness.tuning
    S = [robustness.compute_s(f, t.Mt, t.s1, t.s2) for f in tf]
    dif = curves[1]

    def planes():
        return [torch.full((H, W), float("nan"), dtype=torch.float32, device=DEV) for _ in comp]

    def frames(maps):
        Rs = planes()
        _lib.call("hhsr_rob_frames", _lib.ptr_array(cms), len(cms), H // 2, W // 2, _lib.ptr(rm), _lib.ptr(sig2),
                  _lib.ptr(idx), _lib.ptr_array(tf), ny, nx, ts, None if maps is None else _lib.ptr_array(maps), float(t.Mt),
                  float(t.s1), float(t.s2), _lib.ptr(dif), dif.numel(), float(t.t), _lib.ptr_array(Rs), 0, 0, _lib.stream())
        return Rs

    single = planes()
    for k in range(len(cms)):
        _lib.call("hhsr_rob_frame", _lib.ptr(cms[k]), H // 2, W // 2, _lib.ptr(rm), _lib.ptr(sig2), _lib.ptr(idx),
                  _lib.ptr(tf[k]), ny, nx, ts, _lib.ptr(S[k]), _lib.ptr(dif), dif.numel(), float(t.t), _lib.ptr(single[k]),
                  _lib.stream())
    given, inline = frames(S), frames(None)
    torch.cuda.synchronize()
    for k in range(len(cms)):
        assert not np.isnan(N(given[k])).any(), f"frame {k}: pixels left unwritten"
        d = np.abs(N(single[k]) - N(given[k])).max()
        print(f"frame {k}: hhsr_rob_frame vs hhsr_rob_frames max |dR| {d:.3g}; "
              f"S given vs S = NULL max |dR| {np.abs(N(given[k]) - N(inline[k])).max():.3g}")
        assert np.array_equal(_bits(single[k]), _bits(given[k])), f"frame {k}: hhsr_rob_frame != hhsr_rob_frames ({d})"
        assert np.array_equal(_bits(given[k]), _bits(inline[k])), f"frame {k}: S given != S = NULL"
