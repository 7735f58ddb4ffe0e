"""GPU parity tests: every HIP kernel (through the C ABI / the Python operator API) against the CPU
oracle on identical inputs, the committed golden vectors, and end-to-end bursts.

Tolerances (float32 path): integer block-matching flow exact except float32 near-ties;
ICA flow <= 2e-4 px; covariances rel 1e-4; robustness abs 1e-4; accumulators rel 2e-5; final image abs
1e-4 on [0,1] (bulk) with a small allowance for block-matching near-tie outliers end to end."""
import numpy as np
import pytest
import torch

import oracle
from helpers import (flipped_tiles, assert_explained, base_config, acc_pattern, assert_close, smooth, bm_inputs, check_bm,
                     merge_frames)

pytestmark = pytest.mark.gpu

import handheld_super_resolution as hsr  # noqa: E402
from handheld_super_resolution import (utils_image, alignment, block_matching, ICA, kernels, robustness, merge,  # noqa: E402
                                       utils, synthetic as synth)

DEV = "cuda"

# Allowed numbers of tiles (over all comp frames of the test's burst) whose block-matching decision differs from the
# oracle's — float32 near-ties, see helpers.flipped_tiles.  Measured on MI355X: NONE in any of these bursts, at any size
# (PARITY.md; round 1's end-to-end outliers were border pixels with denormal weights, now k_merge_border's) — so the
# budgets are zero and every image / robustness difference has to be within tolerance everywhere.  Should a future
# kernel change flip a near-tie, the footprint rule of helpers.assert_explained keeps the image check meaningful.
FLIP_BUDGET = {"c1": 0, "ts32": 0, "ts64": 0, "ragged2": 0, "ragged1.5": 0, "ragged3": 0, "matrix": 0,
               "c2_full": 0, "c4_crop": 0,
               # L1_ref_effective rounds the incoming level-0 flow (flow <- round_half_even(flow)): a tile whose upscaled
               # level-1 flow lies within float32 ICA noise (1e-6 px) of k + 0.5 rounds the other way — measured: 1 of the
               # 94 000 tile-frames of the 12 MP burst
               "c2_full_eff": 2}


def T(a, dtype=torch.float32):
    return torch.as_tensor(np.ascontiguousarray(a), dtype=dtype, device=DEV)


def N(t):
    return t.detach().cpu().numpy()


# ------------------------------------------------------------------------------------------ grey / pyramid
@pytest.mark.parametrize("shape", [(48, 40), (50, 42), (31, 45), (512, 384), (56, 84), (126, 196), (378, 504)])
def test_grey_fft(shape):
    img = np.random.default_rng(1).random(shape, dtype=np.float32)
    want = oracle.grey_fft(img)
    assert_close(N(utils_image.compute_grey_images(T(img), "FFT")), want, 0, 3e-6, "planned r2c")
    assert_close(N(utils_image.compute_grey_images(T(img), "FFT_torch")), want, 0, 3e-6, "torch r2c")
    assert_close(N(utils_image.compute_grey_images(T(img), "FFT_c2c")), want, 0, 3e-6, "c2c")


def test_grey_fused_vs_library_plans(monkeypatch):
    """The fused in-LDS FFT kernels (default where the sizes factor into 2/3/5) and the rocFFT plans
    (fallback) implement the same low-pass."""
    img = np.random.default_rng(3).random((240, 400), dtype=np.float32)  # 200 = 5*5*4*2, 240 = 5*4*4*3
    want = oracle.grey_fft(img)
    outs = {}
    for mode in ("4", "0"):
        monkeypatch.setenv("HHSR_GREY_PLAN", mode)
        utils_image._grey_plans.clear()
        outs[mode] = N(utils_image.compute_grey_images(T(img), "FFT"))
        assert_close(outs[mode], want, 0, 3e-6, "plan " + mode)
    utils_image._grey_plans.clear()
    assert np.abs(outs["4"] - outs["0"]).max() < 2e-6


def test_grey_fused_one_column_per_workgroup(monkeypatch):
    """Long columns (e.g. 6000 rows at 48 MP) run the column kernel with one column per workgroup; forced here
    on a small image and checked against the two-column schedule and the float64 oracle."""
    img = np.random.default_rng(4).random((240, 400), dtype=np.float32)
    want = oracle.grey_fft(img)
    outs = {}
    for nc in ("2", "1"):
        monkeypatch.setenv("HHSR_FFT_NC", nc)
        utils_image._grey_plans.clear()
        outs[nc] = N(utils_image.compute_grey_images(T(img), "FFT"))
        assert_close(outs[nc], want, 0, 3e-6, "columns per workgroup " + nc)
    utils_image._grey_plans.clear()
    assert np.array_equal(outs["1"], outs["2"])


def test_grey_fused_row_kernel_variants(monkeypatch):
    """Row kernels: one row per 256-thread workgroup where the row fits (the default up to 4000-pixel rows) and row pairs in
    512-thread workgroups (forced here with HHSR_FFT_NT_ROWS=512; long rows) — both against the float64 oracle, on an image
    with the bench's row length, an odd row count (a ragged last row pair) and on a small one."""
    for shape in ((26, 4000), (241, 400), (378, 504)):
        img = np.random.default_rng(6).random(shape, dtype=np.float32)
        want = oracle.grey_fft(img)
        outs = {}
        for nt in ("256", "512"):
            monkeypatch.setenv("HHSR_FFT_NT_ROWS", nt)
            utils_image._grey_plans.clear()
            outs[nt] = N(utils_image.compute_grey_images(T(img), "FFT"))
            assert_close(outs[nt], want, 0, 3e-6, f"{shape} row kernels with {nt} threads")
        assert np.abs(outs["256"] - outs["512"]).max() < 2e-6
    monkeypatch.delenv("HHSR_FFT_NT_ROWS")
    utils_image._grey_plans.clear()


def test_grey_fused_radix7_sensor_size(monkeypatch):
    """4032 x 3024 (the common 12 MP sensor; 2016 = 2^5 3^2 7, 3024 = 2^4 3^3 7) runs on the fused FFT kernels
    (radix 7 / 14 butterflies) and agrees with the library plans."""
    img = torch.rand((3024, 4032), device=DEV, generator=torch.Generator(device=DEV).manual_seed(5))
    outs = {}
    for mode in ("4", "0"):
        monkeypatch.setenv("HHSR_GREY_PLAN", mode)
        utils_image._grey_plans.clear()
        outs[mode] = utils_image.compute_grey_images(img, "FFT").clone()
    utils_image._grey_plans.clear()
    assert float((outs["4"] - outs["0"]).abs().max()) < 3e-6
    # constant image in -> same constant out (DC bin only), any size
    flat = torch.full((3024, 4032), 0.37, device=DEV)
    monkeypatch.setenv("HHSR_GREY_PLAN", "4")
    assert float((utils_image.compute_grey_images(flat, "FFT") - 0.37).abs().max()) < 2e-6
    utils_image._grey_plans.clear()


def test_grey_static_plan_passes_equal_run_time_passes(monkeypatch):
    """The FFT kernels' compile-time plans (csrc/hhsr_fft.hip: SPlan, HHSR_STATIC_ROWS / _COLS — every LDS offset an
    immediate, index arithmetic hoisted out of the row loop) against the run-time passes (HHSR_FFT_STATIC=0) on the same
    tables, for every size with a plan: rows only, columns only, both; single frame and batches; and against the float64
    oracle at the bench's size."""
    gen = torch.Generator(device=DEV).manual_seed(11)
    worst = {}
    for shape, batches in (((3000, 4000), (1, 3, 5)), ((3024, 4032), (1, 2)), ((6000, 8000), (1, 2))):
        imgs = [torch.rand(shape, device=DEV, generator=gen) for _ in range(max(batches))]
        imgs[-1][::2] *= 0.25  # (strong vertical frequencies: rows differ)

        def run(mask, n):
            monkeypatch.setenv("HHSR_FFT_STATIC", str(mask))
            utils_image._grey_plans.clear()
            if n == 1:
                return [utils_image.compute_grey_images(imgs[0], "FFT").clone()]
            return [o.clone() for o in utils_image.compute_grey_images_batch(imgs[:n], "FFT")]

        for n in batches:
            want = run(0, n)
            for mask in (1, 2, 3):
                got = run(mask, n)
                for i in range(n):
                    worst[shape] = max(worst.get(shape, 0.0), float((got[i] - want[i]).abs().max()))
        if shape == (3000, 4000):
            monkeypatch.delenv("HHSR_FFT_STATIC")
            utils_image._grey_plans.clear()
            for i in (0, 4):
                assert_close(N(utils_image.compute_grey_images(imgs[i], "FFT")), oracle.grey_fft(N(imgs[i])), 0, 3e-6, f"static plans {i}")
        del imgs
    utils_image._grey_plans.clear()
    print("static plans vs run-time passes, max abs difference:", worst)
    # (the same operations on the same tables; hipcc contracts other multiply-add pairs: observed ~4e-7)
    assert all(v < 2e-6 for v in worst.values()), worst


def test_grey_golden(golden):
    g = golden("grey")
    for tag in "abc":
        assert_close(N(utils_image.compute_grey_images(T(g["in_" + tag]), "FFT")), g["out_" + tag], 0, 3e-6, tag)
    assert_close(N(utils_image.compute_grey_images(T(g["dec_in"]), "decimating")), g["dec_out"], 0, 1e-7, "dec")


@pytest.mark.parametrize("shape", [(70, 83), (300, 517)])
@pytest.mark.parametrize("f", [2, 4])
def test_downsample(shape, f):
    img = np.random.default_rng(2).random(shape, dtype=np.float32)
    assert_close(N(utils_image.cuda_downsample(T(img), "gaussian", f)), oracle.downsample(img, f), 0, 1e-6, f"f{f}")


def test_pyramid_golden(golden):
    g = golden("downsample")
    pyr = alignment.build_gaussian_pyramid(T(g["img2"]), [1, 2, 4, 2])
    for i in range(4):
        assert_close(N(pyr[3 - i]), g[f"pyr{i}"], 0, 1e-6, f"pyr{i}")


# ------------------------------------------------------------------------------------------ alignment pieces
@pytest.mark.parametrize("ts", [8, 16, 32, 64])
def test_grad_hessian(ts):
    lvl = smooth(np.random.default_rng(3), 3 * 64 + 5, 2 * 64 + 9)
    gx, gy, H = ICA.init_ica(T(lvl), ts)
    ogx, ogy, oH = oracle.init_ica(lvl, ts)
    assert_close(N(gx), ogx, 0, 0, "gx")
    assert_close(N(gy), ogy, 0, 0, "gy")
    assert_close(N(H), oH, 2e-5, 1e-7, "H")


@pytest.mark.parametrize("ts,r", [(8, 4), (16, 4), (16, 1), (32, 4), (64, 4), (16, 9)])
def test_bm_l2(ts, r):
    rng = np.random.default_rng(4 + ts + r)
    ref, mov, flow = bm_inputs(rng, ts, r, 5, 6, (2, -3))
    cfg = base_config(ts=16)
    cfg.block_matching.tuning.tile_sizes = [ts] * 4
    cfg.block_matching.tuning.search_radii = [r] * 4
    f = T(flow)
    block_matching.align_lvl_block_matching_L2(T(ref), None, T(mov), f, 0, cfg)
    want, cost = oracle.bm_l2(ref, mov, flow, ts, r, return_cost=True)
    check_bm(N(f), want, cost, f"bm_l2 ts={ts} r={r}")


def test_bm_l2_accepts_the_reference_tiled_tensor():
    """Upstream callers pass the tiled, zero-padded reference level [ny, nx, ts + 2r, ts + 2r] (block_matching.py:20,
    alignment.py:56-60, 131): same result as with the level itself; a mismatching tensor raises TypeError."""
    ts, r = 16, 4
    rng = np.random.default_rng(3)
    ref, mov, flow = bm_inputs(rng, ts, r, 5, 6, (2, -3))
    cfg = base_config(ts=16)
    cfg.block_matching.tuning.tile_sizes = [ts] * 4
    cfg.block_matching.tuning.search_radii = [r] * 4
    f0, f1 = T(flow), T(flow)
    block_matching.align_lvl_block_matching_L2(T(ref), None, T(mov), f0, 0, cfg)
    tiled = torch.nn.functional.pad(T(ref).unfold(0, ts, ts).unfold(1, ts, ts), (r, r, r, r))
    assert tiled.shape == (5, 6, ts + 2 * r, ts + 2 * r)
    block_matching.align_lvl_block_matching_L2(tiled, None, T(mov), f1, 0, cfg)
    assert torch.equal(f0, f1)
    with pytest.raises(TypeError):
        block_matching.align_lvl_block_matching_L2(tiled[:, :, 1:], None, T(mov), T(flow), 0, cfg)
    with pytest.raises(TypeError):
        block_matching.align_lvl_block_matching_L2(T(ref)[None], None, T(mov), T(flow), 0, cfg)


def test_bm_l2_golden(golden):
    g = golden("bm_l2")
    for tag in ("t16", "t8", "t32"):
        ts, r = (int(v) for v in g[tag + "_ts_r"])
        cfg = base_config(ts=16)
        cfg.block_matching.tuning.tile_sizes = [ts] * 4
        cfg.block_matching.tuning.search_radii = [r] * 4
        f = T(g[tag + "_flow_in"])
        block_matching.align_lvl_block_matching_L2(T(g[tag + "_ref"]), None, T(g[tag + "_mov"]), f, 0, cfg)
        _, cost = oracle.bm_l2(g[tag + "_ref"], g[tag + "_mov"], g[tag + "_flow_in"], ts, r, return_cost=True)
        check_bm(N(f), g[tag + "_flow_out"], cost, "golden " + tag)


@pytest.mark.parametrize("ts,r", [(16, 1), (16, 4), (32, 2), (64, 1)])
def test_bm_l1(ts, r):
    rng = np.random.default_rng(40 + ts + r)
    ref, mov, flow = bm_inputs(rng, ts, r, 4, 5, (1, -1))
    cfg = base_config(ts=16)
    cfg.block_matching.tuning.tile_sizes = [ts] * 4
    cfg.block_matching.tuning.search_radii = [r] * 4
    f = T(flow)
    block_matching.align_lvl_block_matching_L1(T(ref), T(mov), f, 0, cfg)
    want, cost = oracle.bm_l1(ref, mov, flow, ts, r, return_cost=True)
    check_bm(N(f), want, cost, f"bm_l1 ts={ts} r={r}")
    f = T(flow)
    block_matching.align_lvl_block_matching_L1(T(ref), T(mov), f, 0, cfg, effective=True)
    assert_close(N(f), oracle.bm_l1(ref, mov, flow, ts, r, effective=True), 0, 0, "L1 effective")


def test_bm_errors():
    cfg = base_config(ts=16)
    cfg.block_matching.tuning.tile_sizes = [8] * 4
    z = torch.zeros(16, 16, device=DEV)
    with pytest.raises(NotImplementedError):
        block_matching.align_lvl_block_matching_L1(z, z, torch.zeros(2, 2, 2, device=DEV), 0, cfg)
    cfg.block_matching.tuning.tile_sizes = [12] * 4
    with pytest.raises(NotImplementedError):
        block_matching.align_lvl_block_matching_L2(z, None, z, torch.zeros(1, 1, 2, device=DEV), 0, cfg)
    with pytest.raises(NotImplementedError):
        ICA.align_lvl_ica(z, z, z, torch.zeros(1, 1, 2, 2, device=DEV), z, torch.zeros(1, 1, 2, device=DEV), 0, cfg)


@pytest.mark.parametrize("ts", [8, 16, 32, 64])
@pytest.mark.parametrize("bug", [True, False])
def test_ica(golden, ts, bug):
    g = golden("ica")
    ref, mov, flow0 = g[f"t{ts}_ref"], g[f"t{ts}_mov"], g[f"t{ts}_flow_in"]
    cfg = base_config(ts=16)
    cfg.block_matching.tuning.tile_sizes = [ts] * 4
    cfg.compat.ica64_row_bug = bug
    gx, gy, H = ICA.init_ica(T(ref), ts)
    f = T(flow0)
    ICA.align_lvl_ica(T(ref), gx, gy, H, T(mov), f, 0, cfg)
    ogx, ogy, oH = oracle.init_ica(ref, ts)
    want = oracle.ica(ref, ogx, ogy, oH, mov, flow0, ts, 3, ica64_row_bug=bug)
    assert_close(N(f), want, 0, 2e-4, f"ica ts={ts}")
    if bug:  # and against the reference's own output
        assert_close(N(f), g[f"t{ts}_flow_out"], 0, 2e-4, f"ica golden ts={ts}")


def test_ica_singular_tile_untouched():
    ts = 16
    ref = np.zeros((32, 32), np.float32)  # zero gradients -> det = 0
    mov = np.random.default_rng(5).random((32, 32), dtype=np.float32)
    cfg = base_config(ts=16)
    gx, gy, H = ICA.init_ica(T(ref), ts)
    f0 = np.full((2, 2, 2), 0.37, np.float32)
    f = T(f0)
    ICA.align_lvl_ica(T(ref), gx, gy, H, T(mov), f, 0, cfg)
    assert_close(N(f), f0, 0, 0, "singular")


@pytest.mark.parametrize("ts,r,metric", [(8, 4, "L2"), (16, 4, "L2"), (16, 1, "L1"), (32, 4, "L2"), (32, 2, "L1"),
                                         (16, 1, "L1_ref_effective")])
def test_fused_align_level(ts, r, metric):
    """hhsr_align_level == hhsr_bm_* followed by hhsr_ica (and == the oracle), incl. border tiles."""
    rng = np.random.default_rng(100 + ts + r)
    ny, nx = 5, 6
    ref, mov, flow = bm_inputs(rng, ts, r, ny, nx, (1, -2))
    cfg = base_config(ts=16, metrics=(metric,) * 4)
    cfg.block_matching.tuning.tile_sizes = [ts] * 4
    cfg.block_matching.tuning.search_radii = [r] * 4
    gx, gy, H = ICA.init_ica(T(ref), ts)
    f_fused = T(flow)
    alignment.align_lvl(T(ref), None, None, gx, gy, H, T(mov), f_fused, 0, cfg)
    cfg.hip = {"fused_align": False}
    f_sep = T(flow)
    alignment.align_lvl(T(ref), None, None, gx, gy, H, T(mov), f_sep, 0, cfg)
    assert_close(N(f_fused), N(f_sep), 0, 2e-5, f"fused vs separate ts={ts} {metric}")
    ogx, ogy, oH = oracle.init_ica(ref, ts)
    want = oracle.align_lvl(ref, ogx, ogy, oH, mov, flow, 0, cfg)
    # a tile may differ from the oracle only when its block-matching step sat on a near-tie of the two best costs
    if metric == "L1_ref_effective":
        assert_close(N(f_fused), want, 0, 2e-4, f"fused vs oracle ts={ts} {metric}")
    else:
        _, cost = (oracle.bm_l2 if metric == "L2" else oracle.bm_l1)(ref, mov, flow, ts, r, return_cost=True)
        check_bm(N(f_fused), want, cost, f"fused vs oracle ts={ts} {metric}", atol=2e-4)


@pytest.mark.parametrize("mode", ["nearest", "bilinear", "bicubic"])
def test_upscale(golden, mode):
    g = golden("upscale")
    cfg = base_config(ts=16)
    cfg.block_matching.tuning.flow_upscale_mode = mode
    tol = 0 if mode == "nearest" else 2e-6
    assert_close(N(alignment.upscale_lvl(T(g["flow"]), (11, 15), 2, cfg)), g[mode + "_l2"], tol, tol, mode + " l2")
    assert_close(N(alignment.upscale_lvl(T(g["flow"]), (21, 29), 1, cfg)), g[mode + "_l1"], tol, tol, mode + " l1")


def test_align_fused_upscale_equals_separate_launches():
    """align(): the level kernel taking its incoming flow from the coarser level (fused nearest-neighbour
    upscaling, zero start) == separate memset / hhsr_flow_upscale_nearest launches == two-kernel levels."""
    ref, comp, _ = synth.make_burst(200, 264, 2, seed=21)
    cfg = base_config(ts=16)
    cfg.block_matching.tuning.factors = [1, 2, 2, 2]
    grey_r, grey_c = utils_image.compute_grey_images(T(ref), "FFT"), utils_image.compute_grey_images(T(comp[0]), "FFT")
    state = alignment.init_alignment(grey_r, cfg)
    f_fused = N(alignment.align(*state, grey_c, cfg))
    cfg.hip = {"fused_align": False}
    f_sep = N(alignment.align(*state, grey_c, cfg))
    assert_close(f_fused, f_sep, 0, 2e-5, "fused upscaling vs separate launches")
    assert np.abs(f_fused).max() > 0.5  # the burst really moves


# ------------------------------------------------------------------------------------------ kernels
def test_frame_stats_equals_separate_passes():
    """hhsr_frame_stats (one raw pass) == hhsr_rob_stats + hhsr_cov_from_raw, bit for bit."""
    ref, _, _ = synth.make_burst(134, 202, 1, seed=8)
    cfg = base_config(snr=12.0, ts=16)
    cfa, wb = [[2, 1], [1, 0]], [1.9, 1.0, 1.6]
    m, v, c = kernels.frame_stats(T(ref), cfa, wb, cfg, want_vars=True)
    m2, v2 = robustness.compute_local_stats_from_raw(T(ref), cfa, wb)
    c2 = kernels.estimate_kernels(T(ref), cfg)
    assert_close(N(m), N(m2), 0, 0, "fused means")
    assert_close(N(v), N(v2), 0, 0, "fused vars")
    assert_close(N(c), N(c2), 0, 0, "fused covs")
    m3, v3, _ = kernels.frame_stats(T(ref), cfa, wb, cfg)
    assert v3 is None
    assert_close(N(m3), N(m2), 0, 0, "means without vars")
    om, ov = oracle.local_stats(oracle.guide_image(ref, cfa, wb))
    assert_close(N(m), om, 1e-6, 1e-7, "means vs oracle")
    assert_close(N(v), ov, 1e-5, 1e-7, "vars vs oracle")


@pytest.mark.parametrize("law", ["linear", "hard_threshold"])
def test_cov_golden(golden, law):
    g = golden("kernels")
    cfg = base_config()
    cfg.merging.selection_law = law
    covs = N(kernels.estimate_kernels(T(g["raw"]), cfg))
    assert_close(covs, g["cov_" + law], 1e-4, 1e-6, "cov golden " + law)
    assert_close(covs, oracle.estimate_kernels(g["raw"], cfg), 1e-4, 1e-6, "cov oracle " + law)


def test_cov_random_and_constant():
    rng = np.random.default_rng(6)
    ref, _, _ = synth.make_burst(130, 198, 1, seed=5)
    ref[40:60, 50:90] = 0.3  # constant block -> NaN covariances (linear law, D10)
    cfg = base_config(snr=12.0, ts=16)
    covs = N(kernels.estimate_kernels(T(ref), cfg))
    want = oracle.estimate_kernels(ref, cfg)
    assert np.isnan(want).any()
    assert_close(covs, want, 1e-4, 1e-6, "cov")
    cfg.merging.selection_law = "nope"
    with pytest.raises(ValueError):
        kernels.estimate_kernels(T(ref), cfg)


# ------------------------------------------------------------------------------------------ robustness
def test_robustness_golden(golden):
    g = golden("robustness")
    cfa, wb = g["cfa"].tolist(), g["wb"].tolist()
    cfg = base_config(ts=16)
    m, v = robustness.compute_local_stats_from_raw(T(g["ref"]), cfa, wb)
    assert_close(N(m), g["gmeans"], 1e-6, 1e-8, "guide means")
    assert_close(N(v), g["gvars"], 1e-4, 1e-9, "guide vars")
    rm, rv = robustness.init_robustness(T(g["ref"]), cfa, wb, cfg)
    assert_close(N(rm), g["ref_means"], 1e-6, 1e-8, "ref means")
    assert_close(N(rv), g["ref_vars"], 1e-4, 1e-9, "ref vars")
    curves = robustness.noise_curves_to_device(g["std_curve"], g["diff_curve"], DEV)
    flow = T(g["flow"])
    assert_close(N(robustness.compute_s(flow, 0.8, 2, 12)), g["S"], 0, 0, "S")
    cm, _ = robustness.compute_local_stats_from_raw(T(g["comp"]), cfa, wb)
    assert_close(N(robustness.upscale_warp_stats(cm, 16, flow)), g["comp_means_up"], 1e-6, 1e-8, "warped")
    r, R = robustness.compute_robustness(T(g["comp"]), T(g["ref_means"]), T(g["ref_vars"]), flow, cfa, wb, curves, cfg,
                                         return_R=True)
    assert_close(N(R), g["R"], 0, 1e-4, "R")
    assert_close(N(r), g["r"], 0, 1e-4, "r")
    assert (N(r)[:3] == 0).all() and (N(r)[:, :3] == 0).all()  # D6
    cfg.robustness.enabled = False
    cfg.robustness.save_mask = False
    ones = robustness.compute_robustness(T(g["comp"]), None, None, flow, cfa, wb, curves, cfg)
    assert (N(ones) == 1).all()


def test_ref_planes_equal_separate_kernels():
    """hhsr_ref_planes == hhsr_rob_upscale x 2 + hhsr_rob_sigma, bit for bit (incl. the D6 +inf border and a size
    that is not a multiple of the 32-pixel tile)."""
    ref, _, _ = synth.make_burst(138, 202, 1, seed=9)
    cfa, wb = [[0, 1], [1, 2]], [1.7, 1.0, 1.3]
    m, v = robustness.compute_local_stats_from_raw(T(ref), cfa, wb)
    std, _ = robustness.noise_curves_to_device(*synth.noise_curves(synth.ALPHA_ISO100, synth.BETA_ISO100), DEV)
    means, (sig, idx) = robustness.ref_planes(m, v, std)
    means2, vars2 = robustness.upscale_warp_stats(m), robustness.upscale_warp_stats(v)
    sig2, idx2 = robustness.noise_sigma_sq(means2, vars2, std)
    assert_close(N(means), N(means2), 0, 0, "ref means")
    assert_close(N(sig), N(sig2), 0, 0, "sigma^2")
    assert np.array_equal(N(idx), N(idx2))
    assert np.isinf(N(means)[:, 0, :]).all() and np.isinf(N(means)[:, :, 0]).all()  # D6


def test_robustness_random():
    rng = np.random.default_rng(7)
    H, W, ts = 96, 144, 32
    wb = [1.8, 1.0, 1.4]
    ref, comp, _ = synth.make_burst(H, W, 2, seed=21, wb=wb, occluder=True, max_shift=1.5)
    cfa = [[1, 0], [2, 1]]  # GRBG
    cfg = base_config(ts=ts, snr=18.0)
    std, dif = synth.noise_curves(helpers_alpha(), helpers_beta())
    flow = rng.uniform(-2, 2, ((H + ts - 1) // ts, (W + ts - 1) // ts, 2)).astype(np.float32)
    om, ov = oracle.init_robustness(ref, cfa, wb, cfg)
    want = oracle.compute_robustness(comp[0], om, ov, flow, cfa, wb, (std, dif), cfg)
    rm, rv = robustness.init_robustness(T(ref), cfa, wb, cfg)
    curves = robustness.noise_curves_to_device(std, dif, DEV)
    r = robustness.compute_robustness(T(comp[0]), rm, rv, T(flow), cfa, wb, curves, cfg)
    assert_close(N(r), want, 0, 1e-4, "r", max_bad_frac=1e-3)


def helpers_alpha():
    return synth.ALPHA_ISO100


def helpers_beta():
    return synth.BETA_ISO100


# ------------------------------------------------------------------------------------------ merge
@pytest.mark.parametrize("tag,scale,kern,do_ref", [("s2", 2, "steerable", True), ("s15", 1.5, "steerable", True),
                                                   ("s1", 1, "steerable", True), ("s3", 3, "steerable", False),
                                                   ("s2iso", 2, "iso", True)])
@pytest.mark.parametrize("f64", [False, True])
def test_merge_golden(golden, tag, scale, kern, do_ref, f64):
    g = golden("merge")
    H, W = g["comp"].shape
    cfg = base_config(ts=16, scale=scale)
    cfg.hip = {"weight_fp64": f64}  # True: the reference's float64 weight typing; False: default fast path
    cfg.merging.kernel = kern
    oh, ow = round(scale * H), round(scale * W)
    num, den = T(acc_pattern(oh, ow, 0)), T(acc_pattern(oh, ow, 5))
    merge.merge(T(g["comp"]), T(g["flow"]), T(g["covs"]), T(g["r"]), num, den, g["cfa"].tolist(), cfg)
    assert_close(N(num), g[tag + "_num"], 2e-5, 1e-6, tag + " num")
    assert_close(N(den), g[tag + "_den"], 2e-5, 1e-6, tag + " den")
    if do_ref:
        num, den = T(acc_pattern(oh, ow, 0)), T(acc_pattern(oh, ow, 5))
        merge.merge_ref(T(g["ref"]), T(g["covs_ref"]), num, den, g["cfa"].tolist(), cfg)
        assert_close(N(num), g[tag + "_numref"], 2e-5, 1e-6, tag + " numref")
        assert_close(N(den), g[tag + "_denref"], 2e-5, 1e-6, tag + " denref")


def test_rob_sum_kernel_and_fused_denoiser_path():
    """hhsr_rob_sum (the float64 accumulated robustness of several frames in one pass, with the float32 decision map) against
    torch's float64 sum and RobustnessSum.decisions_of, values on both sides of the threshold within float32 rounding; and
    main() with the accumulated-robustness merge denoiser at x2 and x3 (the fused comp merge + merge_ref + divide path of
    round 6) against the sequential operator path (config.hip.fused_merge = False: merge() frame by frame): identical images
    and identical accumulated robustness."""
    from handheld_super_resolution.robustness import RobustnessSum

    gen = torch.Generator(device=DEV).manual_seed(3)
    H, W, n = 96, 130, 5
    rs = [torch.rand((H, W), device=DEV, generator=gen) for _ in range(n)]
    rs[0][:8] = 1.0
    rs[1][:8] = 1.0
    rs[2][:8] = float(np.nextafter(np.float32(1.0), np.float32(0.0)))  # 1 + 1 + 0.99999994: 3 in float32, not in float64
    rs[3][:8] = 0.0
    rs[4][:8] = 0.0
    acc = RobustnessSum((H, W), torch.device(DEV)).add_many(rs)
    want = torch.zeros((H, W), dtype=torch.float64, device=DEV)
    for r in rs:
        want += r
    assert torch.equal(acc.sum, want)
    acc2 = RobustnessSum((H, W), torch.device(DEV)).add_many(rs[:2]).add_many(rs[2:])  # chained calls (load)
    assert torch.equal(acc2.sum, want)
    for mfc in (3.0, 2.0, 2.5, 3.0000001):
        assert torch.equal(acc.for_decisions(mfc), RobustnessSum.decisions_of(want, mfc)), mfc
        a = acc.for_decisions(mfc).double()
        assert torch.equal(a <= mfc, want <= mfc) and torch.equal(a < mfc, want < mfc), mfc
    assert float(want[0, 0]) < 3.0 and float(want[0, 0].float()) == 3.0  # the case the float32 sum decides differently
    # HHSR_ROB_SUM_MIN5: un-filtered maps in, the 5x5 clamp-border minimum taken on the way into the sum == local_min() per
    # frame, then the sum — bit for bit, also chained (load) and on a map that is not a multiple of the kernel's 64 x 16 tiles
    from handheld_super_resolution.robustness import local_min

    want_min = torch.zeros((H, W), dtype=torch.float64, device=DEV)
    for r in rs:
        want_min += local_min(r)
    acc3 = RobustnessSum((H, W), torch.device(DEV)).add_many(rs, unfiltered=True)
    assert torch.equal(acc3.sum, want_min)
    acc4 = RobustnessSum((H, W), torch.device(DEV)).add_many(rs[:3], unfiltered=True).add_many(rs[3:], unfiltered=True)
    assert torch.equal(acc4.sum, want_min)
    assert torch.equal(acc3.for_decisions(2.0), RobustnessSum.decisions_of(want_min, 2.0))

    for scale, shape in ((2, (640, 704)), (3, (592, 640))):
        ref, comp, _ = synth.make_burst(*shape, 4, seed=21 + scale, max_shift=2.0, occluder=True)

        def cfg_fn(**hip):
            cfg = base_config(ts=16, scale=scale)
            cfg.robustness.save_mask = True
            cfg.accumulated_robustness_denoiser.enabled = True
            cfg.accumulated_robustness_denoiser.merge.enabled = True
            if hip:
                cfg.hip = hip
            return cfg

        out_f, dbg_f = hsr.main(ref, comp, cfg_fn())
        out_s, dbg_s = hsr.main(ref, comp, cfg_fn(fused_merge=False))
        assert torch.equal(dbg_f["accumulated robustness"], dbg_s["accumulated robustness"])
        same = (out_f == out_s) | (out_f.isnan() & out_s.isnan())
        worst = float(torch.nan_to_num(out_f - out_s, nan=0.0).abs().max())
        # (the fused kernels sum the comp frames in the order merge() does; the float32-weight kernels differ from the per-frame
        # operator kernels' float64 weight chain by rounding: 2e-5 relative like test_merge_golden)
        assert bool(same.all()) or worst <= 2e-5, (scale, worst)


def test_merge_ref_denoiser_golden(golden):
    g = golden("merge")
    H, W = g["ref"].shape
    cfg = base_config(ts=16, scale=2)
    cfg.accumulated_robustness_denoiser.enabled = True
    cfg.accumulated_robustness_denoiser.merge.enabled = True
    num, den = T(acc_pattern(2 * H, 2 * W, 0)), T(acc_pattern(2 * H, 2 * W, 5))
    merge.merge_ref(T(g["ref"]), T(g["covs_ref"]), num, den, g["cfa"].tolist(), cfg, T(g["acc_rob"]))
    assert_close(N(num), g["den_numref"], 2e-5, 1e-6, "denoiser numref")
    assert_close(N(den), g["den_denref"], 2e-5, 1e-6, "denoiser denref")
    # HHSR_REF_DIVIDE: reference frame + normalisation in one pass == merge_ref, then divide (bit for bit; den untouched)
    for use_den in (True, False):
        c2 = cfg if use_den else base_config(ts=16, scale=2)
        acc = T(g["acc_rob"]) if use_den else None
        n1, d1 = T(acc_pattern(2 * H, 2 * W, 0)), T(acc_pattern(2 * H, 2 * W, 5))
        merge.merge_ref(T(g["ref"]), T(g["covs_ref"]), n1, d1, g["cfa"].tolist(), c2, acc)
        utils.divide(n1, d1)
        n2, d2 = T(acc_pattern(2 * H, 2 * W, 0)), T(acc_pattern(2 * H, 2 * W, 5))
        merge.merge_ref(T(g["ref"]), T(g["covs_ref"]), n2, d2, g["cfa"].tolist(), c2, acc, divide=True)
        assert torch.equal(n1.isnan(), n2.isnan()) and torch.equal(torch.nan_to_num(n1), torch.nan_to_num(n2)), use_den
        assert torch.equal(d2, T(acc_pattern(2 * H, 2 * W, 5))), use_den
        # HHSR_REF_FAST: float32 weights where the denoiser does not widen (the fused merge's reference-frame arithmetic)
        n3, d3 = T(acc_pattern(2 * H, 2 * W, 0)), T(acc_pattern(2 * H, 2 * W, 5))
        merge.merge_ref(T(g["ref"]), T(g["covs_ref"]), n3, d3, g["cfa"].tolist(), c2, acc, fast=True)
        tag = "den_" if use_den else "s2_"
        assert_close(N(n3), g[tag + "numref"], 2e-5, 1e-6, "fast numref")
        assert_close(N(d3), g[tag + "denref"], 2e-5, 1e-6, "fast denref")


@pytest.mark.parametrize("kern", ["handheld", "iso"])
def test_merge_x2_kernels_equal_tile_kernel(kern):
    """scale 2: the first-generation one-thread-per-LR-pixel kernel == the 16x16 HR tile kernel bit for bit; the
    wave-per-parity-class kernel k_merge_x2 (uniform geometry, weighted covariance blend, single v_exp_f32) to 2e-5
    relative — including the fused accumulated robustness, partial (chained) launches, a frame pushed partly out of
    the image and an image that is not a tile multiple (general per-pixel body inside k_merge_x2)."""
    H, W, ts = 72, 104, 16
    ref, fr = merge_frames(H, W, 4, ts, 77, base_config(ts=ts, scale=2))
    fr[1] = (fr[1][0], fr[1][1] + 9.5, fr[1][2], fr[1][3])  # a frame pushed partly out of the image
    cfa = [[2, 1], [1, 0]]
    tf = [tuple(T(a) for a in f) for f in fr]

    def cfg_for(which):
        c = base_config(ts=ts, scale=2)
        c.merging.kernel = kern
        c.hip = {"merge_kernel": which}
        return c

    rc = T(oracle.estimate_kernels(ref, cfg_for("auto")))

    def run(which, chained=True):
        cfg = cfg_for(which)
        out, den = torch.empty(2 * H, 2 * W, 3, device=DEV), torch.empty(2 * H, 2 * W, 3, device=DEV)
        acc = torch.zeros(H, W, device=DEV)
        if chained:
            merge.merge_burst(tf[:2], None, None, out, den, cfa, cfg, do_ref=False, divide=False, store_den=True, acc_r=acc)
            merge.merge_burst(tf[2:], T(ref), rc, out, den, cfa, cfg, load_acc=True, acc_r=acc)
        else:
            merge.merge_burst(tf, T(ref), rc, out, None, cfa, cfg, acc_r=acc)
        return N(out), N(acc)

    out_t, acc_t = run("tile")
    out_q, acc_q = run("x2_v1")
    assert_close(out_q, out_t, 0, 0, "x2_v1 vs tile kernel")
    assert_close(acc_q, acc_t, 0, 0, "x2_v1 vs tile accumulated robustness")
    assert_close(acc_q, sum(f[3] for f in fr), 1e-6, 1e-6, "accumulated robustness")
    for chained in (True, False):
        out_x, acc_x = run("auto", chained)
        assert_close(out_x, out_t, 2e-5, 1e-6, f"k_merge_x2 vs tile kernel (chained={chained})")
        if chained:  # same association (r0 + r1) + (r2 + r3)
            assert_close(acc_x, acc_t, 0, 0, "k_merge_x2 vs tile accumulated robustness")
        else:
            assert_close(acc_x, acc_t, 1e-6, 1e-6, "k_merge_x2 accumulated robustness, one launch")
    # num / den partial sums of the vectorised store path (multi-GPU ranks)
    cfg = cfg_for("auto")
    pn, pd = torch.empty(2 * H, 2 * W, 3, device=DEV), torch.empty(2 * H, 2 * W, 3, device=DEV)
    merge.merge_burst(tf, None, None, pn, pd, cfa, cfg, do_ref=False, divide=False, store_den=True)
    tn, td = torch.empty_like(pn), torch.empty_like(pd)
    merge.merge_burst(tf, None, None, tn, td, cfa, cfg_for("tile"), do_ref=False, divide=False, store_den=True)
    assert_close(N(pn), N(tn), 2e-5, 1e-7, "partial num")
    assert_close(N(pd), N(td), 2e-5, 1e-7, "partial den")
    # 5x5 local minimum of the robustness taken inside the merge == hhsr_local_min5 followed by the merge
    for which in ("auto", "x2_v1"):
        cfg = cfg_for(which)
        assert merge.can_fuse_local_min(cfg, (H, W))
        tf_min = [(f[0], f[1], f[2], robustness.local_min(f[3])) for f in tf]
        want, acc_w = torch.empty(2 * H, 2 * W, 3, device=DEV), torch.zeros(H, W, device=DEV)
        merge.merge_burst(tf_min, T(ref), rc, want, None, cfa, cfg, acc_r=acc_w)
        got, acc_g = torch.empty(2 * H, 2 * W, 3, device=DEV), torch.zeros(H, W, device=DEV)
        merge.merge_burst(tf, T(ref), rc, got, None, cfa, cfg, acc_r=acc_g, local_min=True)
        assert_close(N(got), N(want), 0, 0, f"fused local minimum ({which})")
        assert_close(N(acc_g), N(acc_w), 0, 0, f"fused local minimum, accumulated robustness ({which})")
    assert not merge.can_fuse_local_min(cfg_for("tile"), (H, W))
    cfg5 = base_config(ts=ts, scale=5)  # x2 and x3 have kernels that take the minimum themselves; other scales do not
    assert not merge.can_fuse_local_min(cfg5, (H, W))
    with pytest.raises(RuntimeError):
        merge.merge_burst(tf, T(ref), rc, torch.empty(5 * H, 5 * W, 3, device=DEV), None, cfa, cfg5, local_min=True)


@pytest.mark.parametrize("kern", ["handheld", "iso"])
def test_merge_x3_kernel_equals_tile_kernel(kern):
    """scale 3: the wave-per-parity-class kernel generalised to 3 x 3 sub-pixels (k_merge_xs<3>: uniform float64 geometry
    per frame, per-thread float32 reference-frame positions) against the 16 x 16 HR tile kernel (float64 geometry per
    pixel), 2e-5 relative — fused accumulated robustness, chained launches, a frame pushed partly out of the image, an
    image that is not a tile multiple (generic per-pixel path inside k_merge_xs), fused local minimum, row slabs."""
    H, W, ts = 80, 112, 16
    ref, fr = merge_frames(H, W, 4, ts, 78, base_config(ts=ts, scale=3))
    fr[1] = (fr[1][0], fr[1][1] + 9.5, fr[1][2], fr[1][3])
    fr[2] = (fr[2][0], (fr[2][1] - 0.1).astype(np.float32), fr[2][2], fr[2][3])  # small negative flows too
    cfa = [[2, 1], [1, 0]]
    tf = [tuple(T(a) for a in f) for f in fr]

    def cfg_for(which):
        c = base_config(ts=ts, scale=3)
        c.merging.kernel = kern
        c.hip = {"merge_kernel": which}
        return c

    rc = T(oracle.estimate_kernels(ref, cfg_for("auto")))

    def run(which, chained, lmin=False):
        cfg = cfg_for(which)
        frames = tf if not lmin or which == "auto" else [(f[0], f[1], f[2], robustness.local_min(f[3])) for f in tf]
        out, den = torch.empty(3 * H, 3 * W, 3, device=DEV), torch.empty(3 * H, 3 * W, 3, device=DEV)
        acc = torch.zeros(H, W, device=DEV)
        kw = dict(local_min=lmin and which == "auto")
        if chained:
            merge.merge_burst(frames[:2], None, None, out, den, cfa, cfg, do_ref=False, divide=False, store_den=True, acc_r=acc, **kw)
            merge.merge_burst(frames[2:], T(ref), rc, out, den, cfa, cfg, load_acc=True, acc_r=acc, **kw)
        else:
            merge.merge_burst(frames, T(ref), rc, out, None, cfa, cfg, acc_r=acc, **kw)
        return N(out), N(acc)

    for chained in (False, True):
        for lmin in (False, True):
            out_t, acc_t = run("tile", chained, lmin)
            out_x, acc_x = run("auto", chained, lmin)
            assert_close(out_x, out_t, 2e-5, 1e-6, f"k_merge_xs<3> vs tile kernel (chained={chained}, lmin={lmin})")
            assert_close(acc_x, acc_t, 1e-6, 1e-6, f"accumulated robustness (chained={chained}, lmin={lmin})")
    # partial sums (num, den) and a row slab
    cfg = cfg_for("auto")
    pn, pd = torch.empty(3 * H, 3 * W, 3, device=DEV), torch.empty(3 * H, 3 * W, 3, device=DEV)
    merge.merge_burst(tf, None, None, pn, pd, cfa, cfg, do_ref=False, divide=False, store_den=True)
    tn, td = torch.empty_like(pn), torch.empty_like(pd)
    merge.merge_burst(tf, None, None, tn, td, cfa, cfg_for("tile"), do_ref=False, divide=False, store_den=True)
    # (4e-5: the frames whose window leaves the image — here the one pushed out by 9.5 px and the small negative flows
    # at column 0 — run the uniform code with border masks since round 4, a different float32 evaluation order than the
    # tile kernel's per-pixel border code; measured 2.9e-5 at one of 241 920 values, everything else <= 2e-5)
    assert_close(N(pn), N(tn), 4e-5, 1e-7, "partial num")
    assert_close(N(pd), N(td), 4e-5, 1e-7, "partial den")
    whole = torch.empty(3 * H, 3 * W, 3, device=DEV)
    merge.merge_burst(tf, T(ref), rc, whole, None, cfa, cfg)
    slab = torch.empty(96, 3 * W, 3, device=DEV)
    merge.merge_burst(tf, T(ref), rc, slab, None, cfa, cfg, rows=(48, 96), out_height=3 * H)
    assert torch.equal(torch.nan_to_num(slab, nan=-1.0), torch.nan_to_num(whole[48:144], nan=-1.0))
    assert merge.can_fuse_local_min(cfg_for("auto"), (H, W)) and not merge.can_fuse_local_min(cfg_for("tile"), (H, W))


def test_merge_border_bands_float64_chain():
    """The border bands (reference window centred on the outermost raw row / column) are computed with the reference's
    float64 weight chain by k_merge_border: identical to the float64 validation mode there, for every float32 kernel,
    with and without the fused local minimum — a colour whose only samples have denormal weights is num / den of two
    denormals in the reference (merge.py:419-434), not 0 / 0."""
    H, W, ts = 64, 80, 16
    for scale in (2, 3, 1.5):
        c64 = base_config(ts=ts, scale=scale)
        c64.hip = {"weight_fp64": True}
        ref, fr = merge_frames(H, W, 3, ts, 5, c64)
        tf = [tuple(T(a) for a in f) for f in fr]
        rc = T(oracle.estimate_kernels(ref, c64))
        sH, sW = round(scale * H), round(scale * W)
        want = torch.empty(sH, sW, 3, device=DEV)
        merge.merge_burst(tf, T(ref), rc, want, None, [[0, 1], [1, 2]], c64)
        want = N(want)
        band = np.zeros((sH, sW), bool)
        nb = int(np.ceil(scale))  # at least the rows / columns whose window centre is row / column 0 or H-1 / W-1
        band[:1], band[-nb:], band[:, :1], band[:, -nb:] = True, True, True, True
        for which in (["auto", "x2_v1", "tile", "generic"] if scale == 2 else ["auto", "generic"]):
            c = base_config(ts=ts, scale=scale)
            c.hip = {"merge_kernel": which}
            got = torch.empty(sH, sW, 3, device=DEV)
            merge.merge_burst(tf, T(ref), rc, got, None, [[0, 1], [1, 2]], c)
            got = N(got)
            assert_close(got[band], want[band], 0, 0, f"border band x{scale} {which}")
            assert_close(got, want, 2e-5, 1e-6, f"interior x{scale} {which}")


@pytest.mark.parametrize("scale", [3, 5, 6])
def test_merge_integer_scale_geometry_decisions(scale):
    """Odd / composite integer scales: the float32 weight kernels take exactly the window-centre decisions of the
    reference's float64 evaluation (merge.py:319-345), also for flows whose fractional part is a float32 neighbour of a
    carry threshold (2s - 2rem - 1)/(2s) and for small negative flows (where flow - floor(flow) is inexact in float32) —
    a flipped centre pixel would move a window by one raw pixel and show as an O(0.1) difference."""
    H, W, ts = 48, 64, 16
    c64 = base_config(ts=ts, scale=scale)
    c64.hip = {"weight_fp64": True}
    ref, fr = merge_frames(H, W, 2, ts, 9, c64)
    # adversarial flows: k + threshold +- 1 ulp for every remainder class, both signs
    thr = sorted({(2 * scale - 2 * rem - 1) / (2 * scale) for rem in range(scale)} | {0.0, 0.5})
    vals = []
    for k in (-3.0, -1.0, 0.0, 2.0):
        for t in thr:
            f = np.float32(k + t)
            vals += [f, np.nextafter(f, np.float32(-10)), np.nextafter(f, np.float32(10))]
    vals = np.array(vals, np.float32)
    ny, nx = fr[0][1].shape[:2]
    rng = np.random.default_rng(1)
    for k in range(2):
        flow = vals[rng.integers(0, len(vals), (ny, nx, 2))]
        fr[k] = (fr[k][0], flow.astype(np.float32), fr[k][2], fr[k][3])
    tf = [tuple(T(a) for a in f) for f in fr]
    rc = T(oracle.estimate_kernels(ref, c64))
    sH, sW = scale * H, scale * W
    want = torch.empty(sH, sW, 3, device=DEV)
    merge.merge_burst(tf, T(ref), rc, want, None, [[0, 1], [1, 2]], c64)
    for which in ("auto", "generic"):
        c = base_config(ts=ts, scale=scale)
        c.hip = {"merge_kernel": which}
        got = torch.empty(sH, sW, 3, device=DEV)
        merge.merge_burst(tf, T(ref), rc, got, None, [[0, 1], [1, 2]], c)
        assert_close(N(got), N(want), 2e-5, 1e-6, f"x{scale} {which} vs float64 geometry")
    num, den = torch.zeros(sH, sW, 3, device=DEV), torch.zeros(sH, sW, 3, device=DEV)
    n64, d64 = torch.zeros_like(num), torch.zeros_like(den)
    for f in tf:
        merge.merge(*f, num, den, [[0, 1], [1, 2]], base_config(ts=ts, scale=scale))
        merge.merge(*f, n64, d64, [[0, 1], [1, 2]], c64)
    # (un-normalised sums.  A flipped decision moves a 3x3 window by a raw pixel: O(1e-2 .. 1e-1).  The tolerance of 1e-3
    # leaves room for ONE kind of pixel: flow ~ -1 at the first raw row extrapolates the covariance (D11) to a nearly
    # singular matrix that amplifies the float32 rounding of the blend — measured 3e-5 (x3) and 2.3e-4 (x6) on one pixel;
    # everywhere else the sums agree to 2e-5)
    for a_, b_, w_ in ((num, n64, "num"), (den, d64, "den")):
        assert_close(N(a_), N(b_), 1e-3, 1e-6, f"x{scale} per-frame kernel {w_}")
        assert_close(N(a_)[2 * scale:], N(b_)[2 * scale:], 2e-5, 1e-6, f"x{scale} per-frame kernel {w_}, rows off the top border")


def test_merge_burst_more_frames_than_one_launch_holds():
    """70 frames > HHSR_MAX_FRAMES (64): merge_burst chains two launches through the accumulators (with the fused
    local minimum and accumulated robustness) == per-frame merges."""
    H, W, ts, n = 32, 48, 16, 70
    cfg = base_config(ts=ts, scale=2)
    rng = np.random.default_rng(12)
    ref, comp, _ = synth.make_burst(H, W, 3, seed=5)
    covs = T(oracle.estimate_kernels(comp[0], cfg))
    tf = []
    for k in range(n):
        flow = T(rng.uniform(-1.5, 1.5, (H // ts, W // ts, 2)).astype(np.float32))
        tf.append((T(comp[k % 2]), flow, covs, T(rng.random((H, W), dtype=np.float32))))
    cfa = [[0, 1], [1, 2]]
    rc = T(oracle.estimate_kernels(ref, cfg))
    got, acc = torch.empty(2 * H, 2 * W, 3, device=DEV), torch.zeros(H, W, device=DEV)
    merge.merge_burst(tf, T(ref), rc, got, None, cfa, cfg, acc_r=acc, local_min=True)
    num, den = torch.zeros(2 * H, 2 * W, 3, device=DEV), torch.zeros(2 * H, 2 * W, 3, device=DEV)
    want_acc = torch.zeros(H, W, device=DEV)
    for f in tf:
        r = robustness.local_min(f[3], want_acc)
        merge.merge(f[0], f[1], f[2], r, num, den, cfa, cfg)
    merge.merge_ref(T(ref), rc, num, den, cfa, cfg)
    utils.divide(num, den)
    assert_close(N(got), N(num), 2e-5, 1e-6, "70-frame burst")
    assert_close(N(acc), N(want_acc), 1e-6, 1e-5, "70-frame accumulated robustness")


@pytest.mark.parametrize("scale", [1, 2, 3])
def test_merge_burst_equals_sequential(scale):
    H, W, ts = 64, 96, 16
    cfg = base_config(ts=ts, scale=scale)
    ref, fr = merge_frames(H, W, 3, ts, 31, cfg)
    cfa = [[0, 1], [1, 2]]
    oh, ow = scale * H, scale * W
    num, den = torch.zeros(oh, ow, 3, device=DEV), torch.zeros(oh, ow, 3, device=DEV)
    tf = [tuple(T(a) for a in f) for f in fr]
    for f in tf:
        merge.merge(*f, num, den, cfa, cfg)
    rc = T(oracle.estimate_kernels(ref, cfg))
    merge.merge_ref(T(ref), rc, num, den, cfa, cfg)
    num_seq, den_seq = num.clone(), den.clone()
    utils.divide(num, den)
    out = torch.empty_like(num)
    merge.merge_burst(tf, T(ref), rc, out, None, cfa, cfg)
    # same taps; the fused kernel sums parity classes over all frames and evaluates the reference frame's
    # weights in float32 (merge_ref keeps the reference's float64 typing)
    assert_close(N(out), N(num), 2e-5, 1e-6, "fused == sequential")
    # partial sums (the multi-GPU shape): shard A + shard B == all
    nA, dA = torch.empty_like(num), torch.empty_like(num)
    nB, dB = torch.empty_like(num), torch.empty_like(num)
    merge.merge_burst(tf[0::2], None, None, nA, dA, cfa, cfg, do_ref=False, divide=False, store_den=True)
    merge.merge_burst(tf[1::2], None, None, nB, dB, cfa, cfg, do_ref=False, divide=False, store_den=True)
    nS, dS = nA + nB, dA + dB
    merge.merge_burst([], T(ref), rc, nS, dS, cfa, cfg, load_acc=True, do_ref=True, divide=False, store_den=True)
    # (x2: k_merge_x2 blends the covariances with bilinear weights and takes one v_exp_f32 per tap — 2e-5 relative
    # to the per-frame kernel, the merge tolerance; the other scales share the per-frame kernel's arithmetic)
    tol = (2e-5, 1e-7) if scale in (2, 3) else (1e-6, 1e-7)  # x2 / x3: the wave-per-parity-class kernels
    assert_close(N(nS), N(num_seq), *tol, "sharded num")
    assert_close(N(dS), N(den_seq), *tol, "sharded den")
    # and against the oracle
    onum, oden = np.zeros((oh, ow, 3), np.float32), np.zeros((oh, ow, 3), np.float32)
    for f in fr:
        oracle.merge(*f, onum, oden, cfa, cfg)
    oracle.merge_ref(ref, oracle.estimate_kernels(ref, cfg), onum, oden, cfa, cfg)
    assert_close(N(num_seq), onum, 2e-5, 1e-6, "num vs oracle")
    assert_close(N(den_seq), oden, 2e-5, 1e-6, "den vs oracle")
    with np.errstate(all="ignore"):
        assert_close(N(out), onum / oden, 2e-5, 1e-6, "fused output vs oracle")


def test_divide_add():
    rng = np.random.default_rng(8)
    a = rng.random((37, 53, 3), dtype=np.float32)
    b = rng.random((37, 53, 3), dtype=np.float32)
    b[0, 0, 0] = 0
    a[0, 0, 0] = 0
    ta = T(a)
    utils.divide(ta, T(b))
    with np.errstate(all="ignore"):
        assert_close(N(ta), a / b, 0, 0, "divide")  # 0/0 = NaN kept
    ta = T(a[..., 0])
    utils.add(ta, T(b[..., 0]))
    assert_close(N(ta), a[..., 0] + b[..., 0], 0, 0, "add")
    # pointers that are not 16-byte aligned (contiguous views at odd offsets): same misalignment -> scalar head +
    # float4 body, different misalignments -> scalar kernel
    flat_a, flat_b = a.ravel(), b.ravel()
    for oa, ob, n in ((1, 1, 1001), (3, 3, 2), (2, 1, 777), (0, 3, 640), (1, 0, 5)):
        base_a, base_b = T(flat_a), T(flat_b)
        va, vb = base_a[oa:oa + n], base_b[ob:ob + n]
        utils.divide(va, vb)
        with np.errstate(all="ignore"):
            want = flat_a.copy()
            want[oa:oa + n] = flat_a[oa:oa + n] / flat_b[ob:ob + n]
        assert_close(N(base_a), want, 0, 0, f"divide at offsets {oa}, {ob}")  # (and nothing outside the view touched)
        base_a = T(flat_a)
        va = base_a[oa:oa + n]
        utils.add(va, vb)
        want = flat_a.copy()
        want[oa:oa + n] = flat_a[oa:oa + n] + flat_b[ob:ob + n]
        assert_close(N(base_a), want, 0, 0, f"add at offsets {oa}, {ob}")


def test_abi_error_reporting():
    from handheld_super_resolution import _lib

    with pytest.raises(RuntimeError, match="invalid argument"):
        _lib.call("hhsr_divide", _lib.ptr(None), _lib.ptr(None), 4, _lib.stream())


# ------------------------------------------------------------------------------------------ end to end
def test_e2e_golden_128(golden):
    g = golden("e2e_128")
    ref, comp, _ = synth.make_burst(128, 128, 3, seed=int(g["seed"]), max_shift=2.0, occluder=True)
    cfg = base_config(ts=16, scale=2)
    cfg.block_matching.tuning.factors = [1, 2, 2, 2]
    cfg.debug = True
    out, dbg = hsr.main(ref, comp, cfg)
    # measured (PARITY.md): flow 2e-6 px, r 8e-6, output 3e-6 — asserted with a 10x margin, no outliers
    assert_close(np.stack(dbg["flow"]), g["flow"], 0, 5e-5, "flow")
    assert_close(np.stack(dbg["robustness"]), g["r"], 0, 1e-4, "r")
    assert_close(N(dbg["accumulated robustness"]), g["acc_r"], 0, 1e-4, "acc r")
    o = N(out)
    assert_close(o, g["out"], 0, 5e-5, "output")
    # sequential (operator API) path gives the same image as the fused burst merge
    cfg2 = base_config(ts=16, scale=2)
    cfg2.block_matching.tuning.factors = [1, 2, 2, 2]
    cfg2.hip = {"fused_merge": False}
    out2, _ = hsr.main(ref, comp, cfg2)
    assert_close(N(out2), o, 2e-5, 1e-6, "sequential == fused")


def test_e2e_golden_x1_denoiser(golden):
    """The reference's own result for x1 / BGGR / white balance / accumulated-robustness merge denoiser."""
    from test_oracle_golden import x1_config

    g = golden("e2e_x1")
    cfa, wb = ((2, 1), (1, 0)), (1.9, 1.0, 1.6)
    ref, comp, _ = synth.make_burst(128, 160, 3, seed=int(g["seed"]), max_shift=2.0, occluder=True, cfa=cfa, wb=wb)
    cfg = x1_config(cfa, wb)
    cfg.debug = True
    out, dbg = hsr.main(ref, comp, cfg)
    # measured (PARITY.md): flow 2e-6 px, r 8e-6, output 3e-6 — asserted with a 10x margin, no outliers
    assert_close(np.stack(dbg["flow"]), g["flow"], 0, 5e-5, "flow")
    assert_close(np.stack(dbg["robustness"]), g["r"], 0, 1e-4, "r")
    assert_close(N(dbg["accumulated robustness"]), g["acc_r"], 0, 1e-4, "acc r")
    o = N(out)
    assert_close(o, g["out"], 0, 5e-5, "output")
    # non-debug path: the batched front end, the comp frames through ONE fused merge launch (float32 weight chain, like the
    # headline path), hhsr_rob_sum, then merge_ref + divide (round 6; the debug path above is the per-frame operator path)
    cfg2 = x1_config(cfa, wb)
    out2, _ = hsr.main(ref, comp, cfg2)
    assert_close(N(out2), g["out"], 0, 5e-5, "fast path vs the reference's output")
    assert_close(N(out2), o, 0, 2e-6, "fast path vs debug path")
    cfg3 = x1_config(cfa, wb)  # ... and the per-frame path without the debug copies: bit-identical to the debug path
    cfg3.hip = {"fused_merge": False}
    out3, _ = hsr.main(ref, comp, cfg3)
    assert_close(N(out3), o, 0, 0, "debug path == sequential fast path")


@pytest.mark.parametrize("tag", ["s15", "s3", "s2iso", "ts32"])
def test_e2e_golden_scales(golden, tag):
    """The reference's own main() at x1.5 (GRBG sensor, white balance: the any-scale kernel), x3 with 4 frames (the x3
    class kernel) and x2 with isotropic kernels on a GBRG sensor (tools/refsim stage e2e_scales); debug and fast paths."""
    from helpers import e2e_scales_case

    g = golden("e2e_scales")
    ref, comp, _, cfg_fn = e2e_scales_case(tag)
    cfg = cfg_fn()
    cfg.debug = True
    out, dbg = hsr.main(ref, comp, cfg)
    assert_close(np.stack(dbg["flow"]), g[f"{tag}_flow"], 0, 5e-5, "flow")
    assert_close(np.stack(dbg["robustness"]), g[f"{tag}_r"], 0, 1e-4, "r")
    assert_close(N(dbg["accumulated robustness"]), g[f"{tag}_acc_r"], 0, 1e-4, "acc r")
    o = N(out)
    assert_close(o, g[f"{tag}_out"], 0, 5e-5, "output")
    out2, _ = hsr.main(ref, comp, cfg_fn())  # non-debug (chunk-batched, graph-replayed) path
    assert_close(N(out2), g[f"{tag}_out"], 0, 5e-5, "output, fast path")
    assert_close(N(out2), o, 2e-5, 1e-6, "debug path vs fast path")


def _e2e_vs_oracle(ref, comp, cfg_fn, ts, what, max_flipped, out_atol=1e-4, flow_atol=1e-4, r_atol=1e-4, acc_atol=3e-4,
                   parallel=False, stray=(0, 0.0)):
    """HIP main() against the oracle on one burst, every difference accounted for (tolerances ~10x the measured
    differences of PARITY.md: flow 8e-6 px, r 7e-6, accumulated r 1.4e-5, image 6.4e-5): flows equal to `flow_atol` except on
    tiles whose block-matching decision flipped (count <= max_flipped, the measured number); robustness, accumulated
    robustness and the output image equal to their tolerances everywhere OUTSIDE the footprint of those tiles."""
    H, W = ref.shape
    cap = {}
    if parallel:  # one worker process per frame (bit-identical to oracle.main, tests/test_oracle_kat.py), the accumulation
        # in its C form (oracle.cfast: bit-identical to oracle/merge.py on what the same file compares)
        want, wdbg, _ = oracle.main_parallel(ref, comp, cfg_fn(), capture=cap, fast=True)
    else:
        want, wdbg = oracle.main(ref, comp, cfg_fn(), capture=cap)
    cfg = cfg_fn()
    cfg.debug = True
    out, dbg = hsr.main(ref, comp, cfg)
    scale = cfg.scale
    gflow, oflow = np.stack(dbg["flow"]), np.stack(cap["flow"])
    flipped = flipped_tiles(gflow, oflow)
    assert int(flipped.sum()) <= max_flipped, f"{what}: {int(flipped.sum())} flipped tiles (allowed {max_flipped})"
    assert_close(gflow[~flipped], oflow[~flipped], 0, flow_atol, what + " flow (un-flipped tiles)")
    assert_explained(np.stack(dbg["robustness"]), np.stack(cap["r"]), r_atol, flipped, ts, (H, W), 1.0, what + " r",
                     max_flipped, per_frame=True)
    o = N(out)
    assert o.shape == want.shape
    assert_explained(o, want, out_atol, flipped, ts, (H, W), scale, what + " output", max_flipped, stray=stray)
    if "accumulated robustness" in wdbg:
        assert_explained(N(dbg["accumulated robustness"]), wdbg["accumulated robustness"], acc_atol, flipped, ts, (H, W),
                         1.0, what + " acc r", max_flipped)
    return o, want, flipped


@pytest.mark.parametrize("metric0", ["L1", "L2", "L1_ref_effective"])
def test_e2e_c1_512(metric0):
    """BASELINE config C1: 512x512, 3 frames, x1 (demosaick only), Ts=16."""
    ref, comp, _ = synth.make_burst(512, 512, 3, seed=1234, max_shift=4.0)
    _e2e_vs_oracle(ref, comp, lambda: base_config(ts=16, scale=1, metrics=(metric0, "L2", "L2", "L2")), 16,
                   f"C1 {metric0}", max_flipped=FLIP_BUDGET["c1"])


@pytest.mark.parametrize("ts,snr", [(32, 18.0), (64, 10.0)])
def test_e2e_large_tiles(ts, snr):
    """Ts = 32 / 64 (lower-SNR bursts), x2, 768x1024."""
    H, W = 768, 1024
    a, b = 16 * synth.ALPHA_ISO100, 16 * synth.BETA_ISO100
    ref, comp, _ = synth.make_burst(H, W, 2, seed=7, alpha=a, beta=b, max_shift=3.0)

    def cfg0():
        cfg = base_config(ts=ts, scale=2, snr=snr)
        if ts == 64:
            cfg.block_matching.tuning.factors = [1, 2, 2, 2]  # keeps >= 1 tile at the coarsest level at this size
        cfg.noise_model.alpha, cfg.noise_model.beta = a, b
        std, dif = synth.noise_curves(a, b)
        cfg.noise_model.update({"std_curve": std.tolist(), "diff_curve": dif.tolist()})
        return cfg

    _e2e_vs_oracle(ref, comp, cfg0, ts, f"Ts={ts}", max_flipped=FLIP_BUDGET[f"ts{ts}"])


@pytest.mark.parametrize("shape,scale", [((502, 618), 2), ((486, 520), 1.5), ((512, 640), 3)])
def test_e2e_ragged_sizes_and_scales(shape, scale):
    """Frame sizes that are not multiples of the tile size (circular padding of the reference frame only,
    D16; partial tiles at the right / bottom) and non-power-of-two scales (float64 geometry path)."""
    H, W = shape
    ref, comp, _ = synth.make_burst(H, W, 3, seed=23, max_shift=3.0, occluder=True)
    o, want, _ = _e2e_vs_oracle(ref, comp, lambda: base_config(ts=16, scale=scale, metrics=("L1", "L2", "L2", "L2")), 16,
                                f"ragged x{scale}", max_flipped=FLIP_BUDGET[f"ragged{scale}"])
    with np.errstate(all="ignore"):
        assert np.nanpercentile(np.abs(o - want), 99) < 2e-4


def _opt_robustness_off(c):
    c.robustness.enabled = False
    c.robustness.save_mask = False  # (the reference's sanitize_config refuses the combination)


def _opt_bilinear(c):
    c.block_matching.tuning.flow_upscale_mode = "bilinear"


def _opt_bicubic(c):
    c.block_matching.tuning.flow_upscale_mode = "bicubic"


def _opt_iso(c):
    c.merging.kernel = "iso"


def _opt_law(c):
    c.merging.selection_law = "hard_threshold" if c.merging.selection_law == "linear" else "linear"


def _opt_save_mask(c):
    c.robustness.save_mask = True


def _opt_fp64(c):
    c.hip = {"weight_fp64": True}


def _opt_one_stream(c):
    c.hip = {"streams": 1}


@pytest.mark.parametrize("opt", [_opt_robustness_off, _opt_bilinear, _opt_bicubic, _opt_iso, _opt_law, _opt_save_mask,
                                 _opt_fp64, _opt_one_stream], ids=lambda f: f.__name__[5:])
def test_e2e_config_matrix(opt, capsys):
    """One option at a time away from the base configuration, HIP main() vs the oracle; plus verbose = 2 (timers,
    host synchronisation, per-frame path) giving the same image as the quiet pipelined path."""
    ref, comp, _ = synth.make_burst(128, 160, 3, seed=6, max_shift=2.0, occluder=True)

    def cfg0(verbose=0):
        c = base_config(ts=16, scale=2)
        c.block_matching.tuning.factors = [1, 2, 2, 2]
        opt(c)
        c.verbose = verbose
        return c

    o, want, flipped = _e2e_vs_oracle(ref, comp, cfg0, 16, "matrix " + opt.__name__[5:],
                                      max_flipped=FLIP_BUDGET["matrix"])
    out_q, _ = hsr.main(ref, comp, cfg0())  # quiet, pipelined, fused (the debug run above is the per-frame path)
    assert_close(N(out_q), o, 2e-5, 1e-6, "quiet (fused, pipelined) == debug (per-frame)")
    out_v, _ = hsr.main(ref, comp, cfg0(verbose=3))
    printed = capsys.readouterr().out
    assert "Total ellapsed time" in printed
    for msg in ("Alignment initialized (Total)", "Image aligned (Total)", "Robustness estimated (Total)",
                "Burst merged (Total)", "- grey images estimated by FFT"):
        assert msg in printed, msg  # the reference's per-stage timers (super_resolution.py:72-81), verbose >= 2 / 3
    assert_close(N(out_v), o, 2e-5, 1e-6, "verbose (sequential) == debug")


@pytest.mark.parametrize("n_comp", [0, 1, 2])
def test_e2e_few_frames_and_foreign_inputs(n_comp):
    """Bursts of 1-3 frames (0 comp frames = the reference frame alone) against the oracle; strided float64 /
    host-tensor inputs give the same result as contiguous float32 arrays."""
    ref, comp, _ = synth.make_burst(128, 160, 3, seed=2)

    def cfg0():
        c = base_config(ts=16, scale=2)
        c.block_matching.tuning.factors = [1, 2, 2, 2]
        return c

    out, _ = hsr.main(ref, comp[:n_comp], cfg0())
    want, _ = oracle.main(ref, comp[:n_comp], cfg0())
    assert_close(N(out), want, 2e-5, 1e-5, f"{n_comp} comp frames")
    wide = np.zeros((128, 320), np.float64)
    wide[:, ::2] = ref
    out2, _ = hsr.main(wide[:, ::2], torch.from_numpy(comp[:n_comp]), cfg0())
    assert_close(N(out2), N(out), 0, 0, "strided float64 / host tensor inputs")


def test_process_facade():
    from oracle import post

    ref, comp, _ = synth.make_burst(512, 512, 3, seed=3)
    cfg = hsr.default_config()
    cfg.verbose = 0
    cfg.block_matching.tuning.tile_size = 16
    cfg.block_matching.tuning.metrics = ["L2"] * 4
    burst = {"ref": ref, "comp": comp, "cfa_pattern": [[0, 1], [1, 2]], "white_balance": [1.0, 1.0, 1.0],
             "alpha": synth.ALPHA_ISO100, "beta": synth.BETA_ISO100, "orientation": 6}
    img, dbg = hsr.process(burst, cfg)
    assert img.shape == (512, 512, 3) and img.dtype == np.float32
    assert cfg.block_matching.tuning.tile_sizes == [16, 16, 16, 8]  # derived in place like the reference
    assert isinstance(dbg["accumulated robustness"], np.ndarray)
    # = main() on the prepared config, then the reference's default post-processing (unsharp mask radius 3 amount 1.5,
    # gamma 1/2.2; configs/default.yaml:44-53) and the EXIF orientation (super_resolution.py:303-356)
    out, mdbg = hsr.main(ref, comp, cfg)
    want = post.apply_orientation(post.postprocess(N(out), False, False, True, {"enabled": True, "amount": 1.5, "radius": 3}),
                                  6)
    assert_close(img, want, 0, 2e-6, "process == postprocess(main)")
    assert_close(dbg["accumulated robustness"], post.apply_orientation(N(mdbg["accumulated robustness"]), 6), 0, 0, "acc r")
    cfg2 = hsr.default_config()
    cfg2.verbose = 0
    cfg2.block_matching.tuning.tile_size = 16
    cfg2.block_matching.tuning.metrics = ["L2"] * 4
    cfg2.postprocessing.enabled = False
    img2, _ = hsr.process(dict(burst, orientation=1), cfg2)
    assert_close(img2, N(out), 0, 0, "postprocessing off: process == main")


def test_post_path(golden):
    """The step after the path on the device against the reference's own outputs (golden "post":
    orientation, median frame-count denoiser, postprocess without sharpening) and against the oracle (gauss denoiser,
    unsharp mask, NaN pixels, orientation folded into the postprocess store)."""
    from oracle import post
    from handheld_super_resolution import raw2rgb, config as hcfg

    g = golden("post")
    for ori in range(1, 9):
        assert_close(N(utils_image.apply_orientation(T(g["ori_in"]), ori)), g[f"ori{ori}"], 0, 0, f"orientation {ori}")
        assert_close(N(utils_image.apply_orientation(T(g["ori_in"][..., 0]), ori)), g[f"ori{ori}"][..., 0], 0, 0,
                     f"plane orientation {ori}")
        assert np.array_equal(utils_image.apply_orientation(g["ori_in"], ori), g[f"ori{ori}"])  # NumPy in, NumPy out
    mcfg = hcfg.Config({"enabled": True, "radius_max": 3, "max_frame_count": 8})
    med = utils_image.frame_count_denoising_median(T(g["med_in"]), T(g["med_racc"]), mcfg, scale=int(g["med_scale"]))
    assert_close(N(med), g["med_out"], 0, 0, "median denoiser vs the reference's kernel")
    with pytest.raises(RuntimeError, match="overflows"):
        utils_image.frame_count_denoising_median(T(g["med_in"]), T(g["med_racc"]),
                                                 hcfg.Config({"radius_max": 9, "max_frame_count": 8}), scale=2)
    rng = np.random.default_rng(5)
    img = rng.random((37, 53, 3)).astype(np.float32)
    racc = rng.uniform(0, 10, (19, 27))
    gcfg = hcfg.Config({"enabled": True, "sigma_max": 1.5, "max_frame_count": 8})
    for half in (True, False):
        got = utils_image.frame_count_denoising_gauss(T(img), T(racc), gcfg, scale=2, half_index=half)
        assert_close(N(got), post.frame_count_denoising_gauss(img, racc, gcfg, 2, half), 0, 1e-6, f"gauss denoiser {half}")
        got = utils_image.frame_count_denoising_median(T(img), T(racc), mcfg, scale=2, half_index=half)
        assert_close(N(got), post.frame_count_denoising_median(img, racc, mcfg, 2, half), 0, 0, f"median denoiser {half}")
    # postprocess without sharpening: the reference's outputs
    off = hcfg.Config({"enabled": False})
    x2c = g["pp_xyz2cam"]
    pin = T(g["pp_in"])
    assert_close(N(raw2rgb.postprocess(None, pin, False, False, True, off, False, x2c)), g["pp_gamma_only"], 0, 1e-6, "gamma")
    assert_close(N(raw2rgb.postprocess(None, pin, True, False, True, off, False, x2c)), g["pp_ccm_gamma"], 0, 1e-6, "ccm + gamma")
    assert_close(N(raw2rgb.postprocess(None, pin, True, False, False, off, True, x2c)), g["pp_ccm_devig"], 0, 1e-6, "ccm + devignette")
    assert_close(N(raw2rgb.postprocess(None, pin, True, False, True, None, False, np.zeros((3, 3)))), g["pp_zero_ccm"], 0, 1e-6,
                 "zero colour matrix")
    assert_close(raw2rgb.get_color_matrix(None, x2c), g["pp_ccm"], 0, 1e-7, "colour matrix")
    with pytest.raises(NotImplementedError):
        raw2rgb.postprocess(None, pin, False, True, True, off)
    # sharpening (+ everything else, NaN pixels, every orientation) against the oracle
    big = (rng.random((45, 70, 3)) * 1.1 - 0.05).astype(np.float32)
    big[0, 3, 1] = np.nan
    sharp = hcfg.Config({"enabled": True, "amount": 1.5, "radius": 3})
    for ori in (1, 3, 6, 7):
        for ccm in (False, True):
            got = raw2rgb.postprocess(None, T(big), ccm, False, True, sharp, False, x2c, orientation=ori)
            want = post.apply_orientation(post.postprocess(big, ccm, False, True, sharp, False, x2c), ori)
            assert_close(N(got), want, 0, 2e-6, f"unsharp + gamma, orientation {ori}, ccm {ccm}")
    got = raw2rgb.postprocess(None, T(big), True, False, True, hcfg.Config({"enabled": True}), True, x2c)
    want = post.postprocess(big, True, False, True, {"enabled": True}, True, x2c)  # fall-back radius 3, amount 0.5
    assert_close(N(got), want, 0, 2e-6, "sharpening defaults + devignetting")


def test_process_frame_count_denoisers():
    """process() with the median / gauss frame-count denoisers: = main() (merge-stage denoiser active too, as upstream:
    any of the three switches sets accumulated_robustness_denoiser.enabled) followed by the denoisers of the oracle."""
    from oracle import post

    ref, comp, _ = synth.make_burst(512, 512, 3, seed=4, occluder=True)
    for which in ("median", "gauss"):
        cfg = hsr.default_config()
        cfg.verbose = 0
        cfg.scale = 2
        cfg.block_matching.tuning.tile_size = 16
        cfg.block_matching.tuning.metrics = ["L2"] * 4
        cfg.postprocessing.enabled = False
        cfg.accumulated_robustness_denoiser[which].enabled = True
        burst = {"ref": ref, "comp": comp, "cfa_pattern": [[0, 1], [1, 2]], "white_balance": [1.0, 1.0, 1.0],
                 "alpha": synth.ALPHA_ISO100, "beta": synth.BETA_ISO100}
        img, dbg = hsr.process(burst, cfg)
        assert cfg.accumulated_robustness_denoiser.enabled is True
        out, mdbg = hsr.main(ref, comp, cfg)
        sub = cfg.accumulated_robustness_denoiser[which]
        fn = post.frame_count_denoising_median if which == "median" else post.frame_count_denoising_gauss
        want = fn(N(out), N(mdbg["accumulated robustness"]), sub, 2)
        assert_close(img, want, 0, 1e-6 if which == "gauss" else 0, f"process with the {which} denoiser")


def test_frame_count_denoisers_grey_index():
    """`mode: grey`: the post-hoc denoisers index the accumulated robustness with int(round(y / scale))
    (utils_image.py:203-204, 260-261), not with the Bayer branch's half-resolution index — at the operator level and
    through process() on a monochrome burst."""
    from oracle import post

    rng = np.random.default_rng(2)
    img = rng.random((96, 128, 3), dtype=np.float32)
    acc = (rng.random((48, 64)) * 4).astype(np.float32)
    cfg = hsr.default_config().accumulated_robustness_denoiser
    for which, fn, ofn, tol in (("median", utils_image.frame_count_denoising_median, post.frame_count_denoising_median, 0),
                                ("gauss", utils_image.frame_count_denoising_gauss, post.frame_count_denoising_gauss, 1e-6)):
        got = N(fn(T(img), T(acc), cfg[which], scale=2, mode="grey"))
        assert_close(got, ofn(img, acc, cfg[which], 2, half_index=2), 0, tol, f"{which}, grey index")
        bayer = N(fn(T(img), T(acc), cfg[which], scale=2))
        assert_close(bayer, ofn(img, acc, cfg[which], 2, half_index=True), 0, tol, f"{which}, bayer index")
        assert not np.array_equal(got, bayer)
    ref, comp, _ = synth.make_burst(512, 512, 3, seed=8, cfa=MONO, occluder=True)
    c = hsr.default_config()
    c.verbose = 0
    c.mode = "grey"
    c.block_matching.tuning.tile_size = 16
    c.block_matching.tuning.metrics = ["L2"] * 4
    c.postprocessing.enabled = False
    c.accumulated_robustness_denoiser.median.enabled = True
    burst = {"ref": ref, "comp": comp, "alpha": synth.ALPHA_ISO100, "beta": synth.BETA_ISO100}
    out, dbg = hsr.process(burst, c)
    o, mdbg = hsr.main(ref, comp, c)
    want = post.frame_count_denoising_median(N(o), N(mdbg["accumulated robustness"]), c.accumulated_robustness_denoiser.median,
                                             c.scale, half_index=2)
    assert_close(out[..., 0], want[..., 0], 0, 0, "process(mode: grey) with the median denoiser")


# ------------------------------------------------------------------------------------------ burst front end
@pytest.mark.parametrize("sensor", ["rggb10", "bggr14", "grbg12"])
def test_load_dng_burst_golden(golden, sensor, tmp_path, monkeypatch):
    """The product's load_dng_burst (normalisation on the GPU) against what the reference's own loader returned for the
    same synthetic sensor (golden `frontend`): same stand-in decoder objects in the place of rawpy / exifread, every
    return value equal — frames bit for bit."""
    import sys
    import types
    from handheld_super_resolution import utils_dng

    g = golden("frontend")
    t = sensor
    counts = g[f"{t}_counts"]
    paths = []
    for i in range(counts.shape[0]):
        p = tmp_path / f"im_{i:02d}.dng"
        p.write_bytes(b"stand-in")
        paths.append(str(p))

    class FakeRaw:
        def __init__(self, path):
            self.raw_image = counts[paths.index(str(path))]
            self.white_level = int(g[f"{t}_white"])
            self.black_level_per_channel = g[f"{t}_black"].tolist()
            self.camera_whitebalance = g[f"{t}_wb"].tolist()
            self.raw_pattern = g[f"{t}_pattern"].astype(np.uint8)

        def __enter__(self):
            return self

        def __exit__(self, *a):
            return False

    class Tag:
        def __init__(self, values):
            self.values = values

        def __str__(self):
            return str(self.values[0])

    class Ratio:
        def __init__(self, v):
            self.v = v

        def decimal(self):
            return float(self.v)

    tags = {"EXIF ISOSpeedRatings": Tag([int(g[f"{t}_iso_in"])]), "Image Tag 0xC621": Tag([Ratio(v) for v in g[f"{t}_ccm_in"]])}
    monkeypatch.setitem(sys.modules, "rawpy", types.SimpleNamespace(imread=lambda p: FakeRaw(p)))
    monkeypatch.setitem(sys.modules, "exifread", types.SimpleNamespace(process_file=lambda f, **kw: dict(tags)))
    ref_raw, raw_comp, iso, _, cfa, xyz2cam, wb, ref_path = utils_dng.load_dng_burst(str(tmp_path))
    assert np.array_equal(N(ref_raw), g[f"{t}_ref"]) and np.array_equal(N(raw_comp), g[f"{t}_comp"])
    assert iso == int(g[f"{t}_iso"]) and np.array_equal(cfa, g[f"{t}_cfa"]) and ref_path.endswith("im_00.dng")
    assert np.array_equal(xyz2cam, g[f"{t}_xyz2cam"]) and list(wb) == g[f"{t}_wb"].tolist()


@pytest.mark.parametrize("shape", [(3, 64, 96), (2, 50, 70)])
def test_normalize_raw_bit_exact(shape):
    """hhsr_normalize_raw_u16 == the NumPy expression of utils_dng.py:149-160, bit for bit (incl. a width that is
    not a multiple of the 8-pixel vector path)."""
    from handheld_super_resolution import utils_dng

    rng = np.random.default_rng(9)
    raw = rng.integers(0, 16384, shape, dtype=np.uint16)
    cfa, bl, wl, wb = [[2, 1], [1, 0]], [63, 64, 66], 16383, [1.91, 1.0, 1.57, 1.0]
    got = N(utils_dng.normalize_burst(raw, bl, wl, wb, cfa))
    want = oracle.frontend.normalize_burst(raw, bl, wl, wb, cfa)
    assert got.dtype == np.float32 and np.array_equal(got, want)
    assert np.array_equal(N(utils_dng.normalize_burst(raw[0], bl, wl, wb, cfa)), want[0])
    with pytest.raises(TypeError):
        utils_dng.normalize_burst(raw.astype(np.float32), bl, wl, wb, cfa)


def test_monte_carlo_noise_curves_gpu():
    from handheld_super_resolution import fast_monte_carlo as mc

    a, b = synth.ALPHA_ISO100 * 4, synth.BETA_ISO100 * 4
    s1, d1 = mc.run_fast_MC(a, b, seed=5)
    s2, d2 = mc.run_fast_MC(a, b, seed=5)
    assert np.array_equal(s1, s2) and np.array_equal(d1, d2)  # seeded: reproducible
    sa, da = synth.noise_curves(a, b)
    assert np.abs(s1[100:900] / sa[100:900] - 1).max() < 0.005 and np.abs(d1[100:900] / da[100:900] - 1).max() < 0.01
    rng = np.random.default_rng(1)
    for i in (0, 2, 999):
        dm, sm = oracle.frontend.unitary_mc(a, b, i / 1000, 50000, rng)
        assert abs(s1[i] / sm - 1) < 0.02 and abs(d1[i] / dm - 1) < 0.03


def test_process_default_noise_curves_include_clipping():
    """process() without explicit curves runs the reference's estimator (run_fast_MC: clipped Poisson-Gaussian patches),
    not the analytic un-clipped law: within ~3 sigma of black / saturation the two differ by tens of percent, which
    changes the robustness in shadows and highlights."""
    ref, comp, _ = synth.make_burst(512, 512, 2, seed=3)
    a, b = synth.ALPHA_ISO100 * 16, synth.BETA_ISO100 * 16
    cfg = hsr.default_config()
    cfg.verbose = 0
    cfg.block_matching.tuning.tile_size = 16
    hsr.process({"ref": ref, "comp": comp, "cfa_pattern": [[0, 1], [1, 2]], "white_balance": [1.0, 1.0, 1.0],
                 "alpha": a, "beta": b}, cfg)
    std, dif = np.array(cfg.noise_model.std_curve), np.array(cfg.noise_model.diff_curve)
    sa, da = synth.noise_curves(a, b)
    rng = np.random.default_rng(1)
    for i in (0, 1, 1000):  # black, near black, saturation: clipped regime
        dm, sm = oracle.frontend.unitary_mc(a, b, i / 1000, 100000, rng)
        assert abs(std[i] / sm - 1) < 0.02 and abs(dif[i] / dm - 1) < 0.03, (i, std[i], sm, dif[i], dm)
        assert std[i] < 0.8 * sa[i], (i, std[i], sa[i])  # the un-clipped law is far off here
    assert np.abs(std[200:800] / sa[200:800] - 1).max() < 0.01  # ... and right in the mid-tones
    cfg2 = hsr.default_config()
    cfg2.verbose = 0
    cfg2.block_matching.tuning.tile_size = 16
    cfg2.noise_model.estimator = "analytic"
    hsr.process({"ref": ref, "comp": comp, "cfa_pattern": [[0, 1], [1, 2]], "white_balance": [1.0, 1.0, 1.0],
                 "alpha": a, "beta": b}, cfg2)
    assert np.allclose(cfg2.noise_model.std_curve, sa)


def test_process_integer_burst_and_monte_carlo_estimator():
    """process() on sensor counts + metadata (normalised on the GPU) == process() on the normalised floats; the
    Monte-Carlo estimator option produces curves and runs."""
    ref, comp, _ = synth.make_burst(256, 256, 3, seed=4)
    wb, bl, wl = [1.8, 1.0, 1.4], [64, 64, 64], 4095
    cfa = [[0, 1], [1, 2]]
    # counts whose normalisation is NOT the identity on the synthetic floats: build counts first
    gains = np.array([[wb[cfa[i][j]] / wb[1] for j in range(2)] for i in range(2)], np.float64)
    g = np.tile(gains, (128, 128))
    to_counts = lambda x: np.clip(np.rint(x / g * (wl - 64) + 64), 0, wl).astype(np.uint16)  # noqa: E731
    ref_c, comp_c = to_counts(ref), to_counts(comp)
    stack = oracle.frontend.normalize_burst(np.concatenate([ref_c[None], comp_c]), bl, wl, wb, cfa)

    def cfg0():
        c = hsr.default_config()
        c.verbose = 0
        c.block_matching.tuning.tile_size = 16
        c.block_matching.tuning.factors = [1, 2, 2, 2]
        c.block_matching.tuning.metrics = ["L2"] * 4
        return c

    meta = {"cfa_pattern": cfa, "white_balance": wb, "alpha": synth.ALPHA_ISO100, "beta": synth.BETA_ISO100}
    img_i, _ = hsr.process({"ref": ref_c, "comp": comp_c, "black_levels": bl, "white_level": wl, **meta}, cfg0())
    img_f, _ = hsr.process({"ref": stack[0], "comp": stack[1:], **meta}, cfg0())
    assert_close(img_i, img_f, 0, 0, "integer burst == normalised burst")
    # main() itself takes sensor counts when config.hip.raw_norm is given: pinned uint16 tensors, uploaded and
    # normalised frame by frame on the pipeline streams — bit-identical to the normalised float frames
    cm = cfg0()
    hsr.prepare_config(cm, stack[0], synth.ALPHA_ISO100, synth.BETA_ISO100, cfa, wb)
    cm.hip = {"raw_norm": {"black_levels": bl, "white_level": wl}}
    out_c, _ = hsr.main(torch.from_numpy(ref_c).pin_memory(), [torch.from_numpy(c).pin_memory() for c in comp_c], cm)
    cf = cfg0()
    hsr.prepare_config(cf, stack[0], synth.ALPHA_ISO100, synth.BETA_ISO100, cfa, wb)
    out_f, _ = hsr.main(stack[0], stack[1:], cf)
    assert_close(N(out_c), N(out_f), 0, 0, "main(counts) == main(normalised)")
    with pytest.raises(ValueError):
        hsr.main(ref_c, comp_c, cf)  # counts without raw_norm
    c = cfg0()
    c.noise_model.estimator = "monte_carlo"
    c.noise_model.seed = 7
    img_m, _ = hsr.process({"ref": stack[0], "comp": stack[1:], **meta}, c)
    # (default post-processing: the unsharp mask's 25-tap blur spreads the NaN border pixels — D6 — 12 pixels inwards,
    # exactly as scipy.ndimage.gaussian_filter does upstream)
    assert len(c.noise_model.std_curve) == 1001 and np.isfinite(img_m[16:-16, 16:-16]).all()
    assert np.abs(img_m[16:-16, 16:-16] - img_f[16:-16, 16:-16]).max() < 0.05  # clipped-regime curves only move r slightly


def test_full_size_properties():
    """BASELINE config C2 geometry (3000x4000, x2): size-independent properties on the GPU path."""
    H, W = 3000, 4000
    ref, comp, _ = synth.make_burst_torch(H, W, 3, DEV, seed=11)
    cfg = base_config(ts=16, scale=2, metrics=("L1", "L2", "L2", "L2"))
    cfg.debug = False
    # (1) a frame identical to the reference aligns with zero flow and is fully robust off the border
    pipe = hsr.BurstPipeline(cfg).init_ref(ref)
    raw, flow, covs, r = pipe.process_frame(ref)
    # (the reference frame is circularly padded 3000 -> 3008 rows and the moving frame is not — D16 — so the
    # bottom tile rows legitimately see a different image; check the upper half)
    ny = flow.shape[0]
    assert float(flow[: ny // 2].abs().max()) == 0.0
    assert bool((r[:3] == 0).all()) and bool((r[:, :3] == 0).all())  # D6
    assert float(r[3: H // 2, 3:].min()) == 1.0  # clamp(s2 * exp(0) - t, 0, 1)
    # (2) known translation is recovered (median over tiles) to a few hundredths of a pixel
    shifts = synth.frame_shifts(3, 11)
    _, flow1, _, r1 = pipe.process_frame(comp[0])
    med = flow1.reshape(-1, 2).median(0).values.cpu().numpy()
    # (the reference's ICA takes half Gauss-Newton steps — un-normalised gradients, D9 — so 3 iterations
    # leave a residual of up to ~1/4 px from the integer block-matching result)
    assert np.abs(med + shifts[1]).max() < 0.35, (med, shifts[1])
    assert float(r1.mean()) > 0.8
    # (3) fused burst merge == per-frame operator path, bitwise, and sharded partial sums agree
    out, _ = hsr.main(ref, comp, cfg)
    cfg2 = base_config(ts=16, scale=2, metrics=("L1", "L2", "L2", "L2"))
    cfg2.hip = {"fused_merge": False}
    out2, _ = hsr.main(ref, comp, cfg2)
    assert out.shape == (6000, 8000, 3)
    # (border pixels whose only sample of a colour has a denormal weight are ratios of two denormals: their
    # value is quantisation noise in any arithmetic, so allow a 1e-6 fraction of outliers)
    ok = ((out - out2).abs() <= 2e-5 * out2.abs() + 1e-6) | (out.isnan() & out2.isnan())
    assert float((~ok).float().mean()) < 1e-6, int((~ok).sum())
    # (4) constant-colour scene (no noise) reproduces the colour: kernel regression is a partition of unity
    const = torch.full((H, W), 0.4, device=DEV)
    cfg3 = base_config(ts=16, scale=2, metrics=("L2", "L2", "L2", "L2"))
    o3, _ = hsr.main(const, const[None].repeat(2, 1, 1), cfg3)
    inner = o3[8:-8, 8:-8]
    assert float((inner - 0.4).abs().max()) < 1e-5


@pytest.mark.parametrize("metric0", ["L1", "L1_ref_effective"])
def test_c2_full_size_against_oracle(metric0):
    """BASELINE config C2 at FULL size — 3000x4000, 8 frames, x2 -> 48 MP — against the oracle (one worker process per
    comp frame), every difference attributed to a flipped block-matching tile.  Both readings of the
    headline configuration's level-0 metric (configs/default.yaml:17 `L1`; upstream's L1 kernels are undefined
    behaviour): the intended SAD argmin, and `L1_ref_effective` = what the hardware most likely
    does with the uninitialised shift (flow <- round(flow))."""
    H, W = 3000, 4000
    # the intended-L1 reading with the configuration's own 8 frames (7 oracle workers, ~1.5 min); the other with 3
    ref, comp, _ = synth.make_burst(H, W, 8 if metric0 == "L1" else 3, seed=1234)
    _e2e_vs_oracle(ref, comp, lambda: base_config(ts=16, scale=2, metrics=(metric0, "L2", "L2", "L2")), 16,
                   f"C2 full size {metric0}",
                   max_flipped=FLIP_BUDGET["c2_full" if metric0 == "L1" else "c2_full_eff"], parallel=True,
                   # (L1_ref_effective: ONE of the 144 M output values at 2.1e-4 away from any flipped tile — an isolated
                   # flow-sensitive pixel, see tests/test_fuzz_parity.py)
                   stray=(0, 0.0) if metric0 == "L1" else (4, 1e-3))


@pytest.mark.timeout(1200)
def test_c3_full_size_two_sided_four_frames():
    """a FULL-SIZE comparison with the oracle in both directions inside the driver's suite (until now only in
    profiles/r05_c3_full_oracle.txt, builder-run): the C3 geometry — 3000 x 4000, x2 -> 48 MP, default metrics
    [L1, L2, L2, L2], robustness on — with 4 frames (one oracle worker per comp frame), through tools/full_size_oracle.py's
    logic and the fuzz contract's rules (tests/test_fuzz_parity.py):
      alignment   at most FLIP_BUDGET flipped block-matching tiles in one cluster, the others <= 1e-4 px;
      side H      HIP vs the oracle's robustness + kernels + merge on HIP's flows: same NaN pattern, robustness <= 1e-4,
                  every value <= 1e-4 where every frame is accepted, and where one is being rejected only what the
                  oracle's merge ALONE on HIP's flows and HIP's robustness maps does not show;
      side O      the same with the oracle's flows injected into HIP;
      merge alone on identical flows and robustness maps: every one of the 144 M values <= 1e-4."""
    import os
    import sys

    sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tools"))
    from full_size_oracle import chunked_side
    from helpers import alignment_part, MAX_FLIP_TILES, MAX_ICA_TILES

    H, W, NF, scale = 3000, 4000, 4, 2
    ref, comp, _ = synth.make_burst(H, W, NF, seed=4242)

    def cfg_fn(**hip):
        cfg = base_config(ts=16, scale=scale, metrics=("L1", "L2", "L2", "L2"))
        cfg.robustness.save_mask = True
        if hip:
            cfg.hip = hip
        return cfg

    def hip(cfg):
        cfg.debug = True
        out, dbg = hsr.main(ref, comp, cfg)
        res = out.cpu().numpy(), np.stack(dbg["flow"]), np.stack(dbg["robustness"])
        del out, dbg
        torch.cuda.empty_cache()
        return res

    workers = NF - 1
    o, gflow, hr = hip(cfg_fn())
    cap, cap_h = {}, {}
    want, _, _ = oracle.main_parallel(ref, comp, cfg_fn(), workers=workers, capture=cap, fast=True)
    oflow, o_r = np.stack(cap["flow"]), np.stack(cap["r"])
    al, _ = alignment_part(gflow, oflow)
    print("alignment:", al)
    assert al["nflip"] <= MAX_FLIP_TILES and al["one_cluster"] and al["n_ica"] <= MAX_ICA_TILES and al["dflow"] <= 1e-4, al
    want_h, _, _ = oracle.main_parallel(ref, comp, cfg_fn(), workers=workers, capture=cap_h, fast=True, flows=list(gflow))
    want_hm, _, _ = oracle.main_parallel(ref, comp, cfg_fn(), workers=workers, fast=True, flows=list(gflow), rob=list(hr))
    side_h = chunked_side((H, W), scale, o, want_h, hr, np.stack(cap_h["r"]), want_hm)
    del want_h, want_hm, o
    oi, _, hr_i = hip(cfg_fn(inject_flows=[f for f in oflow]))
    want_om, _, _ = oracle.main_parallel(ref, comp, cfg_fn(), workers=workers, fast=True, flows=list(oflow), rob=list(hr_i))
    side_o = chunked_side((H, W), scale, oi, want, hr_i, o_r, want_om)
    for tag, s in (("H", side_h), ("O", side_o)):
        print(f"side {tag}: {s}")
        assert s["nan_mis"] == 0 and s["m_nan"] == 0, (tag, s)
        assert s["dr"] <= 1e-4, (tag, s)
        assert s["m_max"] <= 1e-4 and s["m_n"] == 0, (tag, s)          # merge alone: everywhere
        assert s["outside"] == 0 and s["unexplained"] == 0, (tag, s)   # whole chain: only what the robustness explains


def test_c4_substitute_13_frames_sensor_size():
    """BASELINE config C4 (a real 13-frame DNG burst) cannot run: no DNG burst and no decoder exist offline.  Its stated
    substitute: 13 frames of 4032x3024, x2, robustness on, white balance != 1, BGGR — size-independent
    properties at full size, and a 512x512 crop of the same burst against the oracle (all 13 frames)."""
    H, W, NF = 3024, 4032, 13
    cfa, wb = ((2, 1), (1, 0)), (2.0, 1.0, 1.5)
    ref, comp, shifts = synth.make_burst(H, W, NF, seed=77, cfa=cfa, wb=wb, max_shift=3.0)

    def cfg0(**hip):
        c = base_config(ts=16, scale=2, metrics=("L1", "L2", "L2", "L2"))
        c.exif = {"cfa_pattern": [list(r) for r in cfa], "iso": 100, "white_balance": list(wb)}
        c.robustness.save_mask = True
        if hip:
            c.hip = hip
        return c

    tref, tcomp = T(ref), T(comp)
    out, dbg = hsr.main(tref, tcomp, cfg0())
    assert out.shape == (2 * H, 2 * W, 3)
    # run-to-run determinism of the 3-stream pipeline: bitwise
    out_b, dbg_b = hsr.main(tref, tcomp, cfg0())
    assert torch.equal(torch.nan_to_num(out, nan=-1.0), torch.nan_to_num(out_b, nan=-1.0))
    assert torch.equal(dbg["accumulated robustness"], dbg_b["accumulated robustness"])
    # sequential operator path (per-frame merge, separate local minimum) == fused pipelined path
    out_s, dbg_s = hsr.main(tref, tcomp, cfg0(fused_merge=False, streams=1))
    ok = ((out - out_s).abs() <= 2e-5 * out_s.abs() + 1e-6) | (out.isnan() & out_s.isnan())
    assert int((~ok).sum()) == 0
    assert_close(N(dbg["accumulated robustness"]), N(dbg_s["accumulated robustness"]), 1e-6, 1e-5, "acc r")
    # the burst's known translations are recovered and most of the image is merged from (almost) all frames
    acc = dbg["accumulated robustness"]
    assert float(acc[8:-8, 8:-8].mean()) > 0.8 * (NF - 1)
    assert bool(torch.isfinite(out[4:-4, 4:-4]).all())
    # the white-balanced channels come back with their gains: channel means follow the scene's (0.5 per channel x gain)
    m = out[64:-64, 64:-64].mean((0, 1)).cpu().numpy()
    assert abs(m[0] / m[1] - 2.0) < 0.1 and abs(m[2] / m[1] - 1.5) < 0.1, m
    del out_b, out_s, dbg_b, dbg_s
    # a crop of the same burst against the oracle
    c, y0, x0 = 512, 1216, 1792
    _e2e_vs_oracle(ref[y0:y0 + c, x0:x0 + c], comp[:, y0:y0 + c, x0:x0 + c], cfg0, 16, "C4 substitute crop",
                   max_flipped=FLIP_BUDGET["c4_crop"], parallel=True)


def test_c5_geometry_48mp_x3():
    """BASELINE config C5 geometry: 6000x8000, x3 -> 18000x24000 (432 MP, 5.2 GB of output) on one GPU with 3 frames:
    size-independent properties (x3 takes the generic-scale merge kernels and their border bands)."""
    H, W = 6000, 8000
    ref, comp, shifts = synth.make_burst_torch(H, W, 3, DEV, seed=5)
    cfg = base_config(ts=16, scale=3, metrics=("L1", "L2", "L2", "L2"))
    out, _ = hsr.main(ref, comp, cfg)
    assert out.shape == (3 * H, 3 * W, 3)
    assert bool(torch.isfinite(out[6:-6, 6:-6]).all())
    # fused burst merge == per-frame operator path
    cfg2 = base_config(ts=16, scale=3, metrics=("L1", "L2", "L2", "L2"))
    cfg2.hip = {"fused_merge": False}
    out2, _ = hsr.main(ref, comp, cfg2)
    ok = ((out - out2).abs() <= 2e-5 * out2.abs() + 1e-6) | (out.isnan() & out2.isnan())
    assert int((~ok).sum()) == 0
    del out2
    # known translation recovered
    pipe = hsr.BurstPipeline(cfg).init_ref(ref)
    _, flow1, _, r1 = pipe.process_frame(comp[0])
    med = flow1.reshape(-1, 2).median(0).values.cpu().numpy()
    assert np.abs(med + shifts[1]).max() < 0.35, (med, shifts[1])
    # a row slab computed on a sub-image (the multi-GPU step B) == the same rows of the whole-image result, bitwise
    from handheld_super_resolution import distributed as hdist

    eng = hdist.HipEngine(cfg).init_ref(ref)
    flows = eng.align_frames([comp[0], comp[1]])
    r0, r1 = 9024, 9024 + 2304  # multiples of the x3 kernel's 48-row workgroup grid (distributed.SLAB_ALIGN)
    slab, _ = eng.merge_rows([comp[0], comp[1]], flows, r0, r1, float(flows[..., 1].abs().max()))
    # (bitwise also at x3: positions are evaluated in full-frame coordinates — hhsr_merge_burst's lr_row_offset)
    assert torch.equal(torch.nan_to_num(slab, nan=-1.0), torch.nan_to_num(out[r0:r1], nan=-1.0))
    del out, slab
    # constant-colour scene (no noise) reproduces the colour: kernel regression is a partition of unity
    const = torch.full((H, W), 0.4, device=DEV)
    o3, _ = hsr.main(const, const[None].repeat(2, 1, 1), base_config(ts=16, scale=3, metrics=("L2",) * 4))
    assert float((o3[12:-12, 12:-12] - 0.4).abs().max()) < 1e-5


def test_determinism_streams_and_wave_fences():
    """Run-to-run determinism: the same burst twice through the 3-stream pipeline, and through 4 streams (k_align_wave
    replaces workgroup barriers by wave-level fences; the frames of a burst share the reference-frame state across
    streams) — flow, robustness and output bitwise equal to the single-stream run."""
    ref, comp, _ = synth.make_burst(768, 1024, 7, seed=3, max_shift=3.0, occluder=True)
    tref, tcomp = T(ref), T(comp)

    def run(streams):
        cfg = base_config(ts=16, scale=2, metrics=("L1", "L2", "L2", "L2"))
        cfg.hip = {"streams": streams}
        pipe = hsr.BurstPipeline(cfg).init_ref(tref)
        frames = pipe.process_frames([tcomp[i] for i in range(6)])
        out, _ = hsr.main(tref, tcomp, cfg)
        torch.cuda.synchronize()
        return [f[1].clone() for f in frames], [f[3].clone() for f in frames], out

    base = run(1)
    for streams in (3, 3, 4, 4):
        got = run(streams)
        for a, b in zip(got[0], base[0]):
            assert torch.equal(a, b), f"flow differs with {streams} streams"
        for a, b in zip(got[1], base[1]):
            assert torch.equal(a, b), f"robustness differs with {streams} streams"
        assert torch.equal(torch.nan_to_num(got[2], nan=-1.0), torch.nan_to_num(base[2], nan=-1.0))


# ------------------------------------------------------------------------------------------ frame sharding
def _shard_cfg(scale, denoiser):
    cfg = base_config(ts=16, scale=scale)
    if denoiser:
        cfg.accumulated_robustness_denoiser.enabled = True
        cfg.accumulated_robustness_denoiser.merge.enabled = True
    return cfg


def _shard_worker(rank, world, port, out_path, scale=2, denoiser=False, n_frames=4):
    import os
    import torch.distributed as dist
    from handheld_super_resolution import distributed as hdist

    os.environ["MASTER_ADDR"] = "127.0.0.1"
    os.environ["MASTER_PORT"] = str(port)
    dist.init_process_group("gloo", rank=rank, world_size=world)  # the processes share the one GPU of the test box
    try:
        torch.cuda.set_device(0)
        ref, comp, _ = synth.make_burst(512, 512, n_frames, seed=17, max_shift=2.0)
        out, dbg = hdist.main_sharded(ref, comp, _shard_cfg(scale, denoiser))
        if rank == 0:
            np.savez(out_path, out=out.cpu().numpy(), acc_r=dbg["accumulated robustness"].cpu().numpy())
        else:
            assert out is None
        # an engine kept across bursts with device-resident frames replays both steps from HIP graphs (eager, capture,
        # replay, replay on new content): every step equals the host-array result above
        cfg = _shard_cfg(scale, denoiser)
        eng = hdist.HipEngine(cfg)
        dref, dcomp = torch.as_tensor(ref).cuda(), torch.as_tensor(comp).cuda()
        for it in range(4):
            if it == 3:
                ref2, comp2, _ = synth.make_burst(512, 512, n_frames, seed=18, max_shift=2.0)
                want2, _ = hdist.main_sharded(ref2, comp2, _shard_cfg(scale, denoiser))
                dref.copy_(torch.as_tensor(ref2))
                dcomp.copy_(torch.as_tensor(comp2))
            o, d = hdist.main_sharded(dref, dcomp, cfg, engine=eng)
            if rank == 0:
                w = out if it < 3 else want2
                assert torch.equal(torch.nan_to_num(o.cpu()), torch.nan_to_num(w.cpu())), f"graph step {it}"
        if n_frames > 1:
            assert eng._plans and not getattr(eng, "_plan_error", None), "the rows plan was not captured"
    finally:
        dist.destroy_process_group()


def _spawn_sharded(tmp_path, world, **kw):
    import socket
    import torch.multiprocessing as mp

    with socket.socket() as s:
        s.bind(("127.0.0.1", 0))
        port = s.getsockname()[1]
    out_path = str(tmp_path / "o.npz")
    mp.spawn(_shard_worker, args=(world, port, out_path, kw.get("scale", 2), kw.get("denoiser", False),
                                  kw.get("n_frames", 4)), nprocs=world, join=True)
    return np.load(out_path)


@pytest.mark.parametrize("world,scale,denoiser,n_frames", [(3, 3, False, 5), (3, 1, True, 3)])
def test_sharded_hip_engine_variants(tmp_path, world, scale, denoiser, n_frames):
    """3 ranks on the one GPU: x3 (generic tile merge kernel, padded slabs, a rank without frames when the burst
    has 2 comp frames) and the accumulated-robustness denoiser (whole-accumulator reduce + rank-0 finish)."""
    got = _spawn_sharded(tmp_path, world, scale=scale, denoiser=denoiser, n_frames=n_frames)
    ref, comp, _ = synth.make_burst(512, 512, n_frames, seed=17, max_shift=2.0)
    want, dbg = hsr.main(ref, comp, _shard_cfg(scale, denoiser))
    assert_close(got["out"], N(want), 2e-5, 1e-6, "sharded == single", max_bad_frac=1e-5)
    assert_close(got["acc_r"], N(dbg["accumulated robustness"]), 0, 1e-6, "acc_r")


def test_sharded_hip_engine_world2(tmp_path):
    """The HIP engine behind main_sharded(): 2 ranks (gloo rendezvous, both on cuda:0) == single process."""
    got = _spawn_sharded(tmp_path, 2)
    ref, comp, _ = synth.make_burst(512, 512, 4, seed=17, max_shift=2.0)
    cfg = base_config(ts=16, scale=2)
    want, dbg = hsr.main(ref, comp, cfg)
    assert_close(got["out"], N(want), 2e-5, 1e-6, "sharded == single", max_bad_frac=1e-5)
    assert_close(got["acc_r"], N(dbg["accumulated robustness"]), 0, 1e-6, "acc_r")
    # and world_size 1 through the same code path
    from handheld_super_resolution import distributed as hdist

    o1, _ = hdist.main_sharded(ref, comp, base_config(ts=16, scale=2))
    assert_close(N(o1), N(want), 2e-5, 1e-6, "main_sharded(world=1) == main", max_bad_frac=1e-5)


# ------------------------------------------------------------------------------------------ mode: grey (monochrome)
MONO = ((1, 1), (1, 1))  # synthetic "CFA" that samples the scene's green plane everywhere


def test_mono_stages_golden(golden):
    """`mode: grey`: per-pixel covariances, one-channel robustness (with the reference's stretched statistics upscale)
    and the one-channel merge / merge_ref against outputs of the reference's own functions and against the oracle."""
    g = golden("grey_mode")
    cfa, wb = [[0, 1], [1, 2]], [1.0, 1.0, 1.0]
    cfg = base_config(mode="grey")
    covs = N(kernels.estimate_kernels(T(g["k_raw"]), cfg))
    assert covs.shape == g["k_raw"].shape + (2, 2)
    assert_close(covs, g["k_cov"], 1e-4, 1e-6, "mono covs")
    rm, rv = robustness.init_robustness(T(g["r_ref"]), cfa, wb, cfg)
    assert tuple(rm.shape) == (1,) + g["r_ref"].shape
    assert_close(N(rm), g["r_means"], 1e-6, 1e-8, "mono ref means")
    assert_close(N(rv), g["r_vars"], 1e-4, 1e-9, "mono ref vars")
    curves = robustness.noise_curves_to_device(np.array(cfg.noise_model.std_curve), np.array(cfg.noise_model.diff_curve), DEV)
    r, R = robustness.compute_robustness(T(g["r_comp"]), T(g["r_means"]), T(g["r_vars"]), T(g["r_flow"]), cfa, wb, curves,
                                         cfg, return_R=True)
    assert_close(N(r), g["r_out"], 0, 1e-4, "mono r")
    H, W = g["m_comp"].shape
    for f64 in (False, True):
        for tag, scale, kern in (("s2", 2, "steerable"), ("s15", 1.5, "steerable"), ("s3", 3, "steerable"),
                                 ("s2iso", 2, "iso")):
            cfg = base_config(ts=16, scale=scale, mode="grey")
            cfg.hip = {"weight_fp64": f64}
            cfg.merging.kernel = kern
            oh, ow = round(scale * H), round(scale * W)
            num, den = T(acc_pattern(oh, ow, 0)), T(acc_pattern(oh, ow, 5))
            merge.merge(T(g["m_comp"]), T(g["m_flow"]), T(g["m_covs"]), T(g["m_r"]), num, den, cfa, cfg)
            assert np.array_equal(N(num)[..., 1:], acc_pattern(oh, ow, 0)[..., 1:]), "channels 1, 2 untouched"
            assert_close(N(num), g[f"m_{tag}_num"], 2e-5, 1e-6, f"mono {tag} num f64={f64}")
            assert_close(N(den), g[f"m_{tag}_den"], 2e-5, 1e-6, f"mono {tag} den f64={f64}")
            num, den = T(acc_pattern(oh, ow, 0)), T(acc_pattern(oh, ow, 5))
            merge.merge_ref(T(g["m_ref"]), T(g["m_covs_ref"]), num, den, cfa, cfg)
            assert_close(N(num), g[f"m_{tag}_numref"], 2e-5, 1e-6, f"mono {tag} numref")
            assert_close(N(den), g[f"m_{tag}_denref"], 2e-5, 1e-6, f"mono {tag} denref")
    cfg = base_config(ts=16, scale=2, mode="grey")
    cfg.accumulated_robustness_denoiser.enabled = True
    cfg.accumulated_robustness_denoiser.merge.enabled = True
    num, den = T(acc_pattern(2 * H, 2 * W, 0)), T(acc_pattern(2 * H, 2 * W, 5))
    merge.merge_ref(T(g["m_ref"]), T(g["m_covs_ref"]), num, den, cfa, cfg, T(g["m_acc_rob"]))
    assert_close(N(num), g["m_den_numref"], 2e-5, 1e-6, "mono denoiser numref")  # channels 1, 2 NOT overwritten
    assert_close(N(den), g["m_den_denref"], 2e-5, 1e-6, "mono denoiser denref")


def test_mono_rob_frame_vector_kernel_vs_float64_kernel():
    """hhsr_mono_rob_frame: the 4-pixels-per-thread float32 kernel (W % 4 == 0, 16-byte aligned planes) against the
    reference-typed float64 kernel the library falls back to for an unaligned R, on flows that leave the image, sit on
    round-half-even ties (x.5), are NaN / huge, and on non-finite reference means; R within 1e-4, same zeros at the
    out-of-image pixels."""
    from handheld_super_resolution import _lib
    rng = np.random.default_rng(77)
    H, W, ts = 208, 336, 16
    ny, nx = -(-H // ts), -(-W // ts)
    cfg = base_config(mode="grey")
    ref = rng.random((H, W), dtype=np.float32)
    comp = np.clip(ref + 0.03 * rng.standard_normal((H, W)).astype(np.float32), 0, 1)
    comp[40:90, 100:180] = rng.random((50, 80), dtype=np.float32)  # an occluder: R spans 0 .. 1
    flow = (rng.standard_normal((ny, nx, 2)) * 6).astype(np.float32)
    flow[0, :, 1] = -30.0          # above the image
    flow[:, 0, 0] = -2.5           # tie + left border
    flow[3, 3] = (0.5, 1.5)        # ties on both axes
    flow[4, 4] = (np.nan, 0.0)
    flow[5, 5] = (1e30, -1e30)
    flow[-1, :, 1] = 25.0          # below
    flow[:, -1, 0] = 3.0           # right border / outside
    flow[6, 6] = (0.0, 0.0)
    cfa, wb = [[0, 1], [1, 2]], [1.0, 1.0, 1.0]
    rm, rv = robustness.init_robustness(T(ref), cfa, wb, cfg)
    rm[0, 120:124, 200:204] = float("nan")
    rm[0, 130, 210] = float("inf")
    curves = robustness.noise_curves_to_device(np.array(cfg.noise_model.std_curve), np.array(cfg.noise_model.diff_curve), DEV)
    std_curve, diff_curve = curves
    sig = robustness.mono_sigma_sq(rm, rv, std_curve)
    cm = kernels.mono_frame_stats(T(comp), cfg, covs=False)[0]
    t = cfg.robustness.tuning
    fl = T(flow)
    S = robustness.compute_s(fl, t.Mt, t.s1, t.s2)
    outs = []
    for off in (0, 1):  # off = 1: R starts 4 bytes past a 16-byte boundary -> the float64 kernel
        buf = torch.full((H * W + 4,), -1.0, dtype=torch.float32, device=DEV)
        R = buf[off:off + H * W].view(H, W)
        _lib.call("hhsr_mono_rob_frame", _lib.ptr(cm), H, W, _lib.ptr(rm), _lib.ptr(sig), _lib.ptr(fl), ny, nx, ts,
                  _lib.ptr(S), _lib.ptr(diff_curve), int(diff_curve.numel()), float(t.t), _lib.ptr(R), _lib.stream())
        outs.append(N(R))
        assert float(buf[off + H * W:].min()) == -1.0 and (off == 0 or float(buf[0]) == -1.0)
    a, b = outs
    assert np.isfinite(a).all() and np.isfinite(b).all() and a.min() >= 0 and a.max() <= 1
    assert 0.05 < (b > 0.5).mean() < 0.95 and ((b > 0) & (b < 1)).mean() > 0.05, "inputs do not exercise R"
    assert_close(a, b, 0, 1e-4, "mono R: float32 vector kernel vs float64 kernel")
    assert (a[:ts] == 0).all() and (b[:ts] == 0).all()  # first tile row: warped outside the image


def test_mono_burst_merge_tile_kernel_vs_generic():
    """`mode: grey`, x2: hhsr_merge_burst takes the LDS-staged tile kernel with a per-pixel covariance window
    (k_merge_burst_quad<.., MONO>); it must agree with the generic per-pixel kernel (config.hip.merge_kernel: generic)
    on flows large enough to push windows over the image border, NaN covariances included."""
    rng = np.random.default_rng(5)
    H, W, n = 208, 272, 3
    cfa = [[0, 1], [1, 2]]
    frames = []
    for k in range(n):
        raw = smooth(rng, H, W)
        flow = (rng.standard_normal((H // 16, W // 16, 2)) * (1.5 + 4 * k)).astype(np.float32)
        flow[0, 0] = (-9.0, 7.5)  # windows over the top-left corner
        cov = np.zeros((H, W, 2, 2), np.float32)
        a, b, c = 0.3 + rng.random((H, W)), 0.2 * rng.standard_normal((H, W)), 0.3 + rng.random((H, W))
        cov[..., 0, 0], cov[..., 0, 1], cov[..., 1, 0], cov[..., 1, 1] = a, b, b, c
        cov[40:44, 60:70] = np.nan  # flat regions (D10)
        r = rng.random((H, W)).astype(np.float32)
        r[100:120, 30:50] = 0
        frames.append((T(raw), T(flow), T(cov), T(r)))
    ref, ref_cov = T(smooth(rng, H, W)), frames[0][2].clone()
    outs = {}
    for kern in ("auto", "generic"):
        for iso in (False, True):
            cfg = base_config(ts=16, scale=2, mode="grey")
            cfg.hip = {"merge_kernel": kern}
            if iso:
                cfg.merging.kernel = "iso"
            num = torch.empty((2 * H, 2 * W, 3), dtype=torch.float32, device=DEV)
            merge.merge_burst(frames, ref, ref_cov, num, None, cfa, cfg, do_ref=True, divide=True)
            outs[kern, iso] = N(num)
    for iso in (False, True):
        a, b = outs["auto", iso], outs["generic", iso]
        assert np.isnan(a[..., 1:]).all() and np.isnan(b[..., 1:]).all()  # 0 / 0: the accumulators have three channels
        assert_close(a[..., 0], b[..., 0], 2e-5, 1e-6, f"mono x2 tile kernel vs generic, iso={iso}")
    assert not np.array_equal(outs["auto", False][..., 0], outs["auto", True][..., 0], equal_nan=True)
    # the 5 x 5 minimum of Alg. 9 taken inside the merge (HHSR_MERGE_LOCAL_MIN) == applied beforehand, bit for bit
    cfg = base_config(ts=16, scale=2, mode="grey")
    assert merge.can_fuse_local_min(cfg, (H, W)) and not merge.can_chain(cfg, (H, W))
    pre = [(f[0], f[1], f[2], robustness.local_min(f[3])) for f in frames]
    a = torch.empty((2 * H, 2 * W, 3), dtype=torch.float32, device=DEV)
    b = torch.empty_like(a)
    acc_a, acc_b = torch.zeros((H, W), device=DEV), torch.zeros((H, W), device=DEV)
    merge.merge_burst(frames, ref, ref_cov, a, None, cfa, cfg, acc_r=acc_a, local_min=True)
    merge.merge_burst(pre, ref, ref_cov, b, None, cfa, cfg, acc_r=acc_b, local_min=False)
    assert torch.equal(torch.nan_to_num(a, nan=-1.0), torch.nan_to_num(b, nan=-1.0)) and torch.equal(acc_a, acc_b)


def test_e2e_mono_golden(golden):
    """main() with `mode: grey` against the reference's own result on the same 128x128 x3 monochrome burst: channel 0
    is the image, channels 1 and 2 are NaN (0/0: the accumulators always have three channels)."""
    from test_oracle_golden import grey_e2e_inputs

    g = golden("grey_mode")
    ref, comp, cfg = grey_e2e_inputs(g)
    cfg.debug = True
    out, dbg = hsr.main(ref, comp, cfg)
    assert_close(np.stack(dbg["flow"]), g["e_flow"], 0, 5e-5, "flow")
    assert_close(np.stack(dbg["robustness"]), g["e_r"], 0, 1e-4, "r")
    assert_close(N(dbg["accumulated robustness"]), g["e_acc_r"], 0, 1e-4, "acc r")
    o = N(out)
    assert np.isnan(o[..., 1:]).all()
    assert_close(o, g["e_out"], 0, 5e-5, "output")
    _, _, cfg2 = grey_e2e_inputs(g)  # fast path: multi-stream front end + fused burst merge
    out2, dbg2 = hsr.main(ref, comp, cfg2)
    assert_close(N(out2), o, 2e-5, 1e-6, "fast path == debug path")
    assert_close(N(dbg2["accumulated robustness"]), g["e_acc_r"], 0, 1e-4, "acc r (fused)")
    _, _, cfg3 = grey_e2e_inputs(g)  # sequential operator-API merge
    cfg3.hip = {"fused_merge": False}
    out3, _ = hsr.main(ref, comp, cfg3)
    assert_close(N(out3), o, 2e-5, 1e-6, "sequential == fused")


@pytest.mark.parametrize("shape,scale,iso", [((501, 619), 2, False), ((486, 520), 1.5, False), ((480, 640), 3, True)])
def test_e2e_mono_vs_oracle(shape, scale, iso):
    """Monochrome bursts of other sizes (odd dimensions are fine without a Bayer grid), scales and the iso kernel."""
    H, W = shape
    ref, comp, _ = synth.make_burst(H, W, 3, seed=66, cfa=MONO, max_shift=2.5, occluder=True)

    def cfg_fn():
        cfg = base_config(ts=16, scale=scale, mode="grey")
        cfg.robustness.save_mask = True
        if iso:
            cfg.merging.kernel = "iso"
        return cfg

    o, want, flipped = _e2e_vs_oracle(ref, comp, cfg_fn, 16, f"mono {shape} x{scale}", 0)
    assert np.isnan(o[..., 1:]).all() and np.isfinite(o[..., 0]).mean() > 0.99


def test_mono_single_rank_is_main():
    from handheld_super_resolution import distributed as hdist

    cfg = base_config(mode="grey")
    cfg.block_matching.tuning.factors = [1, 2, 2, 2]
    assert merge.can_fuse_local_min(cfg, (128, 128)) is True  # (x2 tile kernel; the generic kernels of other scales: no)
    assert merge.can_fuse_local_min(base_config(mode="grey", scale=3), (128, 128)) is False
    ref, comp, _ = synth.make_burst(128, 128, 2, seed=1, cfa=MONO)
    out, _ = hdist.main_sharded(ref, comp, cfg)  # world size 1 is main()
    assert np.isfinite(N(out)[..., 0]).mean() > 0.99


def test_process_mono_burst():
    """process() with `mode: grey` on an in-memory monochrome burst (no CFA / white balance needed): = main() on the
    prepared config + post-processing; channel 0 is the image."""
    from oracle import post

    ref, comp, _ = synth.make_burst(512, 512, 3, seed=8, cfa=MONO)
    cfg = hsr.default_config()
    cfg.verbose = 0
    cfg.mode = "grey"
    cfg.block_matching.tuning.tile_size = 16
    cfg.block_matching.tuning.metrics = ["L2"] * 4
    cfg.postprocessing.do_color_correction = False  # a colour matrix would mix the two NaN channels into channel 0
    burst = {"ref": ref, "comp": comp, "alpha": synth.ALPHA_ISO100, "beta": synth.BETA_ISO100, "orientation": 3}
    img, dbg = hsr.process(burst, cfg)
    assert img.shape == (512, 512, 3) and np.isnan(img[..., 1:]).all()
    out, _ = hsr.main(ref, comp, cfg)
    o = N(out)
    want = post.apply_orientation(post.postprocess(o, False, False, True, {"enabled": True, "amount": 1.5, "radius": 3}), 3)
    # the unsharp mask spreads the D6 / border NaNs of channel 0 by its radius: compare away from them
    ok = np.isfinite(want[..., 0]) & np.isfinite(img[..., 0])
    assert ok.mean() > 0.9
    assert np.abs(img[..., 0][ok] - want[..., 0][ok]).max() < 2e-6
    # the image is the super-resolved scene: close to the noise-free green plane at the output grid
    assert np.nanmean(np.abs(o[..., 0] - np.nanmean(o[..., 0]))) > 0.01


@pytest.mark.parametrize("scale,mode", [(2, "bayer"), (1.5, "bayer"), (2, "grey")])
def test_host_bursts_prefetch(scale, mode):
    """Page-locked host frames: all uploads are queued up front on the upload stream instead of frame by frame —
    bit-identical to device-resident frames and to pageable NumPy frames, float32 and uint16 counts."""
    ref, comp, _ = synth.make_burst_torch(512, 640, 8, torch.device(DEV), seed=21)
    ref_p, comp_p = ref.cpu().pin_memory(), [comp[i].cpu().pin_memory() for i in range(comp.shape[0])]

    def cfg_fn(**hip):
        cfg = base_config(ts=16, scale=scale)
        cfg.mode = mode
        cfg.robustness.save_mask = True
        cfg.hip = hip
        return cfg

    want, wdbg = hsr.main(ref, comp, cfg_fn())  # device-resident
    for hip in ({}, {"streams": 1}):
        for r_, c_ in ((ref_p, comp_p), (ref_p, torch.stack(comp_p).pin_memory()), (N(ref), N(comp))):
            got, dbg = hsr.main(r_, c_, cfg_fn(**hip))
            assert_close(N(got), N(want), 0, 0, f"x{scale} {mode} {hip}")
            assert_close(N(dbg["accumulated robustness"]), N(wdbg["accumulated robustness"]), 0, 0, "accumulated robustness")
    # uint16 counts: uploaded as counts, normalised on the device
    black, white = 64.0, 1023.0
    counts = lambda t: torch.from_numpy(np.clip(np.rint(N(t) * (white - black) + black), 0, white).astype(np.uint16))  # noqa: E731
    ref16, comp16 = counts(ref), [counts(comp[i]) for i in range(comp.shape[0])]
    outs = []
    for pin in (False, True):
        cfg = cfg_fn(raw_norm={"black_levels": [black] * 3, "white_level": white})
        r_ = ref16.pin_memory() if pin else ref16
        c_ = [c.pin_memory() for c in comp16] if pin else comp16
        outs.append(N(hsr.main(r_, c_, cfg)[0]))
    assert_close(outs[1], outs[0], 0, 0, "uint16 counts: prefetched vs per-frame uploads")


# ------------------------------------------------------------------------------------------ HIP graph replay
def test_graph_replay_equals_eager():
    """An engine kept across bursts captures main() in a HIP graph on its second call with the same device tensors and
    replays it afterwards: bit-identical to the eager path, also on new content in the same buffers; what cannot be
    captured runs eagerly."""
    from handheld_super_resolution import distributed as hdist
    from handheld_super_resolution.graph import GraphRunner

    def cfg_fn(**hip):
        cfg = base_config(ts=16, scale=2)
        cfg.robustness.save_mask = True
        cfg.hip = hip
        return cfg

    ref, comp, _ = synth.make_burst_torch(512, 640, 6, torch.device(DEV), seed=11)
    want, wdbg = hsr.main(ref, comp, cfg_fn())
    want, wacc = want.clone(), wdbg["accumulated robustness"].clone()
    eng = hdist.HipEngine(cfg_fn())
    o1, _ = eng.single(ref, comp)  # eager (creates the per-stream plans)
    assert not eng._runner.graphs
    assert_close(N(o1), N(want), 0, 0, "first call (eager)")
    o2, d2 = eng.single(ref, comp)  # capture + first replay
    assert len(eng._runner.graphs) == 1 and not eng._runner.disabled
    assert_close(N(o2), N(want), 0, 0, "capture + replay")
    assert_close(N(d2["accumulated robustness"]), N(wacc), 0, 0, "accumulated robustness from the graph")
    o3, _ = eng.single(ref, comp)
    assert o3.data_ptr() == o2.data_ptr()  # static output of the graph
    assert_close(N(o3), N(want), 0, 0, "replay")
    ref2, comp2, _ = synth.make_burst_torch(512, 640, 6, torch.device(DEV), seed=12)
    want2 = hsr.main(ref2, comp2, cfg_fn())[0].clone()
    ref.copy_(ref2)
    comp.copy_(comp2)
    o4, _ = eng.single(ref, comp)
    assert_close(N(o4), N(want2), 0, 0, "replay on new content in the same buffers")
    assert not np.array_equal(N(want2), N(want), equal_nan=True)
    o5, _ = eng.single(ref2, comp2)  # other tensors: eager again, then their own graph
    assert_close(N(o5), N(want2), 0, 0, "other input tensors")
    eng.single(ref2, comp2)
    assert len(eng._runner.graphs) == 2
    # lists of frames, host arrays, debug / verbose configurations and config.hip.graph = False stay eager
    eng_l = hdist.HipEngine(cfg_fn())
    frames = [comp2[i] for i in range(comp2.shape[0])]
    for _ in range(3):
        ol, _ = eng_l.single(ref2, frames)
    assert len(eng_l._runner.graphs) == 1
    assert_close(N(ol), N(want2), 0, 0, "list of frames")
    eng_off = hdist.HipEngine(cfg_fn(graph=False))
    for _ in range(3):
        oo, _ = eng_off.single(ref2, comp2)
    assert eng_off._runner is None
    assert_close(N(oo), N(want2), 0, 0, "graph off")
    eng_h = hdist.HipEngine(cfg_fn())
    for _ in range(2):
        oh, _ = eng_h.single(N(ref2), N(comp2))
    assert eng_h._runner is None
    assert_close(N(oh), N(want2), 0, 0, "host arrays")
    # the configuration edited in place (as the reference's process() does): the engine drops its graphs
    eng.config.merging.tuning.k_detail = float(eng.config.merging.tuning.k_detail) * 1.25
    cfg_k = cfg_fn()
    cfg_k.merging.tuning.k_detail = eng.config.merging.tuning.k_detail
    want_k = hsr.main(ref, comp, cfg_k)[0].clone()
    ok_, _ = eng.single(ref, comp)
    assert eng._runner is not None and not eng._runner.graphs
    assert_close(N(ok_), N(want_k), 0, 0, "after an in-place edit of the configuration")
    assert not np.array_equal(N(want_k), N(want2), equal_nan=True)
    eng.single(ref, comp)
    ok2, _ = eng.single(ref, comp)
    assert eng._runner.graphs
    assert_close(N(ok2), N(want_k), 0, 0, "re-captured with the edited configuration")
    eng.config.merging.tuning.k_detail = cfg_fn().merging.tuning.k_detail
    for _ in range(3):
        eng.single(ref, comp)
    # a function that reads back to the host cannot be captured: the runner falls back to eager execution
    r = GraphRunner(lambda x: x * float(x.sum().item()), torch.device(DEV))
    a = torch.ones(4, device=DEV)
    r(a)
    out = r(a)
    assert r.disabled and torch.equal(out, a * 4)
    assert torch.equal(r(a), a * 4)
    torch.cuda.synchronize()
    o6, _ = eng.single(ref, comp)  # the device is fine after the failed capture
    assert_close(N(o6), N(want2), 0, 0, "replay after a failed capture elsewhere")


# ------------------------------------------------------------------------------------------ chunk-batched front end
def test_batched_operators_equal_single():
    """The *_batch entry points (one launch per stage for a chunk of frames: FFT phases, pyramid levels, alignment
    levels, raw pass) give every frame the bits of the single-frame entry points — also for lists longer than
    HHSR_MAX_BATCH (rounds) and through a plan that holds fewer spectra than frames."""
    from handheld_super_resolution import _lib

    n = _lib.MAX_BATCH + 3
    ref, comp, _ = synth.make_burst_torch(384, 512, n + 1, torch.device(DEV), seed=33)
    frames = [comp[i] for i in range(n)]
    cfg = base_config(ts=16, scale=2, metrics=("L1", "L2", "L2", "L2"))
    cfg.block_matching.tuning.factors = [1, 2, 2, 2]
    greys = utils_image.compute_grey_images_batch(frames, "FFT")
    for g, f in zip(greys, frames):
        assert torch.equal(g, utils_image.compute_grey_images(f, "FFT"))
    assert torch.equal(utils_image.compute_grey_images_batch(frames[:3], "FFT")[2], greys[2])  # (a smaller batch, same plan)
    pyrs = alignment.build_gaussian_pyramids(greys, cfg.block_matching.tuning.factors)
    for p, g in zip(pyrs, greys):
        for a, b in zip(p, alignment.build_gaussian_pyramid(g, cfg.block_matching.tuning.factors)):
            assert torch.equal(a, b)
    state = alignment.init_alignment(utils_image.compute_grey_images(ref, "FFT"), cfg)
    assert alignment.can_align_batch(cfg)
    flows = alignment.align_batch(state[0], state[5], pyrs, cfg)
    for fl, g, p in zip(flows, greys, pyrs):
        assert torch.equal(fl, alignment.align(*state, g, cfg, moving_pyramid=p))
    cfa, wb = [[0, 1], [1, 2]], [1.9, 1.0, 1.6]
    stats = kernels.frame_stats_batch(frames, cfa, wb, cfg)
    for (m, _, c), f in zip(stats, frames):
        m1, _, c1 = kernels.frame_stats(f, cfa, wb, cfg)
        assert torch.equal(m, m1) and torch.equal(torch.nan_to_num(c), torch.nan_to_num(c1))


@pytest.mark.parametrize("hip", [{"chunk": 8}, {"chunk": 3, "streams": 2}, {"streams": 1}])
def test_batched_front_end_equals_per_frame(hip):
    """main() with the chunk-batched front end (default) == main() with one launch per frame and stage
    (config.hip.batch: false), bit for bit, for several chunk sizes / stream counts."""
    ref, comp, _ = synth.make_burst_torch(512, 640, 10, torch.device(DEV), seed=44, max_shift=3.0)

    def run(**h):
        cfg = base_config(ts=16, scale=2, metrics=("L1", "L2", "L2", "L2"))
        cfg.robustness.save_mask = True
        cfg.hip = h
        out, dbg = hsr.main(ref, comp, cfg)
        return torch.nan_to_num(out, nan=-1.0), dbg["accumulated robustness"]

    want = run(batch=False)
    got = run(**hip)
    assert torch.equal(got[0], want[0]) and torch.equal(got[1], want[1])


def test_batched_front_end_equals_per_frame_mono():
    """The same for a monochrome burst (`mode: grey`: the frames are their own grey images — pyramid and alignment
    levels one launch per chunk, per-pixel statistics per frame), graph replay included."""
    ref, comp, _ = synth.make_burst_torch(512, 640, 7, torch.device(DEV), seed=45, max_shift=3.0, cfa=MONO)

    def run(**h):
        cfg = base_config(ts=16, scale=2, mode="grey")
        cfg.robustness.save_mask = True
        cfg.hip = h
        outs = [hsr.main(ref, comp, cfg) for _ in range(3)]  # third call: replayed from the HIP graph
        return [(torch.nan_to_num(o, nan=-1.0), d["accumulated robustness"]) for o, d in outs]

    want = run(batch=False, graph=False)[0]
    for got in run() + run(chunk=3, streams=2):
        assert torch.equal(got[0], want[0]) and torch.equal(got[1], want[1])


def test_merge_burst_chain_equals_single_launch():
    """merge_burst_chain (a chain of launches: the frames that have arrived are merged into parked parity-class
    accumulators, the last link adds the rest, the reference frame and the normalisation) == merge_burst (one launch), bit
    for bit — also for tiles that the early links run wave-uniform but a LATER frame's flow sends down the per-pixel path
    (the last link recomputes them), for tiles at the image border, with the fused 5 x 5 minimum and the fused accumulated
    robustness, for 2 to 5 links."""
    ref, comp, _ = synth.make_burst_torch(512, 640, 10, torch.device(DEV), seed=3, max_shift=3.0)
    for lmin, accr in ((True, True), (False, False)):
        cfg = base_config(ts=16, scale=2, metrics=("L1", "L2", "L2", "L2"))
        pipe = hsr.BurstPipeline(cfg).init_ref(ref)
        frames = pipe.process_frames([comp[i] for i in range(9)], None, fuse_local_min=lmin)
        # frame 7 (a late link) gets a huge flow in an interior tile and one that pushes a window over the border; frame 2
        # (an early link) another
        fl = frames[7][1].clone()
        fl[10, 12] = torch.tensor([140.0, -95.0], device=DEV)
        fl[3, 37] = torch.tensor([60.0, 2.0], device=DEV)
        frames[7] = (frames[7][0], fl, frames[7][2], frames[7][3])
        fl = frames[2][1].clone()
        fl[20, 5] = torch.tensor([-90.0, 30.0], device=DEV)
        frames[2] = (frames[2][0], fl, frames[2][2], frames[2][3])
        H, W = ref.shape
        want = torch.empty((2 * H, 2 * W, 3), dtype=torch.float32, device=DEV)
        acc_w = torch.zeros((H, W), dtype=torch.float32, device=DEV) if accr else None
        merge.merge_burst(frames, pipe.ref, pipe.ref_covs, want, None, pipe.cfa, cfg, acc_r=acc_w, local_min=lmin)
        assert merge.can_chain(cfg, (H, W))
        cls = merge.chain_buffer((H, W), torch.device(DEV))
        for cuts in ((1,), (5,), (8,), (9,), (4, 6), (2, 3, 7, 8), (3, 9)):
            got = torch.full_like(want, -7.0)
            acc_g = torch.full((H, W), -7.0, dtype=torch.float32, device=DEV) if accr else None
            cls.fill_(float("nan"))
            done = 0
            for k in cuts:
                merge.merge_burst_chain(frames[:k], done, pipe.ref, pipe.ref_covs, got, pipe.cfa, cfg, cls, False, local_min=lmin)
                done = k
            merge.merge_burst_chain(frames, done, pipe.ref, pipe.ref_covs, got, pipe.cfa, cfg, cls, True, acc_r=acc_g,
                                    local_min=lmin)
            assert torch.equal(torch.nan_to_num(got, nan=-1.0), torch.nan_to_num(want, nan=-1.0)), f"cuts={cuts} lmin={lmin}"
            if accr:
                assert torch.equal(acc_g, acc_w)
    cfg3 = base_config(ts=16, scale=3)
    assert not merge.can_chain(cfg3, (512, 640))


# ------------------------------------------------------------------------------------------ host-resident bursts
def test_host_burst_runner_tuning_knobs():
    """config.hip.host_chunk_sizes / merge_link_after (explicit chunks and chained-merge links of a host-resident burst)
    give the eager path's bits; chunk sizes that do not cover the burst are the caller's error, not a silent fall-back."""
    from handheld_super_resolution import distributed as hdist

    ref, comp, _ = synth.make_burst(512, 640, 9, seed=15, max_shift=2.5)
    ref_h, comp_h = torch.from_numpy(ref).pin_memory(), [torch.from_numpy(comp[i]).pin_memory() for i in range(8)]

    def cfg_fn(**hip):
        cfg = base_config(ts=16, scale=2, metrics=("L1", "L2", "L2", "L2"))
        cfg.hip = hip
        return cfg

    want, _ = hsr.main(ref, comp, cfg_fn(graph=False))
    eng = hdist.HipEngine(cfg_fn(host_chunk_sizes=[1, 3, 2, 1, 1], merge_link_after=[1, 2]))
    for it in range(3):
        got, _ = eng.single(ref_h, comp_h)
        assert torch.equal(torch.nan_to_num(got, nan=-1.0), torch.nan_to_num(want, nan=-1.0)), it
    st = eng._host.states[next(iter(eng._host.states))]
    assert not eng._host.disabled and [len(c) for c in st.chunks] == [1, 3, 2, 1, 1] and [k for _, k in st.links] == [4, 6]
    bad = hdist.HipEngine(cfg_fn(host_chunk_sizes=[4, 3]))
    bad.single(ref_h, comp_h)  # (the first call of a shape runs eagerly)
    with pytest.raises(ValueError, match="host_chunk_sizes"):
        bad.single(ref_h, comp_h)


@pytest.mark.parametrize("kind", ["f32_pinned", "f32_numpy", "u16_pinned", "u16_numpy"])
def test_host_burst_runner_equals_eager(kind):
    """Bursts that start in host memory (the reference's signature / timer scope): graph.HostBurstRunner — eager uploads
    into static staging, per-chunk HIP graphs — gives the eager path's bits on every call (eager, capture, replay,
    replay on new content), for page-locked and pageable frames, float32 frames and uint16 sensor counts."""
    from handheld_super_resolution import distributed as hdist

    black, white = 64.0, 1023.0

    def burst(seed):
        ref, comp, _ = synth.make_burst(512, 640, 9, seed=seed, max_shift=2.5)
        if kind.startswith("u16"):
            c = lambda a: np.clip(np.rint(a * (white - black) + black), 0, white).astype(np.uint16)  # noqa: E731
            ref, comp = c(ref), c(comp)
        return ref, comp

    def cfg_fn(graph):
        cfg = base_config(ts=16, scale=2, metrics=("L1", "L2", "L2", "L2"))
        cfg.robustness.save_mask = True
        cfg.hip = {"graph": graph}
        if kind.startswith("u16"):
            cfg.hip["raw_norm"] = {"black_levels": [black] * 3, "white_level": white}
        return cfg

    def host(a):
        t = torch.from_numpy(a)
        return t.pin_memory() if kind.endswith("pinned") else a

    ref0, comp0 = burst(5)
    ref_h, comp_h = host(ref0), [host(comp0[i]) for i in range(comp0.shape[0])]
    want, wdbg = hsr.main(ref0, comp0, cfg_fn(False))  # eager
    eng = hdist.HipEngine(cfg_fn(True))
    for it in range(4):
        if it == 3:  # new content in the same host buffers
            ref1, comp1 = burst(6)
            want, wdbg = hsr.main(ref1, comp1, cfg_fn(False))
            for dst, src in zip([ref_h, *comp_h], [ref1, *comp1]):
                (dst if not torch.is_tensor(dst) else dst.numpy())[...] = src
        got, dbg = eng.single(ref_h, comp_h)
        assert torch.equal(torch.nan_to_num(got, nan=-1.0), torch.nan_to_num(want, nan=-1.0)), f"{kind} call {it}"
        assert torch.equal(dbg["accumulated robustness"], wdbg["accumulated robustness"])
    st = eng._host.states[next(iter(eng._host.states))]
    assert not eng._host.disabled and st != "seen" and len(st.g_chunks) >= 2, getattr(eng._host, "error", None)
    if kind.startswith("f32"):  # upload-bound bursts chain the merge: 8 comp frames = chunks 4, 2, 1, 1 -> links after 4 and 6
        assert st.chain and [k for _, k in st.links] == [4, 6]
    else:
        assert not st.chain and not st.links


@pytest.mark.parametrize("n_comp", [1, 2, 3])
def test_host_burst_runner_tiny_bursts(n_comp):
    """Bursts of 2-4 frames through the runner (one chunk, no chain, single-frame chunks): eager, capture, replay."""
    from handheld_super_resolution import distributed as hdist

    ref, comp, _ = synth.make_burst(512, 640, n_comp + 1, seed=13, max_shift=2.0)
    cfg = base_config(ts=16, scale=2)
    want = hsr.main(T(ref), T(comp), base_config(ts=16, scale=2))[0]
    eng = hdist.HipEngine(cfg)
    for it in range(3):
        got, _ = eng.single(ref, [comp[i] for i in range(n_comp)])
        assert torch.equal(torch.nan_to_num(got, nan=-1.0), torch.nan_to_num(want, nan=-1.0)), f"call {it}"
    st = next(iter(eng._host.states.values()))
    assert not eng._host.disabled and st != "seen" and not st.chain


def test_main_numpy_serving_loop():
    """main() itself, called again and again with NumPy arrays and the same configuration object (the reference's
    signature in a serving loop), goes through the runner from the third call on and still hands out fresh tensors."""
    from handheld_super_resolution import super_resolution as sr

    ref, comp, _ = synth.make_burst(512, 640, 6, seed=8, max_shift=2.0)
    cfg = base_config(ts=16, scale=2)
    outs = [hsr.main(ref, comp, cfg)[0] for _ in range(4)]
    for o in outs[1:]:
        assert torch.equal(torch.nan_to_num(o), torch.nan_to_num(outs[0]))
    assert len({o.data_ptr() for o in outs}) == 4
    runner = [r for c, _, r in sr._main_runners if c is cfg][0]
    assert not runner.disabled and any(s != "seen" for s in runner.states.values())
    cfg.scale = 1  # edited in place: a new runner, the eager result of the new configuration
    o1 = hsr.main(ref, comp, cfg)[0]
    assert tuple(o1.shape) == (512, 640, 3)
    cfg2 = base_config(ts=16, scale=1)
    assert torch.equal(torch.nan_to_num(o1), torch.nan_to_num(hsr.main(ref, comp, cfg2)[0]))


# ------------------------------------------------------------------------------------------ multi-GPU: seam, reduce
def _seam_burst():
    ref, comp, _ = synth.make_burst(512, 512, 4, seed=17, max_shift=0.0)
    comp = comp.copy()
    yy = np.arange(512, dtype=np.float32)[:, None]
    comp[1] = np.clip(comp[1] + 0.06 * np.exp(-(((yy - 250) / 8.0) ** 2)), 0, 1).astype(np.float32)
    flows = np.zeros((3, 32, 32, 2), np.float32)
    flows[1, 14, :, 1] = 3.0  # irregular flow directly above slab 1's sub-image (raw rows from 240 = tile row 15 on)
    return ref, comp, flows


def _shard_worker2(rank, world, port, out_path, strategy, seam):
    import os
    import torch.distributed as dist
    from handheld_super_resolution import distributed as hdist

    os.environ["MASTER_ADDR"] = "127.0.0.1"
    os.environ["MASTER_PORT"] = str(port)
    dist.init_process_group("gloo", rank=rank, world_size=world)
    try:
        torch.cuda.set_device(0)
        cfg = base_config(ts=16, scale=2)
        cfg.robustness.save_mask = True
        if seam:
            ref, comp, flows = _seam_burst()

            class SeamEngine(hdist.HipEngine):  # "alignment" returns the crafted field (this rank's frames of it)
                def align_frames(self, comp_imgs):
                    mine = hdist.shard_indices(3, rank, world)
                    return torch.as_tensor(flows[mine], device="cuda")

            eng = SeamEngine(cfg)
        else:
            ref, comp, _ = synth.make_burst(512, 512, 6, seed=17, max_shift=2.0)
            eng = hdist.HipEngine(cfg)
        dref, dcomp = torch.as_tensor(ref).cuda(), torch.as_tensor(comp).cuda()
        outs = []
        for it in range(3):  # eager, capture, replay
            o, d = hdist.main_sharded(dref, dcomp, cfg, engine=eng, strategy=strategy)
            if rank == 0:
                outs.append((o.cpu().numpy().copy(), d["accumulated robustness"].cpu().numpy().copy()))
        if rank == 0:
            for o, a in outs[1:]:
                assert np.array_equal(o, outs[0][0], equal_nan=True) and np.array_equal(a, outs[0][1])
            np.savez(out_path, out=outs[0][0], acc_r=outs[0][1])
    finally:
        dist.destroy_process_group()


def _spawn2(tmp_path, world, strategy, seam):
    import socket
    import torch.multiprocessing as mp

    with socket.socket() as s:
        s.bind(("127.0.0.1", 0))
        port = s.getsockname()[1]
    out_path = str(tmp_path / "o.npz")
    mp.spawn(_shard_worker2, args=(world, port, out_path, strategy, seam), nprocs=world, join=True)
    return np.load(out_path)


def test_sharded_seam_flow_irregularity(tmp_path):
    """irregular flow directly above a sub-image.  S (3 x 3 TILE neighbourhood) is evaluated on the
    full gathered field (flow_rows of hhsr_rob_frames), so the row-sharded HIP result is the single-GPU one bit for bit;
    the slice-only evaluation of round 2 differs on this burst."""
    ref, comp, flows = _seam_burst()
    cfg = base_config(ts=16, scale=2)
    cfg.robustness.save_mask = True
    cfg.hip = {"inject_flows": [f for f in flows]}
    want, wdbg = hsr.main(ref, comp, cfg)
    got = _spawn2(tmp_path, 2, "rows", True)
    assert np.array_equal(got["out"], N(want), equal_nan=True)
    assert np.array_equal(got["acc_r"], N(wdbg["accumulated robustness"]))
    # the case is real: the sub-image of slab 1 with S from the slice (no rows around it) differs
    sub = hsr.BurstPipeline(base_config(ts=16, scale=2)).init_ref(T(ref[240:]), alignment=False)
    f1 = T(flows[1])
    a = sub.process_frame(T(comp[1, 240:]), flow=f1[15:].contiguous().clone())[3]
    sub.flow_rows = (15, 0)
    b = sub.process_frame(T(comp[1, 240:]), flow=f1[15:])[3]
    assert float((a - b).abs().max()) > 1e-3


@pytest.mark.parametrize("world", [2, 3])
def test_sharded_reduce_strategy(tmp_path, world):
    """strategy="reduce" (north star): frames one per rank through the whole chain, reduce-scatter of the float32
    accumulators over row slabs, reference frame + normalisation per slab — equals the single-GPU result up to the
    summation order of the partial sums; replayed from HIP graphs on the second / third burst."""
    ref, comp, _ = synth.make_burst(512, 512, 6, seed=17, max_shift=2.0)
    cfg = base_config(ts=16, scale=2)
    cfg.robustness.save_mask = True
    want, wdbg = hsr.main(ref, comp, cfg)
    got = _spawn2(tmp_path, world, "reduce", False)
    assert_close(got["out"], N(want), 0, 2e-6, "reduce strategy == single")
    assert_close(got["acc_r"], N(wdbg["accumulated robustness"]), 0, 2e-6, "acc_r")


def _bench_shared_gpu(ranks, *extra):
    import json
    import os
    import subprocess
    import sys

    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    env = dict(os.environ, HHSR_BENCH_SHARE_GPU="1")
    for k in ("WORLD_SIZE", "RANK", "LOCAL_RANK", "MASTER_PORT"):
        env.pop(k, None)
    p = subprocess.run([sys.executable, os.path.join(root, "bench.py"), "--gpus", str(ranks), "--backend", "gloo", *extra,
                        "--full", "--no-cpu-baseline"], capture_output=True, text=True, env=env, timeout=850)  # (host legs: N = 1 only)
    lines = [l for l in p.stdout.splitlines() if l.startswith("{")]
    assert p.returncode == 0 and len(lines) == 1, p.stderr[-3000:]
    return json.loads(lines[0])


def _check_two_strategy_line(rec, ranks, headline):
    other = "reduce" if headline == "rows" else "rows"
    assert rec["n_gpus"] == ranks and rec["rccl_ranks"] == ranks and rec["ranks_agree"] and rec["backend"] == "gloo"
    assert rec["value"] > 0 and rec["strategy"] == headline and headline in rec["config"]["parallelism"]
    assert rec["engine"].startswith("HipEngine") and "HIP graph replay" in rec["launch"]
    assert not rec.get("errors"), rec.get("errors")
    st = rec["strategies"]  # BOTH curves in one record (VERDICT r4 #2a): the driver only passes --gpus N
    assert st[headline]["headline"] and st[headline]["ms_per_step"] == rec["ms_per_step"] and not st[other]["headline"]
    for k in (headline, other):
        assert st[k]["value"] > 0 and st[k]["compute_only_max_rank_ms"] is not None
        assert 0 < st[k]["compute_only_max_rank_ms"] <= st[k]["ms_per_step"] * 1.5  # (shared GPU: ranks contend; sanity only)
    assert "all_gather_in_bytes" in st["rows"]["rccl_bytes_per_rank"] and "reduce_scatter_in_bytes" in st["reduce"]["rccl_bytes_per_rank"]


@pytest.mark.timeout(900)
@pytest.mark.parametrize("strategy", ["rows", "reduce"])
def test_bench_two_ranks_share_the_gpu(strategy):
    """`bench.py --gpus 2` with the real HipEngine: the script re-executes itself under torch.distributed.run, two ranks
    rendezvous over gloo (RCCL needs one GPU per rank; HHSR_BENCH_SHARE_GPU=1 puts both on device 0), run
    main_sharded with the chosen strategy from HIP graphs and rank 0 prints ONE JSON line with n_gpus = 2 that carries
    BOTH strategies' timings."""
    rec = _bench_shared_gpu(2, "--strategy", strategy, "--height", "768", "--width", "1024", "--frames", "6", "--steps", "3",
                            "--warmup", "2")
    _check_two_strategy_line(rec, 2, strategy)


@pytest.mark.timeout(900)
def test_bench_eight_ranks_share_the_gpu():
    """VERDICT r4 #2b: the rank count the target names through the command the driver runs — `bench.py --gpus 8` (only the
    backend differs: gloo, eight processes on the one GPU), 20 frames (19 comp frames: 3, 3, 3, 2, 2, 2, 2, 2) at 1024 x 1024,
    default strategy `rows` as the headline and `reduce` next to it in the same record, every rank replaying HIP graphs."""
    rec = _bench_shared_gpu(8, "--height", "1024", "--width", "1024", "--frames", "20", "--steps", "3", "--warmup", "2")
    _check_two_strategy_line(rec, 8, "rows")


# ------------------------------------------------------------------------------------------ round 4: RCCL, C3 / C5 multi-rank
def _slab_checksum(t):
    """Order-sensitive 2 x 64-bit checksum of a float32 tensor's BIT PATTERNS (NaN payloads included), row chunk by row
    chunk on the device: equal checksums <=> bitwise equal slabs for every practical purpose, whatever the size."""
    flat = t.reshape(-1).view(torch.int32)
    a = b = 0
    step = 1 << 26
    for i in range(0, flat.numel(), step):
        x = flat[i:i + step].to(torch.int64)
        w = (torch.arange(i, i + x.numel(), device=t.device, dtype=torch.int64) % 1000003) + 1
        a = (a + int(x.sum())) & 0xFFFFFFFFFFFFFFFF
        b = (b + int((x * w).sum())) & 0xFFFFFFFFFFFFFFFF
    return a, b


def _big_cfg(scale, hip=None):
    cfg = base_config(ts=16, scale=scale, metrics=("L1", "L2", "L2", "L2"))
    cfg.hip = dict(hip or {})
    return cfg


def _big_worker(rank, world, port, out_dir, H, W, nf, scale, strategy, save):
    import json
    import os
    import torch.distributed as dist
    from handheld_super_resolution import distributed as hdist

    os.environ["MASTER_ADDR"] = "127.0.0.1"
    os.environ["MASTER_PORT"] = str(port)
    dist.init_process_group("gloo", rank=rank, world_size=world)  # the ranks share the one GPU of the test box
    try:
        torch.cuda.set_device(0)
        dev = torch.device("cuda", 0)
        ref, comp, _ = synth.make_burst_torch(H, W, nf, dev, seed=1234)
        cfg = _big_cfg(scale)
        eng = hdist.HipEngine(cfg)
        sums = []
        for it in range(3):  # eager, capture, replay (rows: RowsPlan; reduce: partial / finish graphs)
            slab, dbg = hdist.main_sharded(ref, comp, cfg, engine=eng, gather=False, strategy=strategy)
            torch.cuda.synchronize()
            sums.append(_slab_checksum(slab))
        assert sums[1] == sums[0] and sums[2] == sums[0], f"rank {rank}: eager / capture / replay differ: {sums}"
        if strategy == "rows":
            assert eng._plans and not getattr(eng, "_plan_error", None), getattr(eng, "_plan_error", None)
        rec = {"rows": list(dbg["rows"]), "sum": list(sums[0]), "recomputed": bool(dbg.get("flow_bound_recomputed", False))}
        if save:
            np.save(os.path.join(out_dir, f"slab{rank}.npy"), slab.cpu().numpy())
        with open(os.path.join(out_dir, f"rank{rank}.json"), "w") as f:
            json.dump(rec, f)
    finally:
        dist.destroy_process_group()


def _spawn_big(tmp_path, world, *a):
    import json
    import socket
    import torch.multiprocessing as mp

    with socket.socket() as s_:
        s_.bind(("127.0.0.1", 0))
        port = s_.getsockname()[1]
    mp.spawn(_big_worker, args=(world, port, str(tmp_path), *a), nprocs=world, join=True)
    return [json.load(open(tmp_path / f"rank{r}.json")) for r in range(world)]


@pytest.mark.timeout(1500)
@pytest.mark.parametrize("world,strategy", [(2, "rows"), (2, "reduce"), (8, "rows"), (8, "reduce")])
def test_c3_full_size_sharded(tmp_path, world, strategy):
    """BASELINE config C3 at FULL size — 3000 x 4000, 20 frames, x2 — through main_sharded with 2 and with 8 ranks (the rank
    count C3 names: 19 comp frames -> 3, 3, 3, 2, 2, 2, 2, 2; round 5) sharing the GPU (gloo rendezvous; engine kept: eager,
    capture, replay): "rows" (uneven slabs on the x2 tile grid) equals main() bit for bit on every slab, "reduce" within
    float32 summation order (2e-6)."""
    H, W, nf = 3000, 4000, 20
    recs = _spawn_big(tmp_path, world, H, W, nf, 2, strategy, strategy == "reduce")
    ref, comp, _ = synth.make_burst_torch(H, W, nf, DEV, seed=1234)
    want, _ = hsr.main(ref, comp, _big_cfg(2))
    assert recs[0]["rows"][0] == 0 and recs[-1]["rows"][1] == 2 * H
    assert all(recs[r]["rows"][1] == recs[r + 1]["rows"][0] and recs[r]["rows"][1] > recs[r]["rows"][0] for r in range(world - 1))
    for r, rec in enumerate(recs):
        r0, r1 = rec["rows"]
        if strategy == "rows":
            assert not rec["recomputed"]
            assert tuple(rec["sum"]) == _slab_checksum(want[r0:r1]), f"slab {r} ({r0}:{r1}) differs from main()"
        else:
            got = torch.from_numpy(np.load(tmp_path / f"slab{r}.npy")).to(DEV)
            w = want[r0:r1]
            assert bool((got.isnan() == w.isnan()).all())
            assert float((torch.nan_to_num(got) - torch.nan_to_num(w)).abs().max()) <= 2e-6
            del got


@pytest.mark.timeout(1800)
@pytest.mark.parametrize("world,nf", [(2, 7), (8, 20)])
def test_c5_geometry_sharded(tmp_path, world, nf):
    """BASELINE config C5's geometry — 6000 x 8000, x3 -> 18000 x 24000 — through main_sharded("rows"): 7 frames on 2 ranks,
    and (round 5) C5 ITSELF — 20 frames on 8 ranks — all sharing the one GPU: every slab bitwise equal to main()
    (checksums of the bit patterns: a slab is 0.65 - 2.6 GB)."""
    H, W = 6000, 8000
    recs = _spawn_big(tmp_path, world, H, W, nf, 3, "rows", False)
    ref, comp, _ = synth.make_burst_torch(H, W, nf, DEV, seed=1234)
    want, _ = hsr.main(ref, comp, _big_cfg(3))
    assert recs[0]["rows"][0] == 0 and recs[-1]["rows"][1] == 3 * H
    for r, rec in enumerate(recs):
        r0, r1 = rec["rows"]
        assert not rec["recomputed"]
        assert tuple(rec["sum"]) == _slab_checksum(want[r0:r1]), f"slab {r} ({r0}:{r1}) differs from main()"


def _rccl_worker(rank, port, out_path):
    import os
    import torch.distributed as dist
    from handheld_super_resolution import distributed as hdist

    os.environ["MASTER_ADDR"] = "127.0.0.1"
    os.environ["MASTER_PORT"] = str(port)
    os.environ.setdefault("HSA_ENABLE_IPC_MODE_LEGACY", "0")
    torch.cuda.set_device(0)
    dev = torch.device("cuda", 0)
    dist.init_process_group("nccl", rank=0, world_size=1, device_id=dev)   # RCCL, the call bench.py makes
    try:
        assert dist.get_backend() == "nccl"
        ref, comp, _ = synth.make_burst(512, 640, 7, seed=21, max_shift=2.0)
        dref, dcomp = torch.as_tensor(ref).cuda(), torch.as_tensor(comp).cuda()
        res = {}
        for strategy in ("rows", "reduce"):
            cfg = base_config(ts=16, scale=2)
            cfg.robustness.save_mask = True
            cfg.hip = {"stage_frames": 2}  # world 1: two frames per stage -> three all-gathers per burst
            eng = hdist.HipEngine(cfg)
            outs = []
            for it in range(3):  # eager, capture, replay: the collectives run between the graphs every time
                o, d = hdist.main_sharded(dref, dcomp, cfg, engine=eng, strategy=strategy, force_sharded=True,
                                          gather=(it != 1))
                torch.cuda.synchronize()
                outs.append(o.cpu().numpy().copy())
            assert np.array_equal(outs[1], outs[0], equal_nan=True) and np.array_equal(outs[2], outs[0], equal_nan=True)
            if strategy == "rows":
                assert eng._plans and not getattr(eng, "_plan_error", None), getattr(eng, "_plan_error", None)
            res[strategy] = outs[0]
            res[strategy + "_acc"] = d["accumulated robustness"].cpu().numpy()
        # a caller-given flow bound: no host read, the device flag comes back
        cfg = base_config(ts=16, scale=2)
        o, d = hdist.main_sharded(dref, dcomp, cfg, strategy="rows", force_sharded=True, max_flow=16.0)
        assert not bool(d["flow_bound_exceeded"])
        np.savez(out_path, **res)
    finally:
        dist.destroy_process_group()


@pytest.mark.timeout(600)
def test_rccl_one_rank_group(tmp_path):
    """The RCCL call sites — init_process_group("nccl", device_id=), all_gather_into_tensor (sync and async_op between the
    two streams of a RowsPlan), reduce_scatter_tensor on the packed accumulators, all_reduce, gather — executed on a
    1-rank RCCL group through main_sharded(force_sharded=True): both strategies equal main()."""
    import socket
    import torch.multiprocessing as mp

    with socket.socket() as s_:
        s_.bind(("127.0.0.1", 0))
        port = s_.getsockname()[1]
    out_path = str(tmp_path / "o.npz")
    mp.spawn(_rccl_worker, args=(port, out_path), nprocs=1, join=True)
    got = np.load(out_path)
    ref, comp, _ = synth.make_burst(512, 640, 7, seed=21, max_shift=2.0)
    cfg = base_config(ts=16, scale=2)
    cfg.robustness.save_mask = True
    want, dbg = hsr.main(ref, comp, cfg)
    assert np.array_equal(got["rows"], N(want), equal_nan=True)
    assert np.array_equal(got["rows_acc"], N(dbg["accumulated robustness"]))
    assert_close(got["reduce"], N(want), 0, 2e-6, "reduce on RCCL == main")
    assert_close(got["reduce_acc"], N(dbg["accumulated robustness"]), 0, 2e-6, "acc_r")


def _corner_worker(rank, world, port, out_path, variant):
    import os
    import torch.distributed as dist
    from handheld_super_resolution import distributed as hdist

    os.environ["MASTER_ADDR"] = "127.0.0.1"
    os.environ["MASTER_PORT"] = str(port)
    dist.init_process_group("gloo", rank=rank, world_size=world)
    try:
        torch.cuda.set_device(0)
        ref, comp, cfg, strategy = _corner_case(variant)
        eng = hdist.HipEngine(cfg)
        dref, dcomp = torch.as_tensor(ref).cuda(), torch.as_tensor(comp).cuda()
        outs = []
        for it in range(3):
            o, d = hdist.main_sharded(dref, dcomp, cfg, engine=eng, strategy=strategy)
            if rank == 0:
                outs.append((o.cpu().numpy().copy(), d["accumulated robustness"].cpu().numpy().copy()))
        if rank == 0:
            for o, a in outs[1:]:
                assert np.array_equal(o, outs[0][0], equal_nan=True) and np.array_equal(a, outs[0][1])
            np.savez(out_path, out=outs[0][0], acc_r=outs[0][1])
    finally:
        dist.destroy_process_group()


def _corner_case(variant):
    if variant == "reduce_denoiser":
        ref, comp, _ = synth.make_burst(512, 512, 4, seed=17, max_shift=2.0)
        return ref, comp, _shard_cfg(2, True), "reduce"
    if variant == "reduce_denoiser_x15":
        ref, comp, _ = synth.make_burst(512, 512, 4, seed=17, max_shift=2.0)
        return ref, comp, _shard_cfg(1.5, True), "reduce"
    assert variant in ("mono_rows", "mono_reduce")
    ref, comp, _ = synth.make_burst(512, 512, 5, seed=8, cfa=MONO, max_shift=2.0)
    cfg = base_config(ts=16, scale=2, mode="grey")
    cfg.robustness.save_mask = True
    return ref, comp, cfg, variant.split("_")[1]


@pytest.mark.timeout(900)
@pytest.mark.parametrize("variant,world", [("reduce_denoiser", 2), ("reduce_denoiser_x15", 3), ("mono_rows", 2), ("mono_reduce", 3)])
def test_sharded_corners(tmp_path, variant, world):
    """Corners main() supports and round 3's main_sharded refused: strategy "reduce" with the accumulated-robustness denoiser
    (the reduced robustness is all-reduced BEFORE the reference frame is merged per slab, merge.py:223-228) and monochrome
    bursts on several ranks (always frame-sharded: the one-channel robustness is not row-local)."""
    import socket
    import torch.multiprocessing as mp

    with socket.socket() as s_:
        s_.bind(("127.0.0.1", 0))
        port = s_.getsockname()[1]
    out_path = str(tmp_path / "o.npz")
    mp.spawn(_corner_worker, args=(world, port, out_path, variant), nprocs=world, join=True)
    got = np.load(out_path)
    ref, comp, cfg, _ = _corner_case(variant)
    want, dbg = hsr.main(ref, comp, cfg)
    w = N(want)
    if variant.startswith("mono"):  # channels 1, 2 are 0 / 0 = NaN in this mode (three-channel accumulators upstream)
        assert np.isnan(got["out"][..., 1:]).all() or np.array_equal(np.isnan(got["out"]), np.isnan(w))
        assert_close(got["out"][..., 0], w[..., 0], 0, 2e-6, "mono sharded == single")
    else:
        assert_close(got["out"], w, 0, 2e-6, "reduce + denoiser == single")
    assert_close(got["acc_r"], N(dbg["accumulated robustness"]), 0, 2e-6, "acc_r")


def test_main_runner_is_thread_safe():
    """main() routes host-resident bursts through a cached HostBurstRunner whose result tensor is
    static.  Two threads calling main() with the SAME configuration object and different bursts must each get their own
    pixels (the clone happens inside the runner's lock, and the next replay is ordered behind it)."""
    import threading

    cfg = base_config(ts=16, scale=2)
    bursts = [synth.make_burst(512, 640, 5, seed=sd, max_shift=2.0)[:2] for sd in (31, 32)]
    cfg_ref = base_config(ts=16, scale=2)
    cfg_ref.hip = {"graph": False}
    want = [hsr.main(r, c, cfg_ref)[0].clone() for r, c in bursts]
    for r, c in bursts * 2:  # eager, capture, replays: the runner is live before the threads start
        hsr.main(r, c, cfg)
    errors = []

    def loop(k):
        try:
            torch.cuda.set_device(0)
            for _ in range(12):
                out, _ = hsr.main(*bursts[k], cfg)
                if not torch.equal(torch.nan_to_num(out), torch.nan_to_num(want[k])):
                    errors.append(k)
        except Exception as e:  # noqa: BLE001
            errors.append(repr(e))

    threads = [threading.Thread(target=loop, args=(k,)) for k in (0, 1)]
    for t in threads:
        t.start()
    for t in threads:
        t.join()
    assert not errors, errors


def test_rows_plan_flow_bound_retry():
    """distributed.RowsPlan sizes its sub-image for the flow bound its first burst measured; a later burst in the same
    buffers whose flows exceed it is detected ON THE DEVICE, recomputed eagerly with its own bound (bit-identical to
    main()) and the next capture takes the larger bound over."""
    from handheld_super_resolution import distributed as hdist

    cfg = base_config(ts=16, scale=2)
    cfg.robustness.save_mask = True
    ref1, comp1, _ = synth.make_burst(512, 640, 5, seed=41, max_shift=0.4)
    seed2 = next(sd for sd in range(42, 200) if np.abs(synth.frame_shifts(5, sd, 12.0)[1:, 1]).max() > 10.0)  # |dy| > 10 px
    ref2, comp2, _ = synth.make_burst(512, 640, 5, seed=seed2, max_shift=12.0)
    dref, dcomp = T(ref1), T(comp1)
    eng = hdist.HipEngine(cfg)
    for it in range(3):  # eager (measures the bound), capture, replay
        out, dbg = hdist.main_sharded(dref, dcomp, cfg, engine=eng, force_sharded=True)
        assert not dbg.get("flow_bound_recomputed", False)
    assert eng._plans and not getattr(eng, "_plan_error", None)
    bound1 = next(iter(eng._plans.values())).bound
    want1, _ = hsr.main(ref1, comp1, base_config(ts=16, scale=2))
    assert torch.equal(torch.nan_to_num(out), torch.nan_to_num(want1))
    dref.copy_(T(ref2))
    dcomp.copy_(T(comp2))
    want2, _ = hsr.main(ref2, comp2, base_config(ts=16, scale=2))
    out, dbg = hdist.main_sharded(dref, dcomp, cfg, engine=eng, force_sharded=True)
    assert dbg.get("flow_bound_recomputed", False), "flows of ~12 px must exceed the bound sized for 0.4 px"
    assert torch.equal(torch.nan_to_num(out), torch.nan_to_num(want2))
    assert not eng._plans  # dropped: the next call captures again with the larger bound
    for it in range(2):    # capture, replay
        out, dbg = hdist.main_sharded(dref, dcomp, cfg, engine=eng, force_sharded=True)
        assert not dbg.get("flow_bound_recomputed", False)
        assert torch.equal(torch.nan_to_num(out), torch.nan_to_num(want2))
    assert eng._plans and next(iter(eng._plans.values())).bound > bound1
    # a caller's bound: no host read at all — the plan is sized for it and the device flag comes back in the debug dict
    eng3 = hdist.HipEngine(cfg)
    for it in range(3):
        out, dbg = hdist.main_sharded(dref, dcomp, cfg, engine=eng3, force_sharded=True, max_flow=16.0)
        assert torch.equal(torch.nan_to_num(out), torch.nan_to_num(want2)) and not bool(dbg["flow_bound_exceeded"])
    assert eng3._plans and next(iter(eng3._plans.values())).bound == 16.0 and not next(iter(eng3._plans.values())).check
    for it in range(3):  # ... and one that is too small is REPORTED (the result near slab seams is then the caller's risk)
        out, dbg = hdist.main_sharded(dref, dcomp, cfg, engine=eng3, force_sharded=True, max_flow=4.0)
        assert bool(dbg["flow_bound_exceeded"])


def test_rows_plan_needs_the_same_tensors_not_the_same_addresses():
    """whether a rank replays / captures a RowsPlan or runs eagerly decides which collectives it
    issues, so the decision must be one every rank takes alike.  "The same device addresses as an earlier call" is not: the
    caching allocator may hand a FRESH burst the addresses of a freed one on one rank and not on another.  The address key
    is only trusted while the tensors of its first sighting are alive: a fresh burst at recycled addresses is a first
    sighting again (eager), the caller's SAME tensors coming back are captured on their second call."""
    from handheld_super_resolution import distributed as hdist

    cfg = base_config(ts=16, scale=2)
    ref1, comp1, _ = synth.make_burst(512, 640, 4, seed=41, max_shift=1.0)
    want, _ = hsr.main(ref1, comp1, base_config(ts=16, scale=2))
    eng = hdist.HipEngine(cfg)
    packed = np.concatenate([ref1[None], comp1])  # one allocation of an unusual size: the allocator hands the block back
    seen, recycled = set(), 0
    for it in range(6):  # a fresh burst per call; the previous one is freed before the next is allocated
        buf = T(packed)
        dref, dcomp = buf[0], buf[1:]
        recycled += (dref.data_ptr(), dcomp.data_ptr()) in seen
        seen.add((dref.data_ptr(), dcomp.data_ptr()))
        out, _ = hdist.main_sharded(dref, dcomp, cfg, engine=eng, force_sharded=True)
        assert torch.equal(torch.nan_to_num(out), torch.nan_to_num(want))
        assert not eng._plans, "a fresh burst must not be taken for the second call of the freed one"
        del buf, dref, dcomp, out
    if not recycled:
        pytest.skip("the caching allocator did not recycle the burst's addresses in 6 bursts: situation not reproduced")
    dref, dcomp = T(ref1), T(comp1)
    for it in range(3):  # the SAME tensors: eager, capture, replay
        out, _ = hdist.main_sharded(dref, dcomp, cfg, engine=eng, force_sharded=True)
        assert torch.equal(torch.nan_to_num(out), torch.nan_to_num(want))
        assert bool(eng._plans) == (it >= 1)
    views = [dcomp[i] for i in range(len(dcomp))]  # fresh view objects of the same live storage: the same inputs
    eng2 = hdist.HipEngine(cfg)
    for it in range(2):
        hdist.main_sharded(dref, [dcomp[i] for i in range(len(dcomp))], cfg, engine=eng2, force_sharded=True)
    assert eng2._plans and views[0]._base is dcomp


@pytest.mark.parametrize("kern", ["handheld", "iso"])
def test_merge_x3_edge_frames_all_sides(kern):
    """k_merge_xs<3>'s EDGE frames (round 4): frames whose window leaves the image on every side and at the corners — uniform
    flows of +-20 px along each axis, a diagonal one, one that pushes every position of the left tile column out of the
    frame (no contribution at all) and per-tile random flows of +-6 px — evaluated by the uniform code with clamped staging
    and border masks, against BOTH other implementations of the same arithmetic rules: the 16 x 16 HR tile kernel
    (per-pixel float64 geometry, LDS windows with explicit bounds tests) and the per-pixel kernel (operands from global
    memory).  Every perimeter tile of the image takes the EDGE path for the reference frame."""
    H, W, ts = 96, 112, 16
    ny, nx = H // ts, W // ts
    ref, fr = merge_frames(H, W, 8, ts, 91, base_config(ts=ts, scale=3))
    rng = np.random.default_rng(5)
    flows = [np.full((ny, nx, 2), v, np.float32) for v in ((20.25, 0.4), (-20.25, -0.4), (0.3, 19.6), (-0.3, -19.6),
                                                             (-13.3, 7.7), (-40.0, 0.0))]
    flows.append(rng.uniform(-6, 6, (ny, nx, 2)).astype(np.float32))
    flows.append((rng.uniform(-6, 6, (ny, nx, 2)) - np.array([0.0, 0.999])).astype(np.float32))
    fr = [(f[0], fl, f[2], f[3]) for f, fl in zip(fr, flows)]
    cfa = [[1, 2], [0, 1]]  # GBRG: red in parity class (1, 0)
    tf = [tuple(T(a) for a in f) for f in fr]

    def cfg_for(which):
        c = base_config(ts=ts, scale=3)
        c.merging.kernel = kern
        c.hip = {"merge_kernel": which}
        return c

    rc = T(oracle.estimate_kernels(ref, cfg_for("auto")))
    outs = {}
    for which in ("auto", "tile", "generic"):
        out, den = torch.empty(3 * H, 3 * W, 3, device=DEV), torch.empty(3 * H, 3 * W, 3, device=DEV)
        acc = torch.zeros(H, W, device=DEV)
        merge.merge_burst(tf, T(ref), rc, out, den, cfa, cfg_for(which), divide=False, store_den=True, acc_r=acc)
        outs[which] = (N(out), N(den), N(acc))
    for other in ("tile", "generic"):
        for k, what in enumerate(("num", "den", "accumulated robustness")):
            assert_close(outs["auto"][k], outs[other][k], 4e-5, 1e-7, f"EDGE frames, k_merge_xs<3> vs {other} kernel: {what}")
    # (the two reference implementations agree with each other to 2.4e-6: the same per-pixel arithmetic, the generic kernel
    # with the float64 geometry of the fall-back path)
    assert_close(outs["tile"][0], outs["generic"][0], 2e-5, 1e-7, "tile vs generic num")
