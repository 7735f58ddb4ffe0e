"""Noise curves in the library: hhsr_noise_mc_levels / _workspace / hhsr_noise_mc / hhsr_noise_curves_fill,
run_fast_MC(engine="hip") and process(estimator: "monte_carlo_hip").

The host-only entry points are tested without a device.  On the GPU the kernel is compared with tests/noise_mc_ref.py,
the NumPy statement of the stream in include/hhsr.h, evaluated in float64.  SE below is the standard error of a mean of
n per-pair values, std(per-pair value) / sqrt(n), from the restatement.

Bounds
 - same seed: |hip - float64 restatement| <= 0.02 SE.  Both evaluate the same normals, so the difference is float32
   rounding only (measured: PARITY.md, "Noise curves"); a different counter layout or a lost patch pair lands near 1 SE.
   At n_patches = 1 a sample of one has no spread, so SE is taken from the distribution the sample comes from: the
   per-pair standard deviation of the n_patches = 4133 restatement of the same level, over sqrt(1).
 - independent seeds: |hip(seed A) - restatement(seed B)| <= 6 sqrt(2) SE (the difference of two independent means has
   sqrt(2) SE; 6 of those for 22 values is a 1e-7 event), the same against oracle.frontend.unitary_mc with its own
   generator (same n, so the same SE on both sides).
"""
import ctypes
import functools

import numpy as np
import pytest
import torch

import noise_mc_ref as ref
from handheld_super_resolution import _lib, fast_monte_carlo as mc, synthetic as synth

gpu = pytest.mark.gpu

LEVELS = [1000, 0, 1, 2, 5, 20, 500, 980, 995, 998, 999]  # deliberately unsorted
A4, B4 = synth.ALPHA_ISO100 * 4, synth.BETA_ISO100 * 4
FALLBACK = (0.05, 0.01)
N_ODD = 4133  # no multiple of 64, of 256 or of the chunk; three chunks, the last one partly filled
SEED = 0x1234_5678_9ABC_DEF1  # both key words in use


def i32(a):
    a = np.ascontiguousarray(a, np.int32)
    return a, a.ctypes.data_as(_lib.I32P)


def f64(a):
    a = np.ascontiguousarray(a, np.float64)
    return a, a.ctypes.data_as(_lib.DP)


def test_restatement_philox_known_answers():
    """The Philox4x32-10 of the restatement against the known-answer vectors published with Random123."""
    kat = {0: (0x6627E8D5, 0xE169C58D, 0xBC57AC4C, 0x9B00DBD8), 0xFFFFFFFF: (0x408F276D, 0x41C83B0E, 0xA20BC7C6, 0x6D5451FD)}
    for v, want in kat.items():
        got = ref.philox4x32_10([v], [v], [v], [v], v, v)
        assert tuple(int(w[0]) for w in got) == want


# ---- host only -------------------------------------------------------------------------------------------------------------
def py_levels(alpha, beta):
    """The brightness indices fast_monte_carlo.run_fast_MC simulates (its lines, with its own bound function)."""
    n = mc.N_BRIGHTNESS_LEVELS
    xmin, xmax = mc.get_non_linearity_bound(alpha, beta, mc.TOL)
    imin = int(np.ceil(xmin * n)) + 1
    imax = int(np.floor(xmax * n)) - 1
    if imin > n or imax <= imin:
        return imin, imax, np.arange(n + 1)
    return imin, imax, np.concatenate((np.arange(imin + 1), np.arange(imax, n + 1)))


def c_levels(alpha, beta, cap=1001):
    buf, p = i32(np.full(max(cap, 1), -7))
    n = ctypes.c_int32(-1)
    rc = _lib.load().hhsr_noise_mc_levels(alpha, beta, p if cap else None, cap, ctypes.byref(n))
    return rc, n.value, buf


# (alpha, beta, imin, imax) found by scanning run_fast_MC's own index arithmetic: the edges of its fallback rule
EDGES = [(0.05, 0.00175369, 1000, 527),      # imin = 1000: not above n, the fallback comes from imax <= imin
         (0.05, 0.00177118, 1001, 527),      # imin = 1001 > n
         (0.0301042, 0.000602084, 600, 601),  # imax = imin + 1: the smallest gap that is simulated in two runs (all 1001)
         (0.0301594, 0.000603188, 601, 601),  # imax = imin: fallback
         (0.030049, 0.00060098, 599, 601)]    # imax = imin + 2: exactly one interpolated-only index


def test_levels_match_run_fast_MC():
    profiles = [(synth.ALPHA_ISO100 * k, synth.BETA_ISO100 * k) for k in (1, 4, 16)] + [FALLBACK]
    profiles += [(a, a * f) for a in (1e-5, 1e-4, 1e-3, 5e-3, 0.02, 0.03, 0.2) for f in (1e-4, 0.01, 0.1, 0.5, 0.97)]
    for a, b, imin, imax in EDGES:
        assert py_levels(a, b)[:2] == (imin, imax)  # the profile is the edge it is listed for
        profiles.append((a, b))
    fallbacks = 0
    for a, b in profiles:
        _, _, want = py_levels(a, b)
        rc, n, got = c_levels(a, b)
        assert rc == 0 and n == len(want) and np.array_equal(got[:n], want), (a, b, n, len(want))
        fallbacks += len(want) == 1001
    assert 4 <= fallbacks < len(profiles)
    assert c_levels(synth.ALPHA_ISO100, synth.BETA_ISO100)[1] == 20 + 1001 - 959  # imin 19, imax 959


def test_levels_capacity_and_errors():
    lib = _lib.load()
    rc, n, buf = c_levels(A4, B4, cap=10)  # too small: the count comes back, nothing is written
    assert rc == -1 and n == 39 + 1001 - 922 and (buf == -7).all() and b"invalid argument" in lib.hhsr_last_error()
    assert c_levels(A4, B4, cap=0)[:2] == (-1, n)  # the query form: levels NULL, n 0
    assert c_levels(A4, B4, cap=n)[0] == 0
    buf, p = i32(np.zeros(1001))
    assert lib.hhsr_noise_mc_levels(A4, B4, p, 1001, None) == -1 and not buf.any()
    assert c_levels(float("nan"), B4)[0] == -1 and c_levels(A4, float("inf"))[0] == -1
    # where the reference raises (NaN bound: beta far above alpha; imax > 999: beta just above alpha): all 1001
    for a, b in ((1e-4, 1e-2), (0.01, 0.01002)):
        rc, n, got = c_levels(a, b)
        assert rc == 0 and n == 1001 and np.array_equal(got, np.arange(1001))


def fill(levels, sigma, diff):
    std, dif = f64(np.full(1001, np.nan)), f64(np.full(1001, np.nan))
    lv, sg, df = i32(levels), f64(sigma), f64(diff)
    rc = _lib.load().hhsr_noise_curves_fill(lv[1], len(lv[0]), sg[1], df[1], std[1], dif[1])
    return rc, std[0], dif[0]


def py_fill(imin, imax, levels, sigma, diff):
    """run_fast_MC's copy + interp_MC on given per-level values."""
    n = mc.N_BRIGHTNESS_LEVELS
    brightness = np.arange(n + 1) / n
    sigmas, diffs = np.empty(n + 1), np.empty(n + 1)
    sigmas[levels], diffs[levels] = sigma, diff
    s_l, d_l = mc.interp_MC(brightness[imin - 1:imax + 2], sigmas[imin], sigmas[imax], diffs[imin], diffs[imax])
    sigmas[imin:imax + 1], diffs[imin:imax + 1] = s_l, d_l
    return sigmas, diffs


def test_fill_matches_interp_MC():
    rng = np.random.default_rng(5)
    cases = [(synth.ALPHA_ISO100 * k, synth.BETA_ISO100 * k) for k in (1, 4, 16)] + [EDGES[4][:2]]
    for a, b in cases:
        imin, imax, levels = py_levels(a, b)
        assert len(levels) < 1001
        sigma, diff = rng.uniform(1e-3, 0.1, len(levels)), rng.uniform(1e-4, 0.05, len(levels))
        want_s, want_d = py_fill(imin, imax, levels, sigma, diff)
        for perm in (np.arange(len(levels)), rng.permutation(len(levels))):  # any order of the levels
            rc, got_s, got_d = fill(levels[perm], sigma[perm], diff[perm])
            assert rc == 0
            np.testing.assert_allclose(got_s, want_s, rtol=1e-14, atol=0)
            np.testing.assert_allclose(got_d, want_d, rtol=1e-14, atol=0)
            outside = np.r_[0:imin, imax + 1:1001]
            assert np.array_equal(got_s[outside], want_s[outside]) and np.array_equal(got_d[outside], want_d[outside])


def test_fill_identity_and_errors():
    lib = _lib.load()
    rng = np.random.default_rng(6)
    sigma, diff = rng.uniform(1e-3, 0.1, 1001), rng.uniform(1e-4, 0.05, 1001)
    perm = rng.permutation(1001)
    rc, got_s, got_d = fill(perm, sigma[perm], diff[perm])
    assert rc == 0 and np.array_equal(got_s, sigma) and np.array_equal(got_d, diff)
    lv = np.r_[0:11, 990:1001]
    v = np.ones(len(lv))
    assert fill(lv, v, v)[0] == 0
    for bad in (np.r_[lv[:-1], 1001], np.r_[lv[:-1], -1], np.r_[lv[:-1], 3],  # out of range, given twice
                lv[1:], lv[:-1], np.r_[lv, 500]):                              # 0 / 1000 missing, two gaps
        assert fill(bad, np.ones(len(bad)), np.ones(len(bad)))[0] == -1, bad
        assert b"invalid argument" in lib.hhsr_last_error()
    (_ones, one), (_lvs, lvp) = f64(np.ones(1001)), i32(np.arange(1001))  # (the arrays stay alive with their pointers)
    assert lib.hhsr_noise_curves_fill(lvp, 0, one, one, one, one) == -1
    assert lib.hhsr_noise_curves_fill(lvp, 1002, one, one, one, one) == -1
    for k in range(5):
        args = [lvp, 1001, one, one, one, one]
        args[k if k == 0 else k + 1] = None
        assert lib.hhsr_noise_curves_fill(*args) == -1


def workspace(n_levels, n_patches):
    b = ctypes.c_size_t(0)
    rc = _lib.load().hhsr_noise_mc_workspace(n_levels, n_patches, ctypes.byref(b))
    return rc, b.value


def test_workspace_grows_with_both_arguments():
    assert workspace(1, 1) == (0, 16)  # one partial per curve
    assert workspace(11, N_ODD) == (0, 2 * 11 * 3 * 8)
    chunk = _lib.NOISE_MC_CHUNK
    assert workspace(7, chunk)[1] < workspace(7, chunk + 1)[1] == workspace(7, 2 * chunk)[1] < workspace(8, 2 * chunk)[1]
    assert workspace(150, 100000)[1] < workspace(1001, 100000)[1] < 1 << 20
    assert workspace(1001, 2 ** 31 - 1)[0] == 0
    for bad in ((0, 5), (1002, 5), (5, 0), (5, -1)):
        assert workspace(*bad)[0] == -1
    assert _lib.load().hhsr_noise_mc_workspace(5, 5, None) == -1


def test_noise_mc_argument_errors_touch_no_gpu():
    """Every argument error is -1 with a message, decided on the host: without a device any HIP call would return a
    positive hipError_t instead."""
    lib = _lib.load()
    base = 1 << 32  # nothing is dereferenced on the host
    lv, sg, df, ws = (ctypes.c_void_p(base + (k << 20)) for k in range(4))
    need = workspace(11, N_ODD)[1]
    good = [lv, 11, A4, B4, N_ODD, SEED, sg, df, ws, need, None]

    def refused(pos, value):
        args = list(good)
        args[pos] = value
        rc = lib.hhsr_noise_mc(*args)
        assert rc == -1 and b"hhsr_noise_mc: invalid argument" in lib.hhsr_last_error(), (pos, value, rc)

    for pos in (0, 6, 7, 8):
        refused(pos, None)
    for n_levels in (0, -1, 1002):
        refused(1, n_levels)
    for n_patches in (0, -5):
        refused(4, n_patches)
    refused(9, need - 1)
    refused(9, 0)
    refused(2, -1e-4), refused(3, float("nan")), refused(2, float("inf"))
    refused(0, ctypes.c_void_p(base + 2)), refused(6, ctypes.c_void_p(base + 4)), refused(8, ctypes.c_void_p(base + 4))
    with pytest.raises(RuntimeError, match="hhsr_noise_mc failed"):
        _lib.call("hhsr_noise_mc", None, *good[1:])
    with pytest.raises(ValueError):
        mc.run_fast_MC(A4, B4, engine="numba")


# ---- on the GPU ------------------------------------------------------------------------------------------------------------
def hip_mc(levels, n_patches, seed=SEED, alpha=A4, beta=B4):
    """hhsr_noise_mc on torch's current stream -> (sigma, diff) float64 arrays; the outputs start as NaN and the
    workspace has a guard band, which must come back untouched."""
    lv = torch.tensor(list(levels), dtype=torch.int32, device="cuda")
    n = lv.numel()
    need = workspace(n, n_patches)[1]
    ws = torch.full((need // 8 + 32,), 7.25, dtype=torch.float64, device="cuda")
    out = torch.full((2, n + 8), float("nan"), dtype=torch.float64, device="cuda")
    _lib.call("hhsr_noise_mc", _lib.ptr(lv), n, alpha, beta, n_patches, seed, _lib.ptr(out[0]), _lib.ptr(out[1]),
              _lib.ptr(ws), need, _lib.stream())
    host, guard = out.cpu().numpy(), ws[need // 8:].cpu().numpy()
    assert (guard == 7.25).all() and np.isnan(host[:, n:]).all() and np.isfinite(host[:, :n]).all()
    return host[0, :n], host[1, :n]


@functools.lru_cache(maxsize=None)
def restated(n_patches, seed):
    """(sigma, diff, se_sigma, se_diff) of LEVELS from the float64 restatement; computed once, read-only."""
    out = ref.noise_mc(LEVELS, A4, B4, n_patches, seed, np.float64)
    for a in out:
        a.setflags(write=False)
    return out


def se_ratios(got, want, what):
    """max |hip - restatement| / SE over sigma and diff, printed per curve."""
    rs = np.abs(got[0] - want[0]) / want[2]
    rd = np.abs(got[1] - want[1]) / want[3]
    print(f"{what}: max |d sigma| / SE = {rs.max():.3e}, max |d diff| / SE = {rd.max():.3e}")
    return max(rs.max(), rd.max())


@gpu
def test_stream_matches_the_restatement():
    want = restated(N_ODD, SEED)
    assert (want[2] > 0).all() and (want[3] > 0).all()
    assert se_ratios(hip_mc(LEVELS, N_ODD), want, f"same seed, n_patches = {N_ODD}") <= 0.02
    # the float32 evaluation of the restatement sits where the kernel does (the two differ in libm's last bits only)
    s32, d32, _, _ = ref.noise_mc(LEVELS, A4, B4, N_ODD, SEED, np.float32)
    print(f"float32 restatement vs float64: {se_ratios((s32, d32), want, 'restatement float32'):.3e} SE")


@gpu
def test_stream_single_patch_pair():
    """n_patches = 1: one lane of one workgroup works, everything else is masked."""
    one = ref.noise_mc(LEVELS, A4, B4, 1, SEED, np.float64)
    many = restated(N_ODD, SEED)
    se1 = (one[0], one[1], many[2] * np.sqrt(N_ODD), many[3] * np.sqrt(N_ODD))  # the spread of ONE pair (see the header)
    assert se_ratios(hip_mc(LEVELS, 1), se1, "same seed, n_patches = 1") <= 0.02


@gpu
def test_levels_are_independent_and_runs_reproducible():
    full = hip_mc(range(1001), N_ODD)
    again = hip_mc(range(1001), N_ODD)
    assert np.array_equal(full[0], again[0]) and np.array_equal(full[1], again[1])  # bitwise, run to run
    some = hip_mc(LEVELS, N_ODD)
    assert np.array_equal(some[0], full[0][LEVELS]) and np.array_equal(some[1], full[1][LEVELS])
    for lv in (0, 37, 1000):  # alone in its launch
        s, d = hip_mc([lv], N_ODD)
        assert s[0] == full[0][lv] and d[0] == full[1][lv]
    other = hip_mc(LEVELS, N_ODD, seed=SEED + 1)
    assert (other[0] != some[0]).all() and (other[1] != some[1]).all()
    hi = hip_mc(LEVELS, N_ODD, seed=SEED ^ (1 << 40))  # the high key word counts
    assert (hi[0] != some[0]).all()
    # an index outside 0 .. 1000 is clamped by the kernel
    s, d = hip_mc([-3, 1001, 2 ** 31 - 1, -2 ** 31], N_ODD)
    assert np.array_equal(s, full[0][[0, 1000, 1000, 0]]) and np.array_equal(d, full[1][[0, 1000, 1000, 0]])


@gpu
def test_statistics_at_full_size():
    import oracle.frontend

    n = mc.N_PATCHES
    got = hip_mc(LEVELS, n, seed=11)
    want = restated(n, 12)
    bound = 6 * np.sqrt(2)
    assert se_ratios(got, want, f"independent seeds, n_patches = {n}") <= bound
    rng = np.random.default_rng(1)
    for k in (1, 6, 0):  # levels 0, 500, 1000
        dm, sm = oracle.frontend.unitary_mc(A4, B4, LEVELS[k] / 1000, n, rng)
        rs, rd = abs(got[0][k] - sm) / want[2][k], abs(got[1][k] - dm) / want[3][k]
        print(f"level {LEVELS[k]} vs oracle.frontend.unitary_mc: {rs:.2f} SE (sigma), {rd:.2f} SE (diff)")
        assert rs <= bound and rd <= bound
    # ... and with the same seed the full-size launch (49 chunks) is the restatement's stream too
    assert se_ratios(hip_mc(LEVELS, n, seed=12), want, f"same seed, n_patches = {n}") <= 0.02


@gpu
def test_whole_curves():
    s_hip, d_hip = mc.run_fast_MC(A4, B4, seed=5, engine="hip")
    s_tor, d_tor = mc.run_fast_MC(A4, B4, seed=5, engine="torch")
    assert s_hip.shape == d_hip.shape == (1001,) and s_hip.dtype == np.float64
    assert np.abs(s_hip[100:900] / s_tor[100:900] - 1).max() < 0.005
    assert np.abs(d_hip[100:900] / d_tor[100:900] - 1).max() < 0.01
    sa, da = synth.noise_curves(A4, B4)
    for i in (0, 1, 1000):  # the clipped regime
        assert s_hip[i] < 0.8 * sa[i] and d_hip[i] < 0.8 * da[i], (i, s_hip[i], sa[i], d_hip[i], da[i])
    again = mc.run_fast_MC(A4, B4, seed=5, engine="hip")
    assert np.array_equal(again[0], s_hip) and np.array_equal(again[1], d_hip)
    # the simulated levels are the kernel's values, the rest is hhsr_noise_curves_fill
    imin, imax, levels = py_levels(A4, B4)
    sim = hip_mc(levels, mc.N_PATCHES, seed=5)
    assert np.array_equal(s_hip[:imin], sim[0][:imin]) and np.array_equal(d_hip[imax + 1:], sim[1][imin + 2:])
    s_fb, d_fb = mc.run_fast_MC(*FALLBACK, seed=5, engine="hip", n_patches=20000)
    assert s_fb.shape == d_fb.shape == (1001,) and np.isfinite(s_fb).all() and np.isfinite(d_fb).all()
    assert (s_fb > 0).all() and (d_fb > 0).all()


@gpu
def test_process_with_the_hip_estimator():
    import handheld_super_resolution as hsr

    ref_img, comp, _ = synth.make_burst(512, 512, 2, seed=3)
    a, b = synth.ALPHA_ISO100 * 16, synth.BETA_ISO100 * 16
    burst = {"ref": ref_img, "comp": comp, "cfa_pattern": [[0, 1], [1, 2]], "white_balance": [1.0, 1.0, 1.0],
             "alpha": a, "beta": b}

    def cfg0():
        c = hsr.default_config()
        c.verbose = 0
        c.block_matching.tuning.tile_size = 16
        return c

    cfg = cfg0()
    cfg.noise_model.estimator = "monte_carlo_hip"
    cfg.noise_model.seed = 9
    img, _ = hsr.process(dict(burst), cfg)
    std, dif = mc.run_fast_MC(a, b, seed=9, engine="hip")
    assert np.array_equal(np.array(cfg.noise_model.std_curve), std)
    assert np.array_equal(np.array(cfg.noise_model.diff_curve), dif)
    sa, _ = synth.noise_curves(a, b)
    assert std[0] < 0.8 * sa[0] and std[1000] < 0.8 * sa[1000]  # not the analytic law
    img2, _ = hsr.process(dict(burst, std_curve=std, diff_curve=dif), cfg0())
    assert img.shape == img2.shape and img.shape[2] == 3 and (np.isnan(img) == np.isnan(img2)).all()
    assert np.nanmax(np.abs(img - img2)) <= 5e-5


@gpu
def test_capture_replays_to_the_same_bits():
    from handheld_super_resolution import graph

    lv = torch.tensor(LEVELS, dtype=torch.int32, device="cuda")
    n = lv.numel()
    need = workspace(n, N_ODD)[1]
    ws = torch.empty(need // 8, dtype=torch.float64, device="cuda")
    out = torch.full((2, n), float("nan"), dtype=torch.float64, device="cuda")

    def launch():
        _lib.call("hhsr_noise_mc", _lib.ptr(lv), n, A4, B4, N_ODD, SEED, _lib.ptr(out[0]), _lib.ptr(out[1]), _lib.ptr(ws),
                  need, _lib.stream())

    eager = hip_mc(LEVELS, N_ODD)
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    g = torch.cuda.CUDAGraph()
    with graph.capture(g, side):  # torch.cuda.graph on one stream: a single chain of two kernels
        launch()
    torch.cuda.synchronize()
    assert torch.isnan(out).all()  # captured, not run
    for _ in range(2):
        out.fill_(float("nan"))
        ws.zero_()
        g.replay()
        torch.cuda.synchronize()
        got = out.cpu().numpy()
        assert np.array_equal(got[0], eager[0]) and np.array_equal(got[1], eager[1])
