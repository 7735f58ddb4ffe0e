"""The robustness kernels (csrc/hhsr_robustness.hip) through all their entry points at the cases of
tests/robustness_cases.py: flows on round-half-even ties, flows that put the guide position exactly on the image edge and one
float32 beside it, tiles pushed out of the image, NaN / infinite / huge flows, guide images smaller than the LDS window; the
thresholds of S; the curve index at its ties and clamps; the local minimum at one-pixel images and tile seams.  Expected
values: the oracle, which tests/test_robustness_ref.py holds on the CPU against the reference's statements (census of the
branches reached: that module's docstring).

Bounds (the project's for these quantities, test_hip_parity.py / SURVEY.md 8d): R and r abs 1e-4 with no outlier allowed,
warped means rtol 1e-6 / atol 1e-8 with an equal +inf mask, S, masks, curve indices and the minimum exact.  Every kernel gets
the oracle's guide means and reference planes as inputs, so a difference is the robustness kernel's.

Measured on MI355X (PARITY.md, "robustness border cases")."""
import functools

import numpy as np
import pytest
import torch

import oracle
import robustness_cases as rc
from helpers import assert_close

pytestmark = pytest.mark.gpu

from handheld_super_resolution import _lib, kernels, robustness  # noqa: E402,F401

DEV = "cuda"
CASES = [(g, f) for g in rc.GEOMETRIES for f in rc.FIELDS]
case_ids = dict(ids=lambda c: f"{c[0].name}-{c[1]}")
FUSED = [g for g in rc.GEOMETRIES if g.mode == "bayer" and g.ts % 16 == 0]
G16 = rc.GEOMETRIES[0]  # 80 x 112, ts 16
CFA, WB = [list(r) for r in rc.CFA], list(rc.WB)


def T(a, dtype=torch.float32):
    return torch.as_tensor(np.array(a), dtype=dtype, device=DEV)  # (a copy: the shared cases are read-only)


def N(t):
    return t.detach().cpu().numpy()


def bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def same_bits(got, want, what):
    got, want = np.asarray(got), np.asarray(want)
    assert got.shape == want.shape, what
    assert np.array_equal(np.isnan(got), np.isnan(want)), f"{what}: NaN masks differ"
    ok = np.isnan(want) | (bits(got) == bits(want))
    assert ok.all(), f"{what}: {int((~ok).sum())} of {ok.size} values differ in their bits, first at {tuple(np.argwhere(~ok)[0])}"


@functools.lru_cache(maxsize=None)
def device_ref(g):
    """(cfg, curves, ref means, ref variances, (sigma^2, packed index) or sigma^2) on the device, from the oracle's planes."""
    cfg, (std, dif), om, ov = rc.ref_maps(g)
    curves = robustness.noise_curves_to_device(std, dif, DEV)
    rm, rv = T(om), T(ov)
    sig = robustness.noise_sigma_sq(rm, rv, curves[0]) if g.mode == "bayer" else robustness.mono_sigma_sq(rm, rv, curves[0])
    return cfg, curves, rm, rv, sig


def outside_of(g, name):
    return np.isinf(rc.oracle_maps(g, name)["comp_means_up"][0])


def run_api(g, name):
    """(r, R) of robustness.compute_robustness on the oracle's guide means."""
    cfg, curves, rm, rv, sig = device_ref(g)
    m = rc.oracle_maps(g, name)
    comp = rc.content(g)[1][rc.FIELDS.index(name)]
    r, R = robustness.compute_robustness(T(comp), rm, rv, T(rc.field(g, name)), CFA, WB, curves, cfg, return_R=True,
                                         ref_sigma_sq=sig, comp_means=T(m["cm"]))
    return N(r), N(R)


def check_R(g, name, r, R, what):
    m = rc.oracle_maps(g, name)
    d = float(np.abs(R.astype(np.float64) - m["R"]).max())
    print(f"{what} {g.name} {name}: max |dR| {d:.3g}, max |dr| {float(np.abs(r.astype(np.float64) - m['r']).max()):.3g}")
    assert_close(R, m["R"], 0, 1e-4, f"robustness edges: {what} R ({name})")
    assert_close(r, m["r"], 0, 1e-4, f"robustness edges: {what} r ({name})")
    assert (R[outside_of(g, name)] == 0).all(), f"{what}: R != 0 at a pixel outside the image"


# ---- 1. warp-upsample --------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", CASES, **case_ids)
def test_warp_upsample(case):
    """hhsr_rob_upscale / hhsr_mono_rob_upscale against oracle.upscale_warp_stats; the +inf masks are equal."""
    g, name = case
    m = rc.oracle_maps(g, name)
    got = N(robustness.upscale_warp_stats(T(m["cm"]), g.ts, T(rc.field(g, name))))
    want = m["comp_means_up"]
    assert np.array_equal(np.isinf(got), np.isinf(want)) and not np.isnan(got).any()
    assert_close(got, want, 1e-6, 1e-8, f"robustness edges: warped means ({name})")


# ---- 2. R through every kernel -----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", CASES, **case_ids)
def test_R_vs_oracle(case):
    g, name = case
    # the library's rule (rob_grouped, rob_frames_launch, hhsr_mono_rob_frame) for the aligned planes torch allocates
    if g.mode == "bayer":
        assert (g.ts % 16 == 0) == g.kernel.startswith("k_rob_frames_row4")
        assert (g.ts % 16 == 0 and g.W % 4 != 0) == g.kernel.endswith("_dword")
    else:
        assert (g.W % 4 == 0 and g.ts % 4 == 0) == (g.kernel == "k_mono_rob_frame4")
    r, R = run_api(g, name)
    check_R(g, name, r, R, g.kernel)


@pytest.mark.parametrize("g", FUSED, ids=lambda g: g.name)
def test_R_group_vs_oracle(g):
    """compute_robustness_group: the three fields as three frames of one launch, S evaluated inside the kernel."""
    cfg, curves, rm, rv, sig = device_ref(g)
    comp = rc.content(g)[1]
    cms = [T(rc.oracle_maps(g, f)["cm"]) for f in rc.FIELDS]
    flows = [T(rc.field(g, f)) for f in rc.FIELDS]
    Rs = robustness.compute_robustness_group([T(c) for c in comp], rm, flows, curves, cfg, sig, cms, fuse_local_min=True)
    for f, R in zip(rc.FIELDS, Rs):
        check_R(g, f, N(robustness.local_min(R)), N(R), "group")


# ---- 3. same bits across the entry points --------------------------------------------------------------------------------------
def _abi_inputs(g):
    cfg, curves, rm, rv, (sig2, idx) = device_ref(g)
    cms = [T(rc.oracle_maps(g, f)["cm"]) for f in rc.FIELDS]
    tf = [T(rc.field(g, f)) for f in rc.FIELDS]
    t = cfg.robustness.tuning
    S = [robustness.compute_s(f, t.Mt, t.s1, t.s2) for f in tf]
    return cfg, curves[1], rm, sig2, idx, cms, tf, S, t


def _rob_frames(g, maps, lead=0, index=True):
    """hhsr_rob_frames on the three fields; `lead`: R starts that many floats past a 16-byte boundary."""
    cfg, dif, rm, sig2, idx, cms, tf, S, t = _abi_inputs(g)
    ny, nx = rc.grid(g)
    bufs = [torch.full((g.H * g.W + 8,), float("nan"), dtype=torch.float32, device=DEV) for _ in cms]
    Rs = [b[lead:lead + g.H * g.W].view(g.H, g.W) for b in bufs]
    _lib.call("hhsr_rob_frames", _lib.ptr_array(cms), len(cms), g.H // 2, g.W // 2, _lib.ptr(rm), _lib.ptr(sig2),
              _lib.ptr(idx if index else None), _lib.ptr_array(tf), ny, nx, g.ts, None if maps is None else _lib.ptr_array(maps),
              float(t.Mt), float(t.s1), float(t.s2), _lib.ptr(dif), dif.numel(), float(t.t), _lib.ptr_array(Rs), 0, 0,
              _lib.stream())
    torch.cuda.synchronize()
    for b in bufs:
        assert torch.isnan(b[:lead]).all() and torch.isnan(b[lead + g.H * g.W:]).all(), "written outside R"
    return [N(R) for R in Rs]


def _rob_frame(g, index=True):
    cfg, dif, rm, sig2, idx, cms, tf, S, t = _abi_inputs(g)
    ny, nx = rc.grid(g)
    out = []
    for k in range(len(cms)):
        R = torch.full((g.H, g.W), float("nan"), dtype=torch.float32, device=DEV)
        _lib.call("hhsr_rob_frame", _lib.ptr(cms[k]), g.H // 2, g.W // 2, _lib.ptr(rm), _lib.ptr(sig2),
                  _lib.ptr(idx if index else None), _lib.ptr(tf[k]), ny, nx, g.ts, _lib.ptr(S[k]), _lib.ptr(dif), dif.numel(),
                  float(t.t), _lib.ptr(R), _lib.stream())
        out.append(N(R))
    return out


def test_entry_points_same_bits_at_the_special_flows():
    """80 x 112, ts 16, the three fields: hhsr_rob_frame == hhsr_rob_frames with S given == hhsr_rob_frames with S = NULL
    (NaN flows included: the kernel's own S and k_rob_s skip them alike) == the dword instantiation, reached with R four
    bytes off the 16-byte grid."""
    g = G16
    S = _abi_inputs(g)[7]
    single, given, inline, dword = _rob_frame(g), _rob_frames(g, S), _rob_frames(g, None), _rob_frames(g, S, lead=1)
    for k, f in enumerate(rc.FIELDS):
        assert not np.isnan(given[k]).any(), f"{f}: pixels left unwritten"
        same_bits(single[k], given[k], f"{f}: hhsr_rob_frame vs hhsr_rob_frames")
        same_bits(inline[k], given[k], f"{f}: S = NULL vs the maps of hhsr_rob_s")
        same_bits(dword[k], given[k], f"{f}: dword vs 16-byte instantiation")


# ---- 4. vector kernels against their float64 siblings ------------------------------------------------------------------------
def test_row4_vs_float64_kernel():
    """k_rob_frames_row4 against k_rob_frame (hhsr_rob_frame without the packed curve index) on `ties` and `edges`."""
    g = G16
    fast, slow = _rob_frame(g), _rob_frame(g, index=False)
    for k, f in enumerate(rc.FIELDS[:2]):
        d = float(np.abs(fast[k].astype(np.float64) - slow[k]).max())
        print(f"k_rob_frames_row4 vs k_rob_frame, {f}: max |dR| {d:.3g}")
        assert_close(fast[k], slow[k], 0, 1e-4, f"robustness edges: row4 vs float64 kernel ({f})")
        out = outside_of(g, f)
        assert (fast[k][out] == 0).all() and (slow[k][out] == 0).all()


def test_mono_row4_vs_float64_kernel():
    """k_mono_rob_frame4 against k_mono_rob_frame (R four bytes off the 16-byte grid) on `ties` and `edges`."""
    g = rc.GEOMETRIES[6]
    cfg, curves, rm, rv, sig = device_ref(g)
    ny, nx = rc.grid(g)
    t = cfg.robustness.tuning
    for f in rc.FIELDS[:2]:
        cm, fl = T(rc.oracle_maps(g, f)["cm"]), T(rc.field(g, f))
        S = robustness.compute_s(fl, t.Mt, t.s1, t.s2)
        outs = []
        for off in (0, 1):
            buf = torch.full((g.H * g.W + 4,), -1.0, dtype=torch.float32, device=DEV)
            R = buf[off:off + g.H * g.W].view(g.H, g.W)
            _lib.call("hhsr_mono_rob_frame", _lib.ptr(cm), g.H, g.W, _lib.ptr(rm), _lib.ptr(sig), _lib.ptr(fl), ny, nx, g.ts,
                      _lib.ptr(S), _lib.ptr(curves[1]), int(curves[1].numel()), float(t.t), _lib.ptr(R), _lib.stream())
            outs.append(N(R))
            assert float(buf[off + g.H * g.W:].min()) == -1.0 and (off == 0 or float(buf[0]) == -1.0)
        a, b = outs
        print(f"k_mono_rob_frame4 vs k_mono_rob_frame, {f}: max |dR| {float(np.abs(a.astype(np.float64) - b).max()):.3g}")
        assert_close(a, b, 0, 1e-4, f"robustness edges: mono row4 vs float64 kernel ({f})")
        out = outside_of(g, f)
        assert (a[out] == 0).all() and (b[out] == 0).all()
        check_R(g, f, oracle.local_min(b), b, "k_mono_rob_frame")


# ---- 5. S ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", list(rc.s_cases()))
def test_s_equals_oracle(name):
    flow, Mt = rc.s_cases()[name]
    got = N(robustness.compute_s(T(flow), Mt, rc.S1, rc.S2))
    assert np.array_equal(got, oracle.compute_s(flow, Mt, rc.S1, rc.S2)), (name, got)


def test_s_row_slices():
    """rows_before / rows_after: S of a row slice of the 3 x 4 grids that sees its neighbours in memory equals those rows of
    the full grid's S."""
    for name in ("3x4_equal", "3x4_below", "3x4_above", "3x4_default", "3x4_nan", "3x4_inf"):
        flow, Mt = rc.s_cases()[name]
        full = T(flow)
        want = oracle.compute_s(flow, Mt, rc.S1, rc.S2)
        for lo, hi in ((1, 3), (0, 2), (1, 2)):
            got = N(robustness.compute_s(full[lo:hi], Mt, rc.S1, rc.S2, flow_rows=(lo, 3 - hi)))
            assert np.array_equal(got, want[lo:hi]), (name, lo, hi, got)


@pytest.mark.parametrize("name", [n for n in rc.s_cases() if not n.endswith(("nan", "inf"))])
def test_in_kernel_s(name):
    """The weights k_rob_frames_row4 evaluates itself, inferred from hhsr_rob_frames runs that differ only in S: S = NULL
    gives the bits of the oracle's map, and in every tile other bits than the map with s1 and s2 exchanged."""
    flow, Mt = rc.s_cases()[name]
    ny, nx = flow.shape[:2]
    ts, H, W = 16, 16 * ny, 16 * nx
    rng = np.random.default_rng(3)
    gm = (0.4 + 0.2 * rng.random((3, H // 2, W // 2))).astype(np.float32)
    cm = T(gm + (0.012 * rng.standard_normal(gm.shape)).astype(np.float32))
    std, dif = (T(c, torch.float64) for c in rc.noise_curves())
    rm, (sig2, idx) = robustness.ref_planes(T(gm), T(np.full_like(gm, 1e-5)), std)
    fl = T(flow)
    S = oracle.compute_s(flow, Mt, rc.S1, rc.S2)

    def run(maps):
        R = torch.full((H, W), float("nan"), dtype=torch.float32, device=DEV)
        _lib.call("hhsr_rob_frames", _lib.ptr_array([cm]), 1, H // 2, W // 2, _lib.ptr(rm), _lib.ptr(sig2), _lib.ptr(idx),
                  _lib.ptr_array([fl]), ny, nx, ts, None if maps is None else _lib.ptr_array([maps]), float(Mt), rc.S1,
                  rc.S2, _lib.ptr(dif), dif.numel(), 0.12, _lib.ptr_array([R]), 0, 0, _lib.stream())
        return N(R)

    inline, given, swapped = run(None), run(T(S)), run(T(rc.S1 + rc.S2 - S))
    same_bits(inline, given, f"{name}: S = NULL vs the oracle's map")
    differs = (bits(given) != bits(swapped)).reshape(ny, ts, nx, ts).any(axis=(1, 3))
    assert differs.all(), f"{name}: R does not depend on S in tiles {np.argwhere(~differs).tolist()}"


# ---- 6. sigma^2 and the packed curve index -----------------------------------------------------------------------------------
@pytest.mark.parametrize("ncurve", rc.NCURVES)
def test_sigma_and_packed_index(ncurve):
    means, vars_, std, dif = rc.sigma_case(ncurve)
    with np.errstate(all="ignore"):
        _, want = oracle.robustness.apply_noise_model(np.zeros_like(means), means, vars_, std, dif)
    stdc = T(std, torch.float64)
    sig, idx = robustness.noise_sigma_sq(T(means), T(vars_), stdc)
    assert_close(N(sig), want, 1e-6, 0, f"robustness edges: sigma^2, {ncurve} curve entries")
    packed = N(idx).astype(np.int64)
    for c in range(3):
        assert np.array_equal((packed >> (10 * c)) & 1023, rc.sigma_index(means[c], ncurve)), (ncurve, c)
    assert ((packed >> 30) == 0).all()
    # hhsr_ref_planes on the same constructed planes taken as guide planes == the separate kernels
    gm, gv = T(means), T(vars_)
    m1, (s1, i1) = robustness.ref_planes(gm, gv, stdc)
    m2, v2 = robustness.upscale_warp_stats(gm), robustness.upscale_warp_stats(gv)
    s2, i2 = robustness.noise_sigma_sq(m2, v2, stdc)
    same_bits(N(m1), N(m2), "ref_planes means")
    same_bits(N(s1), N(s2), "ref_planes sigma^2")
    assert np.array_equal(N(i1), N(i2))
    # one channel: k_mono_rob_sigma
    with np.errstate(all="ignore"):
        _, want1 = oracle.robustness.apply_noise_model(np.zeros_like(means[:1]), means[:1], vars_[:1], std, dif)
    assert_close(N(robustness.mono_sigma_sq(T(means[:1]), T(vars_[:1]), stdc)), want1, 1e-6, 0,
                 f"robustness edges: mono sigma^2, {ncurve} curve entries")


# ---- 7. local minimum ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape", rc.LOCAL_MIN_SHAPES, ids=lambda s: f"{s[0]}x{s[1]}")
def test_local_min_exact(shape):
    """hhsr_local_min5 == oracle.local_min, no tolerance; the accumulator grows by exactly that map; nothing is written
    outside H x W (guards of 64 floats around both outputs)."""
    H, W = shape
    R = rc.local_min_case(shape)
    want = oracle.local_min(R)
    G = 64
    acc0 = (np.arange(H * W, dtype=np.float32).reshape(H, W) % 7) * 0.25
    for with_acc in (False, True):
        rbuf = torch.full((H * W + 2 * G,), -7.0, dtype=torch.float32, device=DEV)
        abuf = torch.full((H * W + 2 * G,), -7.0, dtype=torch.float32, device=DEV)
        r, acc = rbuf[G:G + H * W].view(H, W), abuf[G:G + H * W].view(H, W)
        acc.copy_(T(acc0))
        _lib.call("hhsr_local_min5", _lib.ptr(T(R)), H, W, _lib.ptr(r), _lib.ptr(acc if with_acc else None), _lib.stream())
        torch.cuda.synchronize()
        assert np.array_equal(N(r), want), f"{shape}: {int((N(r) != want).sum())} values differ"
        assert np.array_equal(N(acc), acc0 + want if with_acc else acc0)
        for b in (rbuf, abuf):
            assert (N(b[:G]) == -7.0).all() and (N(b[G + H * W:]) == -7.0).all(), "written outside the map"
    assert np.array_equal(N(robustness.local_min(T(R))), want)
