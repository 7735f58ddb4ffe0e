"""The pitch arguments of the C ABI (include/hhsr.h), with padded and guarded buffers.

Every entry point that takes a `pitch` (row stride in elements) is called through `_lib.call` with ctypes arguments, once
on the compact layout every other test uses (pitch == width) and once on a padded one, and for each case

  1. pitched == compact, bit for bit (the pitch changes addresses, not arithmetic);
  2. pitched vs the oracle (or the NumPy expression) at exactly the tolerance of the existing test of the same stage;
  3. no NaN that the oracle's result does not have: every padding element of an input is a quiet NaN (0xFFFF for
     uint16), so any padding value that reaches arithmetic poisons the output;
  4. the whole input buffers, padding included, are bit-identical after the call;
  5. every output lies inside a larger allocation whose guard bands (and, for the outputs that have a pitch, whose
     padding columns) still hold their sentinel afterwards.

4 and 5 are asserted on the compact call too.  Everything a kernel could touch by mistake lies inside allocations of the
test: an out-of-range access shows as a changed sentinel or a NaN, never as a fault.

Layouts (`LAYOUTS`): even2 (pitch W + 2), wide (next multiple of 64 above W + 64), odd (W + 3), lead2 (W + 6, payload 2
elements into the allocation: 8-byte but not 16-byte aligned), lead1 (W + 5, 1 element: 4-byte aligned only).  The Bayer
statistics calls demand an even pitch and an 8-byte aligned raw pointer and hhsr_normalize_raw_u16 16-byte aligned
pointers: they get the layouts they accept.

The second half applies the guard bands to the entry points without a pitch that write whole planes from grids with
remainder tiles, and reaches the kernels that the dispatchers only pick for outputs that are NOT 16-byte aligned (the
first-generation x2 merge, the tile merge at x3, the dword k_rob_frames_row4) or without a packed curve index (k_rob_frame): a C
client produces those with one pointer offset."""
import numpy as np
import pytest
import torch

import oracle
from oracle import cfast
from helpers import assert_close, base_config, bm_inputs, check_bm, smooth
import test_variant_parity as V

pytestmark = pytest.mark.gpu

from handheld_super_resolution import utils_image, robustness, kernels, _lib, synthetic as synth  # noqa: E402

DEV = "cuda"
THREADS = V.THREADS
TOL = V.TOL  # merge: rtol 2e-5 / atol 1e-6 (tests/test_hip_parity.py::test_merge_golden)
SENT = 0x5A5A5A5A  # guard sentinel (as float32 1.5e16, as float64 1.7e130: never NaN); compared as int32
FRONT = 4096       # elements in front of every pitched input, so that a read before row 0 stays inside the allocation
TILE_ROWS = 64     # rows of the tallest workgroup tile of any kernel here (ts = 64 tiles; 48 HR rows of the x3 merge)


def N(t):
    return t.detach().cpu().numpy()


def T(a, dtype=torch.float32):
    return torch.as_tensor(np.ascontiguousarray(a), dtype=dtype, device=DEV)


def cdiv(a, b):
    return -(-a // b)


# ------------------------------------------------------------------------------------------ helpers
LAYOUTS = {  # id: (pitch of a row of W elements, elements before row 0)
    "compact": (lambda W: W, 0),
    "even2": (lambda W: W + 2, 0),
    "wide": (lambda W: ((W + 64) // 64 + 1) * 64, 0),
    "odd": (lambda W: W + 3, 0),
    "lead2": (lambda W: W + 6, 2),
    "lead1": (lambda W: W + 5, 1),
}
ALL = ["even2", "wide", "odd", "lead2", "lead1"]
EVEN = ["even2", "wide", "lead2"]  # even pitch, 8-byte aligned base: what the Bayer statistics accept
NEXT = {"compact": "compact", "even2": "wide", "wide": "odd", "odd": "lead2", "lead2": "lead1", "lead1": "even2"}


def layout(name, W, other=None, even=False):
    """(pitch, lead) of layout `name` for rows of W elements; `other`: a pitch this one must differ from; `even`: an
    even pitch (odd widths)."""
    fn, lead = LAYOUTS[name]
    pitch = fn(W)
    if even and pitch % 2:
        pitch += 1
    if other is not None and pitch == other and name != "compact":
        pitch += 64 if name == "wide" else 4
    return pitch, lead


def pitched(a, pitch, lead=0, poison=None):
    """The 2-D array `a` (H x W, float32 or uint16) inside a device buffer of FRONT + lead + H * pitch + tail elements
    filled with `poison` (default: a quiet NaN, 0xFFFF for uint16; uint16 travels as int16 bits).  Returns (the H x W
    view with row stride `pitch` whose data_ptr() the ABI gets, the whole buffer, the boolean mask of the payload)."""
    a = np.ascontiguousarray(a)
    H, W = a.shape
    assert pitch >= W and a.dtype in (np.float32, np.uint16)
    tail = pitch + FRONT
    start = FRONT + lead
    n = start + H * pitch + tail
    if a.dtype == np.uint16:
        host = np.full(n, 0xFFFF if poison is None else poison, np.uint16)
    else:
        host = np.full(n, np.nan if poison is None else poison, np.float32)
    host[start:start + H * pitch].reshape(H, pitch)[:, :W] = a
    mask = np.zeros(n, bool)
    mask[start:start + H * pitch].reshape(H, pitch)[:, :W] = True
    whole = torch.from_numpy(host.view(np.int16) if a.dtype == np.uint16 else host).to(DEV)
    return whole.as_strided((H, W), (pitch, 1), start), whole, torch.from_numpy(mask).to(DEV)


def guarded(shape, dtype=torch.float32, lead=0, pitch=None, fill=None):
    """An output buffer of `shape` inside a larger allocation with a guard band on both sides: one output row plus
    TILE_ROWS rows (a whole workgroup tile of rows past the end), at least 4096 elements.  Everything, payload included,
    starts as the sentinel SENT unless `fill` (array / tensor / scalar: accumulators, in-place flows) is given.  `lead`
    shifts the payload by that many elements off the allocation's 16-byte grid; `pitch` (2-D shapes) leaves padding columns
    that must keep the sentinel too.  Returns (payload view, check) — check(what) asserts every word outside the payload
    unchanged."""
    shape = tuple(int(s) for s in shape)
    if pitch is None:
        row = int(np.prod(shape[1:])) if len(shape) > 1 else 1
        n_pay = int(np.prod(shape))
    else:
        assert len(shape) == 2 and pitch >= shape[1]
        row, n_pay = pitch, shape[0] * pitch
    guard = cdiv(max(4096, row * (1 + TILE_ROWS)), 4) * 4  # (a multiple of 16 bytes: `lead` alone decides the alignment)
    buf = torch.empty(2 * guard + lead + n_pay, dtype=dtype, device=DEV)
    words = buf.view(torch.int32)
    words.fill_(SENT)
    inside = torch.zeros(buf.numel(), dtype=torch.bool, device=DEV)
    if pitch is None:
        view = buf[guard + lead:guard + lead + n_pay].view(shape)
        inside[guard + lead:guard + lead + n_pay] = True
    else:
        view = buf.as_strided(shape, (pitch, 1), guard + lead)
        inside.as_strided(shape, (pitch, 1), guard + lead).fill_(True)
    if fill is not None:
        view.copy_(torch.as_tensor(fill, dtype=dtype, device=DEV) if not isinstance(fill, torch.Tensor) else fill)
    outside = ~inside.repeat_interleave(buf.element_size() // 4)

    def check(what=""):
        bad = outside & (words != SENT)
        nbad = int(bad.sum())
        assert nbad == 0, (f"{what}: {nbad} words outside the output were written, the first at word "
                           f"{int(bad.nonzero()[0])} (payload starts at element {guard + lead})")

    return view, check


class Call:
    """The buffers of one ABI call: pitched / compact inputs (checked unchanged), guarded outputs (checked confined)."""

    def __init__(self, what):
        self.what, self.ins, self.outs, self.checks = what, [], {}, []

    def inp(self, a, lay, other=None, even=False):
        """2-D input in layout `lay`: (view, pitch)."""
        pitch, lead = layout(lay, np.shape(a)[1], other, even)
        view, whole, _ = pitched(a, pitch, lead)
        self.ins.append((whole, whole.clone()))
        return view, pitch

    def const(self, a, dtype=torch.float32):
        """A compact input without a pitch argument (flows, covariances, robustness maps, Hessians)."""
        t = T(a, dtype)
        self.ins.append((t, t.clone()))
        return t

    def out(self, name, shape, **kw):
        view, chk = guarded(shape, **kw)
        self.outs[name] = view
        self.checks.append((name, chk))
        return view

    def done(self):
        """Synchronise; inputs bit-identical, guards intact; the outputs as NumPy arrays."""
        torch.cuda.synchronize()
        for k, (t, snap) in enumerate(self.ins):
            it = torch.int16 if t.element_size() == 2 else torch.int32
            assert torch.equal(t.view(it), snap.view(it)), f"{self.what}: input {k} was modified"
        for name, chk in self.checks:
            chk(f"{self.what}: {name}")
        return {k: N(v) for k, v in self.outs.items()}


def same_bits(a, b, what):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    assert a.shape == b.shape and a.dtype == b.dtype, (what, a.shape, b.shape)
    it = {2: np.int16, 4: np.int32, 8: np.int64}[a.dtype.itemsize]
    diff = a.view(it) != b.view(it)
    if diff.any():
        k = tuple(np.argwhere(diff)[0])
        raise AssertionError(f"{what}: {int(diff.sum())} of {diff.size} values differ in their bits, the first at "
                             f"{list(map(int, k))}: {a[k]} vs {b[k]}")


def no_new_nan(got, want, what):
    bad = np.isnan(got) & ~np.isnan(np.broadcast_to(want, got.shape))
    assert not bad.any(), (f"{what}: {int(bad.sum())} NaN that the oracle does not have, the first at "
                           f"{np.argwhere(bad)[0].tolist()}")


def both(run, lay, what):
    """run(layout id) -> {name: array} on the compact layout and on `lay`; asserts 1 and returns the pitched result (the
    runs assert 4 and 5 themselves through Call.done)."""
    compact, got = run("compact"), run(lay)
    assert compact.keys() == got.keys()
    for k in got:
        same_bits(got[k], compact[k], f"{what} [{lay}] {k}: pitched vs compact")
    return got


def close(got, want, rtol, atol, what):
    """2 and 3 (assert_close counts a NaN against a number as a mismatch; spelled out for the message)."""
    no_new_nan(got, want, what)
    assert_close(got, want, rtol, atol, what)


# ------------------------------------------------------------------------------------------ pyramid
@pytest.mark.parametrize("lay", ALL)
def test_pad_circular(lay):
    """hhsr_pad_circular, Hp > H, Wp > W, Wp not a multiple of the 256-thread row blocks; the source takes layout `lay`
    and the destination the next one of the table (both pitches vary independently); against np.pad(mode="wrap")."""
    H, W, Hp, Wp = 45, 301, 48, 304
    a = np.random.default_rng(1).random((H, W), dtype=np.float32)

    def run(name):
        c = Call("hhsr_pad_circular")
        src, sp = c.inp(a, name)
        dp, dlead = layout(NEXT[name], Wp, other=sp)
        dst = c.out("dst", (Hp, Wp), pitch=dp, lead=dlead)
        _lib.call("hhsr_pad_circular", _lib.ptr(src), H, W, sp, _lib.ptr(dst), Hp, Wp, dp, _lib.stream())
        return c.done()

    got = both(run, lay, "pad_circular")
    close(got["dst"], np.pad(a, ((0, Hp - H), (0, Wp - W)), mode="wrap"), 0, 0, "pad_circular vs NumPy")


# (H, W) per factor: w2 / 32 x h2 / 16 output tiles = 9 x 10 workgroups, neither side a multiple of the tile
GD_SHAPES = {2: (300, 549), 4: (620, 1101)}
_GD = {}


def _gd_inputs(f):
    if f not in _GD:
        rng = np.random.default_rng(2 + f)
        imgs = [rng.random(GD_SHAPES[f], dtype=np.float32) for _ in range(3)]
        _GD[f] = (imgs, [oracle.downsample(i, f) for i in imgs])
    return _GD[f]


def _gd_dims(f):
    H, W = GD_SHAPES[f]
    h2, w2 = (H - 4 * f) // f, (W - 4 * f) // f
    nblk = cdiv(w2, 32) * cdiv(h2, 16)
    assert nblk > 64 and nblk % 8 and w2 % 32 and h2 % 16
    return H, W, h2, w2


@pytest.mark.parametrize("lay", ALL)
@pytest.mark.parametrize("f", [2, 4])
def test_gauss_decimate(f, lay):
    """hhsr_gauss_decimate, factors 2 and 4, source and destination pitch varied independently; tolerance of
    test_hip_parity.py::test_downsample (1e-6 absolute)."""
    H, W, h2, w2 = _gd_dims(f)
    imgs, want = _gd_inputs(f)
    taps, ntaps = utils_image._taps_for_launch(f)

    def run(name):
        c = Call("hhsr_gauss_decimate")
        src, sp = c.inp(imgs[0], name)
        dp, dlead = layout(NEXT[name], w2, other=sp)
        dst = c.out("dst", (h2, w2), pitch=dp, lead=dlead)
        _lib.call("hhsr_gauss_decimate", _lib.ptr(src), H, W, sp, _lib.ptr(dst), dp, f, taps, ntaps, _lib.stream())
        return c.done()

    got = both(run, lay, f"gauss_decimate f{f}")
    close(got["dst"], want[0], 0, 1e-6, f"gauss_decimate f{f} [{lay}] vs oracle")


@pytest.mark.parametrize("lay", ["even2", "odd", "lead1"])
@pytest.mark.parametrize("n", [3, 9])
@pytest.mark.parametrize("f", [2, 4])
def test_gauss_decimate_batch(f, n, lay):
    """hhsr_gauss_decimate_batch: 3 frames, and 9 = one full launch of HHSR_MAX_BATCH = 8 plus a partial one."""
    H, W, h2, w2 = _gd_dims(f)
    imgs, want = _gd_inputs(f)
    taps, ntaps = utils_image._taps_for_launch(f)
    assert n <= 3 or n > _lib.MAX_BATCH

    def run(name):
        c = Call("hhsr_gauss_decimate_batch")
        srcs = [c.inp(imgs[k % 3], name) for k in range(n)]
        sp = srcs[0][1]
        dp, dlead = layout(NEXT[name], w2, other=sp)
        dsts = [c.out(f"dst{k}", (h2, w2), pitch=dp, lead=dlead) for k in range(n)]
        _lib.call("hhsr_gauss_decimate_batch", _lib.ptr_array([s[0] for s in srcs]), n, H, W, sp, _lib.ptr_array(dsts), dp,
                  f, taps, ntaps, _lib.stream())
        return c.done()

    got = both(run, lay, f"gauss_decimate_batch f{f} n{n}")
    for k in range(n):
        close(got[f"dst{k}"], want[k % 3], 0, 1e-6, f"gauss_decimate_batch f{f} [{lay}] frame {k} vs oracle")


# ------------------------------------------------------------------------------------------ alignment pieces
GNY, GNX = 5, 7  # 35 tiles: 9 workgroups of 4 tiles with a remainder of 3 (k_bm_wave, k_ica_wave)
_BM = {}


def _bm_case(ts, r, shift=(2, -3)):
    """bm_inputs on a 5 x 7 tile grid (half-integer ties, windows leaving the moving level), once per (ts, r)."""
    key = (ts, r, shift)
    if key not in _BM:
        _BM[key] = bm_inputs(np.random.default_rng(4 + ts + r), ts, r, GNY, GNX, shift)
    return _BM[key]


def _grad_hessian(c, lvl_view, H, W, pitch, lead, ts, tag=""):
    """hhsr_grad_hessian into guarded gx / gy AT THE INPUT'S PITCH (the layout contract with hhsr_ica) and a compact hess."""
    gx = c.out(tag + "gx", (H, W), pitch=pitch, lead=lead)
    gy = c.out(tag + "gy", (H, W), pitch=pitch, lead=lead)
    hess = c.out(tag + "hess", (H // ts, W // ts, 2, 2))
    _lib.call("hhsr_grad_hessian", _lib.ptr(lvl_view), H, W, pitch, ts, _lib.ptr(gx), _lib.ptr(gy), _lib.ptr(hess),
              _lib.stream())
    return gx, gy, hess


@pytest.mark.parametrize("lay", ALL)
@pytest.mark.parametrize("ts", [8, 16, 32, 64])
def test_grad_hessian_then_ica(ts, lay):
    """hhsr_grad_hessian on the level of test_hip_parity.py::test_grad_hessian (neither side a multiple of the tile), and
    on a 5 x 7 tile reference level whose gx / gy — written at the input's pitch — feed hhsr_ica at ref_pitch, with the
    moving level at another pitch; the incoming flows are the oracle's block-matching result (oracle.bm_l2, r = 2), the
    flows ICA meets in the pipeline.  Tolerances of test_grad_hessian (gradients exact, Hessian 2e-5 / 1e-7) and of test_ica
    (2e-4 px); at ts = 64 both values of flags bit 0.  The Hessian is compared with the oracle's on test_grad_hessian's
    level, where its 2e-5 relative tolerance was set; on the 5 x 7 tile level an off-diagonal entry at ts = 64 is a sum of
    4096 products that cancel to 0.084 next to diagonal entries of 43, and the float32 sum sits 3.4e-5 (relative to the
    RESULT) from the float64 one in 2 of 140 values, in the compact layout exactly as in the pitched ones.  That Hessian
    is asserted pitched == compact bit for bit and through the flows hhsr_ica computes from it."""
    lvl = smooth(np.random.default_rng(3), 3 * 64 + 5, 2 * 64 + 9)
    ref, mov, flow0 = _bm_case(ts, 2, (1, -2))
    fbm = oracle.bm_l2(ref, mov, flow0, ts, 2)
    n_iter = 3

    def run(name):
        c = Call("hhsr_grad_hessian")
        v, p = c.inp(lvl, name)
        _grad_hessian(c, v, lvl.shape[0], lvl.shape[1], p, layout(name, lvl.shape[1])[1], ts, "lvl_")
        tref, rp = c.inp(ref, name)
        gx, gy, hess = _grad_hessian(c, tref, ref.shape[0], ref.shape[1], rp, layout(name, ref.shape[1])[1], ts)
        res = c.done()
        c = Call("hhsr_ica")
        tref, rp2 = c.inp(ref, name)
        assert rp2 == rp
        tmov, mp = c.inp(mov, name, other=rp)
        th = c.const(N(hess))
        c.ins += [(g._base, g._base.clone()) for g in (gx, gy)]  # (inputs now: guards and padding columns included)
        for bug in ((1, 0) if ts == 64 else (1,)):
            flow = c.out(f"flow_bug{bug}", fbm.shape, fill=fbm)
            _lib.call("hhsr_ica", _lib.ptr(tref), _lib.ptr(gx), _lib.ptr(gy), rp, _lib.ptr(th), _lib.ptr(tmov), mov.shape[0],
                      mov.shape[1], mp, _lib.ptr(flow), GNY, GNX, ts, n_iter, bug, _lib.stream())
        res.update(c.done())
        return res

    got = both(run, lay, f"grad_hessian + ica ts={ts}")
    for tag, img in (("lvl_", lvl), ("", ref)):
        ogx, ogy, oH = oracle.init_ica(img, ts)
        close(got[tag + "gx"], ogx, 0, 0, f"{tag}gx ts={ts} [{lay}]")
        close(got[tag + "gy"], ogy, 0, 0, f"{tag}gy ts={ts} [{lay}]")
        if tag:  # (the Hessian of the block-matching level is judged through what hhsr_ica makes of it: see the docstring)
            close(got[tag + "hess"], oH, 2e-5, 1e-7, f"{tag}hess ts={ts} [{lay}]")
    for bug in ((1, 0) if ts == 64 else (1,)):
        want = oracle.ica(ref, ogx, ogy, oH, mov, fbm, ts, n_iter, ica64_row_bug=bool(bug))
        close(got[f"flow_bug{bug}"], want, 0, 2e-4, f"ica ts={ts} bug={bug} [{lay}]")


@pytest.mark.parametrize("lay", ALL)
@pytest.mark.parametrize("ts,r", [(8, 4), (16, 4), (16, 1), (32, 4), (64, 4)])
def test_bm_l2(ts, r, lay):
    """hhsr_bm_l2 at every tile size it accepts (k_bm_wave<8 / 16 / 32>, k_block_match at 64), ref_pitch != mov_pitch, with
    the flows of bm_inputs whose windows leave the moving level (clamp to edge: where mw and mov_pitch meet); judged like
    test_hip_parity.py::test_bm_l2 (check_bm)."""
    ref, mov, flow0 = _bm_case(ts, r)

    def run(name):
        c = Call("hhsr_bm_l2")
        tref, rp = c.inp(ref, name)
        tmov, mp = c.inp(mov, name, other=rp)
        flow = c.out("flow", flow0.shape, fill=flow0)
        _lib.call("hhsr_bm_l2", _lib.ptr(tref), rp, _lib.ptr(tmov), mov.shape[0], mov.shape[1], mp, _lib.ptr(flow), GNY, GNX,
                  ts, r, _lib.stream())
        return c.done()

    got = both(run, lay, f"bm_l2 ts={ts} r={r}")
    want, cost = oracle.bm_l2(ref, mov, flow0, ts, r, return_cost=True)
    no_new_nan(got["flow"], want, f"bm_l2 ts={ts} r={r} [{lay}]")
    check_bm(got["flow"], want, cost, f"bm_l2 ts={ts} r={r} [{lay}]")


@pytest.mark.parametrize("lay", ALL)
@pytest.mark.parametrize("ts,r", [(16, 1), (16, 4), (32, 2), (64, 1)])
def test_bm_l1(ts, r, lay):
    """hhsr_bm_l1, modes 0 and 1, at every tile size it accepts (zero outside the moving level); judged like
    test_hip_parity.py::test_bm_l1."""
    ref, mov, flow0 = _bm_case(ts, r, (1, -1))

    def run(name):
        c = Call("hhsr_bm_l1")
        tref, rp = c.inp(ref, name)
        tmov, mp = c.inp(mov, name, other=rp)
        for mode in (0, 1):
            flow = c.out(f"flow_mode{mode}", flow0.shape, fill=flow0)
            _lib.call("hhsr_bm_l1", _lib.ptr(tref), rp, _lib.ptr(tmov), mov.shape[0], mov.shape[1], mp, _lib.ptr(flow), GNY,
                      GNX, ts, r, mode, _lib.stream())
        return c.done()

    got = both(run, lay, f"bm_l1 ts={ts} r={r}")
    want, cost = oracle.bm_l1(ref, mov, flow0, ts, r, return_cost=True)
    no_new_nan(got["flow_mode0"], want, f"bm_l1 ts={ts} r={r} [{lay}]")
    check_bm(got["flow_mode0"], want, cost, f"bm_l1 ts={ts} r={r} [{lay}]")
    close(got["flow_mode1"], oracle.bm_l1(ref, mov, flow0, ts, r, effective=True), 0, 0, f"bm_l1 effective ts={ts} [{lay}]")


# ------------------------------------------------------------------------------------------ fused level kernel
_ALIGN = {}
ALIGN_FULL_TABLE = [(16, 1, "L2"), (16, 1, "L1"), (32, 4, "L2")]
ALIGN_PARAMS = [(ts, r, m, "even2") for ts, r, m in V.ALIGN_CASES] + \
               [(ts, r, m, lay) for ts, r, m in ALIGN_FULL_TABLE for lay in ALL if lay != "even2"]


def _align_case(ts, r, metric):
    """The first 3 moving frames of test_variant_parity.py's case on its 37 x 23 tile grid and the oracle's flows and
    costs, once per case."""
    key = (ts, r, metric)
    if key not in _ALIGN:
        cfg = base_config(ts=ts, metrics=(metric,) * 4)
        cfg.block_matching.tuning.tile_sizes = [ts] * 4
        cfg.block_matching.tuning.search_radii = [r] * 4
        ref, movs, flows = V._align_inputs(ts, r, 3, 1000 + 10 * ts + r + V.METRIC_CODE[metric])
        state = oracle.init_ica(ref, ts)
        want = [V._align_oracle(ref, state, movs[k], flows[k], ts, r, metric, cfg) for k in range(3)]
        _ALIGN[key] = (cfg, ref, movs, flows, state, want)
    return _ALIGN[key]


def _align_call(name, entry, ref, hess, movs, flows_in, ts, r, metric, n_iter, coarse=None):
    """hhsr_align_level_batch (or, one frame, hhsr_align_level) with the reference level in layout `name` and the moving
    levels in the same layout at another pitch."""
    c = Call(entry)
    tref, rp = c.inp(ref, name)
    tm = [c.inp(m, name, other=rp) for m in movs]
    mp = tm[0][1]
    assert mp != rp or name == "compact"
    th = c.const(hess)
    flows = [c.out(f"flow{k}", f.shape, fill=f) for k, f in enumerate(flows_in)]
    rh, rw = ref.shape
    mh, mw = movs[0].shape
    if coarse is None:
        tc, cny, cnx, rep, mult = None, 0, 0, 0, 1.0
    else:
        cf, rep, mult = coarse
        tc = [c.const(x) for x in cf]
        cny, cnx = cf[0].shape[:2]
    if entry == "hhsr_align_level":
        _lib.call("hhsr_align_level", _lib.ptr(tref), rh, rw, rp, _lib.ptr(th), _lib.ptr(tm[0][0]), mh, mw, mp,
                  _lib.ptr(flows[0]), V.NY, V.NX, ts, r, V.METRIC_CODE[metric], n_iter, _lib.ptr(tc[0] if tc else None),
                  int(cny), int(cnx), int(rep), float(mult), _lib.stream())
    else:
        _lib.call("hhsr_align_level_batch", _lib.ptr(tref), rh, rw, rp, _lib.ptr(th), _lib.ptr_array([m[0] for m in tm]),
                  len(tm), mh, mw, mp, _lib.ptr_array(flows), V.NY, V.NX, ts, r, V.METRIC_CODE[metric], n_iter,
                  _lib.ptr_array(tc) if tc else None, int(cny), int(cnx), int(rep), float(mult), _lib.stream())
    return c.done()


@pytest.mark.parametrize("ts,r,metric,lay", ALIGN_PARAMS)
def test_align_level_batch(ts, r, metric, lay):
    """Every k_align_wave<ts, r, L1> instantiation with ref_pitch != mov_pitch (its windows are staged through per-thread
    byte offsets built from the two pitches): 3 frames, layout even2 for all sixteen cases and the whole table for three of
    them; judged like test_variant_parity.py (_judge: 2e-4 px, near-tie rule, the exact ties of the windows outside)."""
    cfg, ref, movs, flows, state, want = _align_case(ts, r, metric)
    n_iter = int(cfg.ica.tuning.n_iter)
    hess = state[2]
    got = both(lambda name: _align_call(name, "hhsr_align_level_batch", ref, hess, movs, flows, ts, r, metric, n_iter), lay,
               f"align_level_batch ts={ts} r={r} {metric}")
    for k in range(3):
        no_new_nan(got[f"flow{k}"], want[k][0], f"align ts={ts} r={r} {metric} [{lay}] frame {k}")
        V._judge(got[f"flow{k}"], want[k][0], want[k][1], f"align ts={ts} r={r} {metric} [{lay}] frame {k}", min_ties=3)


@pytest.mark.parametrize("entry,lay", [("hhsr_align_level_batch", "odd"), ("hhsr_align_level", "lead1")])
def test_align_level_coarse_flow_read_in_place(entry, lay):
    """The incoming flow read from the coarser level in place (rep 2, a coarse grid that does not cover the fine one), on
    pitched levels, through hhsr_align_level_batch (3 frames) and once through hhsr_align_level (it forwards); the flow
    buffers start as NaN and are outputs only."""
    ts, r, metric, rep = 16, 2, "L2", 2
    cfg, ref, movs, _, state, _ = _align_case(ts, r, metric)
    n = 3 if entry.endswith("batch") else 1
    rng = np.random.default_rng(rep)
    cny, cnx = (V.NY - 1) // rep, (V.NX - 1) // rep
    coarse = [rng.uniform(-1.2, 1.2, (cny, cnx, 2)).astype(np.float32) / rep for _ in range(n)]
    cfg_up = base_config(ts=ts, metrics=(metric,) * 4)
    cfg_up.block_matching.tuning.tile_sizes = [ts] * 4
    cfg_up.block_matching.tuning.factors = [1, rep, 2, 2]
    cfg_up.block_matching.tuning.flow_upscale_mode = "nearest"
    nan = [np.full((V.NY, V.NX, 2), np.nan, np.float32)] * n
    got = both(lambda name: _align_call(name, entry, ref, state[2], movs[:n], nan, ts, r, metric, int(cfg.ica.tuning.n_iter),
                                        coarse=(coarse, rep, float(rep))), lay, entry + " coarse")
    for k in range(n):
        fin = oracle.upscale_lvl(coarse[k], (V.NY, V.NX), 0, cfg_up)
        want, cost = V._align_oracle(ref, state, movs[k], fin, ts, r, metric, cfg)
        no_new_nan(got[f"flow{k}"], want, f"{entry} coarse frame {k}")
        V._judge(got[f"flow{k}"], want, cost, f"{entry} coarse [{lay}] frame {k}")


# ------------------------------------------------------------------------------------------ per-frame statistics
SH, SW = 300, 524  # quads 150 x 262: 10 x 9 = 90 workgroups of 16 x 32 quads, 90 % 8 = 2, partial tiles on both edges
CFAS = {"rggb": [[0, 1], [1, 2]], "bggr": [[2, 1], [1, 0]], "grbg": [[1, 0], [2, 1]], "gbrg": [[1, 2], [0, 1]],
        "rgbg": [[0, 1], [2, 1]]}  # the last: not a Bayer layout (the run-time colour loop of k_frame_stats)
WBS = {"unit": [1.0, 1.0, 1.0], "wb": [1.9, 1.0, 1.6]}
_STATS = {}


def _stats_case(shape, cfa_id, wb_id):
    """A raw frame with a constant block (NaN covariances under the linear law) and 2 more frames; the oracle's guide
    statistics and covariances of each, on the even crop the kernels work on; once per case."""
    key = (shape, cfa_id, wb_id)
    if key not in _STATS:
        H, W = shape
        cfg = base_config(snr=12.0, ts=16)
        frames = []
        for k in range(3):
            raw = synth.make_burst(H + H % 2, W + W % 2, 1, seed=5 + k)[0][:H, :W].copy()
            raw[40:60, 50:90] = 0.3
            frames.append(raw)
        want = []
        for raw in frames:
            crop = raw[:H - H % 2, :W - W % 2]
            m, v = oracle.local_stats(oracle.guide_image(crop, CFAS[cfa_id], WBS[wb_id]))
            want.append((m, v, oracle.estimate_kernels(crop, cfg)))
        assert np.isnan(want[0][2]).any()
        _STATS[key] = (cfg, frames, want)
    return _STATS[key]


def _bayer_stats(shape, cfa_id, wb_id, lay):
    H, W = shape
    gh, gw = H // 2, W // 2
    cfg, frames, want = _stats_case(shape, cfa_id, wb_id)
    params = kernels._kernel_params(cfg)
    cfa, wb = _lib.cfa_bytes(CFAS[cfa_id]), _lib.doubles(WBS[wb_id])
    what = f"{cfa_id} {wb_id} {H}x{W}"

    def run(name):
        res = {}
        c = Call("hhsr_cov_from_raw")
        raw, p = c.inp(frames[0], name, even=True)
        covs = c.out("cov_covs", (gh, gw, 2, 2))
        _lib.call("hhsr_cov_from_raw", _lib.ptr(raw), H, W, p, _lib.ptr(covs), *params, _lib.stream())
        res.update(c.done())
        c = Call("hhsr_rob_stats")
        raw, p = c.inp(frames[0], name, even=True)
        m1, m2, v2 = c.out("rob_means_only", (3, gh, gw)), c.out("rob_means", (3, gh, gw)), c.out("rob_vars", (3, gh, gw))
        _lib.call("hhsr_rob_stats", _lib.ptr(raw), H, W, p, cfa, wb, _lib.ptr(m1), None, _lib.stream())
        _lib.call("hhsr_rob_stats", _lib.ptr(raw), H, W, p, cfa, wb, _lib.ptr(m2), _lib.ptr(v2), _lib.stream())
        res.update(c.done())
        c = Call("hhsr_frame_stats")
        raw, p = c.inp(frames[0], name, even=True)
        m1, c1 = c.out("fs_means_only", (3, gh, gw)), c.out("fs_covs_only", (gh, gw, 2, 2))
        m2, v2, c2 = c.out("fs_means", (3, gh, gw)), c.out("fs_vars", (3, gh, gw)), c.out("fs_covs", (gh, gw, 2, 2))
        _lib.call("hhsr_frame_stats", _lib.ptr(raw), H, W, p, cfa, wb, _lib.ptr(m1), None, _lib.ptr(c1), *params, _lib.stream())
        _lib.call("hhsr_frame_stats", _lib.ptr(raw), H, W, p, cfa, wb, _lib.ptr(m2), _lib.ptr(v2), _lib.ptr(c2), *params,
                  _lib.stream())
        res.update(c.done())
        c = Call("hhsr_frame_stats_batch")
        raws = [c.inp(f, name, even=True) for f in frames]
        ms = [c.out(f"fsb_means{k}", (3, gh, gw)) for k in range(3)]
        cs = [c.out(f"fsb_covs{k}", (gh, gw, 2, 2)) for k in range(3)]
        _lib.call("hhsr_frame_stats_batch", _lib.ptr_array([r[0] for r in raws]), 3, H, W, raws[0][1], cfa, wb,
                  _lib.ptr_array(ms), _lib.ptr_array(cs), *params, _lib.stream())
        res.update(c.done())
        return res

    got = both(run, lay, "Bayer statistics " + what)
    m, v, cv = want[0]
    # tolerances: test_frame_stats_equals_separate_passes (means 1e-6 / 1e-7, variances 1e-5 / 1e-7) and
    # test_cov_random_and_constant (covariances 1e-4 / 1e-6)
    for k in ("rob_means_only", "rob_means", "fs_means_only", "fs_means"):
        close(got[k], m, 1e-6, 1e-7, f"{what} [{lay}] {k}")
    for k in ("rob_vars", "fs_vars"):
        close(got[k], v, 1e-5, 1e-7, f"{what} [{lay}] {k}")
    for k in ("cov_covs", "fs_covs_only", "fs_covs"):
        close(got[k], cv, 1e-4, 1e-6, f"{what} [{lay}] {k}")
    for k in range(3):
        close(got[f"fsb_means{k}"], want[k][0], 1e-6, 1e-7, f"{what} [{lay}] batch means {k}")
        close(got[f"fsb_covs{k}"], want[k][2], 1e-4, 1e-6, f"{what} [{lay}] batch covs {k}")


@pytest.mark.parametrize("lay", EVEN)
@pytest.mark.parametrize("wb_id", list(WBS))
@pytest.mark.parametrize("cfa_id", list(CFAS))
def test_bayer_statistics(cfa_id, wb_id, lay):
    """hhsr_cov_from_raw, hhsr_rob_stats, hhsr_frame_stats (vars NULL and given) and hhsr_frame_stats_batch (3 frames) on
    the four Bayer patterns and one other 2 x 2 layout, with white balance (1, 1, 1) (the float32 shortcut) and another
    one, in the layouts these calls accept (even pitch, 8-byte aligned raw: the kernel loads pixel pairs)."""
    _bayer_stats((SH, SW), cfa_id, wb_id, lay)


@pytest.mark.parametrize("shape", [(SH + 1, SW), (SH, SW + 1)], ids=["oddH", "oddW"])
def test_bayer_statistics_odd_size(shape):
    """An odd height / width: the last row / column belongs to no quad; the pitch stays even."""
    _bayer_stats(shape, "grbg", "wb", "even2")


@pytest.mark.parametrize("lay", ALL)
def test_mono_frame_stats(lay):
    """hhsr_mono_frame_stats in its three template forms (statistics only, covariances only, both); tolerances of
    test_hip_parity.py::test_mono_stages_golden (covariances 1e-4 / 1e-6, means 1e-6 / 1e-8, variances 1e-4 / 1e-9)."""
    H, W = 150, 263  # 10 x 9 workgroups of 16 x 32 pixels
    cfg = base_config(snr=12.0, ts=16, mode="grey")
    raw = synth.make_burst(H + 1, W + 1, 1, seed=6)[0][:H, :W].copy()
    params = kernels._kernel_params(cfg)
    none = (1.0, 0.0, 0.0, 0.0, 0.0, 1.0, 0.0, 1.0, 0)

    def run(name):
        c = Call("hhsr_mono_frame_stats")
        t, p = c.inp(raw, name)
        m1, v1 = c.out("means_s", (H, W)), c.out("vars_s", (H, W))
        m0 = c.out("means_only", (H, W))
        c2 = c.out("covs_c", (H, W, 2, 2))
        m3, v3, c3 = c.out("means_b", (H, W)), c.out("vars_b", (H, W)), c.out("covs_b", (H, W, 2, 2))
        st = _lib.stream()
        _lib.call("hhsr_mono_frame_stats", _lib.ptr(t), H, W, p, _lib.ptr(m1), _lib.ptr(v1), None, *none, st)
        _lib.call("hhsr_mono_frame_stats", _lib.ptr(t), H, W, p, _lib.ptr(m0), None, None, *none, st)
        _lib.call("hhsr_mono_frame_stats", _lib.ptr(t), H, W, p, None, None, _lib.ptr(c2), *params, st)
        _lib.call("hhsr_mono_frame_stats", _lib.ptr(t), H, W, p, _lib.ptr(m3), _lib.ptr(v3), _lib.ptr(c3), *params, st)
        return c.done()

    got = both(run, lay, "mono_frame_stats")
    m, v = oracle.local_stats(raw[None])
    cv = oracle.estimate_kernels(raw, cfg)
    for k in ("means_s", "means_only", "means_b"):
        close(got[k], m[0], 1e-6, 1e-8, f"mono [{lay}] {k}")
    for k in ("vars_s", "vars_b"):
        close(got[k], v[0], 1e-4, 1e-9, f"mono [{lay}] {k}")
    for k in ("covs_c", "covs_b"):
        close(got[k], cv, 1e-4, 1e-6, f"mono [{lay}] {k}")


# ------------------------------------------------------------------------------------------ merge
V.SENSORS.setdefault("rgbg", ((0, 1), (2, 1)))  # a 2 x 2 layout that is not Bayer (after V's own parametrisation)
ISO, F64, GENERIC, TILE, X2V1, MONO, REF_DIVIDE, REF_FAST = 1, 2, 4, 8, 16, 32, 64, 128
LOAD_ACC, DO_REF, DIVIDE, STORE_DEN, LOCAL_MIN, STORE_CLASSES, LOAD_CLASSES = 1, 2, 4, 8, 16, 32, 64
_LMIN = {}


def _dims(scale):
    H, W, ts = V.SHAPES[scale]
    return H, W, ts, cdiv(H, ts), cdiv(W, ts), round(scale * H), round(scale * W)


def _kflags(sensor):
    return MONO if sensor == "grey" else 0


def _frames(c, scale, sensor, lay, rows=None):
    """The four comp frames and the reference frame of V._merge_inputs in layout `lay` (one pitch for all of them), the
    flows / covariances / robustness maps compact: (pointer tables of raws, flows, covs, rs; ref raw; ref covs; pitch)."""
    ref, ref_covs, frames = V._merge_inputs(scale, sensor)
    raws = [c.inp(f[0], lay) for f in frames]
    tref, p = c.inp(ref, lay)
    assert all(r[1] == p for r in raws)
    return ([r[0] for r in raws], [c.const(f[1]) for f in frames], [c.const(f[2]) for f in frames],
            [c.const(f[3]) for f in frames], tref, c.const(ref_covs), p)


@pytest.mark.parametrize("scale,sensor,lays", [(2, "rggb", ALL), (1.5, "rggb", ["even2", "lead1"]),
                                                (3, "rggb", ["odd", "lead2"]), (2, "grey", ["even2", "lead1"])])
def test_accumulate_and_accumulate_ref(scale, sensor, lays):
    """hhsr_accumulate over the four frames, then hhsr_accumulate_ref without acc_rob: plain, HHSR_REF_DIVIDE and
    HHSR_REF_FAST (+ divide); against the oracle's sums after the comp frames and after the reference frame (_assert_sums)
    and its normalised image (TOL), as test_variant_parity.py::test_merge_launch_forms_vs_oracle judges the same
    operators.  At x2 RGGB also with acc_rob (the accumulated-robustness rule), against cfast.merge_ref."""
    H, W, ts, ny, nx, sH, sW = _dims(scale)
    o = V._oracle_merge(scale, sensor, "steerable")
    ref, ref_covs, frames = V._merge_inputs(scale, sensor)
    cfa = _lib.cfa_bytes(V.SENSORS[sensor])
    kf = _kflags(sensor)
    acc32 = V._acc_want(frames).astype(np.float32)
    with_acc = (scale, sensor) == (2, "rggb")
    cfg_d = V._cfg(scale, sensor)
    cfg_d.accumulated_robustness_denoiser.enabled = True
    cfg_d.accumulated_robustness_denoiser.merge.enabled = True
    dm = cfg_d.accumulated_robustness_denoiser.merge

    def run(name):
        c = Call("hhsr_accumulate")
        raws, flows, covs, rs, tref, trc, p = _frames(c, scale, sensor, name)
        zero = np.zeros((sH, sW, 3), np.float32)
        num, den = c.out("num_c", zero.shape, fill=zero), c.out("den_c", zero.shape, fill=zero)
        for k in range(4):
            _lib.call("hhsr_accumulate", _lib.ptr(raws[k]), H, W, p, _lib.ptr(flows[k]), ny, nx, ts, _lib.ptr(covs[k]),
                      _lib.ptr(rs[k]), cfa, float(scale), kf, _lib.ptr(num), _lib.ptr(den), sH, sW, _lib.stream())
        res = c.done()
        c = Call("hhsr_accumulate_ref")
        tref, p = c.inp(ref, name)
        trc = c.const(ref_covs)
        forms = [("ref", 0), ("div", REF_DIVIDE), ("fast", REF_FAST | REF_DIVIDE)] + ([("acc", 0)] if with_acc else [])
        tacc = c.const(acc32)
        for tag, extra in forms:
            n2, d2 = c.out("num_" + tag, zero.shape, fill=res["num_c"]), c.out("den_" + tag, zero.shape, fill=res["den_c"])
            acc = tag == "acc"
            _lib.call("hhsr_accumulate_ref", _lib.ptr(tref), H, W, p, _lib.ptr(trc), cfa, float(scale), kf | extra,
                      _lib.ptr(tacc if acc else None), int(dm.rad_max) if acc else 0, float(dm.max_multiplier) if acc else 0.0,
                      float(dm.max_frame_count) if acc else 0.0, _lib.ptr(n2), _lib.ptr(d2), sH, sW, _lib.stream())
        res.update(c.done())
        return res

    for lay in lays:
        what = f"x{scale} {sensor} [{lay}]"
        got = both(run, lay, "accumulate x%s %s" % (scale, sensor))
        for k, key in (("num_c", "num_c"), ("den_c", "den_c"), ("num_ref", "num"), ("den_ref", "den")):
            no_new_nan(got[k], o[key], f"{what} {k}")
            V._assert_sums(got[k], o[key], scale, f"{what} {k}")
        ch = (Ellipsis, 0) if sensor == "grey" else Ellipsis  # (grey: channels 1, 2 are left as they are, the oracle's are 0 / 0)
        close(got["num_div"][ch], o["out"][ch], *TOL, what + " REF_DIVIDE image")
        same_bits(got["den_div"], got["den_c"], what + " REF_DIVIDE leaves den as it is")
        close(got["num_fast"][ch], o["out"][ch], *TOL, what + " REF_FAST | REF_DIVIDE image")
        if with_acc:
            assert 0.05 < (acc32 < dm.max_frame_count).mean() < 0.95
            onum, oden = o["num_c"].copy(), o["den_c"].copy()
            cfast.merge_ref(ref, ref_covs, onum, oden, V.SENSORS[sensor], cfg_d, acc_rob=acc32.astype(np.float64),
                            threads=THREADS)
            # (the HIP sums start from HIP's own num_c / den_c, within _assert_sums of the oracle's: the same rule applies)
            V._assert_sums(got["num_acc"], onum, scale, what + " acc_rob num")
            V._assert_sums(got["den_acc"], oden, scale, what + " acc_rob den")


def _lmin_oracle(scale):
    """The oracle's image for RGGB frames whose robustness maps pass through the 5 x 5 minimum first."""
    if scale not in _LMIN:
        ref, ref_covs, frames = V._merge_inputs(scale, "rggb")
        H, W, _ = V.SHAPES[scale]
        cfg = V._cfg(scale, "rggb")
        num = np.zeros((scale * H, scale * W, 3), np.float32)
        den = np.zeros_like(num)
        rmin = [oracle.robustness.local_min(f[3]) for f in frames]
        for f, r in zip(frames, rmin):
            cfast.merge(f[0], f[1], f[2], r, num, den, V.SENSORS["rggb"], cfg, threads=THREADS)
        cfast.merge_ref(ref, ref_covs, num, den, V.SENSORS["rggb"], cfg, threads=THREADS)
        with np.errstate(all="ignore"):
            _LMIN[scale] = (num.astype(np.float64) / den, np.sum([r.astype(np.float64) for r in rmin], axis=0))
    return _LMIN[scale]


# id: (scale, sensor, kflags, flags, layouts) — the kernel hhsr_merge_burst picks is named in the id
MB = {
    "x2_k_merge_x2": (2, "rggb", 0, DO_REF | DIVIDE, ALL),
    "x2_k_merge_x2_gbrg": (2, "gbrg", 0, DO_REF | DIVIDE, ["odd"]),
    "x2_first_generation_forced": (2, "rggb", X2V1, DO_REF | DIVIDE, ["even2", "lead1"]),
    "x2_first_generation_non_bayer": (2, "rgbg", 0, DO_REF | DIVIDE, ["even2", "odd"]),
    "x3_k_merge_x3": (3, "rggb", 0, DO_REF | DIVIDE, ALL),
    "x1_tile": (1, "rggb", 0, DO_REF | DIVIDE, ["even2", "lead1"]),
    "x4_tile": (4, "rggb", 0, DO_REF | DIVIDE, ["odd", "lead2"]),
    "x2_tile_forced": (2, "rggb", TILE, DO_REF | DIVIDE, ["even2", "lead1"]),
    "x2_generic_forced": (2, "rggb", GENERIC, DO_REF | DIVIDE, ["even2", "lead1"]),
    "x1.5_generic_geom_f64": (1.5, "rggb", 0, DO_REF | DIVIDE, ["even2", "odd"]),
    "x2_weight_f64": (2, "rggb", F64, DO_REF | DIVIDE, ["even2", "lead1"]),
    "x2_mono_tile": (2, "grey", MONO, DO_REF | DIVIDE, ["even2", "odd"]),
    "x3_mono_generic": (3, "grey", MONO, DO_REF | DIVIDE, ["even2", "lead1"]),
    "x2_local_min": (2, "rggb", 0, DO_REF | DIVIDE | LOCAL_MIN, ["even2", "lead1"]),
    "x3_local_min": (3, "rggb", 0, DO_REF | DIVIDE | LOCAL_MIN, ["even2", "odd"]),
    "x2_store_den_no_divide": (2, "rggb", 0, DO_REF | STORE_DEN, ["even2", "lead1"]),
    "x3_store_den_no_divide": (3, "rggb", 0, DO_REF | STORE_DEN, ["wide"]),
    "x4_store_den_no_divide": (4, "rggb", 0, DO_REF | STORE_DEN, ["even2"]),
}


def _merge_burst(c, scale, sensor, kflags, flags, lay, num_lead=0, tag=""):
    """One hhsr_merge_burst over the four frames of the input set; outputs num (den with STORE_DEN, acc_r at the integer
    scales with float32 weights) guarded, `num_lead` elements off the 16-byte grid."""
    H, W, ts, ny, nx, sH, sW = _dims(scale)
    raws, flows, covs, rs, tref, trc, p = _frames(c, scale, sensor, lay)
    num = c.out(tag + "num", (sH, sW, 3), lead=num_lead)
    den = c.out(tag + "den", (sH, sW, 3), lead=num_lead) if flags & STORE_DEN else None
    acc = c.out(tag + "acc_r", (H, W), fill=0.0) if float(scale).is_integer() and not kflags & F64 else None
    args = (_lib.ptr_array(raws), _lib.ptr_array(flows), _lib.ptr_array(covs), _lib.ptr_array(rs), 4, H, W, p, ny, nx, ts,
            _lib.ptr(tref), _lib.ptr(trc), None if sensor == "grey" else _lib.cfa_bytes(V.SENSORS[sensor]), float(scale),
            kflags, flags, _lib.ptr(num), _lib.ptr(den), _lib.ptr(acc), sH, sW, 0, sH, 0, _lib.stream())
    return args


def _judge_merge(got, scale, sensor, flags, what, tag=""):
    ref, ref_covs, frames = V._merge_inputs(scale, sensor)
    if flags & LOCAL_MIN:
        want, acc_want = _lmin_oracle(scale)
    else:
        o = V._oracle_merge(scale, sensor, "steerable")
        want, acc_want = o["out"], V._acc_want(frames)
    if flags & DIVIDE:
        img = got[tag + "num"]
        if sensor == "grey":  # channels 1, 2: 0 / 0 = NaN from the x2 tile kernel, left as they are by the generic one
            img, want = img[..., 0], want[..., 0]
        close(img, want, *TOL, what + " image")
    else:
        for k in ("num", "den"):
            no_new_nan(got[tag + k], o[k], f"{what} {k}")
            V._assert_sums(got[tag + k], o[k], scale, f"{what} {k}")
    if tag + "acc_r" in got:
        close(got[tag + "acc_r"], acc_want, 1e-6, 1e-6, what + " accumulated robustness")


@pytest.mark.parametrize("case", list(MB))
def test_merge_burst(case):
    """hhsr_merge_burst with every kernel its dispatcher can pick (forced through kflags where it is not the default), on
    the four-frame input sets of test_variant_parity.py (a frame pushed partly out of the image: the border paths that
    clamp to H - 1 / W - 1 and multiply by the pitch; negative flows; robustness patches of 0); comp frames and ref_raw share
    the one pitch.  Image at TOL, raw sums by _assert_sums, accumulated robustness 1e-6, as that file judges them."""
    scale, sensor, kflags, flags, lays = MB[case]

    def run(name):
        c = Call("hhsr_merge_burst " + case)
        _lib.call("hhsr_merge_burst", *_merge_burst(c, scale, sensor, kflags, flags, name))
        return c.done()

    for lay in lays:
        got = both(run, lay, "merge_burst " + case)
        _judge_merge(got, scale, sensor, flags, f"merge_burst {case} [{lay}]")


@pytest.mark.parametrize("lay", ["even2", "lead1"])
def test_merge_burst_row_slab_of_a_sub_image(lay):
    """A row slab (row0 > 0) of a sub-image (lr_row_offset > 0), x2: the frames are rows [32, H) of the pitched frames —
    the window-of-a-larger-buffer use of a pitch — with the matching rows of the flows, covariances and robustness maps;
    the output rows that lie at least 16 raw rows below the cut (32 output rows: window radius plus the largest flow)
    against the same rows of the oracle's full image at TOL."""
    scale, sensor = 2, "rggb"
    H, W, ts, ny, nx, sH, sW = _dims(scale)
    off = 32
    Hs, row0 = H - off, 32
    nys, nrows = cdiv(Hs, ts), 2 * Hs - row0
    ref, ref_covs, frames = V._merge_inputs(scale, sensor)
    cfa = _lib.cfa_bytes(V.SENSORS[sensor])

    def run(name):
        c = Call("hhsr_merge_burst row slab")
        raws, _, _, _, tref, _, p = _frames(c, scale, sensor, name)
        flows = [c.const(f[1][off // ts:]) for f in frames]
        covs = [c.const(f[2][off // 2:]) for f in frames]
        rs = [c.const(f[3][off:]) for f in frames]
        trc = c.const(ref_covs[off // 2:])
        num = c.out("num", (nrows, sW, 3))
        _lib.call("hhsr_merge_burst", _lib.ptr_array([r[off:] for r in raws]), _lib.ptr_array(flows), _lib.ptr_array(covs),
                  _lib.ptr_array(rs), 4, Hs, W, p, nys, nx, ts, _lib.ptr(tref[off:]), _lib.ptr(trc), cfa, float(scale), 0,
                  DO_REF | DIVIDE, _lib.ptr(num), None, None, 2 * Hs, sW, row0, nrows, off, _lib.stream())
        return c.done()

    got = both(run, lay, "merge_burst row slab")
    want = V._oracle_merge(scale, sensor, "steerable")["out"][2 * off + row0:]
    close(got["num"], want, *TOL, f"merge_burst row slab [{lay}]")


@pytest.mark.parametrize("lay", ["even2", "odd", "lead1"])
def test_merge_burst_chain(lay):
    """hhsr_merge_burst_chain in three links (store frames 0-1; load, add frame 2, store; load, add frame 3 and the
    reference frame, normalise) on pitched frames: equal bit for bit to the single pitched launch and to the compact
    chain, and to the oracle at TOL."""
    scale, sensor = 2, "rggb"
    H, W, ts, ny, nx, sH, sW = _dims(scale)
    cfa = _lib.cfa_bytes(V.SENSORS[sensor])
    nfl = _lib.load().hhsr_merge_chain_bytes(H, W) // 4

    def run(name):
        c = Call("hhsr_merge_burst_chain")
        raws, flows, covs, rs, tref, trc, p = _frames(c, scale, sensor, name)
        num, acc = c.out("num", (sH, sW, 3)), c.out("acc_r", (H, W), fill=0.0)
        cls = c.out("class_acc", (nfl,))
        for n_frames, n_done, flags, last in ((2, 0, STORE_CLASSES, False), (3, 2, LOAD_CLASSES | STORE_CLASSES, False),
                                              (4, 3, LOAD_CLASSES | DO_REF | DIVIDE, True)):
            _lib.call("hhsr_merge_burst_chain", _lib.ptr_array(raws[:n_frames]), _lib.ptr_array(flows[:n_frames]),
                      _lib.ptr_array(covs[:n_frames]), _lib.ptr_array(rs[:n_frames]), n_frames, H, W, p, ny, nx, ts,
                      _lib.ptr(tref if last else None), _lib.ptr(trc if last else None), cfa, float(scale), 0, flags,
                      _lib.ptr(num), None, _lib.ptr(acc if last else None), sH, sW, _lib.ptr(cls), n_done, _lib.stream())
        res = c.done()
        del res["class_acc"]  # (tiles the storing links skip keep the sentinel: not an output of the chain)
        c = Call("hhsr_merge_burst (single launch)")
        _lib.call("hhsr_merge_burst", *_merge_burst(c, scale, sensor, 0, DO_REF | DIVIDE, name, tag="single_"))
        res.update(c.done())
        return res

    got = both(run, lay, "merge_burst_chain")
    same_bits(got["num"], got["single_num"], f"chain vs single launch [{lay}] image")
    same_bits(got["acc_r"], got["single_acc_r"], f"chain vs single launch [{lay}] accumulated robustness")
    _judge_merge(got, scale, sensor, DO_REF | DIVIDE, f"merge_burst_chain [{lay}]")


# ------------------------------------------------------------------------------------------ front end
@pytest.mark.parametrize("W,extra", [(96, 8), (96, 2), (70, 8), (70, 2)],
                         ids=["W96_vector", "W96_scalar_full_rows", "W70_pitch8", "W70_pitch2"])
def test_normalize_raw_u16(W, extra):
    """hhsr_normalize_raw_u16, 3 frames [n][H][pitch], non-trivial black levels and white balance; raw and out 16-byte
    aligned as the header demands.  W % 8 == 0 with pitch W + 8 keeps the 16-byte vector path; with pitch W + 2 the kernel
    takes its scalar path over FULL rows — the one kernel choice made by the pitch, which no compact call reaches — and the
    header promises the NumPy expression bit for bit either way.  W % 8 != 0 takes the scalar path with both."""
    n, H = 3, 50
    rng = np.random.default_rng(9)
    raw = rng.integers(0, 16384, (n, H, W), dtype=np.uint16)
    cfa, bl, wl, wb = [[2, 1], [1, 0]], [63, 64, 66], 16383, [1.91, 1.0, 1.57]

    def run(pitch):
        c = Call("hhsr_normalize_raw_u16")
        view, whole, _ = pitched(raw.reshape(n * H, W), pitch)  # frames follow each other at H * pitch
        c.ins.append((whole, whole.clone()))
        assert view.data_ptr() % 16 == 0
        out = c.out("out", (n, H, W))
        _lib.call("hhsr_normalize_raw_u16", _lib.ptr(view), n, H, W, pitch, _lib.cfa_bytes(cfa), _lib.doubles(bl), float(wl),
                  _lib.doubles(wb), _lib.ptr(out), _lib.stream())
        return c.done()

    compact, got = run(W), run(W + extra)
    same_bits(got["out"], compact["out"], "normalize_raw_u16 pitched vs compact")
    want = oracle.frontend.normalize_burst(raw, bl, wl, wb + [1.0], cfa)
    no_new_nan(got["out"], want, "normalize_raw_u16")
    assert got["out"].dtype == np.float32 and np.array_equal(got["out"], want)  # test_normalize_raw_bit_exact


# ------------------------------------------------------------------------------------------ guards without a pitch
_ROB = {}


def _rob_inputs(H, W, ts, seed):
    """The case of test_variant_parity.py::_rob_case as arrays: everything hhsr_rob_frame(s) reads, and the oracle's maps."""
    key = (H, W, ts, seed)
    if key not in _ROB:
        cfg, cfa, wb, comp, flows, want, rm, rv, curves = V._rob_case(H, W, ts, seed)
        sig = robustness.noise_sigma_sq(rm, rv, curves[0])  # (sigma^2, packed curve indices)
        assert sig[1] is not None
        cms = [robustness.compute_local_stats_from_raw(T(c), cfa, wb, want_vars=False)[0] for c in comp]
        _ROB[key] = (cfg, comp, flows, want, rm, rv, curves, sig, cms)
    return _ROB[key]


def _plane_ops():
    """name -> (run(guard) -> {name: array}): the entry points without a pitch that write whole planes from grids with
    remainder tiles, on the shapes of their existing tests; guard=False: plain torch outputs (the unguarded call)."""
    ops = {}

    def alloc(c, guard):
        def out(name, shape, dtype=torch.float32, fill=None):
            if guard:
                return c.out(name, shape, dtype=dtype, fill=fill)
            t = torch.empty(shape, dtype=dtype, device=DEV)
            t.view(torch.int32).fill_(SENT)
            if fill is not None:
                t.copy_(torch.as_tensor(fill, dtype=dtype, device=DEV))
            c.outs[name] = t
            return t
        return out

    def op(fn):
        def run(guard):
            nonlocal rng
            rng = np.random.default_rng(77)  # (the same inputs in the guarded and the unguarded run)
            c = Call(fn.__name__)
            fn(c, alloc(c, guard))
            return c.done()
        ops[fn.__name__] = run
        return fn

    rng = np.random.default_rng(77)
    std, dif = synth.noise_curves(synth.ALPHA_ISO100, synth.BETA_ISO100)

    @op
    def hhsr_rob_upscale(c, out):  # 69 x 101 guide planes -> 138 x 202 (test_ref_planes_equal_separate_kernels), warped
        lh, lw, ts = 69, 101, 16
        stats = c.const(rng.random((3, lh, lw), dtype=np.float32))
        ny, nx = cdiv(2 * lh, ts), cdiv(2 * lw, ts)
        flow = c.const(rng.uniform(-2, 2, (ny, nx, 2)).astype(np.float32))
        _lib.call("hhsr_rob_upscale", _lib.ptr(stats), lh, lw, None, 0, 0, ts, _lib.ptr(out("ref", (3, 2 * lh, 2 * lw))),
                  _lib.stream())
        _lib.call("hhsr_rob_upscale", _lib.ptr(stats), lh, lw, _lib.ptr(flow), ny, nx, ts,
                  _lib.ptr(out("warped", (3, 2 * lh, 2 * lw))), _lib.stream())

    @op
    def hhsr_ref_planes(c, out):
        lh, lw = 69, 101
        gm, gv = c.const(rng.random((3, lh, lw), dtype=np.float32)), c.const(1e-3 * rng.random((3, lh, lw), dtype=np.float32))
        curve = c.const(std, torch.float64)
        _lib.call("hhsr_ref_planes", _lib.ptr(gm), _lib.ptr(gv), lh, lw, _lib.ptr(curve), len(std),
                  _lib.ptr(out("ref_means", (3, 2 * lh, 2 * lw))), _lib.ptr(out("sigma_sq", (2 * lh, 2 * lw))),
                  _lib.ptr(out("curve_index", (2 * lh, 2 * lw), torch.int32)), _lib.stream())

    @op
    def hhsr_local_min5(c, out):
        H, W = 139, 203
        R = c.const(rng.random((H, W), dtype=np.float32))
        _lib.call("hhsr_local_min5", _lib.ptr(R), H, W, _lib.ptr(out("r", (H, W))), None, _lib.stream())
        _lib.call("hhsr_local_min5", _lib.ptr(R), H, W, _lib.ptr(out("r2", (H, W))),
                  _lib.ptr(out("acc_r", (H, W), fill=0.25)), _lib.stream())

    @op
    def hhsr_rob_sum(c, out):
        H, W, n = 139, 203, 5
        rs = [c.const(rng.random((H, W), dtype=np.float32)) for _ in range(n)]
        for tag, flags in (("plain", 0), ("min5", 2)):
            s64 = out("sum64_" + tag, (H, W), torch.float64)
            _lib.call("hhsr_rob_sum", _lib.ptr_array(rs[:3]), 3, H, W, flags, 2.5, _lib.ptr(s64), None, None, _lib.stream())
            _lib.call("hhsr_rob_sum", _lib.ptr_array(rs[3:]), 2, H, W, flags | 1, 2.5, _lib.ptr(s64),
                      _lib.ptr(out("mask32_" + tag, (H, W))), _lib.ptr(out("decisions32_" + tag, (H, W))), _lib.stream())

    @op
    def hhsr_flow_upscale_nearest(c, out):
        src = c.const(rng.uniform(-2, 2, (11, 18, 2)).astype(np.float32))
        _lib.call("hhsr_flow_upscale_nearest", _lib.ptr(src), 11, 18, _lib.ptr(out("dst", (23, 37, 2))), 23, 37, 2, 2.0,
                  _lib.stream())

    @op
    def hhsr_frame_count_denoise(c, out):
        H, W, scale = 138, 202, 2
        img = c.const(rng.random((H, W, 3), dtype=np.float32))
        acc = c.const(rng.uniform(0, 9, (H // scale, W // scale)).astype(np.float32))
        for kind, strength in ((0, 3.0), (1, 1.5)):
            _lib.call("hhsr_frame_count_denoise", _lib.ptr(img), _lib.ptr(out(f"kind{kind}", (H, W, 3))), H, W, _lib.ptr(acc),
                      H // scale, W // scale, float(scale), kind, strength, 8.0, 1, _lib.stream())

    @op
    def hhsr_postprocess(c, out):
        H, W, radius = 70, 101, 4
        img = c.const(rng.random((H, W, 3), dtype=np.float32))
        x = np.arange(-radius, radius + 1)
        taps = np.exp(-0.5 * (x / 1.5) ** 2)
        ttaps = c.const(taps / taps.sum(), torch.float64)
        ccm = _lib.floats([1.6, -0.4, -0.2, -0.3, 1.5, -0.2, 0.0, -0.5, 1.5])
        for ori in (1, 6, 8):
            shp = (W, H, 3) if ori >= 5 else (H, W, 3)
            _lib.call("hhsr_postprocess", _lib.ptr(img), _lib.ptr(out(f"tmp{ori}", (H, W, 3))), _lib.ptr(out(f"out{ori}", shp)),
                      H, W, ccm, 1, 1.5, _lib.ptr(ttaps), radius, 1, 1, ori, _lib.stream())

    @op
    def hhsr_orient_plane(c, out):
        H, W = 69, 101
        a = c.const(rng.random((H, W), dtype=np.float32))
        for ori in (1, 3, 6, 8):
            _lib.call("hhsr_orient_plane", _lib.ptr(a), _lib.ptr(out(f"out{ori}", (W, H) if ori >= 5 else (H, W))), H, W, ori,
                      _lib.stream())

    def rob(name, H, W, ts, grouped):
        def fn(c, out):
            cfg, comp, flows, want, rm, rv, curves, (sig2, idx), cms = _rob_inputs(H, W, ts, 40 + ts)
            tf = [c.const(f) for f in flows]
            ny, nx = flows[0].shape[:2]
            t = cfg.robustness.tuning
            S = [robustness.compute_s(f, t.Mt, t.s1, t.s2) for f in tf]
            Rs = [out(f"R{k}", (H, W)) for k in range(len(comp))]
            if grouped:
                _lib.call("hhsr_rob_frames", _lib.ptr_array(cms), len(cms), H // 2, W // 2, _lib.ptr(rm), _lib.ptr(sig2),
                          _lib.ptr(idx), _lib.ptr_array(tf), ny, nx, ts, _lib.ptr_array(S), float(t.Mt), float(t.s1),
                          float(t.s2), _lib.ptr(curves[1]), len(dif), float(t.t), _lib.ptr_array(Rs), 0, 0, _lib.stream())
            else:
                for k in range(len(cms)):
                    _lib.call("hhsr_rob_frame", _lib.ptr(cms[k]), H // 2, W // 2, _lib.ptr(rm), _lib.ptr(sig2), _lib.ptr(idx),
                              _lib.ptr(tf[k]), ny, nx, ts, _lib.ptr(S[k]), _lib.ptr(curves[1]), len(dif), float(t.t),
                              _lib.ptr(Rs[k]), _lib.stream())
        fn.__name__ = name
        op(fn)

    rob("hhsr_rob_frames row4", 200, 328, 16, True)
    rob("hhsr_rob_frame row4", 200, 328, 16, False)
    rob("hhsr_rob_frame row4 W%4=2", 200, 330, 32, False)
    rob("hhsr_rob_frame k_rob_frame", 200, 330, 8, False)
    return ops


PLANE_OPS = ["hhsr_rob_upscale", "hhsr_ref_planes", "hhsr_local_min5", "hhsr_rob_sum", "hhsr_flow_upscale_nearest",
             "hhsr_frame_count_denoise", "hhsr_postprocess", "hhsr_orient_plane", "hhsr_rob_frames row4",
             "hhsr_rob_frame row4", "hhsr_rob_frame row4 W%4=2", "hhsr_rob_frame k_rob_frame"]
_OPS = {}


@pytest.mark.parametrize("name", PLANE_OPS)
def test_outputs_without_a_pitch_stay_inside_their_planes(name):
    """The guard half (4 and 5) for the entry points without a pitch that write whole planes from grids with remainder
    tiles: inputs unchanged, guard bands intact, and the guarded result equal bit for bit to the unguarded call (what
    these results are is asserted by the tests of their stages)."""
    if not _OPS:
        _OPS.update(_plane_ops())
    assert sorted(_OPS) == sorted(PLANE_OPS)
    plain, got = _OPS[name](False), _OPS[name](True)
    assert plain.keys() == got.keys() and len(got) > 0
    for k in got:
        same_bits(got[k], plain[k], f"{name} {k}: guarded vs unguarded")


# ------------------------------------------------------------------------------------------ kernels chosen by alignment
@pytest.mark.parametrize("scale,flags", [(2, DO_REF | DIVIDE), (2, DO_REF | STORE_DEN), (3, DO_REF | DIVIDE),
                                         (3, DO_REF | STORE_DEN)])
def test_merge_burst_output_off_the_16_byte_grid(scale, flags):
    """num (and den with STORE_DEN) 4 bytes off the 16-byte grid, inputs compact: hhsr_merge_burst takes the first-generation
    x2 kernel / the 16 x 16 tile kernel at x3 instead of the wave-per-class kernels; against the oracle as above, guards
    intact."""
    def run(lead):
        c = Call("hhsr_merge_burst misaligned output")
        args = _merge_burst(c, scale, "rggb", 0, flags, "compact", num_lead=lead)
        assert (c.outs["num"].data_ptr() % 16 == 4) == bool(lead)
        _lib.call("hhsr_merge_burst", *args)
        return c.done()

    got = run(1)
    _judge_merge(got, scale, "rggb", flags, f"x{scale} misaligned output flags={flags}")
    run(0)  # (the aligned launch under the same guards)


def test_misaligned_outputs_refused_where_no_other_kernel_applies():
    """HHSR_MERGE_LOCAL_MIN at x3 and hhsr_merge_burst_chain need the wave-per-class kernels: on an output off the 16-byte
    grid they return -3 with their documented text instead of launching.  hhsr_rob_frames with S = NULL is refused where
    k_rob_frame is the only kernel (no packed curve index); on a misaligned R it runs (the dword k_rob_frames_row4 evaluates
    the weights itself) and gives the bits of the aligned call with the maps of hhsr_rob_s."""
    lib = _lib.load()
    c = Call("x3 local min, misaligned")
    rc = lib.hhsr_merge_burst(*_merge_burst(c, 3, "rggb", 0, DO_REF | DIVIDE | LOCAL_MIN, "compact", num_lead=1))
    assert rc == -3 and b"HHSR_MERGE_LOCAL_MIN needs the x2 or the x3 kernel" in lib.hhsr_last_error(), lib.hhsr_last_error()
    c.done()
    H, W, ts, ny, nx, sH, sW = _dims(2)
    c = Call("chain, misaligned")
    raws, flows, covs, rs, tref, trc, p = _frames(c, 2, "rggb", "compact")
    num = c.out("num", (sH, sW, 3), lead=1)
    cls = c.out("class_acc", (lib.hhsr_merge_chain_bytes(H, W) // 4,))
    rc = lib.hhsr_merge_burst_chain(_lib.ptr_array(raws), _lib.ptr_array(flows), _lib.ptr_array(covs), _lib.ptr_array(rs), 4,
                                    H, W, p, ny, nx, ts, None, None, _lib.cfa_bytes(V.SENSORS["rggb"]), 2.0, 0, STORE_CLASSES,
                                    _lib.ptr(num), None, None, sH, sW, _lib.ptr(cls), 0, _lib.stream())
    assert rc == -3 and b"needs the wave-per-class x2 kernel" in lib.hhsr_last_error(), lib.hhsr_last_error()
    c.done()
    _, rc, err, _ = _rob_frames_call(Call("rob_frames S = NULL, no curve index"), grouped=True, lead=0, index=False, s_null=True)
    assert rc == -3 and b"S = NULL" in err and b"needs the grouped kernel" in err, (rc, err)
    got, rc, err, _ = _rob_frames_call(Call("rob_frames S = NULL, misaligned R"), grouped=True, lead=1, s_null=True)
    assert rc == 0, (rc, err)
    aligned, rc, err, want = _rob_frames_call(Call("rob_frames S given, aligned R"), grouped=True, lead=0)
    assert rc == 0 and aligned.keys() == got.keys() and len(got) == len(want), (rc, err)
    for k in got:
        same_bits(got[k], aligned[k], f"hhsr_rob_frames {k}: S = NULL on a misaligned R vs S given on an aligned R")


def _rob_frames_call(c, grouped, lead, index=True, s_null=False):
    """hhsr_rob_frames (grouped) / hhsr_rob_frame on the shape of the 16-byte k_rob_frames_row4 (ts % 16 == 0, W % 4 == 0)
    with R `lead` elements off the 16-byte grid, with or without the packed curve index and the maps S: (results, return
    code, message, the oracle's maps)."""
    H, W, ts = 200, 328, 16
    lib = _lib.load()
    cfg, comp, flows, want, rm, rv, curves, (sig2, idx), cms = _rob_inputs(H, W, ts, 40 + ts)
    tf = [c.const(f) for f in flows]
    ny, nx = flows[0].shape[:2]
    t = cfg.robustness.tuning
    S = [robustness.compute_s(f, t.Mt, t.s1, t.s2) for f in tf]
    Rs = [c.out(f"R{k}", (H, W), lead=lead) for k in range(len(comp))]
    pidx = _lib.ptr(idx if index else None)
    if grouped:
        rc = lib.hhsr_rob_frames(_lib.ptr_array(cms), len(cms), H // 2, W // 2, _lib.ptr(rm), _lib.ptr(sig2), pidx,
                                 _lib.ptr_array(tf), ny, nx, ts, None if s_null else _lib.ptr_array(S), float(t.Mt),
                                 float(t.s1), float(t.s2), _lib.ptr(curves[1]), curves[1].numel(), float(t.t),
                                 _lib.ptr_array(Rs), 0, 0, _lib.stream())
    else:
        rc = 0
        for k in range(len(cms)):
            rc = rc or lib.hhsr_rob_frame(_lib.ptr(cms[k]), H // 2, W // 2, _lib.ptr(rm), _lib.ptr(sig2), pidx, _lib.ptr(tf[k]),
                                          ny, nx, ts, _lib.ptr(S[k]), _lib.ptr(curves[1]), curves[1].numel(), float(t.t),
                                          _lib.ptr(Rs[k]), _lib.stream())
    err = lib.hhsr_last_error()
    return c.done(), rc, err, want


@pytest.mark.parametrize("grouped", [False, True], ids=["hhsr_rob_frame", "hhsr_rob_frames"])
@pytest.mark.parametrize("route", ["k_rob_frames_row4_dword", "k_rob_frame"])
def test_rob_frame_kernels_chosen_by_pointer(route, grouped):
    """On the shape of the 16-byte k_rob_frames_row4: with R off the 16-byte grid its dword instantiation runs, without a
    packed curve index k_rob_frame; hhsr_rob_frame and hhsr_rob_frames (S given), against oracle.compute_robustness at the
    1e-4 of test_variant_parity.py::test_robustness_kernels_vs_oracle, guards intact.  R does not depend on the alignment:
    the misaligned call gives the bits of the same call on an aligned R."""
    lead, index = (1, True) if route == "k_rob_frames_row4_dword" else (0, False)
    got, rc, err, want = _rob_frames_call(Call(route), grouped, lead, index)
    assert rc == 0, (rc, err)
    if lead:
        aligned, rc, err, _ = _rob_frames_call(Call(route + ", aligned R"), grouped, 0, index)
        assert rc == 0 and aligned.keys() == got.keys() and len(got) == len(want), (rc, err)
        for k in got:
            same_bits(got[k], aligned[k], f"{route} {k}: R one element off the 16-byte grid vs aligned")
    for k, w in enumerate(want):  # (the oracle's map is r = the 5 x 5 minimum of the thresholded map R the kernels write)
        close(oracle.robustness.local_min(got[f"R{k}"]), w, 0, 1e-4,
              f"{route} ({'hhsr_rob_frames' if grouped else 'hhsr_rob_frame'}) frame {k}")
