"""k_align_wave walks the frames of a launch inside one wave per tile: what depends on the reference tile alone (the staged
tile + halo, the Hessian, the geometry, for r = 1 the lane's reference values and gradients in registers) is set up once and
serves every frame.  Nothing may leak from frame to frame: one hhsr_align_level_batch call of n frames gives every frame
the BITS of n hhsr_align_level calls of one frame each (a single frame runs the loop once).

The launcher lets a wave walk the frames only for launches of LOOP_TILES tiles and more and for r < 4 (below that, and for
r = 4, one wave per (tile, frame)), so every case that matters runs on the small grid of 3 x 5 tiles (one workgroup with a
dead wave) AND on 128 x 192 = LOOP_TILES tiles; 25 x 983 tiles is one tile below the threshold.  The levels of the large grids
(up to 4096 x 6144 pixels for 32-pixel tiles) are generated on the GPU."""
import functools

import numpy as np
import pytest
import torch

import oracle
from helpers import assert_close, base_config, flipped_tiles, smooth

pytestmark = pytest.mark.gpu

from handheld_super_resolution import ICA, _lib, alignment  # noqa: E402

DEV = "cuda"
LOOP_TILES = 24576  # HHSR_ALIGN_LOOP_MIN_TILES of csrc/hhsr_align.hip
SMALL, BIG, BELOW = (3, 5), (128, 192), (25, 983)
assert BIG[0] * BIG[1] == LOOP_TILES and BELOW[0] * BELOW[1] == LOOP_TILES - 1
ICA_M = 2  # margin of the staged window around the block-matching candidates (csrc/hhsr_align.hip)
METRIC_CODE = {"L2": 0, "L1": 1, "L1_ref_effective": 2}
N_ITER = 3


def T(a):
    return torch.as_tensor(np.ascontiguousarray(a), dtype=torch.float32, device=DEV)


def same_bits(a, b):
    return a.shape == b.shape and torch.equal(a.view(torch.int32), b.view(torch.int32))


def _level_np(ts, grid, n, seed=0, flat_tile=False):
    """(reference level [ny ts, nx ts], n moving levels 3 rows / 5 columns smaller: shifted, noisy copies, n incoming flow
    fields).  flat_tile: tile (1, 1) of the reference and its halo have one intensity."""
    ny, nx = grid
    rng = np.random.default_rng(1000 * ts + 10 * ny + nx + seed)
    h, w = ny * ts, nx * ts
    big = smooth(rng, h + 32, w + 32, 1.5)
    ref = big[16:16 + h, 16:16 + w].copy()
    if flat_tile:
        ref[ts - 1:2 * ts + 1, ts - 1:2 * ts + 1] = 0.5
    movs, flows = [], []
    for _ in range(n):
        sy, sx = (int(v) for v in rng.integers(-3, 4, 2))
        mov = big[16 + sy:16 + sy + h - 3, 16 + sx:16 + sx + w - 5].copy()
        mov += 0.01 * rng.standard_normal(mov.shape).astype(np.float32)
        movs.append(mov)
        flows.append(rng.uniform(-1.6, 1.6, (ny, nx, 2)).astype(np.float32))
    return ref, movs, flows


def _level_gpu(ts, grid, n, seed=0, flat_tile=False):
    """_level_np() for the large grids: the same construction from torch's generator on the GPU."""
    ny, nx = grid
    g = torch.Generator(device=DEV)
    g.manual_seed(1000 * ts + 10 * ny + nx + seed)
    rng = np.random.default_rng(1000 * ts + 10 * ny + nx + seed)
    h, w = ny * ts, nx * ts
    pool = torch.nn.functional.avg_pool2d
    big = pool(pool(torch.rand((1, 1, h + 40, w + 40), generator=g, device=DEV), 5, 1), 5, 1)[0, 0]
    big = (big - big.min()) / (big.max() - big.min())
    ref = big[16:16 + h, 16:16 + w].clone()
    if flat_tile:
        ref[ts - 1:2 * ts + 1, ts - 1:2 * ts + 1] = 0.5
    movs, flows = [], []
    for _ in range(n):
        sy, sx = (int(v) for v in rng.integers(-3, 4, 2))
        mov = big[16 + sy:16 + sy + h - 3, 16 + sx:16 + sx + w - 5]
        movs.append((mov + 0.01 * torch.randn(mov.shape, generator=g, device=DEV)).contiguous())
        flows.append(torch.rand((ny, nx, 2), generator=g, device=DEV) * 3.2 - 1.6)
    return ref, movs, flows


@functools.lru_cache(maxsize=None)
def _level(ts, grid, n, seed=0, flat_tile=False):
    """(reference level, its Hessians, n moving levels, n incoming flow fields) on the GPU."""
    if grid[0] * grid[1] * ts * ts <= 1 << 16:
        ref, movs, flows = _level_np(ts, grid, n, seed, flat_tile)
        tref, movs, flows = T(ref), [T(m) for m in movs], [T(f) for f in flows]
    else:
        tref, movs, flows = _level_gpu(ts, grid, n, seed, flat_tile)
    return tref, ICA.init_ica(tref, ts)[2], movs, flows


def _coarse(grid, rep, n, seed=0):
    """n coarse flow fields on a grid that does NOT reach every tile (ty / rep, tx / rep): zero past it."""
    ny, nx = grid
    cny, cnx = max(1, (ny - 1) // rep), max(1, (nx - 1) // rep)
    assert (ny - 1) // rep >= cny or (nx - 1) // rep >= cnx
    rng = np.random.default_rng(77 + rep + seed)
    return [T(rng.uniform(-1.2, 1.2, (cny, cnx, 2)).astype(np.float32) / rep) for _ in range(n)]


def _args(tref, hess, mov0, grid, ts, r, metric, n_iter):
    rh, rw = tref.shape
    mh, mw = mov0.shape
    return (rh, rw, rw), (mh, mw, mw), (grid[0], grid[1], ts, r, METRIC_CODE[metric], int(n_iter))


def _source(mode, coarse, k=None):
    """(coarse pointer(s), cny, cnx, rep, mult) of `mode`: "flow" (in place), "zero" or ("coarse", rep)."""
    if mode == "flow":
        return None, 0, 0, 0, 1.0
    if mode == "zero":
        return None, 0, 0, -1, 1.0
    rep = mode[1]
    cny, cnx = coarse[0].shape[:2]
    return (_lib.ptr_array(coarse) if k is None else _lib.ptr(coarse[k])), cny, cnx, rep, float(rep)


def _outputs(flows, mode):
    """The flow arrays of a launch: copies of the incoming flows (in place), else NaN (every tile must be written)."""
    return [f.clone() if mode == "flow" else torch.full_like(f, float("nan")) for f in flows]


def batch(tref, hess, movs, flows, grid, ts, r, metric, mode="flow", coarse=None, n_iter=N_ITER):
    """ONE hhsr_align_level_batch call over the frames."""
    a, m, g = _args(tref, hess, movs[0], grid, ts, r, metric, n_iter)
    out = _outputs(flows, mode)
    cptr, cny, cnx, rep, mult = _source(mode, coarse)
    _lib.call("hhsr_align_level_batch", _lib.ptr(tref), *a, _lib.ptr(hess), _lib.ptr_array(movs), len(movs), *m,
              _lib.ptr_array(out), *g, cptr, cny, cnx, rep, mult, _lib.stream())
    return out


def single(tref, hess, movs, flows, grid, ts, r, metric, mode="flow", coarse=None, n_iter=N_ITER):
    """len(movs) hhsr_align_level calls, one frame each."""
    a, m, g = _args(tref, hess, movs[0], grid, ts, r, metric, n_iter)
    out = _outputs(flows, mode)
    for k, mov in enumerate(movs):
        cptr, cny, cnx, rep, mult = _source(mode, coarse, k)
        _lib.call("hhsr_align_level", _lib.ptr(tref), *a, _lib.ptr(hess), _lib.ptr(mov), *m, _lib.ptr(out[k]), *g, cptr,
                  cny, cnx, rep, mult, _lib.stream())
    return out


def check(got, want, what):
    assert len(got) == len(want)
    for k, (g, w) in enumerate(zip(got, want)):
        assert not torch.isnan(w).any(), f"{what}: frame {k} has tiles the single-frame launch did not write"
        assert same_bits(g, w), f"{what}: frame {k} of {len(got)} differs from its single-frame launch " \
                                f"({int((g != w).any(-1).sum())} tiles)"


# ------------------------------------------------------------------------------------------ frame counts and tiles
_SINGLE9 = {}


def _single9(grid):
    """The 9 frames of the frame-count sweep launched one by one (computed once per grid)."""
    if grid not in _SINGLE9:
        tref, hess, movs, flows = _level(16, grid, 9)
        _SINGLE9[grid] = single(tref, hess, movs, flows, grid, 16, 1, "L1")
    return _SINGLE9[grid]


@pytest.mark.parametrize("grid", [SMALL, BIG], ids=["3x5", "128x192"])
@pytest.mark.parametrize("n", [1, 2, 3, 4, 5, 8, 9])
def test_frame_counts(n, grid):
    """n frames in one call (9 > HHSR_MAX_BATCH: two launches from the host loop) against n single-frame calls."""
    tref, hess, movs, flows = _level(16, grid, 9)
    got = batch(tref, hess, movs[:n], flows[:n], grid, 16, 1, "L1")
    check(got, _single9(grid)[:n], f"{n} frames, {grid[0]} x {grid[1]} tiles")


def test_single_tile():
    """A 16 x 16 level: one tile, three dead waves in the only workgroup."""
    grid = (1, 1)
    tref, hess, movs, flows = _level(16, grid, 4)
    for mode in ("flow", "zero"):
        check(batch(tref, hess, movs, flows, grid, 16, 1, "L1", mode), single(tref, hess, movs, flows, grid, 16, 1, "L1", mode),
              f"single tile, {mode}")


# ------------------------------------------------------------------------------------------ instantiations
CASES = [  # (ts, r, metric, incoming flow, grid)
    (16, 1, "L1", "zero", SMALL), (16, 1, "L1", "flow", SMALL),
    (16, 4, "L2", ("coarse", 2), SMALL), (16, 4, "L2", ("coarse", 4), SMALL),
    (8, 4, "L2", ("coarse", 2), SMALL), (8, 4, "L2", ("coarse", 4), SMALL),
    (32, 2, "L2", "flow", SMALL), (16, 1, "L1_ref_effective", "flow", SMALL),
    # the same on a grid whose waves walk the frames (r = 4: one wave per (tile, frame) at every size), and the other
    # instantiations with a frame loop
    (16, 1, "L1", "zero", BIG), (16, 1, "L1", "flow", BIG), (16, 1, "L1", "flow", BELOW),
    (16, 4, "L2", ("coarse", 2), BIG), (8, 4, "L2", ("coarse", 4), BIG),
    (32, 2, "L2", "flow", BIG), (16, 1, "L1_ref_effective", "flow", BIG),
    (16, 1, "L2", ("coarse", 2), BIG), (16, 2, "L2", ("coarse", 2), BIG), (16, 2, "L1", "flow", BIG),
    (8, 1, "L2", "flow", BIG), (8, 2, "L2", ("coarse", 4), BIG), (32, 1, "L1", "zero", BIG), (32, 2, "L1", ("coarse", 2), BIG),
]


@pytest.mark.parametrize("ts,r,metric,mode,grid", CASES,
                         ids=[f"ts{c[0]}-r{c[1]}-{c[2]}-{c[3] if isinstance(c[3], str) else 'coarse%d' % c[3][1]}-"
                              f"{c[4][0]}x{c[4][1]}" for c in CASES])
def test_instantiations(ts, r, metric, mode, grid):
    """A chunk of 4 frames (and of 3) through the instantiation, with each source of the incoming flow."""
    tref, hess, movs, flows = _level(ts, grid, 4)
    coarse = _coarse(grid, mode[1], 4) if isinstance(mode, tuple) else None
    want = single(tref, hess, movs, flows, grid, ts, r, metric, mode, coarse)
    what = f"ts={ts} r={r} {metric} {mode} {grid}"
    check(batch(tref, hess, movs, flows, grid, ts, r, metric, mode, coarse), want, what)
    check(batch(tref, hess, movs[:3], flows[:3], grid, ts, r, metric, mode, coarse and coarse[:3]), want[:3], what + " (3)")
    if isinstance(mode, tuple):  # zero past the coarse grid: the last tile column (or row) starts from no flow at all
        zero = single(tref, hess, movs[:1], flows[:1], grid, ts, r, metric, "zero")[0]
        ny, nx = grid
        cny, cnx = coarse[0].shape[:2]
        past = torch.zeros(grid, dtype=torch.bool, device=DEV)
        past[cny * mode[1]:] = True
        past[:, cnx * mode[1]:] = True
        assert past.any() and same_bits(want[0][past], zero[past])


# ------------------------------------------------------------------------------------------ frames that differ in a launch
FRAME2_GAIN = 16.0  # (4 and 8 leave every tile of the 3 x 5 grid of <16, 4> inside its window)


def _different_frames(ts, grid):
    """4 frames of one launch that take different paths through the kernel, on a reference with a flat tile:
      0  zero incoming flow
      1  the incoming flow pushes the windows of the border tiles out of the moving level (both staging arms; the ICA taps
         of those tiles come from global memory: clamped coordinates for ts = 8, zero outside the level otherwise)
      2  a moving level of FRAME2_GAIN times the intensity: the first ICA update throws trunc(flow) out of the staged window
      3  an ordinary frame"""
    tref, hess, movs, flows = _level(ts, grid, 4, seed=5, flat_tile=True)
    movs, flows = list(movs), [f.clone() for f in flows]
    flows[0].zero_()
    out = float(ts + 20)
    flows[1][0, :, 1] = -out
    flows[1][-1, :, 1] = out
    flows[1][:, 0, 0] = -out
    flows[1][:, -1, 0] = out
    movs[2] = movs[2] * FRAME2_GAIN
    return tref, hess, movs, flows


@pytest.mark.parametrize("grid", [SMALL, BIG], ids=["3x5", "128x192"])
@pytest.mark.parametrize("ts,r,metric", [(16, 1, "L1"), (8, 1, "L2"), (16, 4, "L2"), (8, 4, "L2"), (32, 2, "L2")])
def test_frames_that_differ(ts, r, metric, grid):
    tref, hess, movs, flows = _different_frames(ts, grid)
    h = hess.reshape(grid[0], grid[1], 4)[1, 1]
    assert abs(float(h[0] * h[3] - h[1] * h[2])) < 1e-10, "the flat tile is solvable"
    want = single(tref, hess, movs, flows, grid, ts, r, metric)
    # frame 2: after ONE iteration trunc(flow) of some tile is further than r + ICA_M from the window centre round(flow in)
    one = single(tref, hess, movs[2:3], flows[2:3], grid, ts, r, metric, n_iter=1)[0]
    assert bool(((torch.trunc(one) - torch.round(flows[2])).abs() > r + ICA_M).any()), "no ICA step left the staged window"
    # the flat tile keeps its block-matching result: the incoming flow plus an integer shift (L1: the rounded flow)
    for k in range(4):
        d = want[k][1, 1] - (torch.round(flows[k][1, 1]) if metric == "L1" else flows[k][1, 1])
        # (L2 adds the shift to the un-rounded flow: one rounding of a value below 8)
        assert bool(((d - torch.round(d)).abs() <= 1e-6).all() and (torch.round(d).abs() <= r).all()), (k, want[k][1, 1])
    what = f"ts={ts} r={r} {metric} {grid}"
    check(batch(tref, hess, movs, flows, grid, ts, r, metric), want, what)
    for order in ([1, 0, 3, 2], [2, 1, 0], [3, 2]):  # every frame behind every kind of predecessor
        got = batch(tref, hess, [movs[k] for k in order], [flows[k] for k in order], grid, ts, r, metric)
        check(got, [want[k] for k in order], f"{what} order {order}")


@pytest.mark.parametrize("grid", [SMALL, BIG], ids=["3x5", "128x192"])
def test_order_independence(grid):
    """The flows of a 4-frame launch equal those of the same frames launched in reverse order, frame by frame."""
    tref, hess, movs, flows = _level(16, grid, 9)
    fwd = batch(tref, hess, movs[:4], flows[:4], grid, 16, 1, "L1")
    rev = batch(tref, hess, movs[:4][::-1], flows[:4][::-1], grid, 16, 1, "L1")
    check(fwd, rev[::-1], f"reverse order, {grid}")


# ------------------------------------------------------------------------------------------ against the oracle
def test_chain_vs_oracle(shape=(48, 80), n=3, factors=(1, 2, 1), tss=(16, 8, 8), metric0="L1"):
    """The three-level chain through alignment.align_batch (every level one launch for the n frames) against the oracle's
    alignment: flows within 1e-4 px, at most one tile on the other side of a block-matching near-tie (helpers.flipped_tiles).
    Levels 48 x 80, 20 x 36 and 20 x 36 again (decimated twice the level is 6 x 14 and holds no 8-pixel tile).  These launches
    are below LOOP_TILES; the flows of the launches above it are tied to the single-frame launches bit for bit by the tests
    above, and those to the oracle by this test and by tests/test_hip_parity.py / test_variant_parity.py."""
    H, W = shape
    rng = np.random.default_rng(H + W)
    big = smooth(rng, H + 32, W + 32, 2.0)
    ref = big[16:16 + H, 16:16 + W].copy()
    comps = []
    for _ in range(n):
        sy, sx = (int(v) for v in rng.integers(-2, 3, 2))
        comps.append(big[16 + sy:16 + sy + H, 16 + sx:16 + sx + W] + 0.005 * rng.standard_normal((H, W)).astype(np.float32))
    cfg = base_config(ts=tss[0], metrics=(metric0, "L2", "L2"))
    bm = cfg.block_matching.tuning
    bm.factors, bm.tile_sizes, bm.search_radii, bm.metrics = list(factors), list(tss), [1, 4, 4], [metric0, "L2", "L2"]
    state = alignment.init_alignment(T(ref), cfg)
    assert alignment.can_align_batch(cfg)
    pyrs = alignment.build_gaussian_pyramids([T(c) for c in comps], bm.factors)
    got = np.stack([f.cpu().numpy() for f in alignment.align_batch(state[0], state[5], pyrs, cfg)])
    ostate = oracle.init_alignment(ref, cfg)
    want = np.stack([oracle.align(*ostate, c, cfg) for c in comps])
    assert got.shape == want.shape == (n, 3, 5, 2)
    flipped = flipped_tiles(got, want)
    assert int(flipped.sum()) <= 1, f"{int(flipped.sum())} flipped tiles"
    assert_close(got[~flipped], want[~flipped], 0, 1e-4, f"{H} x {W} flows")
