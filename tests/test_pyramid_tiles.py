"""k_gauss_decimate<F> (csrc/hhsr_pyramid.hip) at the edges of its tiles of 16 x 120 (factor 2) and 8 x 60 (factor 4)
outputs: a wave per group of intermediate rows with the source window in registers, 16-byte loads on the interior tiles of
sources whose pitch and pointer allow them, clamped dword loads on the tiles of the right and bottom edge.

Shapes (tests/pyramid_tile_cases.py): one output pixel, exactly one tile, a tile minus one / plus one in each direction,
three tiles plus one in each direction, two tiles plus two columns; widths with W % 4 of 0, 1, 2 and 3.  Buffer layouts:
compact; pitches that are multiples of 4 on a 16-byte aligned pointer (the 16-byte path wherever a tile is interior); pitches
that are no multiple of 4; a pitch that is one but on a pointer one element off the grid (both must fall back to dwords).
Every output of every case is compared with the oracle at the tolerance of tests/test_pitched_buffers.py (rtol 0, atol 1e-6)
and with the bits of the kernel before the re-tiling (tests/golden/pyramid_parent.npz, tools/pyramid_parent_golden.py);
outputs lie between guard bands and start as a NaN pattern that has to be gone afterwards."""
import functools

import numpy as np
import pytest
import torch

import oracle
import pyramid_tile_cases as pc
from helpers import assert_close

pytestmark = pytest.mark.gpu

from handheld_super_resolution import _lib, utils_image  # noqa: E402

FILL = 0x7FC5A5A5  # a NaN no arithmetic produces: an element that still holds it was not written
GUARD = 4096       # elements on either side of every buffer
TOL = (0, 1e-6)    # tests/test_pitched_buffers.py::test_gauss_decimate


def up4(n):
    return (n + 3) // 4 * 4


def not4(n):
    return n + 1 if (n + 1) % 4 else n + 2


# id: (source pitch of W, destination pitch of w2, elements the source starts off the 16-byte grid)
LAYOUTS = {
    "compact": (lambda W: W, lambda w: w, 0),
    "pitch4": (lambda W: up4(W) + 4, lambda w: w + 3, 0),
    "odd": (not4, lambda w: w + 2, 0),
    "lead1": (lambda W: up4(W) + 8, lambda w: not4(w), 1),
}
CASES = [(f, name) for f in (2, 4) for name in pc.shapes(f)]
case_ids = dict(ids=lambda c: f"f{c[0]}-{c[1]}")


def bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def same_bits(got, want, what):
    got, want = np.asarray(got), np.asarray(want)
    assert got.shape == want.shape, f"{what}: shape {got.shape} vs {want.shape}"
    diff = bits(got) != bits(want)
    if diff.any():
        k = tuple(np.argwhere(diff)[0])
        raise AssertionError(f"{what}: {int(diff.sum())} of {diff.size} values differ in their bits, the first at "
                             f"{list(map(int, k))}: {got[k]!r} vs {want[k]!r}")


@functools.lru_cache(maxsize=None)
def want(f, name, k):
    img = pc.special_image(f) if name == "special" else pc.image(f, name, k)
    with np.errstate(all="ignore"):
        return pc.frozen(oracle.downsample(img, f))


class Source:
    """An image with row pitch `pitch`, `lead` elements off the allocation's 16-byte grid, NaN in every padding element."""

    def __init__(self, img, pitch, lead):
        H, W = img.shape
        host = np.full(GUARD + lead + H * pitch + GUARD, np.nan, np.float32)
        host[GUARD + lead:GUARD + lead + H * pitch].reshape(H, pitch)[:, :W] = img
        self.buf = torch.from_numpy(host).cuda()
        self.view = self.buf[GUARD + lead:]
        assert self.view.data_ptr() % 16 == 4 * (lead % 4)


class Dest:
    """h2 x w2 outputs with row pitch `pitch` between guard bands, every word pre-filled with FILL."""

    def __init__(self, h2, w2, pitch):
        self.h2, self.w2, self.pitch = h2, w2, pitch
        self.buf = torch.full((2 * GUARD + h2 * pitch,), FILL, dtype=torch.int32, device="cuda")
        self.view = self.buf[GUARD:]

    def read(self, what):
        got = self.buf.cpu().numpy()
        rows = got[GUARD:GUARD + self.h2 * self.pitch].reshape(self.h2, self.pitch)
        assert (got[:GUARD] == FILL).all() and (got[GUARD + self.h2 * self.pitch:] == FILL).all(), f"{what}: a guard band was written"
        assert (rows[:, self.w2:] == FILL).all(), f"{what}: padding columns were written"
        out = rows[:, :self.w2]
        assert (out != FILL).all(), f"{what}: {int((out == FILL).sum())} of {out.size} outputs were not written"
        return out.view(np.float32).copy()


def decimate(f, imgs, lay, batch):
    """The frames `imgs` (one shape) through hhsr_gauss_decimate_batch (`batch`) or hhsr_gauss_decimate (one frame)."""
    H, W = imgs[0].shape
    h2, w2 = (H - 4 * f) // f, (W - 4 * f) // f
    sp_of, dp_of, lead = LAYOUTS[lay]
    sp, dp = sp_of(W), dp_of(w2)
    srcs = [Source(i, sp, lead) for i in imgs]
    dsts = [Dest(h2, w2, dp) for _ in imgs]
    taps, ntaps = utils_image._taps_for_launch(f)
    if batch:
        _lib.call("hhsr_gauss_decimate_batch", _lib.ptr_array([s.view for s in srcs]), len(imgs), H, W, sp,
                  _lib.ptr_array([d.view for d in dsts]), dp, f, taps, ntaps, _lib.stream())
    else:
        assert len(imgs) == 1
        _lib.call("hhsr_gauss_decimate", _lib.ptr(srcs[0].view), H, W, sp, _lib.ptr(dsts[0].view), dp, f, taps, ntaps,
                  _lib.stream())
    torch.cuda.synchronize()
    return [d.read(f"f{f} {H}x{W} [{lay}] frame {k}") for k, d in enumerate(dsts)]


def check(got, f, name, k, g, what):
    """Every output: the oracle within TOL, and the parent kernel's bits."""
    assert_close(got, want(f, name, k), *TOL, f"{what} vs oracle")
    same_bits(got, g[f"f{f}_special" if name == "special" else pc.golden_key(f, name, k)], f"{what} vs parent")


@pytest.mark.parametrize("lay", list(LAYOUTS))
@pytest.mark.parametrize("case", CASES, **case_ids)
def test_single_frame_and_batch_of_three(golden, case, lay):
    """One frame through hhsr_gauss_decimate and the shape's three images through one batched launch: the oracle, the
    parent's bits, and the first frame alike from both calls."""
    f, name = case
    g = golden("pyramid_parent")
    imgs = [pc.image(f, name, k) for k in range(pc.N_IMAGES)]
    one = decimate(f, imgs[:1], lay, batch=False)[0]
    check(one, f, name, 0, g, f"f{f} {name} [{lay}] single")
    for k, got in enumerate(decimate(f, imgs, lay, batch=True)):
        check(got, f, name, k, g, f"f{f} {name} [{lay}] batch of 3, frame {k}")
        if k == 0:
            same_bits(got, one, f"f{f} {name} [{lay}]: batched vs single")


@pytest.mark.parametrize("lay", ["compact", "pitch4"])
@pytest.mark.parametrize("case", CASES, **case_ids)
def test_batch_of_max_batch_plus_one(golden, case, lay):
    """HHSR_MAX_BATCH + 1 frames (a full launch and one of a single frame), the three images cyclically: a frame's result
    does not depend on its place in the batch."""
    f, name = case
    g = golden("pyramid_parent")
    n = _lib.MAX_BATCH + 1
    got = decimate(f, [pc.image(f, name, k % pc.N_IMAGES) for k in range(n)], lay, batch=True)
    assert len(got) == n
    for k, a in enumerate(got):
        check(a, f, name, k % pc.N_IMAGES, g, f"f{f} {name} [{lay}] batch of {n}, frame {k}")


@pytest.mark.parametrize("lay", list(LAYOUTS))
@pytest.mark.parametrize("f", [2, 4])
def test_signed_zeros_denormals_and_large_values(golden, f, lay):
    """-0.0 (an all -0.0 footprint gives +0.0 only through the sums' leading 0.f +), denormals and +-1e30."""
    got = decimate(f, [pc.special_image(f)], lay, batch=False)[0]
    assert not np.isnan(got).any()
    assert (bits(got) == 0).any() and (np.abs(got) > 1e28).any() and ((got != 0) & (np.abs(got) < 1e-38)).any()
    check(got, f, "special", 0, golden("pyramid_parent"), f"f{f} special [{lay}]")


def test_layouts_reach_both_load_paths():
    """(no GPU work) The layouts give what the launcher decides on: a pitch that is a multiple of 4 on an aligned pointer,
    pitches that are not, and a pointer off the grid."""
    for f, name in CASES:
        W = pc.shapes(f)[name][1]
        assert LAYOUTS["pitch4"][0](W) % 4 == 0 and LAYOUTS["pitch4"][0](W) > W
        assert LAYOUTS["odd"][0](W) % 4 and LAYOUTS["odd"][0](W) > W
        assert LAYOUTS["lead1"][0](W) % 4 == 0 and LAYOUTS["lead1"][2] % 4
