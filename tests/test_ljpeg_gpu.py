"""hhsr_ljpeg_decode on the GPU == hhsr_ljpeg_decode_host == the encoded counts, bit for bit: tiles and strips that the image
crops, Nf = 2, predictors and precisions, mixed tables, pitched output inside guard bands, segment counts around the
launch's tail, and the statuses of a truncated stream and of a code outside its table between valid neighbours."""
import numpy as np
import pytest

import ljpeg_cases as cases
import ljpeg_ref as ref

pytestmark = pytest.mark.gpu


def burst_counts(P, n=2, H=24, W=40, seed=0):
    """Counts of a synthetic burst scaled to P bits, with some samples at 0 and at the maximum."""
    from handheld_super_resolution import synthetic

    refi, comp, _ = synthetic.make_burst(H, W, n, seed=seed, max_shift=1.0)
    stack = np.concatenate([np.asarray(refi)[None], np.asarray(comp)])[:n]
    c = np.clip(np.rint(stack * ((1 << P) - 1)), 0, (1 << P) - 1).astype(np.int64)
    rng = np.random.default_rng(seed)
    c[rng.random(c.shape) < 0.02] = (1 << P) - 1
    c[rng.random(c.shape) < 0.02] = 0
    return c


def check(items, counts, row_elems=None, dedup=True):
    n, H, W = counts.shape
    plan = cases.plan_from_streams(items, n, H, W, dedup=dedup)
    host, hs, hi = cases.decode_host(plan, row_elems)
    gpu, gs, gi = cases.decode_gpu(plan, row_elems)
    assert hi and gi, "guard bands"
    assert not hs.any() and not gs.any(), (hs, gs)
    assert (host == counts).all() and (gpu == counts).all() and (gpu == host).all()
    return plan


@pytest.mark.parametrize("P", [10, 16])
@pytest.mark.parametrize("predictor", [1, 6, 7])
def test_tiles_and_strips_cropped_by_the_image(P, predictor):
    """2 frames of 40 x 24: 16 x 16 tiles (the right tile keeps 8 columns, the bottom tile 8 rows), strips of 7 rows (the last
    is short), each with Nf = 1 and with Nf = 2 at X = seg_w / 2, tables alternating between K.2 per stream and the fixed
    table with 16-bit codes, the output pitched by 13 elements inside guard bands."""
    c = burst_counts(P, seed=P + predictor)
    mixed = lambda k: "fixed" if k % 3 == 1 else "k2"  # noqa: E731
    for layout, size in (("tiles", (16, 16)), ("strips", 7)):
        for Nf in (1, 2):
            items = cases.segment_streams(c, P, layout, size, Nf=Nf, predictor=predictor, tables=mixed)
            plan = check(items, c, row_elems=40 + 13)
            assert len(plan.tables) > 1


def test_line_of_two_tile_rows_and_four_components():
    c = burst_counts(12, seed=5)
    check(cases.segment_streams(c, 12, "tiles", (16, 8), Nf=1, X=32, predictor=4), c)
    check(cases.segment_streams(c, 12, "tiles", (16, 8), Nf=4, X=2, predictor=5), c, row_elems=41)


@pytest.mark.parametrize("W,H,tw,th", [(1040, 16, 16, 16), (4112, 16, 16, 16), (328, 200, 8, 2)])
def test_segment_counts_around_the_launch_tail(W, H, tw, th):
    """65 and 257 segments of one lane each, and 4100 segments, where a workgroup takes three and the last one two."""
    c = burst_counts(10, n=1, H=H, W=W, seed=W)
    items = cases.segment_streams(c, 10, "tiles", (tw, th), Nf=2, predictor=1, tables="fixed" if W == 328 else "k2shared")
    assert len(items) == {1040: 65, 4112: 257, 328: 4100}[W]
    check(items, c)


def test_more_tables_than_the_lds_holds():
    """Tables not deduplicated: 30 of them, above HHSR_LJPEG_LDS_TABLES, so the kernel reads them from global memory."""
    c = burst_counts(14, seed=3)
    plan = check(cases.segment_streams(c, 14, "strips", 4, Nf=2, predictor=6, tables="k2"), c, dedup=False)
    assert len(plan.tables) > 16


def test_status_of_a_truncated_stream_and_of_a_code_outside_its_table():
    """The streams tests/ljpeg_fuzz_main.cpp mutates (the same generator and seed): stream 0 cut at half its entropy-coded
    bytes, and with FF 00 FF 00 — sixteen one bits — as its first bytes, between valid segments."""
    from handheld_super_resolution import _lib

    rng = np.random.default_rng(11)
    s = rng.integers(0, 1 << 10, (6, 8, 2))
    good = ref.encode(s, 10, 1, tables="k2")
    h, data = ref.split(good)
    at = h["data_offset"]
    cut = good[:at + len(data) // 2]
    bad = good[:at] + b"\xff\x00\xff\x00" + good[at + 4:]
    rect = s.reshape(6, 16)
    other = rng.integers(0, 1 << 10, (6, 16))
    other_stream = ref.encode(ref.to_stream_geometry(other, 1, 16), 10, 7, tables="fixed")
    streams = [good, cut, other_stream, bad, good]
    items = [(st, 0, 16 * i, 0, 16, 6) for i, st in enumerate(streams)]
    plan = cases.plan_from_streams(items, 1, 6, 80)
    want = [_lib.LJPEG_OK, _lib.LJPEG_TRUNCATED, _lib.LJPEG_OK, _lib.LJPEG_BAD_CODE, _lib.LJPEG_OK]
    for decode in (cases.decode_host, cases.decode_gpu):
        got, status, intact = decode(plan, row_elems=96)
        assert intact and status.tolist() == want, (decode.__name__, status)
        assert (got[0, :, 0:16] == rect).all() and (got[0, :, 32:48] == other).all() and (got[0, :, 64:80] == rect).all()
    host, gpu = cases.decode_host(plan, 96)[0], cases.decode_gpu(plan, 96)[0]
    assert (host == gpu).all()  # the failed segments too: the same samples up to where each ended
