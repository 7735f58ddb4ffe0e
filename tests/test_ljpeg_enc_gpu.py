"""The lossless-JPEG encoder on the device: hhsr_ljpeg_histogram against np.bincount of ljpeg_ref.categories, and
hhsr_ljpeg_encode against hhsr_ljpeg_encode_host (which tests/test_ljpeg_enc_host.py pins to ljpeg_ref.encode): bytes, offsets,
byte counts and length, on the host cases and on the shapes at which only the kernel can go wrong."""
import numpy as np
import pytest

import ljpeg_enc_cases as enc

pytestmark = pytest.mark.gpu

# csrc/hhsr_ljpeg_enc.hip: a workgroup codes LE_BATCH samples at a time, LE_PER consecutive ones per thread; the offsets scan
# of hhsr_jpeg.hip works on groups of SCAN_GROUP tiles
LE_BATCH, LE_PER, SCAN_GROUP, LE_MAX_GRID = 2048, 8, 2048, 2048  # (LE_MAX_GRID: workgroups of a launch of the coder)


def same(a, b):
    assert a.intact and b.intact
    assert a.length == b.length
    assert (a.offsets == b.offsets).all() and (a.tile_bytes == b.tile_bytes).all()
    assert a.out.size == b.out.size and (a.out == b.out).all()


def check(img, P, predictor, th, tw, row_elems=None, **kw):
    tables = enc.tables_for(img, P, predictor, th, tw)
    host = enc.encode_host(img, P, predictor, th, tw, tables, row_elems=row_elems)
    gpu = enc.encode_gpu(img, P, predictor, th, tw, tables, row_elems=row_elems, **kw)
    same(gpu, host)
    return tables, host


@pytest.mark.parametrize("row_elems", [None, 56 * 3 + 5, 56 * 3 + 6])
@pytest.mark.parametrize("predictor", [1, 4, 7])
def test_histogram(predictor, row_elems):
    """Compact rows, and padded ones (odd: sample by sample; even: the dword loads) inside guard bands; 40 x 56 in 16 x 32
    tiles counts the replicated samples of the right, bottom and corner tiles."""
    img = enc.image("smooth", 40, 56, 3, 16, seed=predictor)
    img[::7, ::5] = enc.image("noise", 40, 56, 3, 16, seed=1)[::7, ::5]
    counts, status, intact = enc.histogram_gpu(img, 16, predictor, 16, 32, row_elems=row_elems)
    assert intact and status == 0
    assert (counts == enc.ref_counts(img, 16, predictor, 16, 32)).all()


def test_histogram_more_items_than_workgroups_and_bad_sample():
    """The histogram launches 1024 workgroups at most: 784 x 768 in 16 x 16 tiles are 2352 items, walked by stride.  A sample
    at or above 2^P sets the status."""
    img = enc.image("smooth", 784, 768, 1, 12, seed=4)
    counts, status, intact = enc.histogram_gpu(img, 12, 1, 16, 16)
    assert intact and status == 0 and (counts == enc.ref_counts(img, 12, 1, 16, 16)).all()
    img[500, 300] = 4096
    counts, status, intact = enc.histogram_gpu(img, 12, 1, 16, 16)
    from handheld_super_resolution import _lib
    assert intact and status == _lib.LJPEG_BAD_SAMPLE


@pytest.mark.parametrize("Nf,P", [(1, 16), (3, 16), (3, 10), (2, 12), (4, 16)])
def test_encode_equals_host(Nf, P):
    check(enc.image("smooth", 40, 56, Nf, P, seed=Nf), P, 1, 16, 32)


@pytest.mark.parametrize("predictor", range(1, 8))
def test_encode_every_predictor(predictor):
    check(enc.image("smooth", 40, 56, 3, 16, seed=predictor), 16, predictor, 16, 32, row_elems=56 * 3 + 5)
    check(enc.image("noise", 20, 24, 1, 16, seed=predictor), 16, predictor, 16, 16)


@pytest.mark.parametrize("kind", ["flat", "alt", "noise"])
def test_encode_edge_contents(kind):
    """One category and a 1-bit code; SSSS 16 without magnitude bits; full-range noise with many stuffed FF bytes."""
    check(enc.image(kind, 40, 56, 3, 16, seed=5), 16, 1, 16, 32)
    check(enc.image(kind, 32, 32, 1, 16, seed=5), 16, 1, 16, 16)


def test_tile_of_several_batches_with_carry():
    """64 x 64 x 3 = 12288 samples: six batches of LE_BATCH; the codes of a photograph-like image have every length, so the
    batch boundaries fall inside a byte (checked on the bit counts) and the unfinished byte is carried."""
    import ljpeg_ref as ref

    img = enc.image("smooth", 64, 64, 3, 16, seed=8)
    assert 64 * 64 * 3 >= 3 * LE_BATCH
    tables, _ = check(img, 16, 1, 64, 64)
    d, ssss = ref.categories(img.astype(np.int64), 16, 1)
    nbits = np.zeros(img.shape, np.int64)
    for c in range(3):
        lens = {s: l for s, (_, l) in ref.codes_of(*tables[c]).items()}
        nbits[:, :, c] = np.vectorize(lens.get)(ssss[:, :, c]) + np.where(ssss[:, :, c] == 16, 0, ssss[:, :, c])
    ends = np.cumsum(nbits.reshape(-1))[LE_BATCH - 1::LE_BATCH]
    assert len(ends) == 6 and (ends[:-1] % 8 != 0).any()
    check(enc.image("noise", 64, 64, 3, 16, seed=9), 16, 5, 64, 64)  # the fullest batches: 2048 x up to 31 bits


@pytest.mark.parametrize("th,tw,Nf", [(16, 16, 1), (48, 48, 1), (16, 48, 3)])
def test_tile_narrower_than_a_batch_or_no_multiple(th, tw, Nf):
    """16 x 16 x 1 = 256 samples, a fraction of LE_BATCH; 48 x 48 = 2304 and 16 x 48 x 3 = 2304: one batch and a partial one."""
    assert th * tw * Nf < LE_BATCH or (th * tw * Nf) % LE_BATCH
    check(enc.image("smooth", 100, 100, Nf, 14, seed=th), 14, 6, th, tw)


def test_more_tiles_than_one_scan_group():
    """16 x 16 tiles over 784 x 768: 49 x 48 = 2352 tiles, more than SCAN_GROUP and more than the LE_MAX_GRID workgroups of
    a launch: the last 304 tiles are the second tile of a workgroup's strided walk."""
    assert (784 // 16) * (768 // 16) > max(SCAN_GROUP, LE_MAX_GRID)
    img = enc.image("smooth", 784, 768, 1, 16, seed=10)
    check(img, 16, 1, 16, 16)


@pytest.mark.parametrize("row_elems", [100 * 3 + 2, 100 * 3 + 7])
def test_padded_rows(row_elems):
    """Even row_elems: dword loads in the tiles inside the image, sample by sample at its right edge; odd: no dword loads."""
    check(enc.image("smooth", 50, 100, 3, 16, seed=11), 16, 4, 32, 32, row_elems=row_elems)


def test_unaligned_output_pointer():
    for shift in (1, 2, 3):
        check(enc.image("noise", 40, 56, 3, 16, seed=12), 16, 1, 16, 32, out_shift=shift)


def test_side_stream_and_two_runs():
    import torch

    img = enc.image("smooth", 64, 96, 3, 16, seed=13)
    tables, host = check(img, 16, 1, 32, 32, stream=torch.cuda.Stream())
    a = enc.encode_gpu(img, 16, 1, 32, 32, tables)
    b = enc.encode_gpu(img, 16, 1, 32, 32, tables)
    same(a, b)


def test_cut_capacity():
    img = enc.image("noise", 40, 56, 3, 16, seed=6)
    tables = enc.tables_for(img, 16, 1, 16, 32)
    whole = enc.encode_host(img, 16, 1, 16, 32, tables)
    for cap in (whole.length // 2, whole.length // 2 + 1, 1, whole.length - 1):
        same(enc.encode_gpu(img, 16, 1, 16, 32, tables, capacity=cap), enc.encode_host(img, 16, 1, 16, 32, tables, capacity=cap))


def test_missing_category_and_bad_sample():
    img = enc.image("smooth", 32, 32, 1, 16, seed=2)
    flat_tables = enc.tables_for(enc.image("flat", 32, 32, 1, 16), 16, 1, 16, 16)
    got = enc.encode_gpu(img, 16, 1, 16, 16, flat_tables)
    assert got.length == enc.UINT64_MAX and got.intact
    img = enc.image("smooth", 16, 16, 1, 10, seed=3)
    img[7, 7] = 1024
    got = enc.encode_gpu(img, 10, 1, 16, 16, enc.tables_for(img, 10, 1, 16, 16))
    assert got.length == enc.UINT64_MAX and got.intact
