"""The lossless-JPEG encoder on the host, no GPU: hhsr_ljpeg_huffman against ljpeg_ref.build_k2, hhsr_ljpeg_encode_host
against ljpeg_ref.encode byte for byte with both decoders giving the samples back, the layout of the result, the cut capacity,
and the host core under sanitizers (tests/ljpeg_enc_main.cpp, a stand-alone program)."""
import ctypes
import os
import shutil
import subprocess

import numpy as np
import pytest

import ljpeg_enc_cases as enc
import ljpeg_ref as ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def fibonacci17():
    f = [1, 2]  # with the reserved point's 1 in front: every sum stays below the next count, so the tree is a chain
    while len(f) < 17:
        f.append(f[-1] + f[-2])
    return f


HUFFMAN_CASES = {
    "one": [0] * 5 + [9] + [0] * 11,
    "two": [0, 7] + [0] * 14 + [3],
    "equal": [5] * 17,
    "geometric": [1 << (16 - i) if i < 12 else 0 for i in range(17)],
    "fibonacci": fibonacci17(),          # with the reserved point: code lengths above 16, figure K.3 acts
    "fibonacci_reversed": fibonacci17()[::-1],
    "powers": [1 << i for i in range(17)],  # 1 (reserved), 1, 2, 4, ...: every merge takes the last sum, a chain 17 deep
}


@pytest.mark.parametrize("name", HUFFMAN_CASES)
def test_huffman_equals_annex_k2(name):
    counts = HUFFMAN_CASES[name]
    bits, values = enc.huffman(counts)
    rb, rv = ref.build_k2(counts)
    assert bits == rb and values == rv
    assert sorted(values) == [i for i, c in enumerate(counts) if c]  # zero counts get no code
    if name in ("fibonacci", "powers"):  # a chain of 18 symbols is 17 deep: K.3 shortened it to the 16-bit limit
        assert bits[15] >= 1 and sum(bits) == 17


def test_huffman_refuses_empty_counts():
    from handheld_super_resolution import _lib

    lib = _lib.load()
    c, b, v, n = np.zeros(17, np.uint64), np.zeros(16, np.uint8), np.zeros(17, np.uint8), ctypes.c_int()
    assert lib.hhsr_ljpeg_huffman(c.ctypes.data, b.ctypes.data, v.ctypes.data, ctypes.byref(n)) == -1
    assert b"invalid argument" in lib.hhsr_last_error()
    assert lib.hhsr_ljpeg_huffman(None, b.ctypes.data, v.ctypes.data, ctypes.byref(n)) == -1


def check_against_reference(img, P, predictor, th, tw, row_elems=None):
    H, W, Nf = img.shape
    tables = enc.tables_for(img, P, predictor, th, tw)
    got = enc.encode_host(img, P, predictor, th, tw, tables, row_elems=row_elems)
    want = enc.ref_streams(img, P, predictor, th, tw, tables)
    assert got.intact and got.length == got.out.size
    enc.check_layout(got, len(want))
    tiles = enc.tiles_of(img, th, tw)
    for i, w in enumerate(want):
        o, nb = int(got.offsets[i]), int(got.tile_bytes[i])
        assert got.out[o:o + nb].tobytes() == w, i
        if nb & 1:
            assert got.out[o + nb] == 0
        if i < 2:  # the pure-Python decoder is slow: two tiles
            assert (ref.decode(w) == tiles[i]).all()
    assert (enc.decode_tiles(got.out, got.offsets, got.tile_bytes, H, W, Nf, th, tw) == img).all()
    return got


@pytest.mark.parametrize("Nf,P", [(1, 16), (3, 16), (3, 10), (2, 12), (4, 16)])
def test_encode_host_equals_reference(Nf, P):
    """40 x 56 in 16 x 32 tiles: right, bottom and corner tiles replicate the edge."""
    check_against_reference(enc.image("smooth", 40, 56, Nf, P, seed=Nf), P, 1, 16, 32)


@pytest.mark.parametrize("predictor", range(1, 8))
def test_encode_host_every_predictor(predictor):
    check_against_reference(enc.image("smooth", 40, 56, 3, 16, seed=predictor), 16, predictor, 16, 32, row_elems=56 * 3 + 5)
    check_against_reference(enc.image("noise", 20, 24, 1, 16, seed=predictor), 16, predictor, 16, 16)


def test_encode_host_flat_image():
    """One category: a 1-bit code, every sample one 0 bit."""
    img = enc.image("flat", 32, 32, 1, 16)
    got = check_against_reference(img, 16, 1, 16, 16)
    tables = enc.tables_for(img, 16, 1, 16, 16)
    assert tables[0] == ([1] + [0] * 15, [0])


def test_encode_host_alternating_0_32768():
    """SSSS 16: a code and no magnitude bits."""
    img = enc.image("alt", 16, 32, 1, 16)
    _, ssss = ref.categories(enc.tiles_of(img, 16, 32)[0].astype(np.int64), 16, 1)
    assert (ssss == 16).sum() > 400
    check_against_reference(img, 16, 1, 16, 32)


def test_encode_host_full_range_noise():
    """Many FF bytes, streams of odd and of even length: the pad byte and the even offsets are both met."""
    img = enc.image("noise", 40, 56, 3, 16, seed=5)
    got = check_against_reference(img, 16, 1, 16, 32)
    assert got.out.tobytes().count(b"\xff\x00") > 50
    assert {int(b) & 1 for b in got.tile_bytes} == {0, 1}


def test_missing_category_is_reported():
    img = enc.image("smooth", 32, 32, 1, 16, seed=2)
    flat_tables = enc.tables_for(enc.image("flat", 32, 32, 1, 16), 16, 1, 16, 16)  # a code for SSSS 0 alone
    got = enc.encode_host(img, 16, 1, 16, 16, flat_tables)
    assert got.length == enc.UINT64_MAX and got.intact


def test_sample_above_precision_is_reported():
    img = enc.image("smooth", 16, 16, 1, 10, seed=3)
    tables = enc.tables_for(img, 10, 1, 16, 16)
    assert enc.encode_host(img, 10, 1, 16, 16, tables).length != enc.UINT64_MAX
    img[7, 7] = 1024
    tables = enc.tables_for(img, 10, 1, 16, 16)  # (every category that occurs has a code: the sample alone is refused)
    assert enc.encode_host(img, 10, 1, 16, 16, tables).length == enc.UINT64_MAX


def test_cut_capacity():
    """About half the result: the prefix is equal, the guard band behind it intact, offsets and length those of the whole."""
    img = enc.image("noise", 40, 56, 3, 16, seed=6)
    tables = enc.tables_for(img, 16, 1, 16, 32)
    whole = enc.encode_host(img, 16, 1, 16, 32, tables)
    for cap in (whole.length // 2, whole.length // 2 + 1, 0, 1, whole.length - 1):
        cut = enc.encode_host(img, 16, 1, 16, 32, tables, capacity=cap)
        assert cut.intact and cut.length == whole.length
        assert (cut.offsets == whole.offsets).all() and (cut.tile_bytes == whole.tile_bytes).all()
        assert cut.out.size == cap and (cut.out == whole.out[:cap]).all()


def test_argument_errors():
    from handheld_super_resolution import _lib

    lib = _lib.load()
    img = enc.image("smooth", 32, 32, 1, 16)
    bits, values = enc.pack_tables(enc.tables_for(img, 16, 1, 16, 16))
    out, off, tb, ln = np.zeros(1 << 16, np.uint8), np.zeros(5, np.uint64), np.zeros(4, np.uint32), np.zeros(1, np.uint64)

    def call(H=32, W=32, Nf=1, row=32, P=16, predictor=1, th=16, tw=16, src=img.ctypes.data, o=out.ctypes.data, b=bits):
        return lib.hhsr_ljpeg_encode_host(src, H, W, Nf, row, P, predictor, th, tw, b.ctypes.data, values.ctypes.data, o,
                                          out.size, off.ctypes.data, tb.ctypes.data, ln.ctypes.data)

    assert call() == 0
    bad_bits = bits.copy()
    bad_bits[0, 0] = 3  # three codes of one bit: no prefix code
    for kwargs in (dict(H=0), dict(Nf=5), dict(row=31), dict(P=1), dict(P=17), dict(predictor=0), dict(predictor=8), dict(th=8),
                   dict(tw=24), dict(tw=65536), dict(W=(1 << 30) + 1, row=1 << 31), dict(H=(1 << 30) + 1), dict(src=None), dict(src=img.ctypes.data + 1), dict(o=img.ctypes.data),
                   dict(b=bad_bits)):
        assert call(**kwargs) == -1 and b"invalid argument" in lib.hhsr_last_error(), kwargs
    sb, mb = ctypes.c_size_t(), ctypes.c_size_t()
    assert lib.hhsr_ljpeg_encode_workspace(32, 32, 1, 16, 20, ctypes.byref(sb), ctypes.byref(mb)) == -1
    assert lib.hhsr_ljpeg_encode_workspace(40, 56, 3, 16, 32, ctypes.byref(sb), ctypes.byref(mb)) == 0
    header = 2 + 19 + 3 * 38 + 14
    assert mb.value == 6 * (header + 2 * -(-31 * 16 * 32 * 3 // 8) + 3)  # the bound hhsr.h derives
    # device pointers are checked the same way, before any HIP call
    assert lib.hhsr_ljpeg_encode(None, 32, 32, 1, 32, 16, 1, 16, 16, None, None, None, 0, None, 0, None, None, None, None) == -1
    assert lib.hhsr_ljpeg_histogram(None, 32, 32, 1, 32, 16, 1, 16, 16, None, None, None, 0, None) == -1


def _clangxx():
    for c in ("/opt/rocm/lib/llvm/bin/clang++", shutil.which("clang++")):
        if c and os.path.exists(c):
            return c
    return None


@pytest.mark.timeout(600)
def test_encoder_under_sanitizers(tmp_path):
    """tests/ljpeg_enc_main.cpp with -fsanitize=address,undefined, run as an ordinary child process: the edge cases at full
    and at cut capacity inside guard bands, decoded again by hhsr_lj::decode_segment."""
    cxx = _clangxx()
    if cxx is None:
        pytest.skip("no clang++")
    exe = str(tmp_path / "ljpeg_enc")
    r = subprocess.run([cxx, "-std=c++17", "-O1", "-g", "-Wall", "-Werror", "-fsanitize=address,undefined",
                        "-fno-sanitize-recover=all", "-fno-omit-frame-pointer", os.path.join(ROOT, "tests", "ljpeg_enc_main.cpp"),
                        "-o", exe], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-3000:]
    r = subprocess.run([exe], capture_output=True, text=True, timeout=500)
    assert r.returncode == 0 and "guards intact" in r.stdout, r.stdout + r.stderr[-3000:]
    assert "Sanitizer" not in r.stderr and "runtime error" not in r.stderr, r.stderr[-3000:]
