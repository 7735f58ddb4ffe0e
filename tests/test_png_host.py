"""PNG output, the host side: hhsr_png_huffman, hhsr_png_file_head / _tail, hhsr_png_crc_combine, hhsr_png_workspace, the
refusals of every entry point, and utils_image.png_option / save_png_bytes.  No device needed: only the built library and
the restatement tests/png_ref.py."""
import ctypes as C
import struct
import zlib

import numpy as np
import pytest

import png_ref as ref

from handheld_super_resolution import _lib, utils_image


# ---- hhsr_png_huffman ---------------------------------------------------------------------------------------------------------
def filtered_rows_counts():
    """Counts of a real filtered stream: a smooth 8-bit RGB image under the adaptive choice, intervals of 300 bytes."""
    img = ref.test_images(40, 72, 3, seed=11)["smooth"]
    rows, bpp = ref.row_bytes(ref.samples(img))
    stream, _ = ref.filtered_stream(rows, bpp, 5)
    c = np.zeros(257, np.uint64)
    c[:256] = ref.byte_counts(stream)
    c[256] = ref.n_intervals(stream.size, 300)
    return c


def fibonacci_counts():
    """40 symbols with Fibonacci counts (unlimited Huffman depth 39 > 15) and the end symbol."""
    c = np.zeros(257, np.uint64)
    a, b = 1, 1
    for s in range(40):
        c[5 * s] = a
        a, b = b, a + b
    c[256] = 1
    return c


def count_cases():
    two = np.zeros(257, np.uint64)
    two[[7, 256]] = (1000, 1)
    two_bytes = np.zeros(257, np.uint64)
    two_bytes[[0, 255, 256]] = (5, 9, 2)
    single = np.zeros(257, np.uint64)
    single[[153, 256]] = (1 << 20, 3)
    return {"uniform": np.full(257, 1000, np.uint64), "two symbols": two, "two byte values": two_bytes,
            "single byte value": single, "fibonacci": fibonacci_counts(), "filtered rows": filtered_rows_counts()}


COUNTS = count_cases()


def unlimited_huffman_depth(counts):
    import heapq

    heap = [(int(c), i, 0) for i, c in enumerate(counts) if int(c)]
    heapq.heapify(heap)
    k = len(heap)
    while len(heap) > 1:
        a, b = heapq.heappop(heap), heapq.heappop(heap)
        k += 1
        heapq.heappush(heap, (a[0] + b[0], k, max(a[2], b[2]) + 1))
    return heap[0][2]


@pytest.mark.parametrize("name", list(COUNTS))
def test_huffman_lengths_are_complete_limited_and_optimal(name):
    counts = COUNTS[name]
    spec = utils_image.png_huffman(counts)
    lens, nbits, hdr = ref.spec_parts(spec)
    used = counts > 0
    assert (lens[~used] == 0).all() and (lens[used] >= 1).all()       # zero counts uncoded, every counted symbol coded
    assert lens.max() <= 15
    assert sum(1 << (15 - int(v)) for v in lens[used]) == 1 << 15      # Kraft sum exactly 1
    cost = int(sum(int(c) * int(v) for c, v in zip(counts, lens)))
    assert cost == ref.package_merge_cost(counts, 15)
    assert 17 + 12 <= nbits <= 3700 and tuple(hdr[:3]) == (0, 0, 1)    # BFINAL 0, BTYPE 10 (LSB first)
    assert not spec[ref.SPEC_HDR_AT + (nbits + 7) // 8:].any()
    if name == "fibonacci":
        assert unlimited_huffman_depth(counts) > 15 and lens.max() == 15


def stream_for(counts, rng):
    """A byte stream whose values are exactly the counted ones (the counts' proportions do not matter for decoding)."""
    values = np.flatnonzero(counts[:256] > 0)
    return values[rng.integers(0, values.size, 1500)].astype(np.uint8)


@pytest.mark.parametrize("name", list(COUNTS))
def test_reference_coder_with_the_library_spec_inflates(name):
    """The block header the library writes is one zlib accepts, for intervals of 1, 7, 300 and >= N bytes."""
    counts = COUNTS[name]
    spec = utils_image.png_huffman(counts)
    data = stream_for(counts, np.random.default_rng(5))
    for interval in (1, 7, 300, data.size, data.size + 100):
        if interval == 1:
            piece = data[:200]
        else:
            piece = data
        d = ref.deflate(piece, interval, spec)
        assert zlib.decompress(d, wbits=-15) == piece.tobytes(), interval
        payload = b"\x78\x01" + d + struct.pack(">I", zlib.adler32(piece.tobytes()))
        assert zlib.decompress(payload) == piece.tobytes(), interval


def test_huffman_refusals():
    lib = _lib.load()
    spec = (C.c_uint8 * _lib.PNG_SPEC_BYTES)()
    good = np.full(257, 3, np.uint64)

    def rc(counts, out=spec):
        c = np.ascontiguousarray(counts, np.uint64)
        return lib.hhsr_png_huffman(c.ctypes.data_as(C.POINTER(C.c_uint64)), out)

    assert rc(good) == 0
    no_end = good.copy()
    no_end[256] = 0
    only_end = np.zeros(257, np.uint64)
    only_end[256] = 4
    huge = good.copy()
    huge[3] = 1 << 60
    for bad in (no_end, only_end, np.zeros(257, np.uint64), huge):
        assert rc(bad) == -1 and b"invalid argument" in lib.hhsr_last_error()
    assert lib.hhsr_png_huffman(None, spec) == -1 and rc(good, None) == -1
    with pytest.raises(ValueError):
        utils_image.png_huffman(np.zeros(256, np.uint64))


# ---- the file's fixed parts -----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("H,W,och,bits,n", [(1, 1, 1, 8, 11), (6000, 8000, 3, 8, 123456789), (3, 70000, 3, 16, (1 << 31) - 7),
                                            (17, 9, 1, 16, 1)])
def test_file_head(H, W, och, bits, n):
    assert utils_image.png_file_head(H, W, och, bits, n).tobytes() == ref.file_head(H, W, och, bits, n)


def test_file_tail_and_whole_file():
    rng = np.random.default_rng(2)
    for n, m in ((1, 1), (5, 300), (70001, 1234)):
        deflate, stream = rng.integers(0, 256, n, np.uint8).tobytes(), rng.integers(0, 256, m, np.uint8).tobytes()
        got = utils_image.png_file_tail(zlib.crc32(deflate), n, zlib.adler32(stream)).tobytes()
        assert got == ref.file_tail(deflate, stream)
    # a whole file from the reference coder and the library's fixed parts: Pillow-independent check through the parser
    img = ref.test_images(9, 17, 3, seed=4)["smooth"]
    q = ref.samples(img)
    rows, bpp = ref.row_bytes(q)
    stream, _ = ref.filtered_stream(rows, bpp, 5)
    counts = np.zeros(257, np.uint64)
    counts[:256] = ref.byte_counts(stream)
    counts[256] = ref.n_intervals(stream.size, 100)
    spec = utils_image.png_huffman(counts)
    d = ref.deflate(stream, 100, spec)
    file_bytes = (utils_image.png_file_head(9, 17, 3, 8, len(d)).tobytes() + d +
                  utils_image.png_file_tail(zlib.crc32(d), len(d), zlib.adler32(stream.tobytes())).tobytes())
    assert file_bytes == ref.png_file(9, 17, 3, 8, stream, 100, spec)
    assert np.array_equal(ref.decode(file_bytes), q)
    PIL = pytest.importorskip("PIL.Image")
    import io

    assert np.array_equal(np.asarray(PIL.open(io.BytesIO(file_bytes))), q)


def test_file_parts_refusals():
    lib = _lib.load()
    buf, n = (C.c_uint8 * 64)(), C.c_size_t(0)
    assert lib.hhsr_png_file_head(4, 4, 3, 8, 10, buf, 64, C.byref(n)) == 0 and n.value == 43
    assert lib.hhsr_png_file_tail(1, 10, 2, buf, 64, C.byref(n)) == 0 and n.value == 20
    bad_heads = [(0, 4, 3, 8, 10, buf, 64), (4, 0, 3, 8, 10, buf, 64), (4, 4, 2, 8, 10, buf, 64), (4, 4, 3, 12, 10, buf, 64),
                 (4, 4, 3, 8, 0, buf, 64), (4, 4, 3, 8, (1 << 31) - 6, buf, 64), (4, 4, 3, 8, 10, None, 64),
                 (4, 4, 3, 8, 10, buf, 42)]
    for args in bad_heads:
        assert lib.hhsr_png_file_head(*args, C.byref(n)) == -1 and b"invalid argument" in lib.hhsr_last_error(), args
    assert n.value == 43  # (the needed size is reported with the refusal of a short buffer)
    for args in [(1, 0, 2, buf, 64), (1, (1 << 31) - 6, 2, buf, 64), (1, 10, 2, None, 64), (1, 10, 2, buf, 19)]:
        assert lib.hhsr_png_file_tail(*args, C.byref(n)) == -1 and b"invalid argument" in lib.hhsr_last_error(), args
    assert lib.hhsr_png_file_head(4, 4, 3, 8, 10, buf, 64, None) == -1 and lib.hhsr_png_file_tail(1, 10, 2, buf, 64, None) == -1
    assert lib.hhsr_png_crc_combine(1, 2, 3, None) == -1


def test_crc_combine():
    rng = np.random.default_rng(9)
    for na, nb in ((0, 0), (0, 5), (5, 0), (1, 1), (3, 4), (1000, 77), (12, 65536 + 3), (7, 1 << 22)):
        a, b = rng.integers(0, 256, na, np.uint8).tobytes(), rng.integers(0, 256, nb, np.uint8).tobytes()
        want = zlib.crc32(a + b)
        assert ref.crc_combine(zlib.crc32(a), zlib.crc32(b), nb) == want      # (the restatement itself, against zlib)
        assert utils_image.png_crc_combine(zlib.crc32(a), zlib.crc32(b), nb) == want, (na, nb)
    # lengths no buffer holds, 2^32 and beyond: against the restatement on Python integers
    for len_b in ((1 << 32) - 1, 1 << 32, (1 << 32) + 5, (1 << 40) + 123, (1 << 63) + 1, (1 << 64) - 1):
        for ca, cb in ((0x12345678, 0x9ABCDEF0), (0xFFFFFFFF, 0), (0, 0xFFFFFFFF), (1, 1)):
            assert utils_image.png_crc_combine(ca, cb, len_b) == ref.crc_combine(ca, cb, len_b), (len_b, ca, cb)
    # ... and one such length against zlib alone: crc32(zeros(2^k)) by doubling from a block zlib checksummed
    z = zlib.crc32(bytes(1 << 24))
    for k in range(24, 33):
        if k == 26:
            assert z == zlib.crc32(bytes(1 << 26))  # (the doubling is right where zlib can still check it)
        z = utils_image.png_crc_combine(z, z, 1 << k)   # zeros(2^(k+1))
    a = b"leading bytes"  # A || zeros(2^33) == (A || zeros(2^32)) || zeros(2^32)
    z32 = zlib.crc32(bytes(1 << 24))
    for k in range(24, 32):
        z32 = utils_image.png_crc_combine(z32, z32, 1 << k)
    half = utils_image.png_crc_combine(zlib.crc32(a), z32, 1 << 32)
    assert utils_image.png_crc_combine(zlib.crc32(a), z, 1 << 33) == utils_image.png_crc_combine(half, z32, 1 << 32)


# ---- hhsr_png_workspace -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("H,W,och,bits,interval", [(40, 72, 3, 8, 300), (33, 65, 1, 16, 1 << 20)])
def test_workspace(H, W, och, bits, interval):
    n, scratch, bound = utils_image.png_workspace(H, W, och, bits, interval)
    bpp = och * bits // 8
    assert n == H * (1 + W * bpp)
    n_int = ref.n_intervals(n, interval)
    assert scratch >= max(24 * n_int + 8 * -(-n_int // 2048), 1024 * min(H, 1024))
    # a byte-uniform stream: every byte value equally often, the least compressible one for a single code
    stream = (np.arange(n) % 256).astype(np.uint8)
    np.random.default_rng(1).shuffle(stream)
    counts = np.zeros(257, np.uint64)
    counts[:256] = ref.byte_counts(stream)
    counts[256] = n_int
    d = ref.deflate(stream, interval, utils_image.png_huffman(counts))
    assert n <= len(d) <= bound
    T = n + n_int
    assert bound == -(-(8 * T + 2 * T // 257 + 1) // 8) + 468 * n_int  # the derivation of include/hhsr.h


def test_workspace_refusals():
    lib = _lib.load()
    a, b, c = C.c_size_t(0), C.c_size_t(0), C.c_size_t(0)
    ok = (8, 8, 3, 8, 4096)
    assert lib.hhsr_png_workspace(*ok, C.byref(a), C.byref(b), C.byref(c)) == 0
    bad = [(0, 8, 3, 8, 4096), (8, 0, 3, 8, 4096), (8, 8, 2, 8, 4096), (8, 8, 3, 12, 4096), (8, 8, 3, 8, 0),
           (8, 8, 3, 8, (1 << 20) + 1), (8, 8, 3, 8, -1),
           (30000, 30000, 3, 8, 4096),        # 2.7e9 stream bytes: more than one IDAT chunk holds
           (23000, 31000, 3, 8, 1)]           # the stream fits (2.14e9 bytes), its bound at 1-byte intervals does not
    for args in bad:
        assert lib.hhsr_png_workspace(*args, C.byref(a), C.byref(b), C.byref(c)) == -1, args
        assert b"invalid argument" in lib.hhsr_last_error()
    assert lib.hhsr_png_workspace(*ok, None, C.byref(b), C.byref(c)) == -1


# ---- refusals of the device entry points, without a device ------------------------------------------------------------------------
BASE = 1 << 32  # (nothing can launch without a device: any aligned address does, as in tests/test_abi.py)


def slot(k, off=0):
    return C.c_void_p(BASE + (k << 24) + off)


def test_filter_refuses_bad_arguments():
    lib = _lib.load()
    H, W = 16, 24
    n, scratch, _ = utils_image.png_workspace(H, W, 3, 8, 4096)

    def call(**kw):
        a = dict(image=slot(0), H=H, W=W, ch=3, och=3, bits=8, filter=5, filtered=slot(1), nbytes=n, counts=slot(2),
                 scratch=slot(3), scratch_bytes=scratch)
        a.update(kw)
        return lib.hhsr_png_filter(a["image"], a["H"], a["W"], a["ch"], a["och"], a["bits"], a["filter"], a["filtered"],
                                   a["nbytes"], a["counts"], a["scratch"], a["scratch_bytes"], None)

    assert call() >= 0  # valid: launches with a device, fails in the runtime without one, never -1
    bad = [dict(image=None), dict(filtered=None), dict(counts=None), dict(scratch=None), dict(H=0), dict(W=-1), dict(ch=2),
           dict(ch=1, och=3), dict(och=2), dict(bits=12), dict(filter=6), dict(filter=-1), dict(nbytes=n - 1),
           dict(scratch_bytes=16 * 1024 - 1), dict(image=slot(0, 2)),
           dict(filtered=slot(1, 8)), dict(counts=slot(2, 4)), dict(scratch=slot(3, 4)), dict(filtered=slot(0, 16)),
           dict(counts=slot(1)), dict(scratch=slot(2, 8)), dict(H=30000, W=30000)]
    for kw in bad:
        assert call(**kw) == -1 and b"invalid argument" in lib.hhsr_last_error(), kw


def test_deflate_refuses_bad_arguments():
    lib = _lib.load()
    n, interval = 5000, 300
    n_int = ref.n_intervals(n, interval)
    need = 24 * n_int + 8
    spec = utils_image.png_huffman(np.full(257, 2, np.uint64))
    spec_p = spec.ctypes.data_as(C.POINTER(C.c_uint8))

    def call(**kw):
        a = dict(filtered=slot(0), n=n, interval=interval, spec=spec_p, scratch=slot(1), scratch_bytes=need, out=slot(2, 1),
                 cap=100, result=slot(3))
        a.update(kw)
        return lib.hhsr_png_deflate(a["filtered"], a["n"], a["interval"], a["spec"], a["scratch"], a["scratch_bytes"],
                                    a["out"], a["cap"], a["result"], None)

    def broken(edit):
        s = spec.copy()
        edit(s)
        return s.ctypes.data_as(C.POINTER(C.c_uint8)), s  # (keep the array alive)

    assert call() >= 0
    specs = [broken(lambda s: s.__setitem__(0, 16)),                       # a length above 15
             broken(lambda s: s.__setitem__(0, 0)),                        # not complete any more
             broken(lambda s: s.__setitem__(256, 0)),                      # no end symbol
             broken(lambda s: s.__setitem__(257, 1)),
             broken(lambda s: s.__setitem__(slice(258, 260), (0, 0))),     # no header
             broken(lambda s: s.__setitem__(slice(258, 260), (255, 255))),
             broken(lambda s: s.__setitem__(260, s[260] | 1))]             # BFINAL set
    bad = [dict(filtered=None), dict(spec=None), dict(scratch=None), dict(out=None), dict(result=None), dict(n=0),
           dict(n=1 << 31), dict(interval=0), dict(interval=(1 << 20) + 1), dict(scratch_bytes=need - 1),
           dict(filtered=slot(0, 2)), dict(scratch=slot(1, 4)), dict(result=slot(3, 4)), dict(out=slot(0, 100)),
           dict(result=slot(2, 8)), dict(scratch=slot(0, 8)), dict(out=slot(2), cap=2 ** 64 - 1)]
    bad += [dict(spec=p) for p, _ in specs]
    for kw in bad:
        assert call(**kw) == -1 and b"invalid argument" in lib.hhsr_last_error(), kw


# ---- Python helpers -----------------------------------------------------------------------------------------------------------------
def test_png_option():
    for name in ("none", "sub", "up", "average", "paeth", "adaptive"):
        assert utils_image.png_option("filter", name) == name
    for bad in ("paeth2", "Adaptive", "", None, 5, True):
        with pytest.raises(ValueError):
            utils_image.png_option("filter", bad)
    assert utils_image.png_option("interval_bytes", None) == utils_image.PNG_INTERVAL_BYTES
    assert utils_image.png_option("interval_bytes", 1) == 1 and utils_image.png_option("interval_bytes", 1 << 20) == 1 << 20
    assert utils_image.png_option("interval_bytes", np.int64(4096)) == 4096
    assert 1 <= utils_image.PNG_INTERVAL_BYTES <= 1 << 20
    for bad in (0, -4, (1 << 20) + 1, 4096.0, "4096", True):
        with pytest.raises(ValueError):
            utils_image.png_option("interval_bytes", bad)
    with pytest.raises(ValueError):
        utils_image.png_option("quality", 3)


def test_save_png_bytes(tmp_path):
    data = np.frombuffer(ref.file_head(2, 2, 1, 8, 5) + b"12345" + ref.file_tail(b"12345", b"abc"), np.uint8)
    path = tmp_path / "a.png"
    utils_image.save_png_bytes(data, path)
    assert path.read_bytes() == data.tobytes()
    for bad in (data.astype(np.uint16), data.reshape(1, -1), data[:4], np.frombuffer(b"\xff\xd8" + bytes(20), np.uint8)):
        with pytest.raises(ValueError):
            utils_image.save_png_bytes(bad, tmp_path / "b.png")
    assert not (tmp_path / "b.png").exists()


def test_encode_png_needs_a_device_tensor():
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        utils_image.encode_png(np.zeros((4, 4, 3), np.float32))


def test_command_line_keeps_the_output_section_for_format_png():
    import importlib.util
    import os

    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    spec = importlib.util.spec_from_file_location(
        "hhsr_run_handheld", os.path.join(root, "handheld-multi-frame-super-resolution_amd", "run_handheld.py"))
    cli = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(cli)

    def cfg(outpath, *overrides):
        return cli.build_config(cli.parse_args(["--impath", "b.npz", "--outpath", outpath, *overrides]))

    out = cfg("o.png", "output.format=png", "output.dtype=uint16", "output.filter=paeth", "output.interval_bytes=4096").output
    assert (out.format, out.dtype, out.filter, out.interval_bytes) == ("png", "uint16", "paeth", 4096)
    assert cfg("o.PNG", "output.format=png").output.format == "png"
    with pytest.raises(ValueError):  # the format is PNG: another suffix contradicts it
        cfg("o.tif", "output.format=png")
    assert dict(cfg("o.png").output) == {"dtype": "uint8"} and dict(cfg("o.tif").output) == {"dtype": "uint16"}  # as before
    assert dict(cfg("o.png", "output.format=raw").output) == {"dtype": "uint8"}
