"""Lossless JPEG on the host, no GPU: the test encoder pinned by an independent decoder, hhsr_ljpeg_parse and
hhsr_ljpeg_decode_host against the encoded counts bit for bit, and the decode core under sanitizers on malformed streams
(tests/ljpeg_fuzz_main.cpp, a stand-alone program)."""
import io
import os
import shutil
import subprocess

import numpy as np
import pytest

import ljpeg_cases as cases
import ljpeg_ref as ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def pillow_matrix(Nf):
    """13 x 17 samples of 8 bits with a saturated and a zero row."""
    s = np.random.default_rng(17 + Nf).integers(0, 256, (13, 17, Nf))
    s[3], s[5] = 255, 0
    return s


@pytest.mark.parametrize("Nf", [1, 3])
@pytest.mark.parametrize("predictor", range(1, 8))
def test_encoder_is_pinned_by_libjpeg(Nf, predictor):
    """The libjpeg-turbo inside Pillow opens 8-bit SOF3 streams: what ljpeg_ref.encode writes decodes there to its input.
    P > 8 and Nf = 2, which Pillow cannot open, go through the same encoder code and the round trip below."""
    from PIL import Image

    s = pillow_matrix(Nf)
    got = np.asarray(Image.open(io.BytesIO(ref.encode(s, 8, predictor)))).reshape(13, 17, Nf)
    assert (got == s).all()


@pytest.mark.parametrize("P,Nf,tables", [(8, 1, "k2"), (10, 2, "k2"), (12, 4, "k2shared"), (14, 2, "fixed"), (16, 1, "fixed"),
                                         (16, 4, "k2"), (2, 3, "k2")])
def test_encoder_round_trip(P, Nf, tables):
    rng = np.random.default_rng(P * 8 + Nf)
    for predictor in range(1, 8):
        s = rng.integers(0, 1 << P, (5, 6, Nf))
        assert (ref.decode(ref.encode(s, P, predictor, tables=tables)) == s).all()


def test_parse_returns_the_header():
    from handheld_super_resolution.dng import parse_ljpeg

    s = np.random.default_rng(3).integers(0, 1 << 12, (6, 9, 2))
    stream = ref.encode(s, 12, 6)
    h, data = ref.split(stream)
    lj = parse_ljpeg(stream)
    assert (lj.P, lj.Y, lj.X, lj.Nf, lj.predictor, lj.point_transform) == (12, 6, 9, 2, 6, 0)
    assert list(lj.table)[:2] == h["comp_table"]
    for th, (bits, values) in h["tables"].items():
        assert list(lj.bits[th]) == bits and list(lj.values[th])[:len(values)] == values and lj.n_values[th] == len(values)
    assert (lj.data_offset, lj.data_length) == (h["data_offset"], len(data))


def _patched(stream, marker, at, value):
    """The stream with the byte `at` bytes into the payload of its first `marker` segment replaced."""
    p = stream.index(bytes([0xFF, marker])) + 4 + at
    return stream[:p] + bytes([value]) + stream[p + 1:]


def test_parse_refuses_by_name():
    from handheld_super_resolution.dng import parse_ljpeg

    s = np.random.default_rng(4).integers(0, 1 << 10, (4, 6, 2))
    good = ref.encode(s, 10, 1)
    parse_ljpeg(good)
    sos_payload = 1 + 2 * 2
    cases_ = {
        "restart interval": ref.encode(s, 10, 1, restart=4),
        "point transform": _patched(good, 0xDA, sos_payload + 2, 1),
        "SOF other than SOF3": good.replace(b"\xff\xc3", b"\xff\xc1", 1),
        "precision P": _patched(good, 0xC3, 0, 17),
        "components Nf": _patched(good, 0xC3, 5, 5),
        "sampling factors": _patched(good, 0xC3, 7, 0x21),
        "table class": _patched(good, 0xC4, 0, 0x10),
        "no prefix code": _patched(good, 0xC4, 1, 3),
        "value above 16": _patched(good, 0xC4, 17, 17),
        "not present": _patched(good, 0xDA, 2, 0x30),
        "predictor": _patched(good, 0xDA, sos_payload, 8),
        "second scan": good[:-2] + b"\xff\xda" + good[-2:],
        "marker length": good[:good.index(b"\xff\xc4") + 2] + b"\xff\xff" + good[good.index(b"\xff\xc4") + 4:],
        "no SOI": b"\x00" + good[1:],
    }
    for what, stream in cases_.items():
        with pytest.raises(ValueError, match=what):
            parse_ljpeg(stream)
    for n in range(len(good) - 3):  # every truncation of the marker segments is refused, none crashes
        if n < ref.split(good)[0]["data_offset"]:
            with pytest.raises(ValueError):
                parse_ljpeg(good[:n])


def contents(P, shape, kind, rng):
    if kind == "random":
        return rng.integers(0, 1 << P, shape)
    if kind == "smooth":
        base = (np.arange(shape[0])[:, None] * 3 + np.arange(shape[1])[None, :] * 5) % (1 << P)
        return (base + rng.integers(0, 4, shape)) % (1 << P)
    raise ValueError(kind)


def one_segment(rect, P, Nf, X, predictor, tables="k2", crop=(0, 0), lead=0):
    """rect [seg_h, seg_w] coded flat as lines of X Nf samples -> decoded image [H, W] (the segment cropped by `crop`)."""
    seg_h, seg_w = rect.shape
    stream = ref.encode(ref.to_stream_geometry(rect, Nf, X), P, predictor, tables=tables)
    H, W = seg_h - crop[0], seg_w - crop[1]
    plan = cases.plan_from_streams([(stream, 0, 0, 0, seg_w, seg_h)], 1, H, W, lead=lead)
    got, status, intact = cases.decode_host(plan, row_elems=W + 3)
    assert intact and status.tolist() == [0], (status, intact)
    return got[0]


@pytest.mark.parametrize("P", [8, 10, 12, 14, 16])
@pytest.mark.parametrize("Nf", [1, 2, 4])
def test_decode_host_equals_the_encoded_counts(P, Nf):
    """Predictors 1-7 x the geometries X Nf = seg_w, 2 seg_w, seg_w / 2 and the smallest streams, random and smooth counts,
    K.2 tables and the fixed table with 16-bit codes, the segment whole and cropped by the image."""
    rng = np.random.default_rng(100 * P + Nf)
    seg_w, seg_h = 16, 6
    for predictor in range(1, 8):
        for line in (seg_w, 2 * seg_w, seg_w // 2):
            for kind, tables, crop in (("random", "k2", (0, 0)), ("smooth", "fixed", (1, 5))):
                rect = contents(P, (seg_h, seg_w), kind, rng)
                got = one_segment(rect, P, Nf, line // Nf, predictor, tables, crop)
                assert (got == rect[:seg_h - crop[0], :seg_w - crop[1]]).all(), (predictor, line, kind)
        small = max(2, Nf)  # X Nf = 2 (Nf = 4: one sample of each component), Y = 1 and 2
        for Y in (1, 2):
            rect = contents(P, (Y, small), "random", rng)
            assert (one_segment(rect, P, Nf, small // Nf, predictor) == rect).all(), (predictor, Y)


def test_difference_32768_and_wrap():
    """P = 16, values alternating 0 and 65535: differences of 32768 do not occur here but +-65535 wrap modulo 2^16 to -+1;
    alternating 0 and 32768 gives SSSS = 16, which carries no extra bits."""
    for lo, hi in ((0, 65535), (0, 32768), (32767, 65535)):
        rect = np.zeros((4, 16), np.int64) + lo
        rect[:, ::2] = hi
        rect[1::2] = rect[1::2, ::-1]
        d, ssss = ref.categories(ref.to_stream_geometry(rect, 1, 16), 16, 1)
        if (lo, hi) == (0, 32768):
            assert (ssss == 16).any()
        for predictor in range(1, 8):
            for tables in ("k2", "fixed"):
                assert (one_segment(rect, 16, 1, 16, predictor, tables) == rect).all()


def test_long_zero_run():
    rect = np.zeros((8, 64), np.int64)
    rect[0, 0] = 1 << 11  # the initial prediction: every difference is 0
    for Nf, predictor in ((1, 1), (2, 4), (4, 7)):
        got = one_segment(rect, 12, Nf, 64 // Nf, predictor)
        assert (got == rect).all()
    flat = np.full((8, 64), 777, np.int64)
    assert (one_segment(flat, 10, 2, 32, 1) == flat).all()


def test_ff_bytes_at_every_refill_position():
    """A sawtooth of +255 per sample at P = 16 codes every sample as `0 11111111`: nine bits, so the run of ones moves through
    every bit and byte alignment and the data holds stuffed FF bytes at every position modulo 8 (the reader refills byte by
    byte from aligned dwords, so positions modulo 4 and 8 are its cases)."""
    n = 16 * 40
    rect = ((32768 + 255 * (1 + np.arange(n))) % 65536).reshape(40, 16)
    stream = ref.encode(ref.to_stream_geometry(rect, 1, 16 * 40), 16, 1)
    h, data = ref.split(stream)
    ff = [i for i in range(len(data) - 1) if data[i] == 0xFF and data[i + 1] == 0x00]
    assert {i % 8 for i in ff} == {0, 2, 4, 6}  # (ten stuffed bytes per nine samples: the blob offsets below give the odd ones)
    assert {(lead + i) % 8 for i in ff for lead in range(4)} == set(range(8))
    for lead in range(4):
        plan = cases.plan_from_streams([(stream, 0, 0, 0, 16, 40)], 1, 40, 16, lead=lead)
        got, status, intact = cases.decode_host(plan)
        assert intact and status.tolist() == [0] and (got[0] == rect).all(), lead


def test_blob_offsets_and_end():
    """A stream beginning at each byte offset 0..3 of the blob and ending at the blob's last byte."""
    rng = np.random.default_rng(9)
    done = set()
    for trial in range(64):
        rect = rng.integers(0, 1 << 10, (5, 12))
        stream = ref.encode(ref.to_stream_geometry(rect, 2, 6), 10, 1 + trial % 7)
        n = len(ref.split(stream)[1])
        lead = (-n) % 4  # so that lead + n is a multiple of 4: the stream ends with the blob
        if lead in done:
            continue
        plan = cases.plan_from_streams([(stream, 0, 0, 0, 12, 5)], 1, 5, 12, lead=lead)
        assert plan.blob.size == lead + n
        got, status, intact = cases.decode_host(plan)
        assert intact and status.tolist() == [0] and (got[0] == rect).all(), lead
        done.add(lead)
    assert done == {0, 1, 2, 3}


def test_argument_errors():
    from handheld_super_resolution import _lib

    lib = _lib.load()
    rect = np.arange(32).reshape(2, 16)
    plan = cases.plan_from_streams([(ref.encode(ref.to_stream_geometry(rect, 1, 16), 8, 1), 0, 0, 0, 16, 2)], 1, 2, 16)
    import ctypes

    out, work, st = np.zeros(64, np.uint16), np.zeros(64, np.uint16), np.zeros(1, np.int32)

    def call(blob_bytes=plan.blob.size, row=16, frame=32, blob_off=0):
        return lib.hhsr_ljpeg_decode_host(plan.blob.ctypes.data + blob_off, blob_bytes, ctypes.addressof(plan.segments), 1,
                                          ctypes.addressof(plan.tables), len(plan.tables), work.ctypes.data, 128,
                                          out.ctypes.data, 1, 2, 16, row, frame, st.ctypes.data)

    assert call() == 0 and (out[:32].reshape(2, 16) == rect).all()
    for kwargs in (dict(blob_bytes=plan.blob.size - 1), dict(row=15), dict(frame=31), dict(blob_off=1)):
        assert call(**kwargs) == -1 and b"invalid argument" in lib.hhsr_last_error(), kwargs
    # a descriptor the decoder refuses: status BAD_SEGMENT, nothing written
    plan.segments[0].table[0] = 5
    out[:] = 7
    assert call() == 0 and st[0] == _lib.LJPEG_BAD_SEGMENT and (out == 7).all()


@pytest.fixture(scope="module")
def fuzz_streams(tmp_path_factory):
    """Three small valid streams and their samples, as files."""
    d = tmp_path_factory.mktemp("ljpeg_fuzz")
    rng = np.random.default_rng(11)
    args = []
    for i, (P, Nf, X, Y, predictor, tables) in enumerate([(10, 2, 8, 6, 1, "k2"), (16, 1, 12, 5, 6, "fixed"),
                                                          (12, 4, 3, 7, 7, "k2shared")]):
        s = rng.integers(0, 1 << P, (Y, X, Nf))
        sp, ep = d / f"s{i}.ljpg", d / f"s{i}.u16"
        sp.write_bytes(ref.encode(s, P, predictor, tables=tables))
        ep.write_bytes(s.astype("<u2").tobytes())
        args += [str(sp), str(ep)]
    return args


def _clangxx():
    for c in ("/opt/rocm/lib/llvm/bin/clang++", shutil.which("clang++")):
        if c and os.path.exists(c):
            return c
    return None


@pytest.mark.timeout(600)
def test_malformed_streams_under_sanitizers(fuzz_streams, tmp_path):
    """tests/ljpeg_fuzz_main.cpp with -fsanitize=address,undefined, run as an ordinary child process: every mutant returns,
    every status is documented, the guards are intact and the sanitizers are silent."""
    cxx = _clangxx()
    if cxx is None:
        pytest.skip("no clang++")
    exe = str(tmp_path / "ljpeg_fuzz")
    r = subprocess.run([cxx, "-std=c++17", "-O1", "-g", "-Wall", "-Werror", "-fsanitize=address,undefined",
                        "-fno-sanitize-recover=all", "-fno-omit-frame-pointer", os.path.join(ROOT, "tests", "ljpeg_fuzz_main.cpp"),
                        "-o", exe], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-3000:]
    r = subprocess.run([exe, *fuzz_streams], capture_output=True, text=True, timeout=500)
    assert r.returncode == 0 and "guards intact" in r.stdout, r.stdout + r.stderr[-3000:]
    assert "Sanitizer" not in r.stderr and "runtime error" not in r.stderr, r.stderr[-3000:]
