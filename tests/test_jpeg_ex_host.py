"""Extended JPEG output without a GPU: hhsr_jpeg_header_ex / hhsr_jpeg_workspace_ex and hhsr_jpeg_huffman against the
restatement tests/jpeg_ex_ref.py, the restated 4:2:0 / optimised files in Pillow (libjpeg), every argument refusal of the new
entry points, and the table code under AddressSanitizer and UBSan in a stand-alone program.  Only host-only entry points
are ever called with valid arguments here."""
import ctypes
import functools
import io
import os
import shutil
import subprocess

import numpy as np
import pytest

import jpeg_ex_ref as ex
import jpeg_ref as ref

from handheld_super_resolution import _lib, utils_image

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
P, SZ = ctypes.c_void_p, ctypes.c_size_t
SHAPES = [(1, 1), (8, 8), (16, 16), (17, 33), (9, 17), (3, 64), (40, 72), (136, 264)]
SETTINGS = [(50, 1), (90, 4), (100, 65535)]  # (quality, restart interval)
KINDS = ["random", "smooth", "constant", "wild"]
# Pillow's 4:2:0 decode against ex.decode_420 of the same coefficients: measured 3 levels over SHAPES x KINDS x SETTINGS (the
# integer IDCT is within 1 level per Y / Cb / Cr sample, the colour conversion amplifies that); asserted: measured + 1, the
# convention of B_RGB in tests/test_jpeg_host.py.
B_420 = 3 + 1


def ids(s):
    return "%dx%d" % s


@functools.lru_cache(maxsize=None)
def restated(shape, kind, quality, sub):
    """int16 coefficients of the restated encoder, RGB — computed once, read-only."""
    img = ref.test_images(shape[0], shape[1], 3, seed=shape[0] * 7 + shape[1] + 3)[kind]
    coef = ex.coefficients(img, quality, sub)
    coef.setflags(write=False)
    return coef


@functools.lru_cache(maxsize=None)
def restated_counts(shape, kind, quality, ri, sub):
    return ex.histogram(restated(shape, kind, quality, sub), ri, sub)


def fibonacci_counts(n, first=0):
    """Counts 1, 1, 2, 3, 5, .. on symbols first .. first + n - 1: the most skewed code a sum of that size can make."""
    c = np.zeros(256, np.uint64)
    a, b = 1, 1
    for s in range(first, first + n):
        c[s] = a
        a, b = b, a + b
    return c


def all_symbols_fibonacci():
    """Counts whose K.2 code exceeds 16 bits and that cover all 12 DC categories / all 162 AC symbols of baseline: four
    tables of Fibonacci-like counts (the rarest symbols double every second step so that 162 of them stay below 2^63)."""
    ac_syms = ref.AC_LUMA[1]
    tabs = []
    for syms, step in ((range(12), 1), (ac_syms, 3)):
        c = np.zeros(256, np.uint64)
        a, b = 1, 1
        for k, s in enumerate(syms):
            c[s] = a
            if k % step == 0:
                a, b = b, a + b
        tabs.append(c)
    return np.stack([tabs[0], tabs[1], tabs[0], tabs[1]])


def huffman_inputs():
    """{name: counts[256]} — the inputs of CPU test 2 and of the sanitiser run."""
    out = {}
    for shape in ((17, 33), (40, 72)):
        for kind in KINDS:
            for (q, ri) in SETTINGS:
                c = restated_counts(shape, kind, q, ri, 1)
                for t in range(4):
                    out[f"{ids(shape)} {kind} q{q} ri{ri} table {t}"] = c[t]
    one = np.zeros(256, np.uint64); one[7] = 5
    two = np.zeros(256, np.uint64); two[3] = two[200] = 9
    big = np.zeros(256, np.uint64); big[::5] = (1 << 40) + np.arange(52, dtype=np.uint64); big[1] = 1
    out.update({"single symbol": one, "two equal": two, "all 256 once": np.ones(256, np.uint64), "near 2^40": big,
                "fibonacci 24": fibonacci_counts(24), "fibonacci 40 from 100": fibonacci_counts(40, 100),
                "all AC symbols": all_symbols_fibonacci()[1], "all DC symbols": all_symbols_fibonacci()[0]})
    return out


def lib_huffman(counts):
    """hhsr_jpeg_huffman of ONE table's counts (as table 0 of two; the other gets a single symbol) -> (bits, vals)."""
    other = np.zeros(256, np.uint64)
    other[0] = 1
    spec = utils_image.jpeg_huffman(np.stack([np.asarray(counts, np.uint64), other]))
    bits = spec[0, :16].tolist()
    assert not spec[0, 16 + sum(bits):].any()  # zero-filled
    return bits, spec[0, 16:16 + sum(bits)].tolist()


def check_table(counts, bits, vals):
    """The properties of CPU test 2."""
    codes = ref.huff_codes((bits, vals))
    assert all(1 <= ln <= 16 for _, ln in codes.values())
    assert all(code != (1 << ln) - 1 for code, ln in codes.values()), "a code is all 1-bits"
    assert sorted(vals) == [s for s in range(256) if int(counts[s])], "exactly the counted symbols"
    assert len(set(vals)) == len(vals)


# ---- 1. header and workspace ------------------------------------------------------------------------------------------------
def handmade_specs(components):
    c = all_symbols_fibonacci()
    return [ex.huffman(c[t]) for t in range(2 if components == 1 else 4)]


@pytest.mark.parametrize("sub", [0, 1])
def test_header_ex_and_workspace_ex_match_the_restatement(sub):
    for components in ((3,) if sub else (1, 3)):
        for specs in (None, handmade_specs(components)):
            arr = None if specs is None else ex.spec_array(specs)
            for (H, W), ri, q in (((1, 1), 1, 50), ((9, 17), 3, 90), ((40, 72), 4, 100), ((40, 72), 65535, 1),
                                  ((65535, 65535), 65535, 75), ((65535, 65535), 1, 75)):
                want = ex.header(H, W, components, q, ri, sub, specs)
                got = utils_image.jpeg_header_ex(H, W, components, q, ri, sub, arr)
                assert got.tobytes() == want, (H, W, ri, components, specs is None)
                assert ex.sof_factors(got)[0][1] == (0x22 if sub else 0x11)
                cb, sb, ms = utils_image.jpeg_workspace_ex(H, W, components, ri, sub)
                wcb, went, whist, wms = ex.workspace(H, W, components, ri, sub)
                assert (cb, sb, ms) == (wcb, max(went, whist), wms), (H, W, ri)
                if sub == 0 and specs is None:  # (.., 0, NULL) is the old function
                    assert got.tobytes() == utils_image.jpeg_header(H, W, components, q, ri).tobytes() == ref.header(H, W, components, q, ri)
                    ocb, osb, oms = utils_image.jpeg_workspace(H, W, components, ri)
                    assert (ocb, oms) == (cb, ms) and osb == went and ms == ref.max_scan_bytes(H, W, components, ri)
    if sub:
        assert utils_image.jpeg_workspace_ex(40, 72, 3, 4, 1)[0] == 768 * 3 * 5


def test_pillow_420_file_has_our_sampling_factors():
    Image = pytest.importorskip("PIL.Image")
    b = io.BytesIO()
    Image.fromarray(np.zeros((16, 16, 3), np.uint8)).save(b, "JPEG", quality=90, subsampling=2)
    ours = utils_image.jpeg_header_ex(16, 16, 3, 90, 1, 1)
    assert ex.sof_factors(b.getvalue()) == ex.sof_factors(ours) == [(1, 0x22, 0), (2, 0x11, 1), (3, 0x11, 1)]


# ---- 2. hhsr_jpeg_huffman -------------------------------------------------------------------------------------------------------
def test_huffman_equals_the_restated_k2():
    limited = 0
    for name, counts in huffman_inputs().items():
        want = ex.huffman(counts)
        got = lib_huffman(counts)
        assert got == (list(want[0]), list(want[1])), name
        check_table(counts, *got)
        limited += max(ex.code_lengths(counts).values()) > 16
    # (equal sums make K.2 pair the Fibonacci numbers up: 24 of them reach 13 bits, 40 reach 21)
    assert max(ex.code_lengths(fibonacci_counts(40, 100)).values()) > 16, "the Fibonacci counts no longer exceed 16 bits"
    assert max(ex.code_lengths(all_symbols_fibonacci()[1]).values()) > 16
    assert limited >= 2
    bits, vals = lib_huffman(huffman_inputs()["two equal"])
    assert (bits[:2], vals) == ([1, 1], [3, 200])  # the tie went to the larger index: 200 is merged first, the longer code


def test_huffman_refuses_all_zero_counts():
    lib = _lib.load()
    ok = np.zeros((4, 256), np.uint64)
    ok[:, 1] = 1
    spec = np.full((4, 272), 0xA5, np.uint8)
    u64, u8 = ctypes.POINTER(ctypes.c_uint64), ctypes.POINTER(ctypes.c_uint8)
    for t in range(4):
        bad = ok.copy()
        bad[t] = 0
        assert lib.hhsr_jpeg_huffman(bad.ctypes.data_as(u64), 4, spec.ctypes.data_as(u8)) == -1
        assert b"invalid argument" in lib.hhsr_last_error() and (spec == 0xA5).all()  # nothing written
    over = ok.copy()
    over[2, 5] = over[2, 6] = 1 << 63  # the sum does not fit 64 bits
    assert lib.hhsr_jpeg_huffman(over.ctypes.data_as(u64), 4, spec.ctypes.data_as(u8)) == -1
    for n in (0, 1, 3, 5):
        assert lib.hhsr_jpeg_huffman(ok.ctypes.data_as(u64), n, spec.ctypes.data_as(u8)) == -1
    assert lib.hhsr_jpeg_huffman(None, 4, spec.ctypes.data_as(u8)) == -1
    assert lib.hhsr_jpeg_huffman(ok.ctypes.data_as(u64), 4, None) == -1
    assert lib.hhsr_jpeg_huffman(ctypes.cast(ok.ctypes.data + 4, u64), 2, spec.ctypes.data_as(u8)) == -1   # misaligned
    assert lib.hhsr_jpeg_huffman(ok.ctypes.data_as(u64), 4, ctypes.cast(ok.ctypes.data + 64, u8)) == -1    # overlap
    assert lib.hhsr_jpeg_huffman(ok.ctypes.data_as(u64), 4, spec.ctypes.data_as(u8)) == 0 and spec[0, 0] == 1


# ---- 3. restated files in Pillow ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape", SHAPES, ids=ids)
def test_restated_420_and_optimised_files_open_in_pillow(shape):
    Image = pytest.importorskip("PIL.Image")
    H, W = shape
    worst = 0
    for kind in KINDS:
        for quality, ri in SETTINGS:
            coef = restated(shape, kind, quality, 1)
            symbols = ex.block_symbols(coef, ri, 1)
            specs = ex.huffman_specs(ex.histogram(coef, ri, 1, symbols), 3)
            std = ex.scan_bytes(coef, ri, 1, None, symbols)
            opt = ex.scan_bytes(coef, ri, 1, specs, symbols)
            assert len(opt) <= len(std), (kind, quality, ri)
            images = []
            for s, scan in ((None, std), (specs, opt)):
                data = ex.header(H, W, 3, quality, ri, 1, s) + scan + b"\xFF\xD9"
                im = Image.open(io.BytesIO(data))
                im.load()
                assert im.size == (W, H) and im.mode == "RGB"
                images.append(np.asarray(im))
            assert np.array_equal(images[0], images[1]), "the optimised file decodes to other pixels"
            d = np.abs(images[0].astype(int) - ex.decode_420(coef, H, W, quality).astype(int)).max()
            worst = max(worst, int(d))
    print(f"Pillow vs restated 4:2:0 decode, {H}x{W}: max {worst}")
    assert worst <= B_420


def test_restated_444_optimised_file_decodes_like_the_standard_one():
    Image = pytest.importorskip("PIL.Image")
    for components in (1, 3):
        img = ref.test_images(40, 72, components, seed=9)["smooth"]
        coef = ref.coefficients(img, 90)
        specs = ex.huffman_specs(ex.histogram(coef, 4), components)
        opt = ex.file_bytes(coef, 40, 72, 90, 4, 0, specs)
        std = ref.file_bytes(coef, 40, 72, 90, 4)
        assert ex.file_bytes(coef, 40, 72, 90, 4) == std and len(opt) < len(std)
        assert np.array_equal(np.asarray(Image.open(io.BytesIO(opt))), np.asarray(Image.open(io.BytesIO(std))))


# ---- 4. refusals ------------------------------------------------------------------------------------------------------------------
def test_argument_refusals_of_the_new_entry_points_do_not_touch_the_gpu():
    """-1 and "invalid argument" before any HIP call; the device pointers are arbitrary aligned addresses."""
    lib = _lib.load()
    H, W, A = 40, 72, 1 << 32
    coef_bytes, scratch_bytes, _ = utils_image.jpeg_workspace_ex(H, W, 3, 4, 1)
    _, entropy_bytes, hist_bytes, _ = ex.workspace(H, W, 3, 4, 1)
    assert coef_bytes == 15 * 768 and scratch_bytes == hist_bytes > entropy_bytes
    buf, n = (ctypes.c_uint8 * 2048)(), SZ(0)
    a, b, c = SZ(0), SZ(0), SZ(0)
    img, coef, scratch, scan, length, counts = (A + (k << 24) for k in range(6))
    cap = 1 << 20
    u8 = ctypes.POINTER(ctypes.c_uint8)
    good = ex.spec_array(ex.STANDARD)

    def broken(row, edit):
        s = good.copy()
        edit(s[row])
        return s

    def dup(r): r[17] = r[16]
    def kraft(r): r[0] = 3            # three codes of length 1
    def ones(r): r[:16] = 0; r[0] = 2  # both codes of length 1: one is all 1-bits
    def empty(r): r[:16] = 0
    def dc12(r): r[16] = 12
    bad_specs = [broken(0, dup), broken(1, kraft), broken(2, ones), broken(3, empty), broken(2, dc12)]

    def sp(s):
        return None if s is None else s.ctypes.data_as(u8)

    def header(H=H, W=W, ch=3, q=90, ri=4, sub=1, spec=None, out=buf, cap=2048, n=ctypes.byref(n)):
        return lib.hhsr_jpeg_header_ex(H, W, ch, q, ri, sub, sp(spec), out, cap, n)

    def workspace(H=H, W=W, ch=3, ri=4, sub=1, a=ctypes.byref(a), b=ctypes.byref(b), c=ctypes.byref(c)):
        return lib.hhsr_jpeg_workspace_ex(H, W, ch, ri, sub, a, b, c)

    def dct(img=img, H=H, W=W, ch=3, och=3, q=90, sub=1, coef=coef, nbytes=coef_bytes):
        return lib.hhsr_jpeg_dct_ex(P(img), H, W, ch, och, q, sub, P(coef), nbytes, None)

    def hist(coef=coef, H=H, W=W, och=3, sub=1, ri=4, counts=counts, scratch=scratch, sbytes=hist_bytes):
        return lib.hhsr_jpeg_histogram(P(coef), H, W, och, sub, ri, P(counts), P(scratch), sbytes, None)

    def entropy(coef=coef, H=H, W=W, och=3, ri=4, sub=1, spec=None, scratch=scratch, sbytes=entropy_bytes, scan=scan, cap=cap,
                length=length):
        return lib.hhsr_jpeg_entropy_ex(P(coef), H, W, och, ri, sub, sp(spec), P(scratch), sbytes, P(scan), cap, P(length), None)

    sizes = [dict(H=0), dict(W=0), dict(H=-8), dict(H=65536), dict(W=65536)]
    restarts = [dict(ri=0), dict(ri=-1), dict(ri=65536)]
    qualities = [dict(q=0), dict(q=101), dict(q=-5)]
    subs = [dict(sub=2), dict(sub=-1), dict(sub=1, och=1)]
    specs = [dict(spec=s) for s in bad_specs]
    cases = {
        header: sizes + restarts + qualities + specs + [dict(sub=2), dict(sub=-1), dict(sub=1, ch=1), dict(ch=0), dict(ch=2),
                                                        dict(out=None), dict(n=None), dict(cap=0), dict(cap=628)],
        workspace: sizes + restarts + [dict(sub=2), dict(sub=-1), dict(sub=1, ch=1), dict(ch=2), dict(a=None), dict(b=None),
                                       dict(c=None)],
        dct: sizes + qualities + subs + [
            dict(img=None), dict(coef=None), dict(ch=2), dict(ch=1, och=3), dict(och=2), dict(ch=1, och=1),  # (grey 4:2:0)
            dict(img=img + 2), dict(coef=coef + 8),                                      # misaligned
            dict(nbytes=coef_bytes - 1), dict(nbytes=0),  # workspace too small
            dict(coef=img), dict(coef=img + H * W * 12 - 16), dict(img=coef + coef_bytes - 4)],  # overlap
        hist: sizes + restarts + subs + [
            dict(coef=None), dict(counts=None), dict(scratch=None), dict(och=2),
            dict(coef=coef + 8), dict(scratch=scratch + 4), dict(counts=counts + 4),     # misaligned
            dict(sbytes=hist_bytes - 1), dict(sbytes=entropy_bytes), dict(sbytes=0),     # workspace too small
            dict(counts=coef + 16), dict(scratch=coef), dict(counts=scratch + hist_bytes - 8),
            dict(scratch=counts + 8184)],                                                # overlap, each pair
        entropy: sizes + restarts + subs + specs + [
            dict(coef=None), dict(scratch=None), dict(scan=None), dict(length=None), dict(och=2), dict(och=0),
            dict(coef=coef + 8), dict(scratch=scratch + 4), dict(length=length + 4),     # misaligned
            dict(sbytes=entropy_bytes - 1), dict(sbytes=0),                              # workspace too small
            dict(scan=coef), dict(scan=coef + coef_bytes - 1), dict(scan=scratch + 8), dict(scratch=coef),
            dict(length=coef + 16), dict(length=scratch + 8), dict(length=scan + 8), dict(length=scan + cap - 8),
            dict(scan=length - cap + 1)],                                                # overlap, each pair
    }
    missed = []
    for call, bad in cases.items():
        for kw in bad:
            rc = call(**kw)
            if not (rc == -1 and b"invalid argument" in lib.hhsr_last_error()):
                missed.append((call.__name__, {k: (v if not isinstance(v, np.ndarray) else "spec") for k, v in kw.items()}, rc,
                               lib.hhsr_last_error()))
    assert not missed, missed
    assert header() == 0 and workspace() == 0 and header(spec=good) == 0  # the host-only calls with everything valid
    assert lib.hhsr_jpeg_header_ex(16, 32, 3, 90, 1, 1, None, buf, 100, ctypes.byref(n)) == -1 and n.value == 629


def test_encode_jpeg_refuses_options_without_a_gpu():
    for name, bad in (("subsampling", "422"), ("subsampling", 0), ("subsampling", None), ("huffman", "optimised"),
                      ("huffman", True), ("subsampling", 4.2)):
        with pytest.raises(ValueError):
            utils_image.jpeg_option(name, bad)
    assert utils_image.jpeg_option("subsampling", 420) == "420" and utils_image.jpeg_option("subsampling", "444") == "444"
    assert utils_image.jpeg_option("huffman", "optimized") == "optimized"
    with pytest.raises(RuntimeError, match="GPU"):
        utils_image.encode_jpeg(np.zeros((8, 8, 3), np.float32), subsampling="420", huffman="optimized")


# ---- 5. the table code under sanitisers -----------------------------------------------------------------------------------------
def test_table_code_under_address_and_ub_sanitizers(tmp_path):
    """csrc/hhsr_jpeg_tables.h compiles without HIP; tests/jpeg_tables_driver.cpp runs it as a program of its own on the
    inputs of test 2 and on headers with hand-made tables, every buffer an exact-length heap allocation."""
    if shutil.which("g++") is None:
        pytest.skip("g++ not available")
    exe = str(tmp_path / "jpeg_tables_driver")
    csrc = os.path.join(ROOT, "handheld-multi-frame-super-resolution_amd", "csrc")
    r = subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-Wall", "-Werror", "-fsanitize=address,undefined",
                        "-fno-sanitize-recover=all", "-static-libasan", "-static-libubsan", "-I" + csrc, os.path.join(ROOT, "tests", "jpeg_tables_driver.cpp"),
                        "-o", exe], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    inputs = huffman_inputs()
    inputs["all zero"] = np.zeros(256, np.uint64)
    lines, want = [], []
    for name, counts in inputs.items():
        lines.append("huffman " + " ".join(str(int(c)) for c in counts))
        spec = ex.huffman(counts)
        want.append("refused" if spec is None else "spec " + ex.spec_array([spec]).tobytes().hex())
    for components, sub in ((1, 0), (3, 0), (3, 1)):
        for specs in (None, handmade_specs(components)):
            for (H, W), ri in (((1, 1), 1), (((40, 72), 4)), ((65535, 65535), 65535)):
                hexspec = "-" if specs is None else ex.spec_array(specs).tobytes().hex()
                lines.append(f"header {H} {W} {components} 90 {ri} {sub} {hexspec}")
                used = specs if specs is not None else ex.STANDARD[:2 if components == 1 else 4]
                want.append(f"codes {sum(len(v) for _, v in used)} header " + ex.header(H, W, components, 90, ri, sub, specs).hex())
    r = subprocess.run([exe], input="\n".join(lines) + "\n", capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and "Sanitizer" not in r.stderr and "runtime error" not in r.stderr, r.stderr[-3000:]
    got = r.stdout.split("\n")[:-1]
    assert len(got) == len(want)
    for name, g, w in zip(list(inputs) + ["header"] * 99, got, want):
        assert g == w, name
