"""dng.parse_dng on the files tests/dng_ref.py writes: every layout and both byte orders come back as written, everything
out of scope is a ValueError that names the tag, and malformed containers are ValueErrors, quickly.  No GPU."""
import struct
import time

import numpy as np
import pytest

import dng_ref

CM = [[0.75, -0.25, 0.125], [-0.5, 1.25, 0.25], [0.0, -0.125, 0.875]]
NP6 = [2e-4, 1e-6, 3e-4, 2e-6, 4e-4, 3e-6]


def counts(bits, H=40, W=48, seed=0):
    return np.random.default_rng(seed).integers(0, 1 << bits, (H, W))


def parse(path):
    from handheld_super_resolution.dng import parse_dng

    return parse_dng(path)


LAYOUTS = [dict(layout="strips", size=16, bits=16), dict(layout="strips", size=7, bits=16), dict(layout="tiles", size=(16, 16), bits=16),
           dict(layout="strips", size=16, bits=10), dict(layout="strips", size=9, bits=12), dict(layout="strips", size=40, bits=14),
           dict(layout="tiles", size=(16, 16), bits=12, compression=7, ljpeg=dict(Nf=2, predictor=1)),
           dict(layout="strips", size=7, bits=14, compression=7, ljpeg=dict(predictor=6))]


@pytest.mark.parametrize("byte_order", ["II", "MM"])
@pytest.mark.parametrize("subifd", [False, True])
@pytest.mark.parametrize("k", range(len(LAYOUTS)))
def test_parse_returns_what_was_written(tmp_path, byte_order, subifd, k):
    kw = dict(LAYOUTS[k])
    c = counts(kw["bits"])
    cfa = (2, 1, 1, 0) if subifd else (1, 0, 2, 1)
    w = dng_ref.write_dng(tmp_path / "a.dng", c, byte_order=byte_order, subifd=subifd, cfa=cfa, black=(60, 61, 62, 63),
                          white=(1 << kw["bits"]) - 5, color_matrix=CM, noise_profile=NP6, iso=6400, iso_in_exif=not subifd,
                          orientation=6, **kw)
    info = parse(tmp_path / "a.dng")
    for field in ("width", "height", "bits", "compression", "layout", "byte_order", "cfa_pattern", "black_levels", "white_level",
                  "white_balance", "orientation"):
        assert getattr(info, field) == w[field], field
    assert info.iso == 3200  # clamped to 100 .. 3200 as upstream
    assert np.array_equal(info.xyz2cam, np.array(CM, np.float32)) and info.noise_profile == NP6
    assert [(s.offset, s.length) for s in info.segments] == list(zip(w["offsets"], w["lengths"]))
    assert [(s.x0, s.y0, s.seg_w, s.seg_h) for s in info.segments] == w["rects"]
    assert info.file_size == len(w["bytes"])
    # green is the green cell on the red row
    r = cfa.index(0)
    assert info.black_levels[1] == (60, 61, 62, 63)[r ^ 1]


def test_single_black_level_and_missing_optional_tags(tmp_path):
    dng_ref.write_dng(tmp_path / "a.dng", counts(16), black=[64], iso=None, neutral=None, drop=(274,))
    info = parse(tmp_path / "a.dng")
    assert info.black_levels == (64.0, 64.0, 64.0) and info.iso is None and info.white_balance is None
    assert info.orientation is None and info.xyz2cam is None and info.noise_profile is None


S, L, R = dng_ref.SHORT, dng_ref.LONG, dng_ref.RATIONAL
REFUSALS = {
    "BigTIFF": dict(big=True),
    "LinearRaw": dict(extra=[(262, S, [34892])]),
    r"Compression \(259\) 8": dict(extra=[(259, S, [8])]),
    r"Compression \(259\) 34892": dict(extra=[(259, S, [34892])]),
    r"Compression \(259\) 5": dict(extra=[(259, S, [5])]),
    "SamplesPerPixel": dict(extra=[(277, S, [3])]),
    "FillOrder": dict(extra=[(266, S, [2])]),
    "PlanarConfiguration": dict(extra=[(284, S, [2])]),
    "CFARepeatPatternDim": dict(extra=[(33421, S, [4, 4])]),
    "CFAPattern": dict(extra=[(33422, dng_ref.BYTE, [0, 1, 3, 2])]),
    "BlackLevelRepeatDim": dict(extra=[(50713, S, [1, 2])]),
    "BlackLevelDeltaH": dict(extra=[(50715, dng_ref.SRATIONAL, [0.0, 0.5, 0.0])]),
    "BlackLevelDeltaV": dict(extra=[(50716, dng_ref.SRATIONAL, [1.0])]),
    "LinearizationTable": dict(extra=[(50712, S, list(range(16)))]),
    "AsShotWhiteXY": dict(neutral=None, extra0=[(50729, R, [0.3127, 0.329])]),
    r"BitsPerSample \(258\) 8": dict(extra=[(258, S, [8])]),
    "packed 12-bit tiles": dict(bits=12, layout="tiles", size=(16, 16)),
    "no IFD with NewSubFileType": dict(extra=[(262, S, [2])]),
}


@pytest.mark.parametrize("what", list(REFUSALS))
@pytest.mark.parametrize("subifd", [False, True])
def test_refusals_name_the_tag(tmp_path, what, subifd):
    kw = dict(REFUSALS[what])
    bits = kw.pop("bits", 16)
    dng_ref.write_dng(tmp_path / "a.dng", counts(bits), bits=bits, subifd=subifd, **kw)
    with pytest.raises(ValueError, match=what):
        parse(tmp_path / "a.dng")


def test_zero_delta_tags_are_accepted(tmp_path):
    dng_ref.write_dng(tmp_path / "a.dng", counts(16), extra=[(50715, dng_ref.SRATIONAL, [0.0] * 48), (50716, dng_ref.SRATIONAL, [0.0] * 40)])
    assert parse(tmp_path / "a.dng").width == 48


def _entry_pos(data, e, ifd_off, tag):
    n = struct.unpack_from(e + "H", data, ifd_off)[0]
    for i in range(n):
        p = ifd_off + 2 + 12 * i
        if struct.unpack_from(e + "H", data, p)[0] == tag:
            return p
    raise KeyError(tag)


def malformed(tmp_path, byte_order):
    """{name: (bytes, what the ValueError names)} of containers broken in one place each."""
    e = "<" if byte_order == "II" else ">"
    w = dng_ref.write_dng(tmp_path / "good.dng", counts(16), byte_order=byte_order, size=8)
    good = bytearray(w["bytes"])
    ifd0 = struct.unpack_from(e + "I", good, 4)[0]
    n0 = struct.unpack_from(e + "H", good, ifd0)[0]
    out = {}

    def patch(name, pos, fmt, value, match):
        b = bytearray(good)
        struct.pack_into(e + fmt, b, pos, value)
        out[name] = (bytes(b), match)

    patch("first IFD behind the end", 4, "I", len(good) + 100, "outside the file")
    patch("strip offsets behind the end", _entry_pos(good, e, ifd0, 273) + 8, "I", len(good) - 4, "StripOffsets")
    patch("count that overflows", _entry_pos(good, e, ifd0, 50714) + 4, "I", 0xFFFFFFFF, "BlackLevel")
    patch("count of the strip table that overflows", _entry_pos(good, e, ifd0, 279) + 4, "I", 0x7FFFFFFF, "StripByteCounts")
    patch("IFD that points at itself", ifd0 + 2 + 12 * n0, "I", ifd0, "loop")
    patch("too many entries", ifd0, "H", 60000, "entries")
    patch("strip table shorter than the image needs", _entry_pos(good, e, ifd0, 278) + 8, "I", 4, "needs 10")
    patch("a strip behind the end", _entry_pos(good, e, ifd0, 257) + 8, "I", 4000, "needs")
    # an EXIF pointer back to IFD0
    patch("ExifIFD that points at IFD0", _entry_pos(good, e, ifd0, 34665) + 8, "I", ifd0, "loop")
    out["truncated file"] = (bytes(good[:ifd0 + 20]), "outside the file")
    out["eight bytes"] = (bytes(good[:8]), "outside the file")
    out["four bytes"] = (bytes(good[:4]), "no TIFF header")
    # the last strip's bytes run past the end of the file
    sb = _entry_pos(good, e, ifd0, 279)
    at = struct.unpack_from(e + "I", good, sb + 8)[0]
    patch("strip byte count behind the end", at + 4 * (w["n_segments"] - 1), "I", len(good), "StripOffsets")
    return out


@pytest.mark.parametrize("byte_order", ["II", "MM"])
def test_malformed_containers_are_value_errors(tmp_path, byte_order):
    for name, (data, match) in malformed(tmp_path, byte_order).items():
        p = tmp_path / "bad.dng"
        p.write_bytes(data)
        t0 = time.perf_counter()
        with pytest.raises(ValueError, match=match):
            parse(p)
        assert time.perf_counter() - t0 < 1.0, name


def test_every_truncation_and_byte_flip_of_the_ifds_is_a_value_error_or_parses(tmp_path):
    """Nothing but ValueError leaves parse_dng: no IndexError, no struct.error, whatever byte of the IFDs is changed."""
    w = dng_ref.write_dng(tmp_path / "good.dng", counts(16, 8, 8), subifd=True, size=8, color_matrix=CM, noise_profile=NP6)
    good = w["bytes"]
    p = tmp_path / "m.dng"
    first = struct.unpack_from("<I", good, 4)[0]
    lo = min(w["offsets"]) + sum(w["lengths"])  # everything behind the raw strips: value blocks and the IFDs
    t0 = time.perf_counter()
    for n in range(0, len(good), 7):
        p.write_bytes(good[:n])
        try:
            parse(p)
        except ValueError:
            pass
    for i in list(range(0, 8)) + list(range(lo, len(good))):
        for v in (0x00, 0xFF, 0x80):
            b = bytearray(good)
            b[i] = v
            p.write_bytes(bytes(b))
            try:
                parse(p)
            except ValueError:
                pass
    assert first > 0 and time.perf_counter() - t0 < 60
