"""dng.parse_dng(path, linearization=True): LinearizationTable, BlackLevelDeltaH / V and the GainMap opcodes of OpcodeList2
come back as written, every refusal names its tag, opcode or field, the same files through plain parse_dng(path) still raise
today's messages; config.dng.linearization; and the sanity of the NumPy restatement the GPU tests compare with.  No GPU."""
import numpy as np
import pytest

import dng_ref
import dng_linearize_ref as R
from dng_ref import LONG, SHORT, SRATIONAL

H, W = 40, 48
RNG = np.random.default_rng(50712)
DH = (RNG.integers(-16, 17, W) / 8.0).tolist()  # multiples of 1 / 8: exact as the rationals dng_ref writes
DV = (RNG.integers(-16, 17, H) / 8.0).tolist()


def counts():
    return np.random.default_rng(7).integers(0, 1 << 16, (H, W))


def four_maps(pv=3, ph=4, skip=()):
    rng = np.random.default_rng(9)
    return [R.make_map(1 + rng.random((pv, ph)), origin=(0.0, 0.0), spacing=(1 / (pv - 1), 1 / (ph - 1)), top=k // 2, left=k % 2)
            for k in range(4) if k not in skip]


def write(path, maps=None, opcodes=None, extra=(), **kw):
    extra = list(extra)
    if opcodes is None and maps is not None:
        opcodes = [R.gain_map_opcode(m) for m in maps]
    if opcodes is not None:
        extra.append(R.opcode_list_entry(opcodes))
    return dng_ref.write_dng(path, counts(), extra=extra, **kw)


def same_maps(got, want):
    assert len(got) == len(want)
    for g, m in zip(got, want):
        assert (g.top, g.left, g.row_pitch, g.col_pitch, g.points_v, g.points_h) == (
            m["top"], m["left"], m["row_pitch"], m["col_pitch"], m["points_v"], m["points_h"])
        assert (g.spacing_v, g.spacing_h, g.origin_v, g.origin_h) == (m["spacing_v"], m["spacing_h"], m["origin_v"], m["origin_h"])
        assert (g.bottom, g.right, g.plane, g.planes, g.map_planes) == (m["bottom"], m["right"], 0, 1, 1)
        assert g.gains.dtype == np.float32 and np.array_equal(g.gains, m["gains"])


@pytest.mark.parametrize("byte_order", ["II", "MM"])
@pytest.mark.parametrize("subifd", [False, True])
def test_everything_comes_back_as_written(tmp_path, byte_order, subifd):
    from handheld_super_resolution import dng

    table = np.random.default_rng(3).integers(0, 1 << 16, 16).tolist()
    maps = four_maps()
    p = tmp_path / "a.dng"
    write(p, maps, extra=[(50712, SHORT, table), (50715, SRATIONAL, DH), (50716, SRATIONAL, DV), (50829, LONG, [0, 0, H, W])],
          byte_order=byte_order, subifd=subifd)
    for undefined in (False, True):
        if undefined:
            R.retype_undefined(p, byte_order)
        info = dng.parse_dng(p, linearization=True)
        assert info.byte_order == byte_order and (info.width, info.height) == (W, H)
        assert info.linearization_table.dtype == np.uint16 and info.linearization_table.tolist() == table
        assert info.black_delta_h.dtype == np.float32 and info.black_delta_h.tolist() == DH
        assert info.black_delta_v.dtype == np.float32 and info.black_delta_v.tolist() == DV
        same_maps(info.gain_maps, maps)
    # today's reader refuses the same file by the first of the tags it meets
    with pytest.raises(ValueError, match=r"BlackLevelDeltaH \(50715\) with a non-zero entry is not applied"):
        dng.parse_dng(p)


@pytest.mark.parametrize("entries", [1, 16, 65536])
def test_table_lengths(tmp_path, entries):
    from handheld_super_resolution import dng

    table = np.random.default_rng(entries).integers(0, 1 << 16, entries).tolist()
    p = tmp_path / "a.dng"
    write(p, extra=[(50712, SHORT, table)])
    info = dng.parse_dng(p, linearization=True)
    assert info.linearization_table.tolist() == table
    assert info.black_delta_h is None and info.black_delta_v is None and info.gain_maps is None
    with pytest.raises(ValueError, match=r"LinearizationTable \(50712\) is not applied"):
        dng.parse_dng(p)


def test_map_geometries_and_skipped_opcodes(tmp_path):
    from handheld_super_resolution import dng

    p = tmp_path / "a.dng"
    one = [R.make_map(1 + np.random.default_rng(1).random((5, 2)), origin=(0.1, 0.2), spacing=(0.2, 0.6), pitch=1, bottom=H, right=W)]
    write(p, one)
    same_maps(dng.parse_dng(p, linearization=True).gain_maps, one)
    assert dng.parse_dng(p).gain_maps is None  # ignored without the keyword, as today
    three = four_maps(skip=(2,))
    write(p, three)
    same_maps(dng.parse_dng(p, linearization=True).gain_maps, three)
    # a single point needs no spacing; an optional unknown opcode before and behind the maps is skipped
    flat = [R.make_map([[1.5]], spacing=(0.0, -1.0), top=1, left=0)]
    write(p, opcodes=[R.opcode(4, b"\1\2\3\4\5\6", flags=1), R.gain_map_opcode(flat[0]), R.opcode(13, b"", flags=3)])
    same_maps(dng.parse_dng(p, linearization=True).gain_maps, flat)
    # all-zero deltas are None, and an empty list has no map
    write(p, opcodes=[], extra=[(50715, SRATIONAL, [0.0] * W), (50716, SRATIONAL, [0.0] * H)])
    info = dng.parse_dng(p, linearization=True)
    assert info.black_delta_h is None and info.black_delta_v is None and info.gain_maps is None
    # OpcodeList1 / OpcodeList3 stay ignored whatever they hold
    write(p, extra=[(51008, dng_ref.BYTE, [9, 9, 9]), (51022, dng_ref.BYTE, [1])])
    assert dng.parse_dng(p, linearization=True).gain_maps is None
    # plain records keep working: the new fields default to None
    assert dng.DngInfo(*range(18)).gain_maps is None


def _m(**kw):
    m = four_maps()[0]
    m.update(kw)
    return m


REFUSALS = {
    "table type": (dict(extra=[(50712, LONG, [1, 2, 3])]), r"LinearizationTable \(50712\) has field type 4"),
    "delta h count": (dict(extra=[(50715, SRATIONAL, DH[:-1])]), r"BlackLevelDeltaH \(50715\) has 47 entries"),
    "delta v count": (dict(extra=[(50716, SRATIONAL, DV + [0.5])]), r"BlackLevelDeltaV \(50716\) has 41 entries"),
    "zero delta count": (dict(extra=[(50715, SRATIONAL, [0.0] * 3)]), r"BlackLevelDeltaH \(50715\) has 3 entries"),
    "list type": (dict(extra=[(51009, SHORT, [0, 0])]), r"OpcodeList2 \(51009\) has field type 3"),
    "no count": (dict(extra=[(51009, dng_ref.BYTE, [0, 0])]), r"OpcodeList2 \(51009\) is truncated: the opcode count"),
    "count beyond the list": (dict(extra=[R.opcode_list_entry([R.gain_map_opcode(_m())], count=2)]),
                              r"OpcodeList2 \(51009\) is truncated: the header of opcode 1"),
    "cut in the gains": (dict(extra=[R.opcode_list_entry([R.gain_map_opcode(_m())], cut=4 + 16 + 76 + 8)]),
                         r"OpcodeList2 \(51009\) is truncated: the parameters of opcode 0 \(OpcodeID 9\)"),
    "cut in a header": (dict(extra=[R.opcode_list_entry([R.gain_map_opcode(_m())], cut=12)]),
                        r"OpcodeList2 \(51009\) is truncated: the header of opcode 0"),
    "short parameters": (dict(opcodes=[R.opcode(9, b"\0" * 40)]), r"GainMap\): parameter size 40 is below"),
    "size against points": (dict(opcodes=[R.gain_map_opcode(_m(), points=(3, 3))]), r"parameter size 124 disagrees with MapPointsV"),
    "MapPlanes": (dict(opcodes=[R.gain_map_opcode(_m(), map_planes=2)]), r"MapPlanes 2"),
    "Planes": (dict(opcodes=[R.gain_map_opcode(_m(), planes=3)]), r"Planes 3"),
    "Plane": (dict(opcodes=[R.gain_map_opcode(_m(), plane=1)]), r"Plane 1"),
    "no points": (dict(opcodes=[R.gain_map_opcode(_m(), points=(0, 4))]), r"MapPointsV 0 outside 1 .. 64"),
    "65 points": (dict(maps=[R.make_map(np.ones((2, 65)), spacing=(1, 1 / 64))]), r"MapPointsH 65 outside 1 .. 64"),
    "spacing 0": (dict(maps=[_m(spacing_v=0.0)]), r"MapSpacingV 0.0 with 3 points"),
    "spacing negative": (dict(maps=[_m(spacing_h=-0.25)]), r"MapSpacingH -0.25 with 4 points"),
    "gain": (dict(maps=[_m(gains=np.array([[1, 1, 1, 1], [1, np.inf, 1, 1], [1, 1, 1, 1]], np.float32))]), r"a non-finite gain"),
    "nan gain": (dict(maps=[_m(gains=np.full((3, 4), np.nan, np.float32))]), r"a non-finite gain"),
    "pitch 1 off the corner": (dict(maps=[_m(row_pitch=1, col_pitch=1, top=1)]), r"Top 1 / Left 0 with RowPitch = ColPitch = 1"),
    "pitch 2 x 1": (dict(maps=[_m(col_pitch=1)]), r"RowPitch 2 / ColPitch 1"),
    "pitch 4": (dict(maps=[_m(row_pitch=4, col_pitch=4)]), r"RowPitch 4 / ColPitch 4"),
    "top 2": (dict(maps=[_m(top=2)]), r"Top 2 / Left 0 with RowPitch = ColPitch = 2"),
    "one position twice": (dict(maps=[_m(top=1, left=1), _m(top=1, left=1)]), r"opcode 1 \(GainMap\): a second map"),
    "pitch 1 and another": (dict(maps=[_m(row_pitch=1, col_pitch=1), _m(top=1)]), r"opcode 1 \(GainMap\): a second map"),
    "bottom": (dict(maps=[_m(bottom=H - 1)]), r"Bottom 39 / Right 65536 do not reach"),
    "right": (dict(maps=[_m(right=W - 2)]), r"Bottom 65536 / Right 46 do not reach"),
    "required unknown opcode": (dict(opcodes=[R.opcode(4, b"\0" * 8, flags=0)]), r"opcode 0 with OpcodeID 4 is not applied"),
    "required behind a map": (dict(opcodes=[R.gain_map_opcode(_m()), R.opcode(1, b"", flags=2)]), r"opcode 1 with OpcodeID 1"),
    "active area with a delta": (dict(extra=[(50829, LONG, [2, 2, H - 2, W - 2]), (50716, SRATIONAL, DV)]), r"ActiveArea \(50829\) \[2, 2, 38, 46\]"),
    "active area with a map": (dict(maps=[_m()], extra=[(50829, SHORT, [0, 0, H, W - 1])]), r"ActiveArea \(50829\)"),
}


@pytest.mark.parametrize("name", list(REFUSALS))
def test_refusals_name_what_they_refuse(tmp_path, name):
    from handheld_super_resolution import dng

    kw, match = REFUSALS[name]
    p = tmp_path / "a.dng"
    write(p, **kw)
    with pytest.raises(ValueError, match="a.dng: .*" + match):
        dng.parse_dng(p, linearization=True)


def test_active_area_alone_stays_ignored(tmp_path):
    from handheld_super_resolution import dng

    p = tmp_path / "a.dng"
    table = list(range(100, 116))
    write(p, extra=[(50829, LONG, [2, 2, H - 2, W - 2]), (50712, SHORT, table)])  # (a table is not defined on the area)
    assert dng.parse_dng(p, linearization=True).linearization_table.tolist() == table


def test_config_key(tmp_path):
    import run_handheld
    from handheld_super_resolution.super_resolution import dng_linearization, dng_options, load_burst
    from test_dng_burst import small_config

    assert dng_linearization(small_config()) == "refuse"
    assert dng_linearization(small_config(dng={"reader": "native"})) == "refuse"
    assert dng_linearization(small_config(dng={"reader": "native", "linearization": "refuse"})) == "refuse"
    cfg = small_config(dng={"reader": "native", "linearization": "apply"})
    assert dng_linearization(cfg) == "apply" and dng_options(cfg) == "native"
    with pytest.raises(ValueError, match="config.dng.linearization 'skip': refuse or apply"):
        dng_linearization(small_config(dng={"reader": "native", "linearization": "skip"}))
    for section in ({"linearization": "apply"}, {"reader": "rawpy", "linearization": "apply"}):
        with pytest.raises(ValueError, match="config.dng.linearization 'apply' needs config.dng.reader 'native'"):
            load_burst(str(tmp_path / "does not exist"), small_config(dng=section))  # before the burst is touched
    args = run_handheld.parse_args(["--impath", "folder", "--outpath", "out.png", "dng.reader=native", "dng.linearization=apply"])
    assert dng_linearization(run_handheld.build_config(args)) == "apply"
    args = run_handheld.parse_args(["--impath", "folder", "--outpath", "out.png", "dng.reader=native"])
    assert dng_linearization(run_handheld.build_config(args)) == "refuse"


def test_restatement_sanity():
    """What must hold of the restatement whatever the kernel does, computed here."""
    from handheld_super_resolution.utils_dng import gain_map_plane

    c = np.random.default_rng(5).integers(0, 4096, (2, H, W))
    levels = ([64, 66.5, 61], 4000.0, [2.1, 1.1, 1.7], [[0, 1], [1, 2]])
    plain = R.linearize(c, *levels)
    ones = R.make_map(np.ones((7, 5)), spacing=(1 / 6, 1 / 4), pitch=1)
    assert np.array_equal(R.linearize(c, *levels, maps=[ones]), plain)  # a constant map of 1.0 is the identity
    g = np.float32(1.37)
    # a 1 x 1 map of g scales the value in front of the white balance by g: with a balance of 1 that is one product
    unbalanced = R.linearize(c, levels[0], levels[1], [1.0, 1.0, 1.0], levels[3])
    assert np.array_equal(R.linearize(c, levels[0], levels[1], [1.0, 1.0, 1.0], levels[3], maps=[R.make_map([[g]], pitch=1)]),
                          unbalanced * g)
    # pixels before the origin and beyond the last point clamp to the edge values
    m = R.make_map(np.arange(1, 7, dtype=np.float32).reshape(2, 3), origin=(0.25, 0.25), spacing=(0.2, 0.2), pitch=1)
    plane = R.gain_plane(m, H, W)
    ys, xs = (np.arange(H) + 0.5) / H, (np.arange(W) + 0.5) / W
    assert (ys <= 0.25).any() and (ys >= 0.45).any() and (xs <= 0.25).any() and (xs >= 0.65).any()
    assert (plane[ys <= 0.25][:, xs <= 0.25] == 1).all() and (plane[ys >= 0.45][:, xs >= 0.65] == 6).all()
    assert (plane[ys <= 0.25][:, xs >= 0.65] == 3).all() and (plane[ys >= 0.45][:, xs <= 0.25] == 4).all()
    inside = plane[(ys > 0.25) & (ys < 0.45)][:, (xs > 0.25) & (xs < 0.65)]
    assert inside.size and (inside > 1).all() and (inside < 6).all() and (np.diff(inside, axis=1) > 0).all()
    # the table clamps counts beyond its end; a missing phase keeps gain 1
    t = np.arange(16, dtype=np.uint16) * 3
    assert np.array_equal(R.linearize(c, *levels, table=t), R.linearize(np.minimum(c, 15) * 3, *levels))
    three = [R.make_map([[2.0]], top=k // 2, left=k % 2) for k in (0, 1, 3)]
    got = R.linearize(c, *levels, maps=three)
    assert np.array_equal(got[:, 1::2, 0::2], plain[:, 1::2, 0::2])  # (a factor 2 is exact in front of the balance or behind)
    assert np.array_equal(got[:, 0::2, 0::2], plain[:, 0::2, 0::2] * 2) and np.array_equal(got[:, 1::2, 1::2], plain[:, 1::2, 1::2] * 2)
    # the package's own NumPy function states the same interpolation
    for mm in (m, ones, four_maps(13, 17)[2]):
        assert np.array_equal(gain_map_plane(mm, H, W), R.gain_plane(mm, H, W))
