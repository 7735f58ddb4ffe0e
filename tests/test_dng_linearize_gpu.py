"""hhsr_linearize_raw_u16 against the NumPy restatement of its contract (tests/dng_linearize_ref.py), bit for bit: every
feature alone and all together, compact and padded rows inside guard bands, all four CFA patterns; the link to
hhsr_normalize_raw_u16; the argument refusals; dng.read_dng_burst(linearization=True) on written folders; process() end to
end."""
import ctypes
import functools
import os

import numpy as np
import pytest
import torch

import dng_ref
import dng_linearize_ref as R
from dng_ref import SHORT, SRATIONAL

pytestmark = pytest.mark.gpu

DEV = "cuda"
N = 3
SENT = 0x5A5A5A5A  # guard sentinel of the output, compared as int32
GUARD = 1024       # elements on either side of input and output
CFAS = ([[0, 1], [1, 2]], [[1, 0], [2, 1]], [[1, 2], [0, 1]], [[2, 1], [1, 0]])
BLACK, WHITE, WB = [64.0, 66.5, 61.0], 4000.0, [2.1, 1.1, 1.7]  # distinct levels per colour, a fractional balance


def maps_for(pv, ph, origin, spacing, seed, positions=(0, 1, 2, 3)):
    rng = np.random.default_rng(seed)
    return [R.make_map((0.75 + rng.random((pv, ph))).astype(np.float32), origin=origin, spacing=spacing, top=k // 2, left=k % 2)
            for k in positions]


@functools.lru_cache(maxsize=None)
def features(H, W):
    """name -> (keywords of the restatement, 16-bit counts?)."""
    rng = np.random.default_rng(H * 1000 + W)
    dh = (rng.integers(-40, 41, W) / 8).astype(np.float32)
    dv = (rng.integers(-40, 41, H) / 16).astype(np.float32)
    table = {n: rng.integers(0, 1 << 16, n).astype(np.uint16) for n in (16, 1024, 65536)}
    wide = maps_for(13, 17, (0.0, 0.0), (1 / 12, 1 / 16), 3)
    f = {
        "table 16": (dict(table=table[16]), False),  # counts up to 4095: most lie beyond its end
        "table 1024": (dict(table=table[1024]), False),
        "table 65536": (dict(table=table[65536]), True),
        "delta h": (dict(delta_h=dh), False),
        "delta v": (dict(delta_v=dv), False),
        "map 1 x 1": (dict(maps=[R.make_map([[1.37]], pitch=1)]), False),
        "maps 2 x 3": (dict(maps=maps_for(2, 3, (0.25, 0.25), (0.2, 0.2), 1)), False),  # pixels outside on both sides
        "map 2 x 3, every pixel": (dict(maps=[dict(maps_for(2, 3, (0.25, 0.25), (0.2, 0.2), 2)[0], row_pitch=1, col_pitch=1)]), False),
        "maps 13 x 17": (dict(maps=wide), False),
        "maps 64 x 64": (dict(maps=maps_for(64, 64, (0.0, 0.0), (1 / 63, 1 / 63), 4)), False),
        "three maps": (dict(maps=maps_for(4, 5, (0.1, -0.2), (0.3, 0.4), 5, positions=(0, 1, 3))), False),
        "everything": (dict(table=table[1024], delta_h=dh, delta_v=dv, maps=wide), False),
        "everything, 16-bit table": (dict(table=table[65536], delta_h=dh, delta_v=dv, maps=wide), True),
    }
    return f


@functools.lru_cache(maxsize=None)
def counts(H, W, wide):
    return np.random.default_rng(H + W + wide).integers(0, (1 << 16) if wide else 4096, (N, H, W)).astype(np.uint16)


def T(a):
    a = np.ascontiguousarray(a)
    return torch.from_numpy(a.view(np.int16) if a.dtype == np.uint16 else a).to(DEV)


def call(c, stride, cfa, black=BLACK, white=WHITE, wb=WB, table=None, delta_h=None, delta_v=None, maps=()):
    """hhsr_linearize_raw_u16 on the counts c [n, H, W] laid out with `stride` elements per row, every padding count 0xFFFF,
    input and output inside guard bands: the float32 result [n, H, W].  The input must come back untouched and the output's
    guard bands must still hold their sentinel."""
    from handheld_super_resolution import _lib

    n, H, W = c.shape
    host = np.full(GUARD + n * H * stride + GUARD, 0xFFFF, np.uint16)
    host[GUARD:GUARD + n * H * stride].reshape(n, H, stride)[:, :, :W] = c
    raw = T(host)
    out = torch.full((GUARD + n * H * W + GUARD,), SENT, dtype=torch.int32, device=DEV)
    tab, dh, dv = (None if v is None else T(v) for v in (table, delta_h, delta_v))
    descs = (_lib.GainMapDesc * max(1, len(maps)))()
    at = 0
    for i, m in enumerate(maps):
        descs[i] = _lib.GainMapDesc(m["top"], m["left"], m["row_pitch"], m["col_pitch"], m["points_v"], m["points_h"],
                                    m["spacing_v"], m["spacing_h"], m["origin_v"], m["origin_h"], at)
        at += m["gains"].size
    gains = T(np.concatenate([m["gains"].reshape(-1) for m in maps])) if maps else None
    _lib.call("hhsr_linearize_raw_u16", ctypes.c_void_p(raw.data_ptr() + 2 * GUARD), n, H, W, stride, _lib.cfa_bytes(cfa),
              _lib.doubles(black), float(white), _lib.doubles(wb), _lib.ptr(tab), 0 if tab is None else tab.numel(),
              _lib.ptr(dh), _lib.ptr(dv), ctypes.addressof(descs) if maps else None, len(maps), _lib.ptr(gains), at,
              ctypes.c_void_p(out.data_ptr() + 4 * GUARD), None)
    torch.cuda.synchronize()
    assert np.array_equal(raw.cpu().numpy().view(np.uint16), host), "the input changed"
    o = out.cpu().numpy()
    assert (o[:GUARD] == SENT).all() and (o[-GUARD:] == SENT).all(), "the output's guard bands changed"
    return o[GUARD:-GUARD].view(np.float32).reshape(n, H, W)


def same_bits(got, want, what):
    bad = got.view(np.uint32) != want.view(np.uint32)
    assert not bad.any(), (what, int(bad.sum()), np.argwhere(bad)[:4].tolist(), got[bad][:4], want[bad][:4])


@pytest.mark.parametrize("padding", [0, 24])
@pytest.mark.parametrize("W,H", [(48, 40), (46, 38), (8, 2)])
def test_kernel_equals_the_restatement(W, H, padding):
    """(48, 40): the 16-byte path; (46, 38): W % 8 = 6, count by count and a tail; (8, 2): one thread per row."""
    for name, (kw, wide) in features(H, W).items():
        c = counts(H, W, wide)
        for cfa in CFAS:
            want = R.linearize(c, BLACK, WHITE, WB, cfa, **kw)
            assert np.isfinite(want).all()
            same_bits(call(c, W + padding, cfa, **kw), want, (name, cfa))


def test_more_than_one_workgroup_and_frame_group():
    """2056 pixels per row (two workgroups, the second with one thread) and 9 frames (two groups of frames)."""
    H, W = 4, 2056
    rng = np.random.default_rng(11)
    c = rng.integers(0, 4096, (9, H, W)).astype(np.uint16)
    kw = dict(table=rng.integers(0, 1 << 16, 1024).astype(np.uint16), delta_h=rng.standard_normal(W).astype(np.float32),
              delta_v=rng.standard_normal(H).astype(np.float32), maps=maps_for(13, 17, (0.0, 0.0), (1 / 12, 1 / 16), 6))
    same_bits(call(c, W, CFAS[1], **kw), R.linearize(c, BLACK, WHITE, WB, CFAS[1], **kw), "2056 x 4 x 9")


def test_nothing_to_apply_is_normalize_raw_u16():
    from handheld_super_resolution.utils_dng import linearize_burst, normalize_burst

    black, white = [64, 66, 61], 4095
    for W, H in ((48, 40), (46, 38)):
        c = counts(H, W, True)
        for cfa in CFAS:
            want = normalize_burst(c, black, white, WB, cfa).cpu().numpy()
            same_bits(call(c, W, cfa, black=black, white=white), want, (W, H, cfa))
            same_bits(linearize_burst(c, black, white, WB, cfa).cpu().numpy(), want, (W, H, cfa))
            same_bits(linearize_burst(c[0], black, white, WB, cfa).cpu().numpy(), want[0], "one frame")


def test_linearize_burst_takes_records_arrays_and_tensors():
    from handheld_super_resolution import dng
    from handheld_super_resolution.utils_dng import linearize_burst

    H, W = 40, 48
    kw, _ = features(H, W)["everything"]
    c = counts(H, W, False)
    want = R.linearize(c, BLACK, WHITE, WB, CFAS[0], **kw)
    records = [dng.GainMap(m["top"], m["left"], m["bottom"], m["right"], 0, 1, m["row_pitch"], m["col_pitch"], m["points_v"],
                           m["points_h"], m["spacing_v"], m["spacing_h"], m["origin_v"], m["origin_h"], 1, m["gains"]) for m in kw["maps"]]
    got = linearize_burst(c.astype(np.int32), BLACK, WHITE, WB, CFAS[0], table=kw["table"].tolist(), delta_h=kw["delta_h"],
                          delta_v=T(kw["delta_v"]), gain_maps=records)
    same_bits(got.cpu().numpy(), want, "records")
    same_bits(linearize_burst(T(c), BLACK, WHITE, WB, CFAS[0], table=T(kw["table"]), delta_h=kw["delta_h"], delta_v=kw["delta_v"],
                              gain_maps=kw["maps"]).cpu().numpy(), want, "mappings and tensors")
    with pytest.raises(ValueError, match="delta_h has 47 entries, 48 expected"):
        linearize_burst(c, BLACK, WHITE, WB, CFAS[0], delta_h=kw["delta_h"][:-1])
    with pytest.raises(ValueError, match="5 gain maps, at most 4"):
        linearize_burst(c, BLACK, WHITE, WB, CFAS[0], gain_maps=kw["maps"] + kw["maps"][:1])
    with pytest.raises(TypeError, match="integer sensor counts"):
        linearize_burst(c.astype(np.float32), BLACK, WHITE, WB, CFAS[0])


def test_argument_refusals():
    from handheld_super_resolution import _lib

    lib = _lib.load()
    H, W = 40, 48
    buf = torch.zeros(1 << 16, dtype=torch.float32, device=DEV)
    base = buf.data_ptr()
    raw, out, tab, dh, dv, gains = (ctypes.c_void_p(base + (k << 15)) for k in range(6))
    cfa, bl, wb = _lib.cfa_bytes(CFAS[0]), _lib.doubles(BLACK), _lib.doubles(WB)

    def desc(**kw):
        f = dict(top=0, left=0, row_pitch=2, col_pitch=2, points_v=2, points_h=3, spacing_v=1.0, spacing_h=0.5, origin_v=0.0,
                 origin_h=0.0, offset=0)
        f.update(kw)
        return _lib.GainMapDesc(**f)

    def run(raw=raw, out=out, tab=tab, table_len=16, maps=(desc(),), n_maps=None, gains=gains, gains_len=64, stride=W, H=H):
        arr = (_lib.GainMapDesc * max(1, len(maps)))(*maps)
        rc = lib.hhsr_linearize_raw_u16(raw, N, H, W, stride, cfa, bl, WHITE, wb, tab, table_len, dh, dv, ctypes.addressof(arr),
                                        len(maps) if n_maps is None else n_maps, gains, gains_len, out, None)
        return rc, lib.hhsr_last_error()

    assert run()[0] == 0  # everything valid: what follows is refused for the one thing that differs
    refused = {
        "a NULL output": dict(out=None),
        "a NULL input": dict(raw=None),
        "table_len 0 with a table": dict(table_len=0),
        "table_len 65537": dict(table_len=65537),
        "a length without a table": dict(tab=None, table_len=16),
        "more than four maps": dict(maps=[desc(top=k // 2, left=k % 2) for k in range(4)] + [desc()]),
        "points above 64": dict(maps=[desc(points_h=65)], gains_len=1 << 12),
        "no point": dict(maps=[desc(points_v=0)]),
        "a misaligned output": dict(out=ctypes.c_void_p(out.value + 8)),
        "a misaligned input": dict(raw=ctypes.c_void_p(raw.value + 2)),
        "a stride below the width": dict(stride=W - 1),
        "a map beyond the gains": dict(gains_len=5),
        "a negative offset": dict(maps=[desc(offset=-1)]),
        "no gains": dict(gains=None),
        "spacing 0 with two points": dict(maps=[desc(spacing_v=0.0)]),
        "a NaN origin": dict(maps=[desc(origin_h=float("nan"))]),
        "pitches 2, 1": dict(maps=[desc(col_pitch=1)]),
        "pitch 1 off the corner": dict(maps=[desc(row_pitch=1, col_pitch=1, left=1)]),
        "pitch 1 with a second map": dict(maps=[desc(row_pitch=1, col_pitch=1), desc(top=1)]),
        "top 2": dict(maps=[desc(top=2)]),
        "one position twice": dict(maps=[desc(), desc()]),
        "too many rows": dict(H=65536),
    }
    for name, kw in refused.items():
        rc, err = run(**kw)
        assert rc == -1 and b"hhsr_linearize_raw_u16: invalid argument" in err, (name, rc, err)
    assert run(maps=[desc(points_v=1, spacing_v=-1.0)])[0] == 0  # the spacing of a single point is not read
    torch.cuda.synchronize()


# ---- folders ------------------------------------------------------------------------------------------------------------------
FH, FW = 40, 48
LAYOUTS = {
    "u16": dict(bits=16, layout="strips", size=16),
    "be12": dict(bits=12, layout="strips", size=16),
    "ljpeg": dict(bits=12, compression=7, layout="tiles", size=(32, 24), ljpeg=dict(Nf=2, predictor=1)),
}


def folder_features(H, W, bits, seed=21):
    rng = np.random.default_rng(seed)
    table = np.sort(rng.integers(0, 1 << 14, 1 << min(bits, 12))).astype(np.uint16)  # 4096 entries, 14-bit linear values
    dh, dv = rng.integers(-16, 17, W) / 8.0, rng.integers(-16, 17, H) / 8.0   # exact as the rationals dng_ref writes
    maps = maps_for(5, 7, (0.0, 0.0), (0.25, 1 / 6), seed)
    return table, dh, dv, maps


def write_folder(folder, layout, c, table, dh, dv, maps, white=16000, **over):
    os.makedirs(folder, exist_ok=True)
    extra = [(50712, SHORT, table.tolist()), (50715, SRATIONAL, dh.tolist()), (50716, SRATIONAL, dv.tolist()),
             R.opcode_list_entry([R.gain_map_opcode(m) for m in maps])]
    written = []
    for i in range(len(c)):
        kw = dict(cfa=(1, 2, 0, 1), black=(250, 252, 249, 251), white=white, neutral=(0.5, 1.0, 0.625), iso=200,
                  noise_profile=[1e-4, 1e-6] * 3, extra=extra, byte_order="MM" if i == 1 else "II", subifd=(i == 2))
        kw.update(LAYOUTS[layout])
        kw.update(over)
        written.append(dng_ref.write_dng(os.path.join(folder, f"im_{i:02d}.dng"), c[i], **kw))
    return written


@pytest.mark.parametrize("layout", list(LAYOUTS))
def test_read_dng_burst_equals_the_restatement_of_the_counts(tmp_path, layout):
    from handheld_super_resolution import dng

    bits = LAYOUTS[layout]["bits"]
    c = np.random.default_rng(31).integers(0, 1 << bits, (N, FH, FW))
    table, dh, dv, maps = folder_features(FH, FW, bits)
    w = write_folder(str(tmp_path), layout, c, table, dh, dv, maps)[0]
    want = R.linearize(c, w["black_levels"], w["white_level"], w["white_balance"], w["cfa_pattern"], table=table,
                       delta_h=dh.astype(np.float32), delta_v=dv.astype(np.float32), maps=maps)
    for decoder in (("gpu", "host") if layout == "ljpeg" else ("host",)):
        b = dng.read_dng_burst(str(tmp_path), decoder=decoder, linearization=True)
        same_bits(torch.cat([b["ref"][None], b["comp"]]).cpu().numpy(), want, (layout, decoder))
        assert b["alpha"] == 1e-4 and b["beta"] == 1e-6  # NoiseProfile is passed on unchanged
        assert len(b["debug"]["infos"][0].gain_maps) == 4 and b["debug"]["infos"][2].linearization_table.size == table.size
    with pytest.raises(ValueError, match="BlackLevelDeltaH"):
        dng.read_dng_burst(str(tmp_path))  # without the keyword: today's refusal


def test_a_file_that_differs_from_file_0_is_named(tmp_path):
    from handheld_super_resolution import dng

    c = np.random.default_rng(32).integers(0, 1 << 16, (N, FH, FW))
    table, dh, dv, maps = folder_features(FH, FW, 16)
    write_folder(str(tmp_path), "u16", c, table, dh, dv, maps)
    other = [dict(m, gains=m["gains"].copy()) for m in maps]
    other[2]["gains"][3, 4] = np.nextafter(other[2]["gains"][3, 4], np.float32(9))
    extra = [(50712, SHORT, table.tolist()), (50715, SRATIONAL, dh.tolist()), (50716, SRATIONAL, dv.tolist()),
             R.opcode_list_entry([R.gain_map_opcode(m) for m in other])]
    dng_ref.write_dng(str(tmp_path / "im_01.dng"), c[1], cfa=(1, 2, 0, 1), extra=extra)
    with pytest.raises(ValueError, match="im_01.dng: gain_maps differs from that of .*im_00.dng"):
        dng.read_dng_burst(str(tmp_path), linearization=True)
    extra[0] = (50712, SHORT, table.tolist()[:-1])
    extra[3] = R.opcode_list_entry([R.gain_map_opcode(m) for m in maps])
    dng_ref.write_dng(str(tmp_path / "im_01.dng"), c[1], cfa=(1, 2, 0, 1), extra=extra)
    with pytest.raises(ValueError, match="im_01.dng: linearization_table differs"):
        dng.read_dng_burst(str(tmp_path), linearization=True)


def test_process_end_to_end(tmp_path):
    """128 x 192 x 3 frames: process(folder, dng.linearization=apply) equals process() of the in-memory burst whose float
    frames are the restatement's output, bit for bit."""
    import handheld_super_resolution as hsr
    from handheld_super_resolution import dng
    import test_dng_burst as B

    c, black, white = B.counts(16)
    rng = np.random.default_rng(41)
    # a compressive raw curve undone: table[count] = the linear value; the identity up to just above the black levels, then a
    # curve that ends at white
    knee = black + 76
    s = np.clip((np.arange(1 << 16) - knee) / (white - knee), 0, 1)
    table = np.where(np.arange(1 << 16) <= knee, np.arange(1 << 16), np.rint(knee + (white - knee) * (0.25 * s + 0.75 * s * s)))
    table = np.clip(table, 0, 65535).astype(np.uint16)
    dh, dv = rng.integers(-64, 65, B.W) / 8.0, rng.integers(-64, 65, B.H) / 8.0
    yy, xx = np.meshgrid(np.linspace(-1, 1, 13), np.linspace(-1, 1, 17), indexing="ij")
    maps = [R.make_map((1 + (0.3 + 0.05 * k) * (yy * yy + xx * xx)).astype(np.float32), spacing=(1 / 12, 1 / 16), top=k // 2, left=k % 2)
            for k in range(4)]  # lens shading: brighter towards the corners, a little different per plane
    extra = [(50712, SHORT, table.tolist()), (50715, SRATIONAL, dh.tolist()), (50716, SRATIONAL, dv.tolist()),
             R.opcode_list_entry([R.gain_map_opcode(m) for m in maps])]
    _, written = B.write_folder(str(tmp_path), "u16 II strips", extra=extra)
    w = written[0]
    out, dbg = hsr.process(str(tmp_path), B.small_config(dng={"reader": "native", "linearization": "apply"}))
    frames = R.linearize(c, w["black_levels"], w["white_level"], w["white_balance"], w["cfa_pattern"], table=table,
                         delta_h=dh.astype(np.float32), delta_v=dv.astype(np.float32), maps=maps)
    burst = dict(dng.read_dng_burst(str(tmp_path), linearization=True))
    same_bits(burst["ref"].cpu().numpy(), frames[0], "the folder's reference frame")
    burst["ref"], burst["comp"] = T(frames[0]), T(frames[1:])
    want, wdbg = hsr.process(burst, B.small_config())
    assert out.shape == (2 * B.H, 2 * B.W, 3) and out.dtype == np.float32 and np.isfinite(out).any()
    assert out.tobytes() == want.tobytes()
    assert dbg["accumulated robustness"].tobytes() == wdbg["accumulated robustness"].tobytes()
    with pytest.raises(ValueError, match="BlackLevelDeltaH"):
        hsr.process(str(tmp_path), B.small_config(dng={"reader": "native"}))


def test_a_folder_without_the_tags_gives_todays_bits(tmp_path):
    from handheld_super_resolution import dng
    from handheld_super_resolution.super_resolution import load_burst
    import test_dng_burst as B

    for name in ("u16 II strips", "12-bit packed strips"):
        folder = str(tmp_path / name.split()[0])
        B.write_folder(folder, name)
        plain = dng.read_dng_burst(folder)
        for b in (dng.read_dng_burst(folder, linearization=True),
                  load_burst(folder, B.small_config(dng={"reader": "native", "linearization": "apply"}))):
            assert b["ref"].cpu().numpy().tobytes() == plain["ref"].cpu().numpy().tobytes()
            assert b["comp"].cpu().numpy().tobytes() == plain["comp"].cpu().numpy().tobytes()
            assert b["debug"]["infos"][0].gain_maps is None and b["debug"]["infos"][0].linearization_table is None
