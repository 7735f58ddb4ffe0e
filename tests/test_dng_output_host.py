"""DNG output without a GPU: the container of dng.dng_head read back with Pillow's IFD reader, every new ValueError of the
output options word for word (from the stage and from process() on a burst that must not be read), and the command line's
three cases."""
import os
import sys

import numpy as np
import pytest

import handheld_super_resolution as hsr
from handheld_super_resolution import dng, super_resolution as sr, utils_dng

import dng_out_cases as out_cases
import dng_ref
import ljpeg_enc_cases as enc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "handheld-multi-frame-super-resolution_amd"))


def host_file(img, th, tw, **meta):
    """A whole file made on the host: hhsr_ljpeg_encode_host behind dng_head."""
    H, W, nf = img.shape
    got = enc.encode_host(img, 16, 1, th, tw, enc.tables_for(img, 16, 1, th, tw))
    n = len(got.tile_bytes)
    head = dng.dng_head(H, W, nf, th, tw, got.offsets[:n], got.tile_bytes, **meta)
    assert len(head) == len(dng.dng_head(H, W, nf, th, tw, **meta))  # known before the encode
    return np.concatenate([np.frombuffer(head, np.uint8), got.out]), head


def test_pillow_reads_the_ifd_of_a_raw_file(tmp_path):
    """What the checks below rest on: Pillow's IFD reader on a file it cannot open as an image (tests/dng_ref.write_dng)."""
    p = tmp_path / "cfa.dng"
    dng_ref.write_dng(str(p), np.arange(24 * 32, dtype=np.uint16).reshape(24, 32))
    from PIL import TiffImagePlugin

    data = p.read_bytes()
    ifd = TiffImagePlugin.ImageFileDirectory_v2(data[:8])
    with open(p, "rb") as f:
        f.seek(int.from_bytes(data[4:8], "little" if data[:2] == b"II" else "big"))
        ifd.load(f)
    assert ifd[256] == 32 and ifd[257] == 24


@pytest.mark.parametrize("nf", [3, 1])
def test_container(nf):
    img = enc.image("smooth", 40, 56, nf, 16, seed=nf)
    m = np.array([[0.9, -0.2, 0.05], [-0.4, 1.3, 0.1], [0.02, -0.15, 0.7]])
    meta = dict(orientation=6, camera_model="Test Camera 1", xyz2cam=m, white_balance=[2.0, 1.25, 1.5, 1.25],
                calibration_illuminant=17)
    data, head = host_file(img, 16, 32, **meta)
    tags, samples = out_cases.decode_file(data)
    assert (samples == img).all()
    want = {"NewSubFileType": 0, "ImageWidth": 56, "ImageLength": 40, "BitsPerSample": (16,) * nf, "Compression": 7,
            "PhotometricInterpretation": 34892, "Orientation": 6, "SamplesPerPixel": nf, "PlanarConfiguration": 1,
            "TileWidth": 32, "TileLength": 16, "DNGVersion": b"\x01\x04\x00\x00", "DNGBackwardVersion": b"\x01\x01\x00\x00",
            "UniqueCameraModel": "Test Camera 1", "BlackLevel": (0,) * nf, "WhiteLevel": (65535,) * nf, "BaselineExposure": 0.0}
    for k, v in want.items():
        got = tags[k]
        assert (out_cases.as_tuple(got) == v if isinstance(v, tuple) else got == v), (k, got, v)
    colour = {"ColorMatrix1", "AnalogBalance", "AsShotNeutral", "CalibrationIlluminant1"}
    assert set(tags) == set(want) | {"TileOffsets", "TileByteCounts"} | (colour if nf == 3 else set())
    if nf == 3:
        assert np.allclose(tags["ColorMatrix1"], m.reshape(-1), atol=1e-6, rtol=0)
        assert np.allclose(tags["AnalogBalance"], (1.6, 1.0, 1.2), atol=1e-6, rtol=0)  # normalised to green
        assert tuple(tags["AsShotNeutral"]) == (1.0, 1.0, 1.0) and tags["CalibrationIlluminant1"] == 17
    # the layout: even length, ascending tags, even value offsets, every value inside the head
    assert len(head) % 2 == 0
    entries = out_cases.raw_entries(data)
    assert [e[0] for e in entries] == sorted(e[0] for e in entries) and len({e[0] for e in entries}) == len(entries)
    for tag, typ, count, at, nbytes in entries:
        if at is not None:
            assert at % 2 == 0 and at + nbytes <= len(head), (tag, at, nbytes)
    offs, cnts = out_cases.as_tuple(tags["TileOffsets"]), out_cases.as_tuple(tags["TileByteCounts"])
    assert offs[0] == len(head) and offs[-1] + cnts[-1] in (data.size, data.size - 1)


def test_container_defaults_and_single_tile():
    """No metadata: the fixed camera model, XYZ -> linear sRGB (D65), illuminant 21, balance 1 1 1, orientation 1; one tile:
    the offset and the count are inline values."""
    img = enc.image("smooth", 16, 16, 3, 16)
    data, head = host_file(img, 16, 16)
    tags, samples = out_cases.decode_file(data)
    assert (samples == img).all()
    assert tags["UniqueCameraModel"] == dng.DEFAULT_CAMERA_MODEL and tags["Orientation"] == 1
    assert np.allclose(tags["ColorMatrix1"], np.array(dng.XYZ_TO_SRGB_D65).reshape(-1), atol=1e-6, rtol=0)
    assert tags["CalibrationIlluminant1"] == 21 and tuple(tags["AnalogBalance"]) == (1.0, 1.0, 1.0)
    assert out_cases.as_tuple(tags["TileOffsets"]) == (len(head),)
    assert [e[3] for e in out_cases.raw_entries(data) if e[0] in (324, 325)] == [None, None]
    for bad in (dict(samples=2), dict(orientation=9), dict(white_balance=[1, 0, 1]), dict(xyz2cam=np.zeros(8))):
        kw = dict(dict(height=16, width=16, samples=3, tile_h=16, tile_w=16), **bad)
        with pytest.raises(ValueError, match="dng_head"):
            dng.dng_head(**kw)
    with pytest.raises(ValueError, match="4 GiB"):
        dng.dng_head(16, 16, 1, 16, 16, [2 ** 32 - 100], [400])


def test_our_reader_still_refuses_linear_raw(tmp_path):
    data, _ = host_file(enc.image("smooth", 16, 16, 3, 16), 16, 16)
    p = tmp_path / "linear.dng"
    utils_dng.save_dng_bytes(data, p)
    assert p.read_bytes() == data.tobytes()
    with pytest.raises(ValueError, match="LinearRaw"):
        dng.parse_dng(p)
    with pytest.raises(ValueError, match="save_dng_bytes"):
        utils_dng.save_dng_bytes(data[1:], p)


# ---- the output options -------------------------------------------------------------------------------------------------------
class Untouchable(dict):
    """A burst whose frames must not be looked at."""

    def __getitem__(self, k):
        raise AssertionError(f"burst[{k!r}] was read")

    get = __getitem__


def config_with(output, post=False):
    cfg = hsr.default_config()
    cfg.verbose = 0
    cfg.output = output
    cfg.postprocessing.enabled = post
    return cfg


TILE = "one integer or [h, w], each a multiple of 16 in 16 .. 65535"


@pytest.mark.parametrize("output,post,message", [
    (dict(format="dng", dtype="uint8"), False, "config.output.format dng holds 16-bit samples: output.dtype 'uint8' contradicts it"),
    (dict(format="dng", dtype="float32"), False, "config.output.format dng holds 16-bit samples: output.dtype 'float32' contradicts it"),
    (dict(format="dng", tile=24), False, f"tile=24: {TILE}"),
    (dict(format="dng", tile=0), False, f"tile=0: {TILE}"),
    (dict(format="dng", tile=65536), False, f"tile=65536: {TILE}"),
    (dict(format="dng", tile=[16, 40]), False, f"tile=[16, 40]: {TILE}"),
    (dict(format="dng", tile=[16, 16, 16]), False, f"tile=[16, 16, 16]: {TILE}"),
    (dict(format="dng", tile="big"), False, f"tile='big': {TILE}"),
    (dict(format="dng", predictor=0), False, "predictor=0: an integer in 1 .. 7"),
    (dict(format="dng", predictor=8), False, "predictor=8: an integer in 1 .. 7"),
    (dict(format="dng"), True, "config.output.format dng holds the linear image: switch post-processing off "
                               "(postprocessing.enabled: false)"),
    (dict(format="dnx"), False, "config.output.format 'dnx': raw, jpeg or png"),
])
def test_output_option_errors(output, post, message):
    for call in (lambda cfg: sr.output_options(cfg), lambda cfg: hsr.process(Untouchable(), cfg)):
        with pytest.raises(ValueError) as e:
            call(config_with(output, post))
        assert str(e.value) == message


def test_output_options():
    opts = sr.output_options
    got = opts(config_with(dict(format="dng")))
    assert got == sr.OutputOptions("dng", "uint16", tile=(utils_dng.DNG_TILE, utils_dng.DNG_TILE), predictor=1)
    got = opts(config_with(dict(format="dng", dtype="uint16", tile=[32, 64], predictor=7)))
    assert (got.tile, got.predictor) == ((32, 64), 7)
    assert opts(config_with(dict(format="dng", tile=128))).tile == (128, 128)
    # new fields at the end, with defaults: what the other formats return is what it was
    assert sr.OutputOptions._fields[:8] == ("format", "dtype", "quality", "restart_mcus", "subsampling", "huffman", "filter",
                                            "interval_bytes")
    assert opts(hsr.default_config()) == sr.OutputOptions("raw", "float32")


# ---- the command line ---------------------------------------------------------------------------------------------------------
def test_command_line_cases(capsys):
    import run_handheld as cli

    def config(*argv):
        return cli.build_config(cli.parse_args(["--impath", "burst.npz", *argv]))

    cfg = config("--outpath", "out.dng", "output.format=dng", "output.tile=128", "verbose=1")
    assert cfg.postprocessing.enabled is False and "post-processing is switched off" in capsys.readouterr().out
    assert sr.output_options(cfg) == sr.OutputOptions("dng", "uint16", tile=(128, 128), predictor=1)
    config("--outpath", "out.dng", "output.format=dng", "verbose=0")
    assert capsys.readouterr().out == ""
    with pytest.raises(NotImplementedError, match="output.format=dng"):
        config("--outpath", "out.dng")
    with pytest.raises(ValueError) as e:
        config("--outpath", "out.tif", "output.format=dng")
    assert str(e.value) == "output.format=dng writes a DNG file: --outpath 'out.tif' does not end in .dng"
    assert config("--outpath", "out.tif").output == {"dtype": "uint16"}  # as before
