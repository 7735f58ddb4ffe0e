"""The burst intake without a GPU: the raw-frame record (raw_frames.RawLayout) built from a burst mapping and from
config.hip.raw_norm, its upload to the host "device", the check of a list of device frames, the integer option check, and
the output-option stage of process() message by message."""
import numpy as np
import pytest
import torch

import handheld_super_resolution as hsr
from handheld_super_resolution import raw_frames as rf, super_resolution as sr, utils_dng
from handheld_super_resolution.config import positive_int
from handheld_super_resolution.raw_frames import COUNTS, FLOAT, PACKED, RawLayout

LEVELS = dict(black_levels=[64, 64.5, 63, 64], white_level=np.int64(1023))
COUNTS16 = np.full((4, 32), 100, np.uint16)


def test_layout_from_a_burst_mapping():
    assert RawLayout.from_burst({}, np.zeros((4, 32), np.float32)) == RawLayout(FLOAT)
    assert RawLayout.from_burst({}, torch.zeros((4, 32), dtype=torch.int32)) == RawLayout(FLOAT)  # tensors: as they are
    assert not RawLayout(FLOAT).is_counts
    lay = RawLayout.from_burst(LEVELS, COUNTS16)
    assert lay == RawLayout(COUNTS, None, None, (64.0, 64.5, 63.0), 1023.0) and lay.is_counts
    assert type(lay.white_level) is float
    with pytest.raises(KeyError, match="black_levels"):
        RawLayout.from_burst({"white_level": 1023}, COUNTS16)
    rows = utils_dng.pack_raw(COUNTS16, "mipi10")
    assert rows.shape == (4, 40)
    for given, stored in [("mipi10", "mipi10"), (1, 1), (np.array("mipi10"), "mipi10"), (np.int64(1), 1), (np.array(1), 1)]:
        lay = RawLayout.from_burst(dict(LEVELS, packing=given), rows)
        assert lay == RawLayout(PACKED, stored, 32, (64.0, 64.5, 63.0), 1023.0) and lay.is_counts  # 40 bytes: 32 pixels
        assert type(lay.packing) is type(stored) and type(lay.width) is int
    assert RawLayout.from_burst(dict(LEVELS, packing="mipi10", width=np.array(30)), rows).width == 30
    padded = utils_dng.pack_raw(COUNTS16, "mipi10", row_bytes=43)
    assert RawLayout.from_burst(dict(LEVELS, packing="mipi10", width=32), padded).width == 32
    with pytest.raises(ValueError, match=r"packed burst: give 'width' \(the rows are longer than their pixels' bytes\)"):
        RawLayout.from_burst(dict(LEVELS, packing="mipi10"), padded)
    with pytest.raises(ValueError, match="packing 'mipi11'"):
        RawLayout.from_burst(dict(LEVELS, packing="mipi11"), rows)


def test_layout_from_raw_norm():
    norm = {"black_levels": [64, 64, 64], "white_level": 1023}
    u16, rows = torch.zeros((4, 32), dtype=torch.uint16), torch.zeros((4, 40), dtype=torch.uint8)
    assert RawLayout.from_raw_norm(None, u16) == RawLayout(FLOAT)
    assert RawLayout.from_raw_norm(norm, torch.zeros((4, 32))) == RawLayout(FLOAT)
    assert RawLayout.from_raw_norm(norm, u16) == RawLayout(COUNTS, None, None, (64.0, 64.0, 64.0), 1023.0)
    packed = dict(norm, packing="mipi10", width=32)
    assert RawLayout.from_raw_norm(packed, rows) == RawLayout(PACKED, "mipi10", 32, (64.0, 64.0, 64.0), 1023.0)
    assert RawLayout.from_raw_norm(packed, torch.zeros((4, 43), dtype=torch.uint8)).width == 32  # padded rows
    assert RawLayout.from_raw_norm(packed, u16).kind == COUNTS  # only 2-D uint8 frames are packed
    assert RawLayout.from_raw_norm(packed, rows[None]).kind == COUNTS
    with pytest.raises(ValueError, match="config.hip.raw_norm: 'packing' needs 'width', the pixels per row"):
        RawLayout.from_raw_norm(dict(norm, packing="mipi10"), rows)
    with pytest.raises(ValueError, match="config.hip.raw_norm: 'width' 34 as mipi10 needs rows of 45 bytes, the frames have 40"):
        RawLayout.from_raw_norm(dict(packed, width=34), rows)
    with pytest.raises(ValueError, match="config.hip.raw_norm: 'width' 0 as mipi10 needs rows of 5 bytes, the frames have 40"):
        RawLayout.from_raw_norm(dict(packed, width=0), rows)


def test_raw_norm_mapping():
    assert RawLayout.from_burst(LEVELS, COUNTS16).raw_norm() == {"black_levels": [64.0, 64.5, 63.0], "white_level": 1023.0}
    rows = utils_dng.pack_raw(COUNTS16, "be12")
    norm = RawLayout.from_burst(dict(LEVELS, packing=np.array("be12")), rows).raw_norm()
    assert norm == {"black_levels": [64.0, 64.5, 63.0], "white_level": 1023.0, "packing": "be12", "width": 32}
    assert RawLayout.from_raw_norm(norm, torch.as_tensor(rows)).raw_norm() == norm  # what BurstPipeline reads back


def test_upload_to_the_host():
    counts, packed = RawLayout.from_burst(LEVELS, COUNTS16), RawLayout.from_burst(dict(LEVELS, packing=1), np.zeros((4, 40), np.uint8))
    t = counts.upload(np.full((2, 2), 1023, np.int64), "cpu")
    assert t.dtype == torch.uint16 and t.tolist() == [[1023, 1023], [1023, 1023]]
    assert counts.upload(COUNTS16, "cpu").dtype == torch.uint16
    for bad in (70000, -1):
        with pytest.raises(ValueError, match="sensor counts outside the uint16 range"):
            counts.upload(np.full((2, 2), bad, np.int32), "cpu")
    assert packed.upload(np.full((4, 40), 255, np.uint8), "cpu").dtype == torch.uint8  # rows of bytes stay
    for f in (np.zeros((2, 2), np.float32), np.zeros((2, 2), np.float64), torch.zeros((2, 2), dtype=torch.float64)):
        assert counts.upload(f, "cpu").dtype == torch.float32  # float data passes, as float32
        with pytest.raises(TypeError, match="integer sensor counts expected: float frames are already white-balanced"):
            counts.upload(f, "cpu", counts_only=True)
    assert counts.upload(torch.zeros((2, 2), dtype=torch.int32), "cpu").dtype == torch.int32  # tensors: as they are
    assert rf.upload_frame(np.full((2, 2), 7, np.int32), "cpu").dtype == torch.uint16


def test_frame_list_check_names_its_caller():
    host = [torch.zeros((32, 48), dtype=torch.int16)]
    for who in ("frame_sharpness", "white_balance_histogram", "noise_histogram"):
        with pytest.raises(RuntimeError, match=f"{who} expects tensors on the GPU"):
            rf.check_device_frames(who, host, (COUNTS, PACKED))
        with pytest.raises(ValueError, match=f"{who}: no frame"):
            rf.check_device_frames(who, [], (FLOAT,))
    with pytest.raises(RuntimeError, match="noise_histogram expects tensors on the GPU"):
        rf.check_device_frames("noise_histogram", [np.zeros((32, 48), np.float32)], (FLOAT,))


def test_positive_int():
    assert positive_int("reference", "candidates", np.int64(3)) == 3 and type(positive_int("a", "b", np.int32(1))) is int
    for bad in (0, -1, True, 2.0, "3", None):
        with pytest.raises(ValueError, match=f"config.noise_model.frames {bad!r}: an integer >= 1"):
            positive_int("noise_model", "frames", bad)


class Untouchable(dict):
    """A burst whose frames must not be looked at."""

    def __getitem__(self, k):
        raise AssertionError(f"burst[{k!r}] was read")

    get = __getitem__


def config_with(output, mode=None, **noise):
    cfg = hsr.default_config()
    cfg.verbose = 0
    cfg.output = output
    cfg.noise_model.update(noise)
    if mode is not None:
        cfg.mode = mode
    return cfg


BAD_OUTPUT = [
    (dict(format="tiff"), {}, "config.output.format 'tiff': raw, jpeg or png"),
    (dict(format="bmp"), dict(source="measure"), "config.output.format 'bmp': raw, jpeg or png"),  # two faults: output's
    (dict(dtype="int8"), {}, "config.output.dtype 'int8': float32, uint8 or uint16"),
    (dict(format="jpeg", dtype="uint16"), {}, "config.output.format jpeg holds 8-bit samples: output.dtype 'uint16' contradicts it"),
    (dict(format="jpeg", dtype="float32"), {}, "config.output.format jpeg holds 8-bit samples: output.dtype 'float32' contradicts it"),
    (dict(format="jpeg", quality=0), {}, "config.output.quality 0: 1 .. 100"),
    (dict(format="jpeg", quality=101), {}, "config.output.quality 101: 1 .. 100"),
    (dict(format="jpeg", restart_mcus=0), {}, "config.output.restart_mcus 0: 1 .. 65535"),
    (dict(format="jpeg", restart_mcus=65536), {}, "config.output.restart_mcus 65536: 1 .. 65535"),
    (dict(format="jpeg", subsampling="422"), {}, "subsampling='422': one of 444, 420"),
    (dict(format="jpeg", huffman="best"), {}, "huffman='best': one of standard, optimized"),
    (dict(format="jpeg", subsampling=420), dict(mode="grey"), "config.output.subsampling 420 needs three components: mode grey writes one"),
    (dict(format="png", dtype="float32"), {}, "config.output.format png holds 8- or 16-bit samples: output.dtype 'float32' contradicts it"),
    (dict(format="png", filter="best"), {}, "filter='best': one of none, sub, up, average, paeth, adaptive"),
    (dict(format="png", interval_bytes=0), {}, "interval_bytes=0: an integer in 1 .. 1048576"),
    (dict(format="png", interval_bytes=2 ** 20 + 1), {}, "interval_bytes=1048577: an integer in 1 .. 1048576"),
]


@pytest.mark.parametrize("output,other,message", BAD_OUTPUT)
def test_output_options_refuse_before_the_burst_is_read(output, other, message):
    """Every ValueError of config.output, word for word, from the stage and from process()."""
    other = dict(other)
    mode = other.pop("mode", None)
    for call in (lambda cfg: sr.output_options(cfg), lambda cfg: hsr.process(Untouchable(), cfg)):
        with pytest.raises(ValueError) as e:
            call(config_with(output, mode, **other))
        assert str(e.value) == message


def test_output_options():
    opts = sr.output_options
    assert opts(hsr.default_config()) == sr.OutputOptions("raw", "float32")
    assert opts(config_with(dict(dtype="uint16"))) == sr.OutputOptions("raw", "uint16")
    assert opts(config_with(dict(format="jpeg"))) == sr.OutputOptions("jpeg", "uint8", 90, None, "444", "standard")
    got = opts(config_with(dict(format="jpeg", quality=75, restart_mcus=8, subsampling=420, huffman="optimized")))
    assert got == sr.OutputOptions("jpeg", "uint8", 75, 8, "420", "optimized")
    got = opts(config_with(dict(format="png", dtype="uint16", filter="paeth", interval_bytes=4096)))
    assert (got.format, got.dtype, got.quality, got.subsampling) == ("png", "uint16", None, None)
    assert got.filter == opts(config_with(dict(format="png", filter="paeth"))).filter and got.interval_bytes == 4096
    assert opts(config_with(dict(quality=0, filter="best"))) == sr.OutputOptions("raw", "float32")  # read with their format only
