"""DNG output on the device: utils_dng.encode_dng read back with Pillow's IFD reader and decoded tile by tile with
hhsr_ljpeg_parse + hhsr_ljpeg_decode_host, and process() with ``output.format: dng`` on the small synthetic burst of the
end-to-end tests."""
import functools

import numpy as np
import pytest
import torch

import handheld_super_resolution as hsr
from handheld_super_resolution import utils_dng, utils_image
from handheld_super_resolution import synthetic as synth

import dng_out_cases as out_cases

pytestmark = pytest.mark.gpu


def device_image(H, W, ch, seed):
    """float32 on the device, mostly in [0, 1], with values outside, a NaN and an infinity (the quantisation's rule)."""
    g = torch.Generator(device="cuda").manual_seed(seed)
    shape = (H, W, ch) if ch else (H, W)
    y = torch.linspace(0, 1, H, device="cuda").reshape(H, 1, *([1] if ch else []))
    img = 0.8 * y + 0.1 * torch.rand(shape, generator=g, device="cuda") - 0.02
    flat = img.reshape(-1)
    flat[5], flat[11], flat[17] = float("nan"), float("inf"), 1.5
    return img


@pytest.mark.parametrize("ch,tile", [(3, [32, 48]), (0, 32), (3, None)])
def test_encode_dng_round_trip(ch, tile):
    """100 x 150 is no multiple of the tiles: the right, bottom and corner tiles replicate and decode to the image alone."""
    img = device_image(100, 150, ch, seed=ch + 1)
    m = np.array([[0.9, -0.2, 0.05], [-0.4, 1.3, 0.1], [0.02, -0.15, 0.7]], np.float32)
    data = utils_dng.encode_dng(img, tile=tile, xyz2cam=m, white_balance=np.array([2.0, 1.0, 1.5]), orientation=3)
    assert data.dtype == np.uint8 and data.ndim == 1
    tags, samples = out_cases.decode_file(data)
    want = utils_image.encode_image(img, "uint16").cpu().numpy()
    assert (samples.reshape(want.shape) == want).all()
    th, tw = (tile if isinstance(tile, list) else (tile, tile)) if tile else (utils_dng.DNG_TILE,) * 2
    assert (tags["TileLength"], tags["TileWidth"], tags["SamplesPerPixel"], tags["Orientation"]) == (th, tw, 3 if ch else 1, 3)
    if ch:
        assert np.allclose(tags["ColorMatrix1"], m.reshape(-1), atol=1e-6, rtol=0)
        assert np.allclose(tags["AnalogBalance"], (2.0, 1.0, 1.5), atol=1e-6, rtol=0)


def test_encode_dng_channel_0_predictors_and_retry():
    img = device_image(70, 90, 3, seed=9)
    want = utils_image.encode_image(img, "uint16").cpu().numpy()
    data = utils_dng.encode_dng(img, channels=1, tile=16, predictor=7)
    tags, samples = out_cases.decode_file(data)
    assert tags["SamplesPerPixel"] == 1 and (samples[:, :, 0] == want[:, :, 0]).all()
    whole = utils_dng.encode_dng(img, tile=32, predictor=4)
    small = utils_dng.encode_dng(img, tile=32, predictor=4, capacity=1000)  # one retry at the reported length
    assert whole.tobytes() == small.tobytes()
    assert (out_cases.decode_file(whole)[1] == want).all()
    with pytest.raises(RuntimeError):
        utils_dng.encode_dng(img.cpu())
    with pytest.raises(ValueError, match="tile=24"):
        utils_dng.encode_dng(img, tile=24)


def test_save_as_dng_takes_the_metadata_of_a_file(tmp_path):
    import dng_ref

    src = tmp_path / "frame.dng"
    dng_ref.write_dng(str(src), np.arange(24 * 32, dtype=np.uint16).reshape(24, 32))
    from handheld_super_resolution.dng import parse_dng

    info = parse_dng(src)
    img = device_image(40, 48, 3, seed=4)
    utils_dng.save_as_dng(img.cpu().numpy(), str(src), str(tmp_path / "out.dng"))
    tags, samples = out_cases.decode_file(np.frombuffer((tmp_path / "out.dng").read_bytes(), np.uint8))
    assert (samples == utils_image.encode_image(img, "uint16").cpu().numpy()).all()
    assert tags["Orientation"] == (info.orientation or 1)
    if info.xyz2cam is not None:
        assert np.allclose(tags["ColorMatrix1"], info.xyz2cam.reshape(-1), atol=1e-6, rtol=0)
    if info.white_balance is not None:
        assert np.allclose(tags["AnalogBalance"], np.array(info.white_balance) / info.white_balance[1], atol=2e-6, rtol=0)


# ---- process() ----------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def burst():
    ref_raw, comp, _ = synth.make_burst(128, 160, 3, seed=21, max_shift=1.5)
    std, diff = synth.noise_curves(synth.ALPHA_ISO100, synth.BETA_ISO100)
    return {"ref": ref_raw, "comp": comp, "cfa_pattern": np.array([[0, 1], [1, 2]]), "white_balance": np.array([1.8, 1.0, 1.5]),
            "alpha": synth.ALPHA_ISO100, "beta": synth.BETA_ISO100, "std_curve": std, "diff_curve": diff}


@functools.lru_cache(maxsize=None)
def processed(output, orientation=1, mode="bayer", median=False):
    cfg = hsr.default_config()
    cfg.verbose = 0
    cfg.scale = 2
    cfg.mode = mode
    cfg.block_matching.tuning.tile_size = 16
    cfg.block_matching.tuning.factors = [1, 2, 2, 2]
    cfg.block_matching.tuning.metrics = ["L2"] * 4
    cfg.postprocessing.enabled = False
    cfg.robustness.save_mask = True
    cfg.accumulated_robustness_denoiser.median.enabled = median
    cfg.output = {"format": "dng", "tile": 64} if output == "dng" else {"dtype": output}
    img, dbg = hsr.process(dict(burst(), orientation=orientation), cfg)
    return img, dbg


def test_process_dng_holds_the_uint16_image():
    want, dbg16 = processed("uint16")
    data, dbg = processed("dng")
    assert data.dtype == np.uint8 and data.ndim == 1
    tags, samples = out_cases.decode_file(data)
    assert want.shape == (256, 320, 3) and (samples == want).all() and samples.min() < samples.max()
    assert tags["Orientation"] == 1 and tags["TileWidth"] == 64
    assert np.allclose(tags["AnalogBalance"], (1.8, 1.0, 1.5), atol=1e-6, rtol=0)
    assert (dbg["accumulated robustness"] == dbg16["accumulated robustness"]).all()
    assert (dbg["robustness mask"] == dbg16["robustness mask"]).all()


def test_process_dng_orientation_goes_into_the_tag():
    want, _ = processed("uint16")            # orientation 1: the unrotated samples
    rotated, dbg16 = processed("uint16", 6)
    data, dbg = processed("dng", 6)
    tags, samples = out_cases.decode_file(data)
    assert tags["Orientation"] == 6 and rotated.shape == (320, 256, 3)
    assert (samples == want).all()
    assert (dbg["accumulated robustness"] == dbg16["accumulated robustness"]).all()  # oriented, as for the other formats
    assert (dbg["robustness mask"] == dbg16["robustness mask"]).all()


def test_process_dng_grey_mode_is_one_sample_per_pixel():
    want, _ = processed("uint16", 1, "grey")
    tags, samples = out_cases.decode_file(processed("dng", 1, "grey")[0])
    assert tags["SamplesPerPixel"] == 1 and "ColorMatrix1" not in tags
    assert want.shape == (256, 320) and (samples[:, :, 0] == want).all()


def test_process_dng_median_denoiser_still_acts():
    plain = out_cases.decode_file(processed("dng")[0])[1]
    tags, samples = out_cases.decode_file(processed("dng", 1, "bayer", True)[0])
    assert (samples == processed("uint16", 1, "bayer", True)[0]).all()
    assert (samples != plain).any()
