"""GPU parity of the fused FFT low-pass at image sizes whose H or W / 2 carry a prime factor 11, 13, 17 or 19 (radix-11 … 19
register butterflies, csrc/hhsr_fft_bfly.h: dft_prime; the PrimePlan kernels and the compile-time plans for 2040- / 2736-point
rows and 3648-point columns, csrc/hhsr_fft.hip) against the float64 oracle, the library plans, and each other.

Tolerance: atol 3e-6 against oracle.grey_fft, the bound of every grey test (tests/test_hip_parity.py::test_grey_fft).

The float64 oracle of a 12 - 20 MP image costs seconds, so each size has ONE random image; the other frames of a batch are
circular shifts of it — the low-pass is a circular convolution, so the oracle of a shifted image is the shifted oracle, exactly,
while every row and column of every frame differs from those of its neighbours.

Measured on an MI355X (profiles/fft_prime_radices.txt, PARITY.md): fused against the oracle <= 5.7e-7, against the library plans
<= 1.37e-6, compile-time plans against run-time passes 4.2e-7, no flipped tile in the burst; 24 s for the file."""
import functools
import time

import numpy as np
import pytest
import torch

import oracle
from helpers import assert_close, base_config

pytestmark = pytest.mark.gpu

from handheld_super_resolution import utils_image, synthetic as synth  # noqa: E402

DEV = "cuda"
FFT_ENV = ("HHSR_GREY_PLAN", "HHSR_FFT_NC", "HHSR_FFT_NT_ROWS", "HHSR_FFT_STATIC")
# 4080 = 2 * 8 15 17, 5472 = 2 * 9 16 19, 3648 = 12 16 19;  323 = 17 19, 286 = 2 11 13: every new radix in a row and a column pass
SIZES = [(3072, 4080), (3648, 5472), (323, 646), (342, 476), (286, 572)]
STATIC_SIZES = {(3072, 4080): (4, 0), (3648, 5472): (5, 4)}  # (row plan id, column plan id) of HHSR_STATIC_ROWS / _COLS
_SPENT = [0.0]  # seconds inside this file's tests (set-up included), summed by the fixture below


def T(a):
    return torch.as_tensor(np.ascontiguousarray(a), dtype=torch.float32, device=DEV)


def N(t):
    return t.detach().cpu().numpy()


@functools.lru_cache(maxsize=None)
def _case(shape):
    """(image, its float64 low-pass) of a size, computed once per session."""
    img = np.random.default_rng(shape[0] * 7 + shape[1]).random(shape, dtype=np.float32)
    return img, oracle.grey_fft(img)


def _frames(shape, n):
    """n frames and their expected results: the size's image circularly shifted by (37 k, 53 k)."""
    img, want = _case(shape)
    return ([np.roll(img, (37 * k, 53 * k), (0, 1)) for k in range(n)],
            [np.roll(want, (37 * k, 53 * k), (0, 1)) for k in range(n)])


@pytest.fixture(autouse=True)
def _fresh_plans(monkeypatch):
    for name in FFT_ENV:
        monkeypatch.delenv(name, raising=False)
    utils_image._grey_plans.clear()
    t0 = time.time()
    yield
    _SPENT[0] += time.time() - t0
    utils_image._grey_plans.clear()


def _live_plans_fused(shape):
    """Every live plan of this size, as the library reports it."""
    infos = [utils_image.grey_plan_info(*shape, plan=p) for k, p in utils_image._grey_plans.items() if k[:2] == shape]
    assert infos
    return infos


@pytest.mark.parametrize("shape", SIZES)
def test_prime_sizes_against_the_oracle(shape, monkeypatch):
    """Single frame and batches of 3 and 5 against the float64 oracle; batch frames bit-identical to single-frame results;
    the live plans report the fused kernels; the fused result agrees with the library plans (HHSR_GREY_PLAN=0)."""
    what = f"{shape[0]}x{shape[1]}"
    imgs, want = _frames(shape, 5)
    ti = [T(i) for i in imgs]
    single = [utils_image.compute_grey_images(t, "FFT").clone() for t in ti]
    for info in _live_plans_fused(shape):
        assert info["fused"] and {11, 13, 17, 19} & set(info["radices_rows"] + info["radices_cols"]), info
    for k in range(5):
        assert_close(N(single[k]), want[k], 0, 3e-6, "fused, single frame")
    for n in (3, 5):
        outs = utils_image.compute_grey_images_batch(ti[:n], "FFT")
        for k in range(n):
            assert torch.equal(outs[k], single[k]), f"{what}: frame {k} of a batch of {n} differs from the single-frame result"
            assert_close(N(outs[k]), want[k], 0, 3e-6, f"fused, batch of {n}")
    infos = _live_plans_fused(shape)
    assert len(infos) == 1 and infos[0]["fused"]  # (the batch plan replaced the single-frame one)
    if shape in STATIC_SIZES:
        assert (infos[0]["static_rows"], infos[0]["static_cols"]) == STATIC_SIZES[shape], infos[0]
    monkeypatch.setenv("HHSR_GREY_PLAN", "0")
    utils_image._grey_plans.clear()
    lib = utils_image.compute_grey_images(ti[0], "FFT")
    assert not _live_plans_fused(shape)[0]["fused"]
    assert_close(N(lib), want[0], 0, 3e-6, "library plans at the same sizes")
    d = float((lib - single[0]).abs().max())
    print(f"{what}: fused vs library plans, max abs difference {d:.2e}")
    assert d < 2e-6  # (test_grey_fused_vs_library_plans)


@pytest.mark.parametrize("shape", sorted(STATIC_SIZES))
def test_prime_static_plans_equal_run_time_passes(shape, monkeypatch):
    """The compile-time plans with a radix 17 / 19 pass against the run-time passes of the PrimePlan kernels on the same
    tables: rows only, columns only, both; single frame and a batch (bound of
    test_grey_static_plan_passes_equal_run_time_passes)."""
    imgs, _ = _frames(shape, 3)
    ti = [T(i) for i in imgs]
    ti[-1][::2] *= 0.25  # (strong vertical frequencies: rows differ)
    rows_id, cols_id = STATIC_SIZES[shape]

    def run(mask, n):
        monkeypatch.setenv("HHSR_FFT_STATIC", str(mask))
        utils_image._grey_plans.clear()
        outs = ([utils_image.compute_grey_images(ti[0], "FFT").clone()] if n == 1 else
                [o.clone() for o in utils_image.compute_grey_images_batch(ti[:n], "FFT")])
        info = _live_plans_fused(shape)[0]
        assert info["fused"]
        assert info["static_rows"] == (rows_id if mask & 1 else 0) and info["static_cols"] == (cols_id if mask & 2 else 0), info
        return outs

    worst = 0.0
    for n in (1, 3):
        want = run(0, n)
        for mask in (1, 2, 3):
            got = run(mask, n)
            for i in range(n):
                worst = max(worst, float((got[i] - want[i]).abs().max()))
    print(f"{shape}: static plans vs run-time passes, max abs difference {worst:.2e}")
    assert worst < 2e-6


@pytest.mark.parametrize("shape", [(323, 646), (286, 572)])
def test_prime_forced_variants(shape, monkeypatch):
    """One kept column per workgroup (HHSR_FFT_NC=1) is bit-identical to two; row pairs in 512-thread workgroups
    (HHSR_FFT_NT_ROWS=512) agree with one row per 256 threads — at sizes where every pass list holds a prime radix."""
    img, want = _case(shape)
    t = T(img)
    outs = {}
    for nc in ("2", "1"):
        monkeypatch.setenv("HHSR_FFT_NC", nc)
        utils_image._grey_plans.clear()
        outs[nc] = N(utils_image.compute_grey_images(t, "FFT"))
        info = _live_plans_fused(shape)[0]
        assert info["fused"] and info["cols_per_workgroup"] == int(nc), info
        assert_close(outs[nc], want, 0, 3e-6, f"columns per workgroup {nc}")
    assert np.array_equal(outs["1"], outs["2"])
    monkeypatch.delenv("HHSR_FFT_NC")
    for nt in ("256", "512"):
        monkeypatch.setenv("HHSR_FFT_NT_ROWS", nt)
        utils_image._grey_plans.clear()
        outs[nt] = N(utils_image.compute_grey_images(t, "FFT"))
        info = _live_plans_fused(shape)[0]
        assert info["fused"] and info["row_threads"] == int(nt), info
        assert_close(outs[nt], want, 0, 3e-6, f"row kernels with {nt} threads")
    assert np.abs(outs["256"] - outs["512"]).max() < 2e-6


def test_prime_constant_image():
    """Constant image in -> the same constant out (DC bin only), as test_grey_fused_radix7_sensor_size checks at 4032 x 3024."""
    flat = torch.full((3072, 4080), 0.37, device=DEV)
    out = utils_image.compute_grey_images(flat, "FFT")
    assert _live_plans_fused((3072, 4080))[0]["fused"]
    assert float((out - 0.37).abs().max()) < 2e-6


def test_prime_size_end_to_end():
    """One burst at 544 x 680 (17 in both transform lengths: 340 = 17 5 4, 544 = 17 16 2) through main() against the oracle:
    no flipped block-matching tile, flows, robustness and image within the tolerances of tests/test_hip_parity.py's
    end-to-end cases."""
    from test_hip_parity import _e2e_vs_oracle

    H, W = 544, 680
    assert utils_image.grey_plan_info(H, W)["fused"]
    ref, comp, _ = synth.make_burst(H, W, 3, seed=1234, max_shift=4.0)
    _e2e_vs_oracle(ref, comp, lambda: base_config(ts=16, scale=1, metrics=("L1", "L2", "L2", "L2")), 16,
                   "prime-factor size 544x680", max_flipped=0)
    infos = _live_plans_fused((H, W))
    assert all(i["fused"] for i in infos), infos


def test_factor_31_size_keeps_the_library_plans():
    """3472 = 2^4 7 31: not fused, and the library plans still match the oracle."""
    shape = (3472, 4624)
    assert not utils_image.grey_plan_info(*shape)["fused"]
    img, want = _case(shape)
    out = utils_image.compute_grey_images(T(img), "FFT")
    assert not _live_plans_fused(shape)[0]["fused"]
    assert_close(N(out), want, 0, 3e-6, "3472x4624 library plans")


def test_zz_wall_time_of_this_file():
    """Prints what the tests above took (the oracle's float64 FFTs are the cost); the file's budget in the GPU suite is a
    minute."""
    print(f"tests/test_fft_primes.py: {_SPENT[0]:.1f} s in its tests")
