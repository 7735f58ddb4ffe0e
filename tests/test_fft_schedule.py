"""The host side of the fused FFT kernels (csrc/hhsr_fft.hip: radix_search / factorize / pick_rb) through the library's
query entry points — no GPU: which image sizes the fused kernels take, with what schedule, and that the schedules of the
7-smooth lengths are what they were before the prime radices 11, 13, 17, 19 existed."""
import ctypes
import json
import os

import pytest

from handheld_super_resolution import _lib, utils_image

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "fft_schedules_7smooth.json")
FFT_ENV = ("HHSR_GREY_PLAN", "HHSR_FFT_NC", "HHSR_FFT_NT_ROWS", "HHSR_FFT_STATIC")

# (H, W): sensor sizes with 11, 13, 17 or 19 in H or W / 2, and toy sizes that carry every one of them
FUSED = [(3072, 4080), (3648, 5472), (6120, 8160), (2448, 3264), (3264, 4896), (2736, 3648), (4160, 6240), (323, 646),
         (342, 476), (544, 680), (286, 572)]
# 3472 = 2^4 7 31;  odd width;  W / 2 = 23 * 16;  H = 23 * 16
NOT_FUSED = [(3472, 4624), (3000, 4001), (480, 736), (368, 640)]


@pytest.fixture(autouse=True)
def _plain_environment(monkeypatch):
    for name in FFT_ENV:
        monkeypatch.delenv(name, raising=False)


def _prod(xs):
    p = 1
    for x in xs:
        p *= x
    return p


@pytest.mark.parametrize("shape", FUSED)
def test_prime_factor_sizes_take_the_fused_kernels(shape):
    H, W = shape
    info = utils_image.grey_plan_info(H, W)
    assert info["fused"], info
    assert _prod(info["radices_rows"]) == W // 2 and _prod(info["radices_cols"]) == H, info
    assert all(2 <= r <= 19 for r in info["radices_rows"] + info["radices_cols"])
    assert {11, 13, 17, 19} & set(info["radices_rows"] + info["radices_cols"])
    assert info["rows_per_workgroup"] in (1, 2, 4) and info["cols_per_workgroup"] in (1, 2)
    assert (info["row_threads"], info["rows_per_workgroup"]) in ((256, 1), (512, 1), (512, 2), (512, 4))
    assert 0 < info["lds_rows"] <= 150 * 1024 and 0 < info["lds_cols"] <= 150 * 1024
    assert W // 4 <= info["kept_bins"] <= W // 4 + 2  # (the highest kept x-bin + 1)


@pytest.mark.parametrize("shape", NOT_FUSED)
def test_other_sizes_keep_the_library_plans(shape):
    info = utils_image.grey_plan_info(*shape)
    assert not info["fused"] and info["radices_rows"] == [] and info["radices_cols"] == [], info


def test_query_follows_the_plan_flags(monkeypatch):
    """HHSR_GREY_PLAN=0 (the library route on the same build) is what the query reports too; argument errors are host-side."""
    monkeypatch.setenv("HHSR_GREY_PLAN", "0")
    assert not utils_image.grey_plan_info(3000, 4000)["fused"]
    monkeypatch.delenv("HHSR_GREY_PLAN")
    assert utils_image.grey_plan_info(3000, 4000)["fused"]
    lib = _lib.load()
    rec = (ctypes.c_int32 * _lib.GREY_INFO_LEN)()
    assert lib.hhsr_grey_plan_query(3000, 4000, 4, rec, _lib.GREY_INFO_LEN - 1) == -1
    assert lib.hhsr_grey_plan_query(3000, 4000, 4, None, _lib.GREY_INFO_LEN) == -1
    assert lib.hhsr_grey_plan_info(None, rec, _lib.GREY_INFO_LEN) == -1


def test_static_plans_are_picked_for_their_sizes():
    """The compile-time plans are used only when the schedule search picks exactly their radices: ids as in
    HHSR_STATIC_ROWS / HHSR_STATIC_COLS."""
    want = {(3000, 4000): (1, 1, [10, 10, 10, 2], [3, 10, 10, 10]),
            (6000, 8000): (2, 2, [10, 10, 10, 4], [10, 10, 10, 6]),
            (3024, 4032): (3, 3, [14, 12, 12], [9, 8, 7, 6]),
            (3072, 4080): (4, 0, [17, 15, 8], None),
            (3648, 5472): (5, 4, [19, 16, 9], [19, 16, 12])}
    for (H, W), (sr, sc, rr, rc) in want.items():
        info = utils_image.grey_plan_info(H, W)
        assert (info["static_rows"], info["static_cols"]) == (sr, sc), (H, W, info)
        assert info["radices_rows"] == rr and (rc is None or info["radices_cols"] == rc), (H, W, info)
    info = utils_image.grey_plan_info(3072, 4080)
    assert (info["rows_per_workgroup"], info["row_threads"]) == (1, 256) and info["lds_rows"] <= 32 * 1024
    info = utils_image.grey_plan_info(3648, 5472)
    assert (info["rows_per_workgroup"], info["row_threads"], info["cols_per_workgroup"]) == (2, 512, 2)


def test_static_switch_shows_in_the_query(monkeypatch):
    monkeypatch.setenv("HHSR_FFT_STATIC", "0")
    info = utils_image.grey_plan_info(3648, 5472)
    assert info["fused"] and (info["static_rows"], info["static_cols"]) == (0, 0)
    assert info["radices_rows"] == [19, 16, 9]


def test_schedules_of_7_smooth_lengths_are_unchanged():
    """Every 7-smooth length up to 8192, for each (sequences per workgroup, threads) combination that pick_rb and the column
    loop ask for: the schedule recorded before the prime radices were added to the search."""
    with open(GOLDEN) as f:
        g = json.load(f)
    combos = [tuple(c) for c in g["combos"]]
    assert combos == [(1, 256), (1, 512), (2, 512), (4, 512)]
    assert len(g["schedules"]) == 316  # 7-smooth numbers in 2 .. 8192
    bad = []
    for n, want in g["schedules"].items():
        for (nb, nt), w in zip(combos, want):
            got = utils_image.grey_radix_schedule(int(n), nb, nt)
            if got != w:
                bad.append((n, nb, nt, got, w))
            assert not got or (_prod(got) == int(n) and max(got) <= 16)
    assert not bad, bad[:10]


def test_prime_schedules_of_the_sensor_lengths():
    """What the search picks for the lengths that motivated the prime radices."""
    assert utils_image.grey_radix_schedule(2040, 1, 256) == [17, 15, 8]
    assert utils_image.grey_radix_schedule(2736, 2, 512) == [19, 16, 9]
    assert utils_image.grey_radix_schedule(3648, 2, 512) == [19, 16, 12]
    assert utils_image.grey_radix_schedule(4080, 1, 512) == [17, 16, 15]
    assert utils_image.grey_radix_schedule(6120, 1, 512) == [17, 15, 8, 3]
    assert utils_image.grey_radix_schedule(23 * 16, 1, 512) == []
    assert utils_image.grey_radix_schedule(6936, 1, 512) == []  # 17 17 24: no split of 24 fits 512 threads
