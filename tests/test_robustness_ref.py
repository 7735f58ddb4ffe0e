"""The oracle of the robustness stage (oracle/robustness.py) held on the CPU at the cases of tests/robustness_cases.py, and
those cases held to what they are for:

* a per-pixel scalar restatement of the reference's warp-upsample (robustness.py:380-415), bit for bit, +inf pattern included;
* the branch census: which (geometry, field) reaches which decision of rob_axis / rob_centre / dodgson3 / rob_row4;
* the transition band: 1 % .. 90 % of the oracle's R lie strictly between 0 and 1 under `ties` and `edges`;
* oracle.compute_s against the reference's statement (NaN neighbours are skipped: fmaxf / fminf), oracle.local_min against a
  25-tap loop, and the constructed S spreads / sigma means against the values they are named after.

Census: stored pixels of each (geometry, field) per branch (keys and their kernel branches: robustness_cases docstring;
columns in the order of robustness_cases.CENSUS_KEYS; an event on either axis counts):

    case                            in     out    tie+    tie-     l=0    n0in   n0out   l=len    nLin   nLout  lowtap hightap  shared   perpx   other  otherB  origin     !ok
    80x112_ts16 ties              8706     254    1760    1760      48      16      96      64       0       0     237     265    8232     474     705       0       0       0
    80x112_ts16 edges             6379    2581    1168    1120      48      32      64      48      32      80     173     397    6034     345     392       0    1536       0
    80x112_ts16 invalid           4240    4720     992    1008      48      16      64      16       0       0     112      96    4064     176     328       0     768    3840
    80x114_ts32 ties              8988     132    1320    1318       0      50      48      50       0       0     160     332    8642     346     312      78       0       0
    80x114_ts32 edges             5821    3299    1248    1216      96      16      50      80      32      32     239     313    5596     225     237      21    2400       0
    80x114_ts32 invalid           4380    4740    1160    1190       0      50      32      50       0       0      81     238    4192     188     184      46    1024    3648
    80x112_ts64 ties              8769     191    2128    2176      48      64      80      64       0       0     237     301    8342     427     869       0       0       0
    80x112_ts64 edges             4402    4558    2944    2816     128       0      16     128       0      48     256     106    4144     258     854       0    4096       0
    80x112_ts64 invalid           3969    4991    1936    1984      48       0      80      64       0       0     110     189    3732     237     693       0    4096     768
    80x112_ts8 ties               8677     283    1464    1464      48      24      80      72       0       0     221     255    8232     445     603       0       0       0
    80x112_ts8 edges              7268    1692    1136    1096      48      32      48      40      40      48     162     288    6992     276     452       0     640       0
    80x112_ts8 invalid            7204    1756    1312    1304      40      16      80      72       0       0     136     247    6836     368     496       0     256    1280
    18x20_ts16 ties                296      64      50      38       4       0      34      16       0       0      37      75     192     104       0       0       0       0
    18x20_ts16 edges               161     199     112     112      32       0       2      32       0       0      51       5     108      53      26       0     104       0
    18x20_ts16 invalid              78     282      48      36       4       0      18      16       0       0       8      65      24      54       0       0     256       8
    4x6_ts16 ties                   20       4       0       0       0       6       4       0       0       0       9      23       0      20       0       0       0       0
    4x6_ts16 edges                  12      12       4      10       6       0       0       4       0       0       8      13       0      12       0       0       0       0
    4x6_ts16 invalid                 0      24       0       0       0       6       0       0       0       0       0       0       0       0       0       0      24       0
    grey_48x64_ts16 ties          3040      32     640     640       0      48      32       0       0       0      80       0    2960      80     256       0       0       0
    grey_48x64_ts16 edges         1523    1549     400     352      48      16      32      48      16      16     125     132    1416     107      36       0    1024       0
    grey_48x64_ts16 invalid       1504    1568     512     512       0      32      32       0       0       0      48       0    1456      48     128       0     256    1280
    grey_48x66_ts16 ties          3021     147     640     688      32      32      50       0       0       0     144       0    2804     217     240       0       0       0
    grey_48x66_ts16 edges         1808    1360     488     456      48      18      32      48      16      18     128     139    1712      96     182       0     800       0
    grey_48x66_ts16 invalid       1520    1648     456     472      16      16      50       0       0       0      48       0    1440      80     128       0     512    1088
"""
import functools

import numpy as np
import pytest

import oracle
import robustness_cases as rc

F32, F64 = np.float32, np.float64
CASES = [(g, f) for g in rc.GEOMETRIES for f in rc.FIELDS]
case_ids = dict(ids=lambda c: f"{c[0].name}-{c[1]}")


def same_bits(got, want, what):
    assert got.dtype == want.dtype == np.float32 and got.shape == want.shape, what
    assert np.array_equal(np.isnan(got), np.isnan(want)), f"{what}: NaN masks differ"
    ok = np.isnan(want) | (got.view(np.uint32) == want.view(np.uint32))
    assert ok.all(), f"{what}: {int((~ok).sum())} values differ, first at {tuple(np.argwhere(~ok)[0])}"


def _dodgson(x):  # utils_image.py:399-406
    x = abs(x)
    if x <= 0.5:
        return -2 * x * x + 1
    if x <= 1.5:
        return x * x - 5 / 2 * x + 1.5
    return 0.0


def upscale_scalar(LR, out_shape, tile_size, flow):
    """cuda_uspcale_dogson (robustness.py:359-421), thread by thread: Python floats are float64; the buffer is float32 and
    takes float32 * float64 + itself, rounded at every tap; s = 2 whatever the map's size."""
    nc, LR_ny, LR_nx = LR.shape
    H, W = out_shape
    HR = np.empty((nc, H, W), F32)
    lr = LR.astype(F64).tolist()  # float32 -> float64 is exact
    f32 = F32
    for y in range(H):
        for x in range(W):
            flow_x = float(flow[y // tile_size, x // tile_size, 0])
            flow_y = float(flow[y // tile_size, x // tile_size, 1])
            LR_y = (y + flow_y + 0.5) / 2 - 0.5
            LR_x = (x + flow_x + 0.5) / 2 - 0.5
            if not (0 <= LR_y < LR_ny and 0 <= LR_x < LR_nx):
                HR[:, y, x] = np.inf
                continue
            center_y, center_x = round(LR_y), round(LR_x)  # round-half-even
            w_acc = 0.0
            buf = [0.0] * nc
            for i in range(-1, 2):
                y_ = int(min(max(center_y + i, 0), LR_ny - 1))
                wy = _dodgson(y_ - LR_y)
                for j in range(-1, 2):
                    x_ = int(min(max(center_x + j, 0), LR_nx - 1))
                    w = wy * _dodgson(x_ - LR_x)
                    for c in range(nc):
                        buf[c] = float(f32(buf[c] + lr[c][y_][x_] * w))
                    w_acc += w
            for c in range(nc):
                HR[c, y, x] = buf[c] / w_acc if w_acc != 0 else np.nan
    return HR


@pytest.mark.parametrize("case", CASES, **case_ids)
def test_scalar_restatement(case):
    g, name = case
    m = rc.oracle_maps(g, name)
    with np.errstate(all="ignore"):
        want = upscale_scalar(m["cm"], (g.H, g.W), g.ts, rc.field(g, name))
    same_bits(np.asarray(m["comp_means_up"]), want, f"{g.name} {name}: oracle.upscale_warp_stats vs the scalar statement")
    ly, lx = rc.positions(g, rc.field(g, name))
    lh, lw = rc.lens(g)
    with np.errstate(all="ignore"):
        outside = ~((ly >= 0) & (ly < lh) & (lx >= 0) & (lx < lw))
    assert np.array_equal(np.isinf(want[0]), outside)


@functools.lru_cache(maxsize=None)
def census_table():
    return {(g.name, f): rc.census(g, rc.field(g, f)) for g, f in CASES}


def format_census():
    short = ["in", "out", "tie+", "tie-", "l=0", "n0in", "n0out", "l=len", "nLin", "nLout", "lowtap", "hightap", "shared",
             "perpx", "other", "otherB", "origin", "!ok"]
    lines = ["    " + "case".ljust(26) + "".join(s.rjust(8) for s in short)]
    for (gn, f), row in census_table().items():
        lines.append("    " + f"{gn} {f}".ljust(26) + "".join(str(row[k]).rjust(8) for k in rc.CENSUS_KEYS))
    return "\n".join(lines)


def test_branch_census():
    """Every branch of the robustness_cases docstring is reached by stored pixels; every Bayer geometry of the fused kernel
    reaches the ties, the edge equalities and the clamped window origin.  The table in this module's docstring is this
    census."""
    table = census_table()
    print("\n" + format_census())
    total = {k: sum(row[k] for row in table.values()) for k in rc.CENSUS_KEYS}
    for k in rc.CENSUS_KEYS:
        assert total[k] > 0, k
    for g in rc.GEOMETRIES:
        rows = [table[g.name, f] for f in rc.FIELDS]
        if g.mode == "bayer" and g.ts % 16 == 0:
            for k in ("tie up", "tie down", "l == 0", "l == len", "clamped origin"):
                assert sum(r[k] for r in rows) > 0, (g.name, k)
        assert rc.kernel_of(g) == g.kernel
    # the ties with the partner pixel at the clamped border: only a width of 2 mod 4 has them (lw odd), see rob_row4
    assert table["80x114_ts32", "ties"]["other way at border"] > 0
    assert format_census() in __doc__, "the census table of the module docstring is out of date"


def test_tie_values_land_on_both_parities():
    """Each special value of `ties` meets pixels with an even and with an odd n = p + floor(f) >> 1 (a tile is at least 8
    pixels wide), and every listed value is in some field of the largest grid."""
    g = rc.GEOMETRIES[3]
    fl = rc.field(g, "ties")
    for v in rc.TIE_VALUES:
        hit = (fl.view(np.uint32) == np.array(v, F32).view(np.uint32))
        assert hit[..., 0].any() and hit[..., 1].any(), v
    for ax in (0, 1):
        for v in (0.5, -0.5, 1.5, -1.5, 2.5):
            ty, tx = np.argwhere(fl[..., ax] == F32(v))[0]
            p = np.arange(g.ts) + (tx if ax == 0 else ty) * g.ts
            l = (p + float(v) + 0.5) / 2 - 0.5
            tie = l[l - np.floor(l) == 0.5]
            assert (np.floor(tie) % 2 == 0).any() and (np.floor(tie) % 2 == 1).any(), v


@pytest.mark.parametrize("case", [c for c in CASES if c[1] != "invalid"], **case_ids)
def test_transition_band(case):
    g, name = case
    R = rc.oracle_maps(g, name)["R"]
    band = float(((R > 0) & (R < 1)).mean())
    print(f"{g.name} {name}: {band:.3f} of R strictly inside (0, 1), {float((R == 1).mean()):.3f} at 1")
    assert 0.01 <= band <= 0.9
    outside = np.isinf(rc.oracle_maps(g, name)["comp_means_up"][0])
    assert (R[outside] == 0).all()


# ---- S ------------------------------------------------------------------------------------------------------------------------
def test_s_spreads_are_what_they_are_named():
    q = F32(0.25)
    for name, (a, b) in rc.S_SPREADS.items():
        a, b = F32(a), F32(b)
        m = F32(F32(a * a) + F32(b * b))
        fused = F32(F64(a) * F64(a) + F64(b) * F64(b)) if name in ("below", "above") else m  # (exact in float64)
        want = {"equal": q, "equal_34": q, "below": np.nextafter(q, F32(0)), "above": np.nextafter(q, F32(1))}[name]
        assert m == want and fused == want, (name, m, fused)


@pytest.mark.parametrize("name", list(rc.s_cases()))
def test_compute_s_follows_the_statement(name):
    """oracle.compute_s == robustness.py:570-612 tile by tile.  A NaN flow is skipped by the running maximum / minimum
    (Numba lowers max / min of two float32 in a CUDA kernel to libdevice's fmaxf / fminf): a tile with a
    NaN neighbour gets the weight of its other neighbours, not s2."""
    flow, Mt = rc.s_cases()[name]
    want = rc.s_statement(flow, Mt)
    got = oracle.compute_s(flow, Mt, rc.S1, rc.S2)
    assert got.dtype == np.float32 and np.array_equal(got, want), (name, got, want)
    if name.endswith(("_equal", "_equal_34", "_below")):
        assert (got == rc.S2).all()  # m == Mt^2 is not above it
    if name.endswith("_above") and flow.shape[:2] != (1, 1):
        assert got[flow.shape[0] // 2, flow.shape[1] // 2] == rc.S1 and (got == rc.S1).sum() >= 2
    if name.endswith("_all_nan"):
        assert got[0, 0] == rc.S2 and got[-1, -1] == rc.S1  # no number in the neighbourhood: inf - (-inf) spreads
    if name == "3x4_nan":
        assert (got == rc.S2).all()  # spreads of 0.4 at most, the NaN skipped
    if name.endswith("_inf"):
        assert (got == rc.S1).any()


def test_s_cases_cover_both_weights():
    both = [set(np.unique(rc.s_statement(f, mt)).tolist()) for f, mt in rc.s_cases().values()]
    assert {rc.S2} in both and {rc.S1, rc.S2} in both


# ---- sigma^2, local minimum -------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("ncurve", rc.NCURVES)
def test_sigma_cases(ncurve):
    means, vars_, std, dif = rc.sigma_case(ncurve)
    idx = rc.sigma_index(means, ncurve)
    assert len(std) == len(dif) == ncurve and idx.min() == 0 and idx.max() == ncurve - 1
    for c in range(3):
        for v in rc.SIGMA_SPECIALS:
            hit = np.isnan(means[c]) if np.isnan(v) else (means[c].view(np.uint32) == np.array(v, F32).view(np.uint32))
            assert hit.sum() >= 2, (c, v)
    if ncurve == 1001:  # the exact .5 ties of 1000 b go to the even index
        assert set(idx[means == F32(0.0625)]) == {62} and set(idx[means == F32(0.1875)]) == {188}
        assert set(idx[means == F32(7.0)]) == {1000} and set(idx[means == F32(-0.5)]) == {0}
    if ncurve == 1024:
        assert set(idx[means == F32(1.0235)]) == {1023}
    st2 = (std * std)[idx]
    fin = np.isfinite(means)
    assert (vars_[fin] > st2[fin]).any() and (vars_[fin] < st2[fin]).any()
    d_p = np.zeros_like(means)
    _, s_sq = oracle.robustness.apply_noise_model(d_p, means, vars_, std, dif)
    want = np.maximum(vars_.astype(F64), st2).sum(0).astype(F32)
    assert np.array_equal(s_sq, want)


@pytest.mark.parametrize("shape", rc.LOCAL_MIN_SHAPES, ids=lambda s: f"{s[0]}x{s[1]}")
def test_local_min_follows_the_loops(shape):
    R = rc.local_min_case(shape)
    got = oracle.local_min(R)
    assert got.dtype == np.float32 and np.array_equal(got, rc.local_min_loops(R))
    if R.size > 1:
        assert R.min() == 0 and R.max() == 1
