"""The oracle of the per-frame pass (oracle.estimate_kernels, oracle.guide_image, oracle.local_stats) held on the CPU at the
cases of tests/frame_stats_cases.py, and those cases held to what they are for:

* a per-quad scalar restatement of the reference's statements (bit for bit, NaN masks included);
* a plain float64 computation of Alg. 5 on the well-conditioned quads, which yields the bound the GPU test reuses;
* the branch census: which image reaches which branch of quad_cov, and that together they reach all of them;
* the hard-threshold rule: at most 0.1 % of a case's quads lie within 1e-5 of the discontinuity A = 1.95.

Case against branch reached (quads over the ten shapes of frame_stats_cases.SHAPES, 7122 per family; hard threshold at the
tuning of SNR 12; "arg<=0" counts raw pixels).  D is 1 - sqrt(l1) / D_tr + D_th before its clamps; a0, a1 outside the
identity branch; "fin": finite covariance (under the linear law a NaN anisotropy makes the covariance NaN: the D >= 1
column is then 0 for the flat images and the steps' flat sides):

    family      D<=0   band  D>=1 fin   A==2   l2<0  A NaN  a0==0  a1==0  both 0  ident T!=0  T01==0 T00!=T11  arg<=0
    noise       7047      0        75     20     13     75      0      0       0           0                0       0
    low_noise      0      0      7122     20     14     75      0      0       0           0                0       0
    ramp_x         0   2642      4480   7047   4200     75      0      0       0           0             7047       0
    ramp_y         0   6602       520   7047   4180     75      0      0       0           0             7047       0
    ramp_xy        0    662      6460   6610   3573     75      0      0       0           0                0       0
    step_v       170      0      6952    170    170   6952      0      0       0           0              170       0
    step_h       714      0      6408    714    714   6408      0      0       0           0              714       0
    step_d1      328      0      6794    328    328   6794      0      0       0           0                0       0
    step_d2      328      0      6794    328    328   6794      0      0       0           0                0       0
    step_noise   170      0      6952     21     10     75      0      0       0           0                0       0
    checker     7033      0        89    850      0     89      0      0       0        6183              850       0
    flat           0      0      7122      0      0   7122      0      0       0           0                0       0
    zeros          0      0      7122      0      0   7122      0      0       0           0                0       0
    negative       0      0      7122      0      0   7122      0      0       0           0                0   28488
    neg_beta    7047      0        75     20     12     75      0      0       0           0                0   14240
    dynamic     6918    103       101     21     11     75      0      0       0           0                0       0
    nan_inner   7047      0        75     20      8     75      0      0       0           0                0       0
    nan_corner  7046      1        75     22      8     75      0      0       0           0                0       0
    sm_x           0   7047        75   7047      0     75      0   7047       0           0             7047       0
    sm_y           0   7047        75   7047      0     75   7047      0       0           0             7047       0
    sm_diag     5055   1992        75   5827      0     75   2911   2911    2911        1220                0       0
    sm_iso      2877   4170        75   3589      0     75   1792   1792    1792        3458                0       0

The 75 NaN anisotropies of every family are the quads of the six degenerate shapes without a gradient sample.  "both 0":
a0 == a1 == 0 outside the identity case, a gradient exactly along the anti-diagonal, where the reference answers
e1 = (0, 1) instead of (1, -1) / sqrt 2 (reproduced bit for bit, left out of the float64 comparison).

`fabs(r1) < fabs(r2)` is reached by no input: T00 and T11 are sums of squares, so -b = T00 + T11 >= 0 and
sq = sqrt(max(delta, 0)) >= 0, hence r1 = (-b + sq) / 2 >= |(-b - sq) / 2| = |r2| whenever both are numbers; with a NaN the
comparison is false, both roots are NaN and the two assignments store the same bits.  |r1| == |r2| needs sq == 0 (r1 and r2
are then the same number) or b == 0 (then T00 = T11 = 0, their product T01 underflows with them and r1 = r2 = 0): the
branch never changes a result, and neither does replacing `>=` by `>`.  The census counts the case and asserts 0."""
import functools

import numpy as np
import pytest

import frame_stats_cases as fc
import oracle
from helpers import ALPHA, BETA


def test_constants_follow_the_helpers():
    assert (fc.ALPHA, fc.BETA) == (float(ALPHA), float(BETA))
    t = fc.config().merging.tuning
    assert (t.k_detail, t.k_denoise, t.D_th, t.D_tr) == (0.31, 4.5, 0.785, 1.18)  # the tuning the census was taken at


def test_raw_for_gat_hits_its_targets():
    for k in (0, 1, 7, 16):
        target = np.float32(96.0 + 2.0 * k)
        v = fc.raw_for_gat(target, fc.ALPHA, fc.BETA)
        assert v.dtype == np.float32 and 0 < v < 1
        assert oracle.kernels.gat(np.array([v]), fc.ALPHA, fc.BETA)[0] == target


def same_bits(got, want, what):
    assert got.dtype == want.dtype == np.float32 and got.shape == want.shape, what
    assert np.array_equal(np.isnan(got), np.isnan(want)), f"{what}: NaN masks differ"
    ok = np.isnan(want) | (got.view(np.uint32) == want.view(np.uint32))
    assert ok.all(), f"{what}: {int((~ok).sum())} values differ, first at {tuple(np.argwhere(~ok)[0])}"


@pytest.mark.parametrize("family", fc.STAT_FAMILIES)
@pytest.mark.parametrize("shape", fc.REF_SHAPES, ids=lambda s: f"{s[0]}x{s[1]}")
def test_scalar_restatement(shape, family):
    """oracle.guide_image / local_stats (Bayer with a white balance, and the frame as its own guide) and
    oracle.estimate_kernels (both laws, Bayer and grey mode) against the per-quad loops of frame_stats_cases on np.float32 /
    np.float64 scalars: equal bit for bit, the sign of a zero included."""
    raw = fc.image(family, *shape)
    guide = oracle.guide_image(raw, fc.GOLDEN_CFA, fc.GOLDEN_WB)
    same_bits(guide, fc.guide_scalar(raw, fc.GOLDEN_CFA, fc.GOLDEN_WB), "guide")
    for g, what in ((guide, "bayer"), (np.asarray(raw)[None], "grey")):
        with np.errstate(all="ignore"):
            m, v = oracle.local_stats(g)
        ms, vs = fc.local_stats_scalar(g)
        same_bits(m, ms, f"{what} means")
        same_bits(v, vs, f"{what} variances")
    if family not in fc.COV_FAMILIES:
        return
    for mode in ("bayer", "grey"):
        for law in fc.LAWS:
            cfg = fc.family_config(family, law, mode)
            same_bits(oracle.estimate_kernels(raw, cfg), fc.cov_scalar(raw, cfg), f"{mode} {law} covariances")


@functools.lru_cache(maxsize=None)
def _case(family, shape, law, mode="bayer"):
    raw = fc.image(family, *shape)
    cfg = fc.family_config(family, law, mode)
    return raw, cfg, oracle.estimate_kernels(raw, cfg)


@functools.lru_cache(maxsize=None)
def census_table(law):
    """{family: {key: count over fc.SHAPES}}"""
    table = {}
    for family in fc.COV_FAMILIES:
        row = dict.fromkeys(fc.CENSUS_KEYS, 0)
        for shape in fc.SHAPES:
            for k, n in fc.census(*_case(family, shape, law)).items():
                row[k] += n
        table[family] = row
    return table


@pytest.mark.parametrize("law", fc.LAWS)
def test_branch_census(law):
    """Taken together the cases reach every branch of quad_cov with a non-trivial count (the table of this module's
    docstring is this census under the hard threshold)."""
    table = census_table(law)
    total = {k: sum(row[k] for row in table.values()) for k in fc.CENSUS_KEYS}
    print(law, total)
    for k in ("D<=0", "D>=1 finite", "A==2", "l2<0", "A NaN", "a0==0", "a1==0", "ident T!=0", "T01==0 T00!=T11", "gat arg<=0"):
        assert total[k] >= 100, (k, total[k])
    assert total["D band"] >= 1000
    assert total["|r1|<|r2|"] == 0  # (module docstring: no input can)
    # what each structured family is for
    n = table["noise"]["D<=0"] + table["noise"]["D>=1 finite"] + table["noise"]["D band"] + (
        table["noise"]["A NaN"] if law == "linear" else 0)
    gradient = n - table["noise"]["A NaN"]  # quads with at least one gradient sample
    assert table["ramp_x"]["T01==0 T00!=T11"] == table["ramp_x"]["A==2"] == gradient
    assert table["ramp_x"]["D band"] >= 1000 and table["ramp_y"]["D band"] >= 1000
    assert table["low_noise"]["D>=1 finite"] >= gradient
    assert table["step_v"]["l2<0"] >= 100 and table["step_h"]["l2<0"] >= 100
    assert table["negative"]["gat arg<=0"] == 4 * n
    assert 0.4 < table["neg_beta"]["gat arg<=0"] / (4 * n) < 0.6
    assert table["sm_x"]["a1==0"] == table["sm_x"]["D band"] == gradient and table["sm_x"]["a0==0"] == 0
    assert table["sm_y"]["a0==0"] == table["sm_y"]["D band"] == gradient and table["sm_y"]["a1==0"] == 0
    assert table["sm_diag"]["a0==a1==0"] >= 1000  # 
    assert table["sm_iso"]["ident T!=0"] >= 1000 and table["checker"]["ident T!=0"] >= 1000


def test_short_mantissa_tensors_are_exact():
    """The four short-mantissa images at 34 x 66: every gradient is a multiple of 1/2 and l2 == 0 exactly wherever the
    tensor has rank 1; `a0 == 0` and `a1 == 0` occur outside the identity case; the 45-degree image has
    T00 == T11 == |T01| != 0 and the isotropic one T01 == 0, T00 == T11 != 0."""
    cfg = fc.config("linear")
    m = {f: fc.intermediates(fc.image(f, 34, 66), cfg) for f in ("sm_x", "sm_y", "sm_diag", "sm_iso")}
    for f, v in m.items():
        for k in ("T00", "T01", "T11"):
            assert np.array_equal(v[k] * 4, np.rint(v[k] * 4)) and np.abs(v[k]).max() <= 16, (f, k)
    x, y, d, iso = m["sm_x"], m["sm_y"], m["sm_diag"], m["sm_iso"]
    assert (x["T00"] > 0).all() and not x["T01"].any() and not x["T11"].any() and not x["l2"].any()
    assert (y["T11"] > 0).all() and not y["T01"].any() and not y["T00"].any() and not y["l2"].any()
    assert (~x["ident"] & (x["a1"] == 0) & (x["a0"] != 0)).all() and (~y["ident"] & (y["a0"] == 0) & (y["a1"] != 0)).all()
    rank1 = (d["T00"] == d["T11"]) & (np.abs(d["T01"]) == d["T00"]) & (d["T00"] > 0)
    assert rank1.sum() > 400 and not d["l2"][rank1].any()
    assert (iso["ident"] & (iso["T00"] > 0)).sum() > 100


@pytest.mark.parametrize("mode", ["bayer", "grey"])
def test_hard_threshold_cap(mode):
    """From the oracle alone: the quads within 1e-5 of A = 1.95, which the covariance comparison leaves out under the hard
    threshold, are at most 0.1 % of every case (a case that is not gets another seed, the cap stays)."""
    for family in fc.COV_FAMILIES:
        for shape in fc.SHAPES:
            raw, cfg, _ = _case(family, shape, "hard_threshold", mode)
            left = int((~fc.compared(raw, cfg)).sum())
            assert left <= fc.MAX_LEFT_OUT * (raw.size // 4 if mode == "bayer" else raw.size), (family, shape, left)
            assert fc.compared(raw, fc.family_config(family, "linear", mode)).all()


def test_float64_reference():
    """The oracle against Alg. 5 in float64 (structure tensor, numpy.linalg.eigh, the same k1 / k2 formulas) on the quads
    with a finite A, (l1 - l2) / (l1 + l2) > 0.05 and D strictly inside (0, 1), every Bayer case, both laws: the largest
    difference relative to the quad's largest entry IS frame_stats_cases.F64_SPREAD (2.134e-5, written down there with its
    cause); the GPU test compares the kernel with the same float64 computation under 4 x that figure."""
    worst, where, quads = 0.0, None, 0
    for law in fc.LAWS:
        for family in fc.COV_FAMILIES:
            for shape in fc.SHAPES:
                raw, cfg, covs = _case(family, shape, law)
                s, n = fc.f64_spread(covs, raw, cfg)
                quads += n
                if s > worst:
                    worst, where = s, (law, family, shape)
    print(f"oracle vs float64 on {quads} well-conditioned quads: {worst:.4e} at {where}; bound {fc.F64_BOUND:.3e}")
    assert quads >= 10000
    assert 0.95 * fc.F64_SPREAD < worst <= fc.F64_SPREAD, (worst, where)
    assert fc.F64_BOUND == 4 * fc.F64_SPREAD
