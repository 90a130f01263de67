"""CPU: the inputs of tests/edge_cases.py do what they claim, by the oracle alone, and the planner reaches the variants.

  bound  every |Y| < 2^31 (the contract's precondition) and both max Y and -min Y at least the case's stated fraction
         of 2^31 (less 0.001): the int32 accumulators are driven to the edge of their range in both directions
  limb   the Q14 table holds W = +-32639 and the limbs hi = +-127, lo = -128, lo = +127, split as the contract does
  sat    the oracle output holds +127 and -127, never -128, and at least 90 % of it is saturated (class (d) rows apart)
  low    the class (d) rows of the bound inputs come out unsaturated at scale 2^5, one count per 512 of y
  fine   hi << 8 alone leaves the int32 range by more than half a count of the scale; a saturating shift shows
  plan   bf_fused_plan names the expected kernel for every case, with the workspace of bf_fused_workspace_bytes
  float  a NumPy emulation of the f16 hi/lo split over range_gains / range_table is finite, meets the bound the GPU
         tests use, and misses it once the 2^-25 sum |x| term is dropped: the tables do exercise the split's floor
"""
import numpy as np
import pytest

import edge_cases as EC
import fused_cases as FC
import oracle as O
from dpdk_dc_sand_amd import _lib

TWO31 = 2 ** 31
_sums = {}


def sums(c):
    """(Y, W, oracle inputs) of a case, computed once per set of inputs (the scale does not enter)."""
    key = c._replace(scale=None, expect=None, frac=None)
    if key not in _sums:
        raw, d, gains = EC.inputs(c)
        _sums[key] = EC.int64_sums(raw, d, gains, bool(c.flags & EC.SIGNED)) + (raw, d, gains)
    return _sums[key]


def ids(cases):
    return [EC.case_id(c) for c in cases]


def test_case_ids_are_unique_and_the_grid_is_left_alone():
    names = ids(EC.INT_CASES)
    assert len(set(names)) == len(names) == sum(
        map(len, (EC.BOUND_CASES, EC.LIMB_CASES, EC.SAT_CASES, EC.LOW_CASES, EC.FINE_CASES)))
    assert len(FC.all_calls()) == 181


def test_bound_phases_give_the_largest_coefficient_sum():
    W = O.quantise_coeffs(O.fused_tables(EC.bound_delays(4, 3), 1, 2, EC.CTOT, 3, xeng_id=EC.XENG, t0=EC.T0,
                                         batch_dt=EC.BDT))
    assert set(np.unique(W)) == {-11585, 11585}
    signs = {(int(np.sign(W[0, 0, 0, 0, 2 * m])), int(np.sign(W[0, 0, 0, 0, 2 * m + 1]))) for m in range(4)}
    assert signs == {(1, 1), (-1, 1), (-1, -1), (1, -1)}  # one beam per quadrant
    assert np.float32(EC.G_MAX) == EC.G_MAX and EC.G_MAX * 16384.0 == 32639  # exactly the admitted maximum


def test_sample_classes():
    for signed in (False, True):
        raw = EC.edge_samples(1, 5, 2, 16, signed, 3)
        x = raw.view(np.int8) if signed else raw
        top = -128 if signed else 255
        assert (x[:, :, :, 0, 0] == top).all() and (x[:, :, :, 2, 1] == top).all()  # (a); pol 1 two rows later
        assert (x[:, :, :, 1, 0, 0] == top).all() and (x[:, :, :, 1, 0, 1] == (127 if signed else 0)).all()  # (b)
        assert len(np.unique(x[:, :, :, 2, 0])) > 10  # (c)
        assert not x[:, :4, :, 3, 0].any() and (x[:, 4, :, 3, 0] == ((1, -1) if signed else (1, 0))).all()  # (d)
        assert (x[:, 4, :, 1, 1] == ((1, -1) if signed else (1, 0))).all()


@pytest.mark.parametrize("c", EC.BOUND_CASES[::2], ids=ids(EC.BOUND_CASES[::2]))
def test_bound_cases_reach_their_fraction_of_the_int32_range(c):
    Y = sums(c)[0]
    hi, lo = int(Y.max()), int(Y.min())
    print(f"{EC.case_id(c)}: max Y / 2^31 = {hi / TWO31:.5f}, -min Y / 2^31 = {-lo / TWO31:.5f}")
    assert hi < TWO31 and -lo < TWO31
    assert hi / TWO31 >= c.frac - 0.001 and -lo / TWO31 >= c.frac - 0.001


@pytest.mark.parametrize("c", EC.BOUND_CASES, ids=ids(EC.BOUND_CASES))
def test_bound_cases_do_not_saturate(c):
    """So a sum that wrapped by 2^32 (128 counts at 2^-11, 85.3 at S6 * 2^-8) cannot hide in the clamp."""
    raw, d, gains = sums(c)[2:]
    q = EC.oracle_int8(c, raw, d, gains).astype(int)
    assert np.abs(q).max() <= (64 if c.scale == 2.0 ** -11 else 86)
    assert np.abs(q).max() >= (64 if c.scale == 2.0 ** -11 else 85) * (c.frac - 0.01)


LIMB_INPUTS = [c for c in EC.LIMB_CASES if c.scale == EC.BOUND_SCALES[0]]


@pytest.mark.parametrize("c", LIMB_INPUTS, ids=ids(LIMB_INPUTS))
def test_limb_cases_hold_the_extreme_limbs(c):
    Y, W = sums(c)[:2]
    assert np.abs(Y).max() < TWO31
    lo = ((W + 128) & 255) - 128  # the contract's balanced split: W = 256 hi + lo
    hi = (W - lo) >> 8
    assert (W == 32639).any() and (W == -32639).any() and np.abs(W).max() == 32639
    assert hi.max() == 127 and hi.min() == -127 and lo.min() == -128 and lo.max() == 127
    print(f"{EC.case_id(c)}: max |Y| / 2^31 = {np.abs(Y).max() / TWO31:.5f}")


@pytest.mark.parametrize("c", EC.SAT_CASES, ids=ids(EC.SAT_CASES))
def test_saturation_cases_saturate_both_ways(c):
    raw, d, gains = sums(c)[2:]
    q = EC.oracle_int8(c, raw, d, gains).reshape(c.B, 2, c.C, c.T, 2 * c.M)
    assert (q == 127).any() and (q == -127).any() and not (q == -128).any()
    share = np.mean([(np.abs(q[:, pol][:, :, EC.row_class(c.T, pol) != 3].astype(int)) == 127).mean()
                     for pol in (0, 1)])
    print(f"{EC.case_id(c)}: {share:.3f} saturated")
    assert share >= 0.9
    if c.scale >= 2.0 ** 12:  # beyond the magic add's exact range
        Y = sums(c)[0]
        s = np.float32(np.float32(c.scale) * np.float32(2.0 ** -14))
        assert (np.abs(Y.astype(np.float32) * s) >= 2.0 ** 22).mean() > 0.5


@pytest.mark.parametrize("c", EC.LOW_CASES, ids=ids(EC.LOW_CASES))
def test_low_cases_resolve_one_coefficient(c):
    """On the class (d) rows y is one coefficient of antenna A - 1 (for int8, the difference or sum of two), and the
    output resolves it: every entry unsaturated, most of them nonzero, 512 of y to the count."""
    Y = sums(c)[0]
    raw, d, gains = sums(c)[2:]
    q = EC.oracle_int8(c, raw, d, gains).reshape(c.B, 2, c.C, c.T, 2 * c.M).astype(int)
    for pol in (0, 1):
        rows = EC.row_class(c.T, pol) == 3
        assert np.abs(Y[:, pol][:, :, rows]).max() <= 2 * 32639
        qd = q[:, pol][:, :, rows]
        assert np.abs(qd).max() < 127 and (np.abs(qd) >= 16).mean() >= 0.5
        np.testing.assert_array_equal(qd, np.rint(Y[:, pol][:, :, rows] / 512.0))
    if not c.flags & EC.SIGNED:  # the parts that cancel: the unsigned correction 128 * colsum is of the order of 2^30
        W = sums(c)[1]
        assert np.abs(128 * W.sum(axis=-2)).max() >= 0.49 * c.frac * TWO31


@pytest.mark.parametrize("c", EC.FINE_CASES, ids=ids(EC.FINE_CASES))
def test_fine_cases_need_the_shift_to_wrap(c):
    """The shifted sum of the high limbs leaves the int32 range by more than half a count while y itself fits and
    stays unclamped: a saturating shift would change the oracle's output."""
    Y, W, raw, d, gains = sums(c)
    assert np.abs(Y).max() < TWO31 and Y.max() / TWO31 >= c.frac - 0.001 and -Y.min() / TWO31 >= c.frac - 0.001
    lo = ((W + 128) & 255) - 128
    hi = (W - lo) >> 8
    assert set(np.unique(W)) == {-16768, 16768} and hi.max() == 66 and lo.min() == -128
    X = O.reorder(raw).view(np.int8).astype(np.int64).reshape(c.B, 2, c.C, c.T, 2 * c.A)
    H, L = np.matmul(X, hi), np.matmul(X, lo)
    np.testing.assert_array_equal(256 * H + L, Y)
    count = TWO31 / 127
    assert (256 * H).min() <= -TWO31 - count / 2  # (W = -16768 has high limb -65: the positive side stays inside)
    s = np.float32(np.float32(c.scale) * np.float32(2.0 ** -14))
    q = EC.oracle_int8(c, raw, d, gains).reshape(Y.shape)
    assert (np.abs(Y.astype(np.float32) * s) < 127.5).all()  # nothing is altered by the clamp
    saturating = np.clip(256 * H, -TWO31, TWO31 - 1) + L
    moved = np.rint(saturating.astype(np.float32) * s) != q
    print(f"{EC.case_id(c)}: a saturating shift would move {moved.mean():.3f} of the output")
    assert moved.mean() >= 1 / 16  # the class (a) rows (1 in 4) x one component of the beams of one quadrant (1 in 4)


@pytest.mark.parametrize("c", EC.INT_CASES, ids=ids(EC.INT_CASES))
def test_planner_names_the_expected_kernel(c):
    assert (FC.workspace_bytes(c) > 0) == c.workspace
    assert FC.planned_name(c) == c.expect


def test_planner_names_the_float_cases():
    for case in EC.FLOAT_FUSED:
        for signed in (False, True):
            for exact in (False, True):
                call = EC.float_fused_call(case, signed, exact)
                assert FC.planned_name(call) == call.expect


def test_weight_bounds_of_the_integer_cases():
    """The C ABI leaves the weight bound to the caller: every case's weights pass bf_check_gains, the library's own
    sufficient condition (the high limb stays int8, A max|x| (sqrt(2) g 2^14 + 1) < 2^31)."""
    for c in EC.INT_CASES:
        g = np.full((c.M, c.A), 1.0 if c.gains is None else c.gains, np.float32)
        _lib.call("bf_check_gains", g.ctypes.data, c.M, c.A, c.flags)


# ---- float beams: the f16 hi/lo split over the whole weight range ------------------------------------------------
def test_range_tables_span_the_split_domain():
    g = EC.range_gains(13, 40, 1)
    assert g.dtype == np.float32 and g.shape == (13, 40) and np.isfinite(g).all()
    assert g.max() == EC.F16_MAX and g.min() == -EC.F16_MAX
    mag = np.abs(g)
    for m, e in enumerate(EC.RANGE_EXPONENTS):
        row = np.delete(mag[m], [20, 39]) if m == 0 else mag[m]
        assert (row >= 2.0 ** (e - 1)).all() and (row < 2.0 ** e).all()
    assert len(set(np.floor(np.log2(mag[12])).astype(int))) == len(EC.RANGE_EXPONENTS)  # the mixed beam
    w = EC.range_table((2, 2, 3, 10, 14), 2)
    assert w.shape == (2, 2, 3, 10, 14) and np.abs(w).max() == EC.F16_MAX and np.abs(w).min() < 2.0 ** -20
    assert not np.array_equal(w[0, 0, 0], w[1, 1, 2])


def split_emulation(signed, dropped_floor):
    """The worst err / bound of y = sum_k x_k (hi_k + lo_k) in float64 over 256 antennas x 13 beams."""
    A, M, T = 256, 13, 32
    rng = np.random.default_rng(5 + signed)
    x = rng.integers(-128, 128, (T, 2 * A)) if signed else rng.integers(0, 256, (T, 2 * A))
    x = x.astype(np.float64)
    g = EC.range_gains(M, A, 9)
    w = np.repeat(np.repeat(g.T, 2, axis=0), 2, axis=1) * rng.uniform(-1, 1, (2 * A, 2 * M)).astype(np.float32)
    w[A] = np.repeat(g[:, A // 2], 2)  # the row that carries +65504 unscaled
    w = w.astype(np.float32)
    y = x @ EC.f16_split(w)
    assert np.isfinite(y).all()
    err = np.abs(y - x @ w.astype(np.float64))
    bound = EC.float_bound(x, w.astype(np.float64))
    if dropped_floor:
        bound = bound - 2.0 ** -25 * np.abs(x).sum(axis=-1, keepdims=True)
    return float((err / bound).max())


@pytest.mark.parametrize("signed", [False, True], ids=["u8", "s8"])
def test_float_split_emulation_meets_the_bound_and_needs_its_floor(signed):
    worst, without = split_emulation(signed, False), split_emulation(signed, True)
    print(f"f16 split emulation: worst err / bound {worst:.3f}; with the 2^-25 sum|x| term dropped {without:.1f}")
    assert worst <= 1.0 < without


def test_float_split_emulation_of_a_table():
    w = EC.range_table((1, 2, 2, 24, 14), 4)
    x = np.random.default_rng(4).integers(0, 256, (1, 2, 2, 16, 24)).astype(np.float64)
    y = np.matmul(x, EC.f16_split(w))
    assert np.isfinite(y).all()
    err = np.abs(y - np.matmul(x, w.astype(np.float64)))
    assert (err <= EC.float_bound(x, w.astype(np.float64))).all()
    assert not (err <= 2.0 ** -20 * np.matmul(x, np.abs(w.astype(np.float64)))).all()


def test_split_overflows_just_above_the_domain():
    """65504 is the last weight the split can carry: from 65520 on f16(w) is infinite and the beams are not finite."""
    assert np.isfinite(EC.f16_split(np.float32([65504, -65504, 65519.99]))).all()
    assert not np.isfinite(EC.f16_split(np.float32([65520]))).any()
