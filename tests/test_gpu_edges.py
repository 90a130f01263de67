"""GPU: both beam paths at the edges of their numeric range (the cases of tests/edge_cases.py; what the inputs reach
is proved on the CPU by tests/test_edge_cases_host.py).

Integer beams: every case runs bf_beamform_fused_ws under the guard-band harness (guards, two fills, the expected kernel
name, the plan asked on the host == the kernel that ran) and must equal oracle.fused_beamform_int8 bit for bit: int32
sums at the edge of their range, the largest admitted weight in every kernel family's limb split, and outputs that
are almost all clamped.  Weights travel as a device table: the C ABI leaves their bound to the caller.

Float beams: weights from 2^-21 to 65504 (range_gains, range_table) through every fused float kernel and every
bf_beamform kernel.  Every output finite and
    |y - exact| <= 2^-20 sum_k |x_k w_k| + 2^-25 sum_k |x_k| (+ 2^-22 sum_k |x_k g_k| with fast phasors),
`exact` the float64 product with the oracle's float32 coefficients (edge_cases.float_bound: derived, no ATOL or RTOL).
Each float test prints its worst err / bound (-s shows it); the worst per family are recorded in DESIGN.md's parity
section."""
import numpy as np
import pytest

import edge_cases as EC
import guarded as gd
import oracle as O
from dpdk_dc_sand_amd import _lib

pytestmark = pytest.mark.gpu
TS, CTOT, XENG, T0, BDT = EC.TS, EC.CTOT, EC.XENG, EC.T0, EC.BDT


@pytest.fixture(scope="module")
def ex(context, command_queue):
    return gd.DeviceExecutor(context, command_queue)


def fused_ws(ex, c, raw, d, gains, out_dtype, oracle):
    """One guarded bf_beamform_fused_ws call of a case (fused_cases.Call or edge_cases.Case); returns the beams."""
    return gd.fused_ws(ex, c, raw, d, gains, out_dtype, oracle, CTOT, XENG, TS, T0, BDT)


# ---- integer beams ------------------------------------------------------------------------------------------------
def ids(cases):
    return [EC.case_id(c) for c in cases]


def integer_case(ex, c):
    raw, d, gains = EC.inputs(c)
    ref = EC.oracle_int8(c, raw, d, gains)
    fused_ws(ex, c, raw, d, gains, np.int8, lambda y: np.testing.assert_array_equal(y, ref))


@pytest.mark.parametrize("c", EC.BOUND_CASES, ids=ids(EC.BOUND_CASES))
def test_int32_sums_at_the_edge_of_their_range(ex, c):
    """Sums within 0.01 % .. 0.3 % of +-2^31 (the ring and item kernels: the most their shapes admit) and nothing
    clamped: a sum that saturated, went through a float, or lost a wrap-around of `128 * colsum` is off by 128 or 85."""
    integer_case(ex, c)


@pytest.mark.parametrize("c", EC.LIMB_CASES, ids=ids(EC.LIMB_CASES))
def test_largest_weight_in_every_limb_split(ex, c):
    """W = +-32639 (high limb +-127), low limbs -128 and +127, through each family's own split."""
    integer_case(ex, c)


@pytest.mark.parametrize("c", EC.SAT_CASES, ids=ids(EC.SAT_CASES))
def test_clamp_when_nearly_everything_saturates(ex, c):
    """+127 and -127, never -128, also where |f32(y) * s| >= 2^22 and the rounding's magic add is no longer exact."""
    integer_case(ex, c)


@pytest.mark.parametrize("c", EC.LOW_CASES, ids=ids(EC.LOW_CASES))
def test_low_bits_of_sums_whose_parts_cancel(ex, c):
    """The class (d) rows at one count per 512 of y: for uint8 samples the sum of (0 - 128) W and the correction
    128 * colsum, each near 2^30, must leave exactly one coefficient."""
    integer_case(ex, c)


@pytest.mark.parametrize("c", EC.FINE_CASES, ids=ids(EC.FINE_CASES))
def test_shifted_high_limbs_wrap_and_come_back(ex, c):
    """(hi << 8) + lo where hi << 8 alone passes 2^31 by 1.5e7, at 127 counts per 2^31: a saturating shift is off by
    0.9 count (at the bound cases' scales it would stay below half a count)."""
    integer_case(ex, c)


# ---- float beams --------------------------------------------------------------------------------------------------
def check_float(label, y, x_real, w, fast_gains=None):
    """Every output finite and within edge_cases.float_bound of the float64 product; prints the worst err / bound."""
    w64 = np.asarray(w, np.float64)
    exact = np.matmul(x_real, w64)
    bound = EC.float_bound(x_real, w64, fast_gains)
    finite = np.isfinite(y).all()
    with np.errstate(invalid="ignore"):
        worst = float((np.abs(y.reshape(exact.shape).astype(np.float64) - exact) / bound).max())
    print(f"EDGE-FLOAT {label} worst err/bound {worst:.4f}")
    assert finite, f"{label}: non-finite beams"
    assert worst <= 1.0, f"{label}: worst err / bound {worst:.3f}"


def as_real(x, signed):
    return (x.view(np.int8) if signed else x).astype(np.float64)


@pytest.mark.parametrize("case", EC.FLOAT_FUSED, ids=[f"{s[0]}x{s[1]}x{s[2]}" for s, _, _ in EC.FLOAT_FUSED])
@pytest.mark.parametrize("signed", [False, True], ids=["u8", "s8"])
@pytest.mark.parametrize("exact", [False, True], ids=["fast", "exact"])
def test_fused_float_beams_over_the_weight_range(ex, case, signed, exact):
    c = EC.float_fused_call(case, signed, exact)
    rng = np.random.default_rng(c.A * 131 + c.M * 7 + c.T)
    raw = rng.integers(0, 256, (c.B, c.A, c.C, c.T, 2, 2), dtype=np.uint8)
    d = EC.random_delays(c.dch, c.M, c.A, c.A * 31 + c.M)
    gains = EC.range_gains(c.M, c.A, c.gains)
    w = O.fused_tables(d, c.B, c.C, CTOT, c.A, xeng_id=XENG, t0=T0, batch_dt=BDT, gains=gains)
    x_real = as_real(O.reorder(raw), signed).reshape(c.B, 2, c.C, c.T, 2 * c.A)
    fast_gains = None if exact else np.repeat(np.repeat(np.abs(gains.T.astype(np.float64)), 2, axis=0), 2, axis=1)
    label = f"{c.expect.split(',')[0]},{'exact' if exact else 'fast'}"
    fused_ws(ex, c, raw, d, gains, np.float32, lambda y: check_float(label, y, x_real, w, fast_gains))


@pytest.mark.parametrize("A,M,NB,B,C,x_off,w_off,name", EC.FLOAT_TABLE,
                         ids=[f"{t[0]}x{t[1]}-{t[7]}" for t in EC.FLOAT_TABLE])
@pytest.mark.parametrize("signed", [False, True], ids=["u8", "s8"])
def test_table_beams_over_the_weight_range(ex, A, M, NB, B, C, x_off, w_off, name, signed):
    rng = np.random.default_rng(A * 7 + M + NB)
    x = rng.integers(0, 256, (B, 2, C, NB, 16, A, 2), dtype=np.uint8)
    w = EC.range_table((B, 2, C, 2 * A, 2 * M), A + M)
    x_real = as_real(x, signed).reshape(B, 2, C, NB * 16, 2 * A)
    bufs = [gd.inp("x", x, x_off), gd.inp("w", w, w_off), gd.out("y", (B, 2, C, NB, 16, 2 * M), np.float32, 16)]

    def launch(p):
        _lib.call("bf_beamform", p["x"], p["w"], p["y"], B, 2, C, NB, A, M, int(signed), ex.queue.handle)

    gd.run_case(ex, bufs, launch, lambda o: check_float(name.split(":")[0], o["y"], x_real, w), name)
