"""GPU: the steering phase at telescope-scale delays, times and bands (the regimes and cases of tests/phase_cases.py;
what they reach is proved on the CPU by tests/test_phase_cases_host.py).

Every regime -- delays of +-5.5e4 samples and beyond, both signs, steering times from seconds to a day, three bands,
an odd channel count, the first, centre and last channels of the band -- goes through every kernel family that
evaluates a phasor, under the guard-band harness (guards, two fills, the expected kernel name; fused calls: the plan
asked on the host == the kernel that ran):

  generators   bf_coeff_gen (three kernels), bf_coeff_gen_time (f32, f16), bf_q14_coeffs (the channel recurrence with
               runs across chc = 0 and ragged runs, and a phasor per channel; unit and weighted): bit for bit
  fused int8   the Q14 contract bit for bit against oracle.fused_beamform_int8: item, generic, w32 (in-kernel
               phasors, whose waves mix fast and exact lanes in the mixed regimes), w32t and w32r (the table)
  fused float  item, generic, wide tw1 / tw2 and the persistent kernel, fast and exact, against the float64 product
               with the oracle's coefficients: finite and within phase_cases.float_bound (derived: no ATOL or RTOL);
               each test prints `PHASE-FLOAT <family> <regime> worst err/bound` (-s shows it; the worst per family and
               regime are recorded in DESIGN.md's parity section)
  fixture      tests/golden/phase_boundary.npz -- coefficients whose Q14 word is decided within 2e-10 of the phasor,
               some of them differently by the fast and the reference's rotation -- through bf_q14_coeffs, one shape of
               every fused int8 family, and the exact float generators: bit for bit.  bf_q14_coeffs shows every word;
               the int8 beams resolve a single word that is off by one count in under 1 % of the cases (a word moves a
               beam by |x| 2^-14 scale, some 1e-4 counts): through the beams the fixture catches a kernel that decides
               such words wrongly as a rule, not one stray word.
"""
import numpy as np
import pytest

import guarded as gd
import oracle as O
import phase_cases as PC
from dpdk_dc_sand_amd import _lib

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def ex(context, command_queue):
    return gd.DeviceExecutor(context, command_queue)


@pytest.fixture(scope="module")
def fixture():
    return PC.load_fixture()


def equal(ref):
    return lambda y: np.testing.assert_array_equal(y, ref)


# ---- generators -----------------------------------------------------------------------------------------------------
def coeff_gen(ex, d, B, P, C, Ctot, A, M, xeng, Ts, off, name):
    bufs = [gd.inp("dv", d, 16), gd.out("w", (B, P, C, 2 * A, 2 * M), np.float32, off)]
    gd.run_case(ex, bufs,
                lambda p: _lib.call("bf_coeff_gen", p["dv"], p["w"], B, P, C, Ctot, A, M, xeng, Ts, ex.queue.handle),
                lambda o: np.testing.assert_array_equal(o["w"], O.coeffs(d, B, P, C, Ctot, A, M, xeng, Ts=Ts)), name)


def coeff_gen_time(ex, d, nt, C, Ctot, A, M, xeng, Ts, t0, step, f16):
    dch, dt = d.shape[0], np.float16 if f16 else np.float32
    bufs = [gd.inp("dv", d, 16), gd.out("w", (nt, C, A, M, 2), dt, 4 if f16 else 8)]

    def oracle(o):
        for t in range(nt):  # the f16 output is the float16 cast of the float32 contract
            cos, sin = O.coeffs_at(np.broadcast_to(d, (C, M, A, 4)), C, Ctot, A, M, xeng, Ts, t0 + t * step)
            np.testing.assert_array_equal(o["w"][t, ..., 0], cos.transpose(0, 2, 1).astype(dt))
            np.testing.assert_array_equal(o["w"][t, ..., 1], sin.transpose(0, 2, 1).astype(dt))

    gd.run_case(ex, bufs, lambda p: _lib.call("bf_coeff_gen_time", p["dv"], dch, p["w"], int(f16), nt, C, Ctot, A, M,
                                              xeng, Ts, t0, step, ex.queue.handle),
                oracle, "coeff_gen_time_kernel:" + ("f16" if f16 else "f32"))


def q14_coeffs(ex, d, g, B, C, Ctot, A, M, xeng, Ts, t0, bdt):
    ref = PC.q14_words(O.quantise_coeffs(O.fused_tables(d, B, C, Ctot, A, xeng_id=xeng, Ts=Ts, t0=t0, batch_dt=bdt,
                                                        gains=g)))
    bufs = [gd.inp("dv", d, 16), gd.out("w", (B, C, M, A), np.uint32, 4)] + ([] if g is None else [gd.inp("g", g, 4)])
    gd.run_case(ex, bufs, lambda p: _lib.call("bf_q14_coeffs", p["dv"], d.shape[0], p.get("g"), p["w"], B, C, A, M,
                                              Ctot, xeng, Ts, t0, bdt, ex.queue.handle),
                lambda o: np.testing.assert_array_equal(o["w"], ref),
                f"q14_table_kernel:{'unit' if g is None else 'gain'},natural")


@pytest.mark.parametrize("g", PC.GEN_CASES, ids=[PC.gen_id(g) for g in PC.GEN_CASES])
def test_generators_bit_for_bit(ex, g):
    reg = PC.BY_NAME[g.regime]
    d, gains = PC.gen_inputs(g)
    t0, bdt = PC.gen_times(g)
    if g.kind == "coeff_gen":
        coeff_gen(ex, d, g.B, 2, g.C, reg.Ctot, g.A, g.M, g.xeng, reg.Ts, g.off, g.expect)
    elif g.kind == "coeff_gen_time":
        coeff_gen_time(ex, d, g.B, g.C, reg.Ctot, g.A, g.M, g.xeng, reg.Ts, t0, bdt, bool(g.off))
    else:
        q14_coeffs(ex, d, gains, g.B, g.C, reg.Ctot, g.A, g.M, g.xeng, reg.Ts, t0, bdt)


# ---- fused int8: the Q14 contract -----------------------------------------------------------------------------------
@pytest.mark.parametrize("c", PC.INT_CASES, ids=[PC.case_id(c) for c in PC.INT_CASES])
def test_fused_int8_bit_for_bit(ex, c):
    reg = PC.BY_NAME[c.regime]
    raw, d, gains = PC.inputs(c)
    t0, bdt = PC.times(c)
    ref = PC.oracle_int8(c, raw, d, gains)
    gd.fused_ws(ex, c, raw, d, gains, np.int8, equal(ref), reg.Ctot, c.xeng, reg.Ts, t0, bdt)


# ---- fused float ----------------------------------------------------------------------------------------------------
def check_float(label, y, x_real, w, fast, R):
    """Every output finite and within phase_cases.float_bound of the float64 product; prints the worst err / bound."""
    w64 = np.asarray(w, np.float64)
    exact = np.matmul(x_real, w64)
    bound = PC.float_bound(x_real, w64, fast, R)
    finite = np.isfinite(y).all()
    with np.errstate(invalid="ignore"):
        worst = float((np.abs(y.reshape(exact.shape).astype(np.float64) - exact) / bound).max())
    print(f"PHASE-FLOAT {label} worst err/bound {worst:.4f}")
    assert finite, f"{label}: non-finite beams"
    assert worst <= 1.0, f"{label}: worst err / bound {worst:.3f}"


@pytest.mark.parametrize("c", PC.FLOAT_CASES, ids=[PC.case_id(c) for c in PC.FLOAT_CASES])
def test_fused_float_within_the_derived_bound(ex, c):
    reg = PC.BY_NAME[c.regime]
    raw, d, _ = PC.inputs(c)
    t0, bdt = PC.times(c)
    signed, fast = bool(c.flags & PC.SIGNED), not c.flags & PC.EXACT
    w = O.fused_tables(d, c.B, c.C, reg.Ctot, c.A, xeng_id=c.xeng, Ts=reg.Ts, t0=t0, batch_dt=bdt)
    xr = O.reorder(raw)
    x_real = (xr.view(np.int8) if signed else xr).astype(np.float64).reshape(c.B, 2, c.C, c.T, 2 * c.A)
    R = float(PC.case_mag(reg, d, c.B, c.C, c.xeng, t0, bdt).max())
    label = f"{c.expect.split(',')[0]},{'fast' if fast else 'exact'} {c.regime}"
    gd.fused_ws(ex, c, raw, d, None, np.float32, lambda y: check_float(label, y, x_real, w, fast, R), reg.Ctot, c.xeng,
                reg.Ts, t0, bdt)


# ---- the adversarial fixture ----------------------------------------------------------------------------------------
FIX_CTOT, FIX_TS, FIX_C, FIX_XENG = PC.FIX.Ctot, PC.FIX.Ts, PC.FIX_C, PC.FIX_XENG


def test_fixture_through_q14_coeffs(ex, fixture):
    """Every entry as one model for all channels (the recurrence, anchored on the fast rotation) and in its own
    channel's plane (a fast phasor per channel); the weighted set under its weights."""
    z = fixture
    for d1, dC, _ in PC.fixture_models(z["tau"], z["phi"], z["channel"], 16, 64):
        for d in (d1, dC):
            q14_coeffs(ex, d, None, 1, FIX_C, FIX_CTOT, 64, 16, FIX_XENG, FIX_TS, 0.0, 0.0)
    for d1, dC, g in PC.fixture_models(z["w_tau"], z["w_phi"], z["w_channel"], 8, 64, z["w_gain"]):
        for d in (d1, dC):
            q14_coeffs(ex, d, g, 1, FIX_C, FIX_CTOT, 64, 8, FIX_XENG, FIX_TS, 0.0, 0.0)


# one shape of each fused int8 family: index into phase_cases.I8_FORMS, signed, weighted
FIX_FUSED = [(2, False, False), (4, True, False), (6, False, False), (7, True, True), (8, False, False),
             (9, False, False), (11, True, False)]


@pytest.mark.parametrize("form,signed,weighted", FIX_FUSED,
                         ids=[PC.I8_FORMS[f][3].format(s="pow2").split("fused_")[1] for f, _, _ in FIX_FUSED])
def test_fixture_through_the_fused_int8_families(ex, fixture, form, signed, weighted):
    (A, M, T), path, ws, name = PC.I8_FORMS[form]
    z = fixture
    p = "w_" if weighted else ""
    flags = PC.OUT_I8 | (PC.SIGNED if signed else 0) | PC.PATH[path]
    # twice the regimes' scale: more of a count per word (saturation stays under the cases' 10 %, checked below)
    scale = 2 * PC.int_scale(A, signed, weighted, True)
    rng = np.random.default_rng(A + M)
    raw = rng.integers(0, 256, (1, A, FIX_C, T, 2, 2), dtype=np.uint8)
    rawv = raw.view(np.int8) if signed else raw
    calls = PC.fixture_models(z[p + "tau"], z[p + "phi"], z[p + "channel"], M, A, z["w_gain"] if weighted else None)
    for n, (d1, dC, g) in enumerate(calls):
        # the layouts alternate over the calls; a single call takes both
        for d in ((d1, dC) if len(calls) == 1 else (dC,) if n % 2 else (d1,)):
            c = PC.PCase("fixture", "i8", A, M, T, 1, FIX_C, FIX_XENG, flags, name.format(s="pow2"), d.shape[0],
                         1 if weighted else None, scale, ws)
            ref = O.fused_beamform_int8(rawv, d, FIX_CTOT, xeng_id=FIX_XENG, Ts=FIX_TS, scale=scale, signed=signed,
                                        gains=g)
            q = np.abs(ref.astype(int))
            assert q.max() >= 8 and np.mean(q == 127) < 0.1
            gd.fused_ws(ex, c, raw, d, g, np.int8, equal(ref), FIX_CTOT, FIX_XENG, FIX_TS, 0.0, 0.0)


def test_fixture_through_the_exact_float_generators(ex, fixture):
    z = fixture
    A, M = 33, 34
    for n, (d1, dC, _) in enumerate(PC.fixture_models(z["tau"], z["phi"], z["channel"], M, A)):
        off, name = ((0, "coeff_gen_block_kernel:nt"), (8, "coeff_gen_tile_kernel"))[n % 2]
        coeff_gen(ex, dC, 1, 2, FIX_C, FIX_CTOT, A, M, FIX_XENG, FIX_TS, off, name)
        coeff_gen_time(ex, d1 if n % 2 else dC, 1, FIX_C, FIX_CTOT, A, M, FIX_XENG, FIX_TS, 0.0, 0.0, False)
