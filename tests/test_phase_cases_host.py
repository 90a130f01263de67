"""CPU: the regimes of tests/phase_cases.py reach what they claim, by the oracle alone; the adversarial fixture meets
its definition; div_denom's Markstein step equals IEEE division on every regime's denominator.

  signs    tau' and phi' of every case take both signs at every steering time
  place    chc = ch - Ctot/2 is negative on the first engine, positive on the last (which ends at Ctot - 1), and
           crosses zero (even Ctot: chc = 0 inside the call; odd Ctot: +-1/2 on either side) in the centre regimes
  guard    the share of coefficients with mag >= 2e5 (phase_cases.guard_mag): exactly 0 in array_low, exactly 1 in
           beyond, 0.03 .. 0.3 in array_top_uhf and 0.4 .. 0.8 in guard_edge -- over the regime's cases together, and
           within every case of at least 2000 coefficients (a 48-pair call's own share scatters by +-0.06); every case
           of the two mixed regimes has 64-lane groups of consecutive (m, a) entries with lanes on both sides
  plan     bf_fused_plan names the expected kernel for every fused case
  scale    the integer cases' oracle output reaches 8 counts and saturates in under 10 % of its entries
  fixture  at least 1024 entries and 16 teeth, 256 weighted entries, every one by the definition (libm)
  div      a Fraction emulation of div_denom (exact fma residuals, one rounding each) over 1e4 steering numerators of
           every regime equals float64 division
"""
from fractions import Fraction

import numpy as np
import pytest

import fused_cases as FC
import oracle as O
import phase_cases as PC

ALL_FUSED = PC.INT_CASES + PC.FLOAT_CASES
_mag = {}


def fused_mag(c):
    if c not in _mag:
        reg = PC.BY_NAME[c.regime]
        t0, bdt = PC.times(c)
        _mag[c] = PC.case_mag(reg, PC.inputs(c)[1], c.B, c.C, c.xeng, t0, bdt)
    return _mag[c]


def gen_mag(g):
    t0, bdt = PC.gen_times(g)
    return PC.case_mag(PC.BY_NAME[g.regime], PC.gen_inputs(g)[0], g.B, g.C, g.xeng, t0, bdt)


def test_case_ids_are_unique_and_every_form_meets_every_regime():
    ids = [PC.case_id(c) for c in ALL_FUSED] + [PC.gen_id(g) for g in PC.GEN_CASES]
    assert len(set(ids)) == len(ids)
    for reg in PC.REGIMES:
        names = {c.expect for c in ALL_FUSED if c.regime == reg.name}
        for _, _, _, name in PC.I8_FORMS:
            assert any(n in names for n in (name.format(s="pow2"), name.format(s="anyscale")))
        for _, _, name in PC.F32_FORMS:
            assert {name.format(e="fast"), name.format(e="exact")} <= names
        assert PC.P2_NAME in names
    assert {c.C for c in PC.FLOAT_CASES if c.expect == PC.P2_NAME} == {2, 3}
    for key in ("nts1", "nts2", "a64", "aany", "pow2", "anyscale"):  # every form of the item kernel, somewhere
        assert any(key in c.expect.split(":")[1].split(",") for c in PC.INT_CASES if c.expect.startswith(PC.I8ITEM))
    combos = {(bool(c.flags & PC.SIGNED), c.gains is not None) for c in PC.INT_CASES}
    assert len(combos) == 4  # signed and unsigned, unit and weighted


@pytest.mark.parametrize("reg", PC.REGIMES, ids=[r.name for r in PC.REGIMES])
def test_models_take_both_signs_at_every_steering_time(reg):
    cases = [(PC.inputs(c)[1], PC.times(c), c.B) for c in ALL_FUSED if c.regime == reg.name]
    cases += [(PC.gen_inputs(g)[0], PC.gen_times(g), g.B) for g in PC.GEN_CASES if g.regime == reg.name]
    for d, (t0, bdt), B in cases:
        assert np.abs(d[..., 2]).max() <= np.float32(np.pi) and np.abs(d[..., 1]).max() <= 2e-9
        assert np.abs(d[..., 3]).max() <= 20 and reg.tau_lo * reg.Ts * (1 - 1e-6) <= np.abs(d[..., 0]).min()
        assert np.abs(d[..., 0]).max() <= reg.tau_hi * reg.Ts * (1 + 1e-6)
        for b in range(B):
            for v in PC.advanced(d, t0 + b * bdt):
                assert (v < 0).any() and (v > 0).any()


@pytest.mark.parametrize("reg", PC.REGIMES, ids=[r.name for r in PC.REGIMES])
def test_channels_sit_where_the_regime_says(reg):
    calls = {(c.C, c.xeng) for c in ALL_FUSED if c.regime == reg.name}
    calls |= {(g.C, g.xeng) for g in PC.GEN_CASES if g.regime == reg.name}
    for C, xeng in calls:
        chc = PC.channels(reg, C, xeng) - reg.Ctot / 2
        assert 0 <= chc[0] + reg.Ctot / 2 and chc[-1] + reg.Ctot / 2 <= reg.Ctot - 1
        if reg.place == "first":
            assert chc[0] == -reg.Ctot / 2 and (chc < 0).all()
        elif reg.place == "last":
            assert chc[-1] == reg.Ctot / 2 - 1 and (chc > 0).all()
        elif reg.Ctot % 2 == 0:
            assert (chc == 0).any() and (chc < 0).any()
        else:
            assert (chc == -0.5).any() and (chc == 0.5).any()
    if reg.place == "centre":  # both signs of chc inside one call, and a channel run of the recurrence across zero
        assert any((PC.channels(reg, C, x) < reg.Ctot / 2).any() and (PC.channels(reg, C, x) > reg.Ctot / 2).any()
                   for C, x in calls)
        run = PC.channels(reg, PC.Q14_C1[reg.name])[:64] - reg.Ctot / 2
        assert run[0] < 0 < run[-1]


@pytest.mark.parametrize("reg", PC.REGIMES, ids=[r.name for r in PC.REGIMES])
def test_share_of_coefficients_past_the_guard(reg):
    mags = [fused_mag(c) for c in ALL_FUSED if c.regime == reg.name]
    mags += [gen_mag(g) for g in PC.GEN_CASES if g.regime == reg.name and g.kind != "coeff_gen"]
    past = sum(int((m >= PC.MAX_MAG).sum()) for m in mags)
    total = sum(m.size for m in mags)
    share = past / total
    largest = max(m.max() for m in mags)
    print(f"{reg.name}: {share:.4f} of {total} coefficients past the guard, largest mag {largest:.4g}")
    if reg.share is not None:
        lo, hi = reg.share
        assert lo <= share <= hi
        for m in mags:
            if m.size >= 2000 or lo == hi:
                assert lo <= (m >= PC.MAX_MAG).mean() <= hi
    if reg.name in PC.MIXED:
        for m in mags:
            mixed, n = PC.mixed_groups(m)
            assert mixed >= 1, f"no mixed group among {n}"
            assert 0 < (m >= PC.MAX_MAG).mean() < 1


def test_largest_rotation_of_the_guard_edge_regime():
    """|rot| reaches 1.8e5, where one ulp of the reference's `initial` is 2.9e-11.  On the last engine mag is about
    3 |rot| (ch + Ctot/2 against ch - Ctot/2), so the coefficients that stay on the fast phasor reach a third of 2e5."""
    g = next(g for g in PC.GEN_CASES if g.regime == "guard_edge" and g.kind == "q14" and g.dch == 1)
    reg = PC.BY_NAME[g.regime]
    d, _ = PC.gen_inputs(g)
    t0, _ = PC.gen_times(g)
    rot = O.coeff_rotation(np.broadcast_to(d, (g.C,) + d.shape[1:]), g.C, reg.Ctot, g.xeng, reg.Ts, t0)
    within = gen_mag(g)[0] < PC.MAX_MAG
    print(f"guard_edge: max |rot| within the guard {np.abs(rot[within]).max():.4g}, overall {np.abs(rot).max():.4g}")
    assert np.abs(rot).max() >= 1.8e5 and np.abs(rot[within]).max() >= 6e4


@pytest.mark.parametrize("c", ALL_FUSED, ids=[PC.case_id(c) for c in ALL_FUSED])
def test_planner_names_the_expected_kernel(c):
    assert (FC.workspace_bytes(c) > 0) == c.workspace
    assert FC.planned_name(c) == c.expect


@pytest.mark.parametrize("c", PC.INT_CASES, ids=[PC.case_id(c) for c in PC.INT_CASES])
def test_integer_cases_are_neither_empty_nor_clamped(c):
    q = np.abs(PC.oracle_int8(c, *PC.inputs(c)).astype(int))
    print(f"{PC.case_id(c)}: scale {c.scale:.3g}, max |q| {q.max()}, saturated {np.mean(q == 127):.4f}")
    assert q.max() >= 8 and np.mean(q == 127) < 0.1


# ---- the fixture ----------------------------------------------------------------------------------------------------
def test_fixture_meets_its_definition():
    z = PC.load_fixture()
    n, nw = len(z["tau"]), len(z["w_tau"])
    assert PC.FIX_MIN <= n <= PC.FIX_MAX and nw >= PC.FIX_MIN_WEIGHTED
    assert z["tau"].dtype == z["phi"].dtype == z["w_tau"].dtype == z["w_gain"].dtype == np.float32
    for p in ("", "w_"):
        ch = z[p + "channel"]
        assert ch.min() >= PC.FIX_CH0 and ch.max() < PC.FIX_CH0 + PC.FIX_C == PC.FIX.Ctot
        assert np.abs(z[p + "tau"]).max() <= PC.FIX.tau_hi * PC.FIX.Ts and (z[p + "tau"] < 0).any()
        assert np.abs(z[p + "phi"]).max() <= np.float32(np.pi) and (z[p + "phi"] < 0).any()
    assert set(np.unique(z["w_gain"])) == set(PC.FIX_GAINS)
    kept, tooth, diff = PC.fixture_flags(z["tau"], z["phi"], z["channel"])
    assert kept.all()
    np.testing.assert_array_equal(tooth, z["is_tooth"])
    assert tooth.sum() >= PC.FIX_MIN_TEETH
    wkept, wtooth, _ = PC.fixture_flags(z["w_tau"], z["w_phi"], z["w_channel"], z["w_gain"])
    assert wkept.all()
    np.testing.assert_array_equal(wtooth, z["w_is_tooth"])
    print(f"fixture: {n} entries, {int(tooth.sum())} teeth, max |fast - ref| {diff.max():.3g} rad "
          f"(teeth {diff[tooth].max():.3g}); {nw} weighted, {int(wtooth.sum())} teeth")
    assert diff.max() < PC.BAND  # the fast rotation stays within the band the entries were chosen with


def test_fixture_models_hold_every_entry_at_its_own_channel():
    z = PC.load_fixture()
    M, A = 16, 64
    calls = PC.fixture_models(z["tau"], z["phi"], z["channel"], M, A)
    assert len(calls) == -(-len(z["tau"]) // (M * A))
    seen1, seenC = set(), set()
    for d1, dC, g in calls:
        assert g is None and d1.shape == (1, M, A, 4) and dC.shape == (PC.FIX_C, M, A, 4)
        seen1 |= set(zip(d1[0, :, :, 0].ravel().tolist(), d1[0, :, :, 2].ravel().tolist()))
        for c in range(PC.FIX_C):
            seenC |= {(t, p, PC.FIX_CH0 + c) for t, p in zip(dC[c, :, :, 0].ravel().tolist(),
                                                              dC[c, :, :, 2].ravel().tolist())}
    entries = set(zip(z["tau"].tolist(), z["phi"].tolist(), z["channel"].tolist()))
    assert {(t, p) for t, p, _ in entries} <= seen1 and entries <= seenC
    wcalls = PC.fixture_models(z["w_tau"], z["w_phi"], z["w_channel"], 5, 19, z["w_gain"])
    seen1, seenC = set(), set()
    for d1, dC, g in wcalls:  # every weighted entry under its own weight, in both layouts
        assert g.shape == (5, 19) and g.dtype == np.float32
        seen1 |= set(zip(d1[0, :, :, 0].ravel().tolist(), d1[0, :, :, 2].ravel().tolist(), g.ravel().tolist()))
        for c in range(PC.FIX_C):
            plane = zip(dC[c, :, :, 0].ravel().tolist(), dC[c, :, :, 2].ravel().tolist(), g.ravel().tolist())
            seenC |= {(t, p, PC.FIX_CH0 + c, w) for t, p, w in plane}
    wentries = set(zip(z["w_tau"].tolist(), z["w_phi"].tolist(), z["w_channel"].tolist(), z["w_gain"].tolist()))
    assert {(t, p, w) for t, p, _, w in wentries} <= seen1 and wentries <= seenC


# ---- div_denom ----------------------------------------------------------------------------------------------------
def div_denom_emulated(a, denom, inv):
    """csrc/bf_phase.hpp div_denom: q0 = RN(a inv); r = fma(-q0, denom, a); r == 0 ? q0 : fma(r, inv, q0)."""
    q0 = a * inv
    r = float(Fraction(a) - Fraction(q0) * Fraction(denom))
    return q0 if r == 0.0 else float(Fraction(r) * Fraction(inv) + Fraction(q0))


@pytest.mark.parametrize("reg", PC.REGIMES, ids=[r.name for r in PC.REGIMES])
def test_div_denom_equals_ieee_division(reg):
    """The numerators of steering_rotation, tau' ch (-pi) and tau' (Ctot/2) (-pi), over the regime's delays at the
    steering time, at the band's edge and centre channels and random ones: 10 000 per denominator."""
    rng = np.random.default_rng(reg.Ctot)
    denom = float(reg.Ctot) * reg.Ts
    inv = 1.0 / denom
    tau, _ = PC.advanced(PC.model(reg, 1, 50, 100, 11)[0], reg.t0)
    tau = tau.ravel()
    ch = rng.integers(0, reg.Ctot, tau.size).astype(np.float64)
    ch[:4] = (0, 1, reg.Ctot - 1, reg.Ctot // 2)
    nums = np.concatenate([tau * ch * -np.pi, tau * (reg.Ctot / 2) * -np.pi])
    assert nums.size >= 10000 and (nums != 0).mean() > 0.99
    bad = [a for a in nums.tolist() if div_denom_emulated(a, denom, inv) != a / denom]
    assert not bad, f"{len(bad)} of {nums.size} quotients differ from IEEE division, e.g. {bad[0]!r} / {denom!r}"
