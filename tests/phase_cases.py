"""The steering argument at telescope scale, as data: regimes, delay models, the guard's magnitude, case lists and the
definitions of the adversarial fixture.  Importable without a GPU.

tests/test_phase_cases_host.py proves from the oracle alone what each regime reaches (signs, channel placement, which
coefficients the Q14 guard sends to the exact path, mixed waves, the planner's kernel names, usable output scales) and
that tests/golden/phase_boundary.npz meets its definition; tests/test_gpu_phase_domain.py runs the cases.

A regime fixes the sample period, the band's channel count, where the call's C channels sit in the band, the largest
delay and the steering time.  Every model draws delays and phases of both signs, phases in +-pi, delay rates in +-2e-9
and phase rates in +-20 rad/s (an 8 km array: +-4.6e4 samples, fringe rates +-17 rad/s).

  regime          Ts        Ctot   channels                 |tau| (samples)   t0       reaches
  array_low       1/1712e6  4096   first engine, chc < 0    <= 5.5e4          100 s    nothing past the guard
  array_top_uhf   1/1088e6  4096   last engine, chc > 0     <= 5.5e4          100 s    a minority past it: mixed waves
  centre_sband    1/1750e6  1000   straddles Ctot / 2       <= 5.5e4          3600 s   chc = 0 inside the call, phi' 7e4
  odd_band        1/1750e6  4095   straddles 2047.5         <= 5.5e4          7 s      half-integer centre
  guard_edge      1/1712e6  32768  last engine              <= 1.2e5          10 s     most past the guard, |rot| 1.9e5
  beyond          1/1712e6  4096   last engine              3e5 .. 4e5        86400 s  all past the guard: exact only

The guard (csrc/bf_phase.hpp, q14_coeffs): a coefficient keeps the fast phasor while
    mag = |f32(tau')| * f32((ch + Ctot/2) |K|) + |f32(phi')| < 2e5,   K = -pi / (Ctot Ts),
tau' = tau + tau_rate dt and phi' = phi + phi_rate dt the model advanced to the batch's time.  `guard_mag` forms it in
float32 as written (the device may fuse the multiply-add: the two differ by at most one float32 ulp of 2e5, 0.016,
which no stated share and, by its margin, no fixture entry depends on).
In `beyond` the delay rate takes the delay's sign: the day-old model's delay has grown, never shrunk back under the
guard, so that every coefficient is past it by construction (independent signs leave under 1 % below it).
"""
import math
from collections import namedtuple

import numpy as np

import edge_cases as EC
import fused_cases as FC
import oracle as O

SIGNED, OUT_I8, EXACT, PATH, S6 = FC.SIGNED, FC.OUT_I8, FC.EXACT, FC.PATH, FC.S6
MAX_MAG = np.float32(2e5)  # kQ14MaxMag
BAND = 2e-10  # the fixture's half-width around a decision point (the kernels' guard band kQ14Eps is 5e-10)
TAU_RATE, PHI_RATE = 2e-9, 20.0

# share: the interval the share of coefficients with mag >= 2e5 must lie in (None: not stated, only reported)
Regime = namedtuple("Regime", "name Ts Ctot place tau_lo tau_hi t0 share")
REGIMES = [
    Regime("array_low", 1 / 1712e6, 4096, "first", 0.0, 5.5e4, 100.0, (0.0, 0.0)),
    Regime("array_top_uhf", 1 / 1088e6, 4096, "last", 0.0, 5.5e4, 100.0, (0.03, 0.3)),
    Regime("centre_sband", 1 / 1750e6, 1000, "centre", 0.0, 5.5e4, 3600.0, None),
    Regime("odd_band", 1 / 1750e6, 4095, "centre", 0.0, 5.5e4, 7.0, None),
    Regime("guard_edge", 1 / 1712e6, 32768, "last", 0.0, 1.2e5, 10.0, (0.4, 0.8)),
    Regime("beyond", 1 / 1712e6, 4096, "last", 3e5, 4e5, 86400.0, (1.0, 1.0)),
]
BY_NAME = {r.name: r for r in REGIMES}
MIXED = ("array_top_uhf", "guard_edge")  # the regimes whose waves hold lanes on both sides of the guard


def k_of(Ctot, Ts):
    """K = -pi / (Ctot Ts) as the host code of every entry point forms it."""
    return -3.141592653589793 / (float(Ctot) * Ts)


def xeng_for(reg, C):
    """The X-engine whose C channels sit where the regime says (first channel = xeng_id * C)."""
    if reg.place == "first":
        return 0
    if reg.place == "last":
        return reg.Ctot // C - 1
    return int((reg.Ctot / 2) // C)


def channels(reg, C, xeng=None):
    first = C * (xeng_for(reg, C) if xeng is None else xeng)
    return np.arange(first, first + C)


def model(reg, dch, M, A, seed):
    """The regime's (dch, M, A, 4) float32 delay model."""
    rng = np.random.default_rng(seed)
    shape = (dch, M, A)
    sign = rng.choice([-1.0, 1.0], shape)
    d = np.zeros(shape + (4,), np.float32)
    d[..., 0] = sign * rng.uniform(reg.tau_lo, reg.tau_hi, shape) * reg.Ts
    rate = rng.uniform(-TAU_RATE, TAU_RATE, shape)
    d[..., 1] = sign * np.abs(rate) if reg.name == "beyond" else rate
    d[..., 2] = rng.uniform(-np.pi, np.pi, shape)
    d[..., 3] = rng.uniform(-PHI_RATE, PHI_RATE, shape)
    return d


def batch_dt(reg, T):
    return T * 2 * reg.Ctot * reg.Ts


def advanced(d, dt):
    """(tau', phi') in float64, as oracle.coeff_rotation advances the model."""
    d = np.asarray(d, np.float32)
    tau, phi = d[..., 0].astype(np.float64), d[..., 2].astype(np.float64)
    if dt != 0.0:
        tau = tau + d[..., 1].astype(np.float64) * dt
        phi = phi + d[..., 3].astype(np.float64) * dt
    return tau, phi


def guard_mag(tau, phi, ch, Ctot, Ts):
    """mag of q14_coeffs for advanced (tau', phi') (float64 arrays) at absolute channels ch: float32."""
    uk = ((np.asarray(ch, np.float64) + Ctot / 2.0) * abs(k_of(Ctot, Ts))).astype(np.float32)
    return np.abs(tau.astype(np.float32)) * uk + np.abs(phi.astype(np.float32))


def case_mag(reg, d, B, C, xeng, t0, bdt):
    """mag of every coefficient of a call: float32 (B, C, M, A)."""
    d = np.asarray(d, np.float32)
    if d.shape[0] == 1 and C > 1:
        d = np.broadcast_to(d, (C,) + d.shape[1:])
    ch = (np.arange(C) + C * xeng)[:, None, None]
    return np.stack([guard_mag(*advanced(d, t0 + b * bdt), ch, reg.Ctot, reg.Ts) for b in range(B)])


def mixed_groups(mag):
    """How many 64-lane groups of consecutive (m, a) entries (per batch and channel) have lanes on both sides of the
    guard, and how many groups there are."""
    B, C, M, A = mag.shape
    past = (mag >= MAX_MAG).reshape(B * C, M * A)
    n = mixed = 0
    for lo in range(0, M * A, 64):
        g = past[:, lo:lo + 64]
        n += g.shape[0]
        mixed += int((g.any(axis=1) & ~g.all(axis=1)).sum())
    return mixed, n


# ---- the decision of the Q14 contract, and the two ways to form the rotation ---------------------------------------
def q14_word(v, g=None):
    """Qc(v) = rint(2^14 RN32(v)), or rint(RN32(RN32(v) g) 2^14) with a weight, as q14_pair takes it.  float64."""
    a = np.asarray(v, np.float64).astype(np.float32)
    if g is not None:
        a = a * np.asarray(g, np.float32)  # one float32 rounding
    return np.rint(a.astype(np.float64) * 16384.0)


def decision_within_band(v, g=None):
    """The contract's word changes within +-BAND of v: a float32 rounding midpoint next to a Q14 boundary."""
    v = np.asarray(v, np.float64)
    return q14_word(v - BAND, g) != q14_word(v + BAND, g)


def fast_rotation(tau, phi, ch, Ctot, Ts):
    """The rotation formed the fast way, (tau chc) K + phi in float64 (no division, no cancellation)."""
    return (np.asarray(tau, np.float64) * (np.asarray(ch, np.float64) - Ctot / 2.0)) * k_of(Ctot, Ts) + \
        np.asarray(phi, np.float64)


def libm_cos_sin(rot):
    """(cos, sin) by math.cos / math.sin, the contract's evaluator, float64."""
    flat = np.asarray(rot, np.float64).ravel()
    c = np.fromiter((math.cos(v) for v in flat), np.float64, flat.size)
    s = np.fromiter((math.sin(v) for v in flat), np.float64, flat.size)
    return c.reshape(np.shape(rot)), s.reshape(np.shape(rot))


# ---- the adversarial fixture (tests/golden/make_phase_fixture.py -> tests/golden/phase_boundary.npz) -----------------
FIX = BY_NAME["array_low"]._replace(name="fixture", place="last", t0=0.0)  # L-band, 4096 channels, |tau| <= 5.5e4
FIX_C = 8
FIX_XENG = FIX.Ctot // FIX_C - 1  # channels 4088 .. 4095
FIX_CH0 = FIX_C * FIX_XENG
FIX_GAINS = np.float32([0.5, 0.75, -1.0, 32639 / 16384])
FIX_MAG_MARGIN = 1.0  # entries keep mag < 2e5 - 1: no entry's side of the guard hangs on how mag is rounded
FIX_MIN, FIX_MIN_TEETH, FIX_MIN_WEIGHTED, FIX_MAX = 1024, 16, 256, 4096


def fixture_rotation(tau, phi, channel):
    """The oracle's float64 rotation of fixture entries (tau, phi float32, absolute channel), zero rates, t0 = 0."""
    tau, phi, channel = (np.asarray(v) for v in (tau, phi, channel))
    rot = np.empty(tau.shape, np.float64)
    for ch in np.unique(channel):
        sel = channel == ch
        d = np.zeros((1, 1, int(sel.sum()), 4), np.float32)
        d[0, 0, :, 0], d[0, 0, :, 2] = tau[sel], phi[sel]
        rot[sel] = O.coeff_rotation(d, 1, FIX.Ctot, 0, FIX.Ts, ch0=int(ch))[0, 0]
    return rot


def fixture_flags(tau, phi, channel, g=None, libm=True):
    """(kept, tooth, |fast - ref|) of entries by the definition: kept = mag < 2e5 and cos or sin of the oracle's
    rotation has its word's decision point within +-BAND; tooth = the word differs when the rotation is formed the
    fast way.  libm = False evaluates with NumPy's cos / sin (the search; the host test uses libm)."""
    rot = fixture_rotation(tau, phi, channel)
    fast = fast_rotation(np.asarray(tau, np.float32), np.asarray(phi, np.float32), channel, FIX.Ctot, FIX.Ts)
    cs = libm_cos_sin if libm else (lambda r: (np.cos(r), np.sin(r)))
    (c, s), (cf, sf) = cs(rot), cs(fast)
    t64, p64 = np.asarray(tau, np.float32).astype(np.float64), np.asarray(phi, np.float32).astype(np.float64)
    mag = guard_mag(t64, p64, channel, FIX.Ctot, FIX.Ts)
    kept = (mag < MAX_MAG - np.float32(FIX_MAG_MARGIN)) & (decision_within_band(c, g) | decision_within_band(s, g))
    tooth = (q14_word(c, g) != q14_word(cf, g)) | (q14_word(s, g) != q14_word(sf, g))
    return kept, tooth, np.abs(fast - rot)


def load_fixture():
    import os
    with np.load(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "phase_boundary.npz")) as z:
        return {k: z[k] for k in z.files}


def fixture_models(tau, phi, channel, M, A, gains=None):
    """Lay fixture entries out as delay models for calls of shape (M, A) over the fixture's 8-channel window:
    a list of (d1 (1, M, A, 4), dC (8, M, A, 4), g (M, A) or None), as many calls as hold every entry.  d1 is one model
    for every channel (each entry is evaluated at all 8 channels, its own among them); dC holds entries in their own
    channel's plane.  With weights, pair i = m A + a has weight FIX_GAINS[i mod 4] and takes entries of that weight
    only.  Entries are taken in order and cyclically: every slot holds a fixture entry."""
    slots = M * A
    ncls = 1 if gains is None else len(FIX_GAINS)
    slot_cls = np.arange(slots) % ncls
    entry_cls = np.zeros(len(tau), int) if gains is None else np.argmax(gains[:, None] == FIX_GAINS[None, :], axis=1)
    members = [np.flatnonzero(entry_cls == k) for k in range(ncls)]
    where = [np.flatnonzero(slot_cls == k) for k in range(ncls)]
    ncalls = max(-(-len(members[k]) // len(where[k])) for k in range(ncls))
    out = []
    for call in range(ncalls):
        d1 = np.zeros((1, slots, 4), np.float32)
        dC = np.zeros((FIX_C, slots, 4), np.float32)
        for k in range(ncls):
            step = call * len(where[k]) + np.arange(len(where[k]))
            pick = members[k][step % len(members[k])]
            d1[0, where[k], 0], d1[0, where[k], 2] = tau[pick], phi[pick]
            for c in range(FIX_C):
                own = members[k][channel[members[k]] == FIX_CH0 + c]
                pick = own[step % len(own)] if len(own) else members[k][step % len(members[k])]
                dC[c, where[k], 0], dC[c, where[k], 2] = tau[pick], phi[pick]
        g = None if gains is None else FIX_GAINS[slot_cls].reshape(M, A).astype(np.float32)
        out.append((d1.reshape(1, M, A, 4), dC.reshape(FIX_C, M, A, 4), g))
    return out


# ---- the cases ------------------------------------------------------------------------------------------------------
# fused int8 forms of the Q14 contract: (A, M, T), path, workspace, name ({s}: pow2 | anyscale), big (A = T = 256)
I8ITEM, I8GEN, W32 = "beamform_fused_i8_item_kernel:", "beamform_fused_i8_kernel:", "beamform_fused_i8_w32_kernel:"
W32T, W32R = FC.W32T, FC.W32R
I8_FORMS = [
    ((64, 8, 16), "auto", False, I8ITEM + "nts1,full,a64,{s}"),
    ((61, 12, 16), "auto", False, I8ITEM + "nts2,partial,aany,{s}"),
    ((64, 16, 16), "auto", False, I8ITEM + "nts2,full,a64,{s}"),
    ((61, 7, 16), "auto", False, I8ITEM + "nts1,partial,aany,{s}"),
    ((130, 9, 16), "generic", False, I8GEN + "nts2"),
    ((19, 3, 16), "generic", False, I8GEN + "nts1"),
    ((72, 33, 16), "wide", False, W32 + "unit"),
    ((72, 33, 16), "wide", False, W32 + "gain"),
    ((64, 40, 16), "wide", True, W32T + "general,buf"),
    ((256, 64, 256), "wide", True, W32T + "straight,pow2"),
    ((256, 40, 256), "wide", True, W32T + "straight,anyscale"),
    ((256, 32, 256), "wide", True, W32R + "pow2"),
    ((256, 32, 256), "wide", True, W32R + "anyscale"),
]
# fused float forms: (A, M, T), path, name ({e}: exact | fast)
F32_FORMS = [
    ((33, 9, 16), "auto", FC.ITEM + "nts2,partial,{e}"),
    ((16, 8, 16), "auto", FC.ITEM + "nts1,full,{e}"),
    ((130, 9, 16), "auto", FC.GEN + "nts2,{e}"),
    ((80, 2, 16), "auto", FC.GEN + "nts1,{e}"),
    ((16, 3, 16), "wide", FC.WIDE + "tw1,{e},unit,buf"),
    ((72, 33, 16), "auto", FC.WIDE + "tw2,{e},unit,buf"),
]
P2_SHAPE, P2_NAME = (256, 32, 256), "beamform_fused_wide_p2_kernel"
# channels per call: small shapes, and the A = T = 256 shapes (C = 2 and 3 for the persistent float kernel)
C_SMALL = {"array_low": 3, "array_top_uhf": 4, "centre_sband": 8, "odd_band": 5, "guard_edge": 8, "beyond": 2}
C_BIG = {"array_low": 3, "array_top_uhf": 2, "centre_sband": 3, "odd_band": 3, "guard_edge": 2, "beyond": 2}

# The fields of fused_cases.Call that the planner and the guarded call read, plus the regime and the engine.
PCase = namedtuple("PCase", "regime family A M T B C xeng flags expect dch gains scale workspace")


def case_id(c):
    x = "s8" if c.flags & SIGNED else "u8"
    kind = c.family if c.family == "i8" else "f32exact" if c.flags & EXACT else "f32fast"
    return f"{c.regime}-{kind}-{c.A}x{c.M}x{c.T}x{c.C}-{x}-{'gain' if c.gains is not None else 'unit'}-dch{c.dch}"


def int_scale(A, signed, gains, pow2):
    """An output scale at which random samples leave the int8 beams neither empty nor clamped: the beams' standard
    deviation is about sqrt(A) rms(x) g scale counts (rms(x) 147 for uint8, 74 for int8 samples; rms g 0.66);
    aim for 16 counts.  Power of two, or S6 times one.  tests/test_phase_cases_host.py checks the oracle's output."""
    sigma = math.sqrt(A) * (74.0 if signed else 147.0) * (0.66 if gains else 1.0)
    if pow2:
        return 2.0 ** round(math.log2(16.0 / sigma))
    return S6 * 2.0 ** round(math.log2(16.0 / sigma / S6))


def _int_cases():
    out = []
    for ri, reg in enumerate(REGIMES):
        for fi, ((A, M, T), path, ws, name) in enumerate(I8_FORMS):
            big = T == 256
            C = (C_BIG if big else C_SMALL)[reg.name]
            # (signed, weighted) cycle over forms and regimes; the ring kernel takes int8 samples only and the
            # in-kernel 32-beam kernel's two names are its unit and weighted forms
            signed = name.startswith(W32R) or ((fi + ri) % 2 == 0 and not (big and M % 32 == 0))  # (else: the ring)
            weighted = name.endswith("gain") or (not name.endswith("unit") and (fi // 2 + ri) % 2 == 1)
            anyscale = "anyscale" in name or ("{s}" in name and (fi + ri) % 3 == 0)
            flags = OUT_I8 | (SIGNED if signed else 0) | PATH[path]
            dch = C if (fi + ri) % 4 == 1 and not big else 1
            out.append(PCase(reg.name, "i8", A, M, T, 2, C, xeng_for(reg, C), flags,
                             name.format(s="anyscale" if anyscale else "pow2"), dch, A + M if weighted else None,
                             int_scale(A, signed, weighted, not anyscale), ws))
    return out


def _float_cases():
    out = []
    for ri, reg in enumerate(REGIMES):
        for fi, ((A, M, T), path, name) in enumerate(F32_FORMS):
            for exact in (False, True):
                C = C_SMALL[reg.name]
                signed = (fi + ri + exact) % 2 == 0
                flags = (SIGNED if signed else 0) | (EXACT if exact else 0) | PATH[path]
                dch = C if (fi + ri) % 3 == 1 else 1
                out.append(PCase(reg.name, "f32", A, M, T, 2, C, xeng_for(reg, C), flags,
                                 name.format(e="exact" if exact else "fast"), dch, None, 1.0, False))
        A, M, T = P2_SHAPE
        for C in sorted({C_BIG[reg.name], 2 if reg.place != "centre" else 3}):
            out.append(PCase(reg.name, "f32", A, M, T, 1, C, xeng_for(reg, C), SIGNED if ri % 2 else 0, P2_NAME, 1,
                             None, 1.0, False))
    return out


INT_CASES = _int_cases()
FLOAT_CASES = _float_cases()


def inputs(c):
    """(raw bytes, delay model, weights or None) of a fused case: uniformly random samples, the regime's model, weights
    of magnitude 0.25 .. 1 and either sign."""
    reg = BY_NAME[c.regime]
    seed = c.A * 131 + c.M * 7 + c.T + c.C + REGIMES.index(reg) * 1009
    rng = np.random.default_rng(seed)
    raw = rng.integers(0, 256, (c.B, c.A, c.C, c.T, 2, 2), dtype=np.uint8)
    d = model(reg, c.dch, c.M, c.A, seed + 1)
    gains = None
    if c.gains is not None:
        gains = (rng.uniform(0.25, 1.0, (c.M, c.A)) * rng.choice([-1.0, 1.0], (c.M, c.A))).astype(np.float32)
    return raw, d, gains


def times(c):
    reg = BY_NAME[c.regime]
    return reg.t0, batch_dt(reg, c.T)


def oracle_int8(c, raw, d, gains):
    reg, signed = BY_NAME[c.regime], bool(c.flags & SIGNED)
    t0, bdt = times(c)
    return O.fused_beamform_int8(raw.view(np.int8) if signed else raw, d, reg.Ctot, xeng_id=c.xeng, Ts=reg.Ts, t0=t0,
                                 batch_dt=bdt, scale=c.scale, signed=signed, gains=gains)


def float_bound(x_real, w, fast, R):
    """edge_cases.float_bound (unit weights on the fast forms) plus the float64 evaluation of the argument in another
    operation order: 8 * 2^-53 * R * sum_k |x_k|, R the case's largest mag (1.8e-9 per unit of sum |x| at R = 2e6)."""
    ones = np.ones(w.shape[-2:]) if fast else None
    return EC.float_bound(x_real, w, ones) + 8 * 2.0 ** -53 * R * np.abs(x_real).sum(axis=-1, keepdims=True)


# generators: (A, M, out offset, expected kernel) of bf_coeff_gen; the tile form ragged in both dimensions
COEFF_GEN = [(33, 34, 8, "coeff_gen_tile_kernel"), (5, 3, 8, "coeff_gen_kernel"),
             (33, 34, 0, "coeff_gen_block_kernel:nt")]
# bf_q14_coeffs: channels per call for the channel recurrence (runs of 64: a ragged second run, or two whole runs on
# the last engine of a band of 2^n channels), and for a model per channel
Q14_C1 = {"array_low": 70, "array_top_uhf": 128, "centre_sband": 70, "odd_band": 70, "guard_edge": 128, "beyond": 128}
Q14_CC = dict(C_SMALL, array_low=8, array_top_uhf=8, odd_band=6, beyond=8)
Q14_SHAPE = (19, 5)  # A, M: 95 words per channel, a full wave and a partial one
GEN_TIME_SHAPE = (5, 3)

# A generator call.  kind: coeff_gen (off: the table's byte offset) | coeff_gen_time (off: 1 = float16 output; B = the
# number of times, t0 + t batch_dt) | q14 (bf_q14_coeffs).  The steering times of the last two are the regime's t0 and
# batch_dt(reg, 256); bf_coeff_gen takes no time and ignores the rates.
Gen = namedtuple("Gen", "regime kind A M B C xeng dch weighted off expect")


def _gen_cases():
    out = []
    for reg in REGIMES:
        C = C_SMALL[reg.name]
        for A, M, off, name in COEFF_GEN:
            out.append(Gen(reg.name, "coeff_gen", A, M, 1, C, xeng_for(reg, C), C, False, off, name))
        A, M = GEN_TIME_SHAPE
        for f16 in (0, 1):
            for dch in (1, C):
                out.append(Gen(reg.name, "coeff_gen_time", A, M, 2, C, xeng_for(reg, C), dch, False, f16,
                               "coeff_gen_time_kernel:" + ("f16" if f16 else "f32")))
        A, M = Q14_SHAPE
        for C, per_channel in ((Q14_C1[reg.name], False), (Q14_CC[reg.name], True)):
            for weighted in (False, True):
                out.append(Gen(reg.name, "q14", A, M, 2, C, xeng_for(reg, C), C if per_channel else 1, weighted, 0,
                               f"q14_table_kernel:{'gain' if weighted else 'unit'},natural"))
    return out


GEN_CASES = _gen_cases()


def gen_id(g):
    return f"{g.regime}-{g.kind}-{g.A}x{g.M}x{g.C}-dch{g.dch}-{'gain' if g.weighted else 'unit'}-{g.off}"


def gen_times(g):
    reg = BY_NAME[g.regime]
    return (0.0, 0.0) if g.kind == "coeff_gen" else (reg.t0, batch_dt(reg, 256))


def gen_inputs(g):
    """(delay model, weights or None) of a generator case; weights up to the Q14 contract's +-1.9."""
    reg = BY_NAME[g.regime]
    seed = g.A * 131 + g.M * 7 + g.C * 3 + g.dch + REGIMES.index(reg) * 1009
    gains = None
    if g.weighted:
        gains = np.random.default_rng(seed + 5).uniform(-1.9, 1.9, (g.M, g.A)).astype(np.float32)
    return model(reg, g.dch, g.M, g.A, seed), gains


def q14_words(w):
    """The (B, C, M, A) words Wc | Ws << 16 of bf_q14_coeffs from a Q14 table (B, 2, C, 2A, 2M) (quantise_coeffs)."""
    wc, ws = w[:, 0, :, 0::2, 0::2], w[:, 0, :, 0::2, 1::2]  # (B, C, A, M): W[2a][2m] = cos, W[2a][2m+1] = sin
    word = (wc.astype(np.int64) & 0xffff) | ((ws.astype(np.int64) & 0xffff) << 16)
    return np.ascontiguousarray(word.transpose(0, 1, 3, 2)).astype(np.uint32)
