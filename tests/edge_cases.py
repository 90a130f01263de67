"""The beam paths at the edges of their numeric range, as data: input builders and case lists, importable without a GPU.

tests/test_edge_cases_host.py proves from the oracle alone that the inputs do what they claim (how close the int32 sums
come to 2^31, which limbs the Q14 tables hold, how much of the output saturates, which kernel the planner names);
tests/test_gpu_edges.py runs them.  The cases are deliberately not part of fused_cases.GRIDS.

Integer beams (the Q14 contract: exact int32 sums, q = sat127(rne(f32(y) * scale * 2^-14))):
  bound  zero delays and rates, beam m at phase f32(pi/4 + (m mod 4) pi/2) for every antenna, so Wc = +-11585 and
         Ws = +-11585 at unit gain and |Wc| + |Ws| is at its maximum; the samples of `edge_samples` then drive one
         component of every beam to the extreme of the int32 range.  Two scales, 2^-11 and S6 * 2^-8: nothing
         saturates, and a sum that wrapped by 2^32 moves the output by 128 or about 85 counts.
  limb   random delay models with every gain +-f32(32639 / 16384), beam 0 at phase 0: W = +-32639 exactly, the
         admitted maximum, whose high limb is +-127.
  sat    the bound cases' shapes, gains and samples at scales 2^-4, 2^12 and S6 * 2^12: the clamp, and f32(y) * s beyond
         2^22 for the last two.  Two things differ from the bound inputs, because with them a tenth and more of the
         output cannot saturate at any scale: the phases start at pi/8 (at pi/4 one component of every beam is
         exactly zero on the class (a) rows, a sixth of the entries), and the random int8 rows are one-sided (zero-mean
         rows leave half of their sums below the clamp at 2^-4).
  low    the bound inputs at scale 2^5, where the other rows saturate and the class (d) rows -- one coefficient left of
         sums whose parts (for uint8: -128 * colsum and its correction, each near 2^30) cancel -- resolve y to 1/512 of
         a count: an error of some hundreds of units in either part shows here, and only here.
  fine   the bound inputs with W = +-16768 (high limb 66, low limb -128) over 500 int8 antennas, at the finest scale
         that does not saturate (2^31 -> 127 counts).  The sum of the high limbs, shifted, passes -2^31 by 1.5e7 and
         the low limbs bring it back; a shift that saturates instead of wrapping is off by 0.9 count.  At the bound
         cases' scales that error stays below half a count whatever the weights (at most A 2^15): only this scale
         shows it.
Float beams (f16 hi/lo split coefficients): `range_gains` / `range_table`, weights from 2^-21 to 65504.
"""
from collections import namedtuple

import numpy as np

import fused_cases as FC
import oracle as O

TS = O.TS_MEERKAT
CTOT, XENG, T0 = 8192, 3, 2.5e-3
BDT = 256 * 8192 * TS
SIGNED, OUT_I8, EXACT, PATH, S6 = FC.SIGNED, FC.OUT_I8, FC.EXACT, FC.PATH, FC.S6

G_MAX = float(np.float32(32639 / 16384))  # rne(G_MAX * 2^14) = 32639: the largest weight of the Q14 contract
BOUND_SCALES = [2.0 ** -11, S6 * 2.0 ** -8]  # the power-of-two and the any-scale form; 2^31 -> 64 and 85 counts
SAT_SCALES = [2.0 ** -4, 2.0 ** 12, S6 * 2.0 ** 12]
LOW_SCALE = 2.0 ** 5  # one count per 512 of y: the class (d) rows, y = one coefficient, land at 16 .. 90 counts
FINE_SCALE = 127 * 2.0 ** -17  # 2^31 -> 127 counts: the finest scale at which sums at the edge do not saturate
G_16768 = 1.44736  # W = +-16768 = 66 * 256 - 128 at the bound phases: high limb 66, low limb -128
F16_MAX = 65504.0

# gains: the magnitude of every weight (None: no weight table, unit gain).  frac: the least max(Y) / 2^31 and
# -min(Y) / 2^31 the case's inputs reach (bound cases).  The other fields are fused_cases.Call's.
Case = namedtuple("Case", "kind A M T B C flags expect gains scale workspace frac dch", defaults=(1,))


def case_id(c):
    s = {BOUND_SCALES[0]: "2^-11", BOUND_SCALES[1]: "S6*2^-8", SAT_SCALES[0]: "2^-4", SAT_SCALES[1]: "2^12",
         SAT_SCALES[2]: "S6*2^12", LOW_SCALE: "2^5", FINE_SCALE: "127*2^-17"}[c.scale]
    g = "unit" if c.gains is None else f"g{c.gains:.4f}"
    x = "s8" if c.flags & SIGNED else "u8"
    return f"{c.kind}-{c.expect.split(':')[0][15:]}-{c.A}x{c.M}x{c.T}x{c.C}-{x}-{g}-{s}"


# ---- inputs --------------------------------------------------------------------------------------------------------
def bound_delays(M, A, first=np.pi / 4):
    """Zero delays and rates; beam m at phase f32(first + (m mod 4) pi/2) for every antenna (one model for all
    channels).  first = pi/4: |Wc| = |Ws|, the largest |Wc| + |Ws|."""
    d = np.zeros((1, M, A, 4), np.float32)
    d[0, :, :, 2] = (first + (np.arange(M) % 4) * (np.pi / 2)).astype(np.float32)[:, None]
    return d


def random_delays(dch, M, A, seed):
    """Random delay models: delays, delay rates, phases and phase rates, as the guard-band suite draws them."""
    rng = np.random.default_rng(seed)
    d = np.zeros((dch, M, A, 4), np.float32)
    d[..., 0] = rng.uniform(0, 10 * TS, (dch, M, A))
    d[..., 1] = rng.uniform(-1e-9, 1e-9, (dch, M, A))
    d[..., 2] = rng.uniform(-np.pi, np.pi, (dch, M, A))
    d[..., 3] = rng.uniform(-1.0, 1.0, (dch, M, A))
    return d


def limb_delays(M, A, seed):
    """Random delay models with beam 0 at phase 0 for every antenna: its coefficients are W = rne(g * 2^14) and 0."""
    d = random_delays(1, M, A, seed)
    d[0, 0] = 0
    return d


def row_class(T, pol):
    """Class 0..3 = (a)..(d) of sample row t of pol `pol`: t mod 4, pol 1 rotated by two rows."""
    return (np.arange(T) + 2 * pol) % 4


def edge_samples(B, A, C, T, signed, seed, one_sided=False):
    """The raw (B, A, C, T, 2, 2) cube (bytes) whose rows are, by row_class,
      (a) every antenna (255, 255), or (-128, -128) for int8 -- the one value whose negation does not fit int8;
      (b) every antenna (255, 0), or (-128, 127);
      (c) uniformly random over the full range (one_sided: int8 over [-128, 0) only, so that the sums of these rows are
          as far from zero as those of uint8 samples);
      (d) zero except antenna A - 1 = (1, 0), or (1, -1): the padded last k-step and the low bits at a large scale."""
    rng = np.random.default_rng(seed)
    lo, hi = (-128, 0 if one_sided else 128) if signed else (0, 256)
    rand = rng.integers(lo, hi, (B, A, C, T, 2, 2))
    x = np.zeros((B, A, C, T, 2, 2), np.int64)
    for pol in (0, 1):
        cls = row_class(T, pol)
        x[:, :, :, cls == 0, pol, :] = (-128, -128) if signed else (255, 255)
        x[:, :, :, cls == 1, pol, :] = (-128, 127) if signed else (255, 0)
        x[:, :, :, cls == 2, pol, :] = rand[:, :, :, cls == 2, pol, :]
        x[:, A - 1, :, cls == 3, pol, :] = (1, -1) if signed else (1, 0)
    return x.astype(np.int8).view(np.uint8) if signed else x.astype(np.uint8)


def inputs(c):
    """(raw bytes, delay models, weight table or None) of an integer case."""
    signed = bool(c.flags & SIGNED)
    seed = c.A * 131 + c.M * 7 + c.T + c.C + signed
    raw = edge_samples(c.B, c.A, c.C, c.T, signed, seed, one_sided=c.kind == "sat")
    if c.kind == "limb":
        sign = np.random.default_rng(seed + 1).choice(np.float32([-1, 1]), (c.M, c.A))
        return raw, limb_delays(c.M, c.A, seed + 2), (sign * np.float32(c.gains)).astype(np.float32)
    gains = None if c.gains is None else np.full((c.M, c.A), c.gains, np.float32)
    return raw, bound_delays(c.M, c.A, np.pi / 8 if c.kind == "sat" else np.pi / 4), gains


def int64_sums(raw, d, gains, signed):
    """Y = X W in int64 with W the oracle's Q14 table: (Y (B, 2, C, T, 2M), W (B, 2, C, 2A, 2M))."""
    B, A, C, T = raw.shape[:4]
    W = O.quantise_coeffs(O.fused_tables(d, B, C, CTOT, A, xeng_id=XENG, t0=T0, batch_dt=BDT, gains=gains))
    xr = O.reorder(raw)
    X = (xr.view(np.int8) if signed else xr).astype(np.int64).reshape(B, 2, C, T, 2 * A)
    return np.matmul(X, W), W


def oracle_int8(c, raw, d, gains):
    signed = bool(c.flags & SIGNED)
    return O.fused_beamform_int8(raw.view(np.int8) if signed else raw, d, CTOT, xeng_id=XENG, t0=T0, batch_dt=BDT,
                                 scale=c.scale, signed=signed, gains=gains)


# ---- the integer cases ---------------------------------------------------------------------------------------------
GEN, W32, ITEM = "beamform_fused_i8_kernel:", "beamform_fused_i8_w32_kernel:", "beamform_fused_i8_item_kernel:"
W32T, W32R = FC.W32T, FC.W32R
# family shapes: A, M, T, C, signed, gains, path, workspace, name ({s}: pow2 | anyscale), fraction of 2^31
SHAPES = [
    # the generic kernel, groups of 64 antennas: both slab widths, the largest A of each sample type
    (724, 4, 16, 2, True, None, "generic", False, GEN + "nts1", 0.99987),
    (363, 9, 16, 2, False, None, "generic", False, GEN + "nts2", 0.99872),
    (363, 9, 16, 2, True, G_MAX, "generic", False, GEN + "nts2", 0.9987),
    (182, 4, 16, 2, False, G_MAX, "generic", False, GEN + "nts1", 0.9975),
    # the 32-beam kernel that evaluates its phasors itself (no workspace); M = 40: a partial slab
    (512, 32, 16, 2, True, 1.4141703, "wide", False, W32 + "gain", 0.99994),
    (512, 32, 16, 2, False, 0.70983654, "wide", False, W32 + "gain", 0.99998),
    (363, 40, 16, 2, False, None, "wide", False, W32 + "unit", 0.99872),
    # the table-driven 32-beam kernels
    (256, 40, 16, 3, False, 1.4197162, "wide", True, W32T + "general,buf", 0.99998),
    (256, 64, 256, 3, False, 1.4197162, "wide", True, W32T + "straight,{s}", 0.99998),
    # the LDS-DMA ring kernel: int8 only, A <= 256, so 0.704 of the bound is the most its shape admits
    (256, 32, 256, 3, True, G_MAX, "wide", True, W32R + "{s}", 0.70),
    # the item kernel: A <= 64 cannot approach the bound; every form, at the largest weight
    (64, 8, 16, 2, True, G_MAX, "auto", False, ITEM + "nts1,full,a64,{s}", 0.17),
    (64, 12, 16, 2, False, G_MAX, "auto", False, ITEM + "nts2,partial,a64,{s}", 0.17),
    (61, 4, 16, 2, False, G_MAX, "auto", False, ITEM + "nts1,partial,aany,{s}", 0.17),
    (61, 16, 16, 2, False, G_MAX, "auto", False, ITEM + "nts2,full,aany,{s}", 0.17),
]
# the limb cases' shapes: where every gain is +-G_MAX the worst-case sum A max|x| (|Wc| + |Ws|) must still fit, so the
# generic and phasor kernels use fewer antennas than above; beam 0 (phase 0) reaches A max|x| 32639
LIMB_SHAPES = [
    (363, 9, 16, 2, True, G_MAX, "generic", False, GEN + "nts2", None),
    (182, 4, 16, 2, False, G_MAX, "generic", False, GEN + "nts1", None),
    (363, 40, 16, 2, True, G_MAX, "wide", False, W32 + "gain", None),
    (182, 32, 16, 2, False, G_MAX, "wide", False, W32 + "gain", None),
    (182, 40, 16, 3, False, G_MAX, "wide", True, W32T + "general,buf", None),
    (256, 40, 256, 2, True, G_MAX, "wide", True, W32T + "straight,{s}", None),
    (256, 32, 256, 2, True, G_MAX, "wide", True, W32R + "{s}", None),
    (64, 8, 16, 2, True, G_MAX, "auto", False, ITEM + "nts1,full,a64,{s}", None),
    (61, 12, 16, 2, True, G_MAX, "auto", False, ITEM + "nts2,partial,aany,{s}", None),
    (64, 16, 16, 2, False, G_MAX, "auto", False, ITEM + "nts2,full,a64,{s}", None),
    (61, 7, 16, 2, False, G_MAX, "auto", False, ITEM + "nts1,partial,aany,{s}", None),
]
# the saturation cases: one bound shape per family and sample type
SAT_SHAPES = [SHAPES[i] for i in (0, 1, 4, 5, 7, 8, 9, 10, 13)]


def _cases(kind, shapes, scales):
    out = []
    for (A, M, T, C, signed, gains, path, workspace, name, frac) in shapes:
        for scale in scales:
            pow2 = scale in (2.0 ** -11, 2.0 ** -4, 2.0 ** 12, LOW_SCALE)
            flags = OUT_I8 | (SIGNED if signed else 0) | PATH[path]
            out.append(Case(kind, A, M, T, 1, C, flags, name.format(s="pow2" if pow2 else "anyscale"), gains, scale,
                            workspace, frac))
    return out


BOUND_CASES = _cases("bound", SHAPES, BOUND_SCALES)
LIMB_CASES = _cases("limb", LIMB_SHAPES, BOUND_SCALES[:1]) + _cases("limb", LIMB_SHAPES[5:8], BOUND_SCALES[1:])
SAT_CASES = _cases("sat", SAT_SHAPES, SAT_SCALES)
LOW_CASES = _cases("low", SHAPES, [LOW_SCALE])
# the 32-beam kernel combines its limb sums once at the end, (hi << 8) + lo; with int8 samples and more than 256
# antennas (beyond the table-driven forms' reach) hi << 8 alone can leave the int32 range while the sum fits.  The
# other kernels shift per group of 64 antennas or sum at most 256 antennas: their shifted sums cannot leave it.
FINE_SHAPES = [(500, 32, 16, 2, True, G_16768, "wide", False, W32 + "gain", 0.99945),
               (500, 40, 16, 3, True, G_16768, "wide", False, W32 + "gain", 0.99945)]
FINE_CASES = _cases("fine", FINE_SHAPES, [FINE_SCALE])
INT_CASES = BOUND_CASES + LIMB_CASES + SAT_CASES + LOW_CASES + FINE_CASES


# ---- float beams: weights over the whole domain of the f16 hi/lo split ----------------------------------------------
RANGE_EXPONENTS = (15, 8, 0, -8, -14, -20)


def _range_classes(rng, n_cols, n_rows):
    """(n_cols, n_rows) float32: column j of magnitude class 2^e, e cycling through RANGE_EXPONENTS, times
    uniform(0.5, 1) with a random sign; the last column mixes all classes along its rows; +-65504 placed exactly."""
    e = np.array(RANGE_EXPONENTS, np.float64)[np.arange(n_cols) % len(RANGE_EXPONENTS)][:, None] * np.ones((1, n_rows))
    e[n_cols - 1] = np.array(RANGE_EXPONENTS, np.float64)[np.arange(n_rows) % len(RANGE_EXPONENTS)]
    w = 2.0 ** e * rng.uniform(0.5, 1.0, (n_cols, n_rows)) * rng.choice([-1.0, 1.0], (n_cols, n_rows))
    w[0, n_rows // 2] = F16_MAX
    w[0, n_rows - 1] = -F16_MAX
    return w.astype(np.float32)


def range_gains(M, A, seed):
    """(M, A) beam weights: beam m of class 2^e (the last beam mixes the classes across antennas), gains[0] holding
    the largest admitted weight +-65504."""
    return _range_classes(np.random.default_rng(seed), M, A)


def range_table(shape, seed):
    """A MatrixMultiply coefficient table (B, P, C, 2A, 2M) with the classes of range_gains per column."""
    B, P, C, K, N = shape
    rng = np.random.default_rng(seed)
    w = np.stack([_range_classes(rng, N, K).T for _ in range(B * P * C)])
    return np.ascontiguousarray(w.reshape(B, P, C, K, N))


def float_bound(x_real, w, fast_gains=None):
    """The derived bound of the float beams against the exact product, no ATOL or RTOL term:
        2^-20 sum_k |x_k w_k|    the project's stated float32 dot-product term (tolerance.py)
      + 2^-25 sum_k |x_k|        f16's subnormal half-spacing: the absolute floor of the hi/lo split per coefficient
      + 2^-22 sum_k |x_k g_k|    fast phasors only: two ulps of a unit phasor, times the weight
    x_real (..., T, 2A) and w (..., 2A, 2M) as float64; fast_gains (2A, 2M) = |g| of row k's antenna, column n's beam.
    """
    ax = np.abs(x_real)
    b = 2.0 ** -20 * np.matmul(ax, np.abs(w)) + 2.0 ** -25 * ax.sum(axis=-1, keepdims=True)
    if fast_gains is not None:
        b = b + 2.0 ** -22 * np.matmul(ax, np.abs(fast_gains))
    return b


def f16_split(w):
    """The kernels' coefficient split (put_split): hi = f16(w), lo = f16(w - hi), as float64 hi + lo."""
    w = np.asarray(w, np.float32)
    with np.errstate(over="ignore", invalid="ignore"):
        hi = w.astype(np.float16)
        lo = (w - hi.astype(np.float32)).astype(np.float16)
        return hi.astype(np.float64) + lo.astype(np.float64)


# float cases: (A, M, T), path, expected name ({e}: exact | fast); every one runs with a range_gains table
FLOAT_FUSED = [
    ((33, 9, 80), "auto", FC.ITEM + "nts2,partial,{e}"), ((64, 16, 256), "auto", FC.ITEM + "nts2,full,{e},staged"),
    ((16, 8, 48), "auto", FC.ITEM + "nts1,full,{e}"), ((5, 3, 16), "auto", FC.ITEM + "nts1,partial,{e}"),
    ((130, 9, 64), "auto", FC.GEN + "nts2,{e}"), ((80, 2, 16), "auto", FC.GEN + "nts1,{e}"),
    ((16, 3, 32), "wide", FC.WIDE + "tw1,{e},gain,buf"), ((656, 20, 32), "wide", FC.WIDE + "tw1,{e},gain,buf"),
    ((72, 33, 64), "auto", FC.WIDE + "tw2,{e},gain,buf"), ((200, 40, 96), "auto", FC.WIDE + "tw2,{e},gain,buf"),
]


def float_fused_call(case, signed, exact):
    (A, M, T), path, expect = case
    flags = (SIGNED if signed else 0) | (EXACT if exact else 0) | PATH[path]
    return FC.Call(A, M, T, 2, 3, flags, expect.format(e="exact" if exact else "fast"), dch=1 if A % 2 else 3,
                   gains=A + M)


RING, TABLE = "beamform_table_ring_kernel:", "beamform_table_kernel:"
# bf_beamform: A, M, NB, B, C, x offset, w offset, expected name (the shapes of test_gpu_guarded for these names)
FLOAT_TABLE = [
    (64, 3, 3, 2, 3, 0, 4, RING + "nts1,r4,w16"), (128, 9, 3, 2, 3, 8, 4, RING + "nts2,r8,w8"),
    (256, 40, 3, 1, 1, 0, 4, RING + "nts2,r16,w16"), (128, 25, 2, 1, 2, 0, 4, RING + "nts4,r8,w16"),
    (64, 64, 2, 1, 2, 8, 4, RING + "nts8,r4,w8"),
    (256, 12, 2, 2, 2, 0, 4, "beamform_table_persist_kernel:nts2,r16,u8"),
    (4, 3, 3, 2, 3, 0, 4, TABLE + "nts1,vec8"), (5, 9, 3, 2, 3, 0, 4, TABLE + "nts2,scalar"),
    (12, 25, 3, 2, 3, 8, 4, TABLE + "nts4,vec8"), (5, 64, 3, 2, 3, 0, 4, TABLE + "nts8,scalar"),
    (64, 64, 16, 1, 2, 16, 16, "beamform_table_os_kernel"), (128, 64, 16, 1, 2, 16, 16, "beamform_table_os_kernel"),
]
