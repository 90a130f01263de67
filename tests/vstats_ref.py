"""NumPy restatement of the voltage-statistics contract (include/bf.h, bf_voltage_stats):

    pw = x_re^2 + x_im^2 of one sample of one pol; for the window t in [j*tint, (j+1)*tint) of (b, a, pol, c), n = tint:
    S1 = sum pw        S2 = sum pw^2                                                           (exact, int64)
    power = float32(float64(S1) * float64(float32(scale)))
    sk    = 0 where S1 == 0, else float32(k * ((nd * float64(S2)) / (float64(S1) * float64(S1)) - 1.0)),
            nd = float64(n), k = (nd + 1) / (nd - 1)
    flags = (S1 == 0) | (sk < float32(lo)) | (sk > float32(hi))                     (float32 compares of the stored sk)

All outputs have shape (B, A, 2, C, T // tint).  S2 < 2^52 for every accepted shape, so the float64 conversions are
exact; every float64 operation below is one NumPy elementwise operation, in the contract's order (NumPy never fuses a
multiply into an add), and the float64 -> float32 cast rounds to nearest even.
"""
import numpy as np


def moments(raw, tint, signed):
    """Exact int64 (S1, S2) of a (B, A, C, T, 2, 2) 8-bit cube, each (B, A, 2, C, T // tint)."""
    raw = np.asarray(raw)
    B, A, C, T = raw.shape[:4]
    assert raw.shape[4:] == (2, 2) and raw.dtype.itemsize == 1 and T % tint == 0
    x = raw.view(np.int8 if signed else np.uint8)
    S1 = np.empty((B, A, 2, C, T // tint), np.int64)
    S2 = np.empty_like(S1)
    for a in range(A):  # antenna by antenna: no whole-cube int64 temporary
        v = x[:, a].astype(np.int64)
        pw = v[..., 0] ** 2 + v[..., 1] ** 2                                             # (B, C, T, 2)
        pw = pw.reshape(B, C, T // tint, tint, 2)
        S1[:, a] = pw.sum(axis=3).transpose(0, 3, 1, 2)
        S2[:, a] = (pw * pw).sum(axis=3).transpose(0, 3, 1, 2)
    return S1, S2


def scale_power(S1, scale):
    assert int(np.max(S1, initial=0)) < 2 ** 53
    return (S1.astype(np.float64) * np.float64(np.float32(scale))).astype(np.float32)


def spectral_kurtosis(S1, S2, tint):
    assert int(np.max(S2, initial=0)) < 2 ** 53
    nd = np.float64(tint)
    k = (nd + 1.0) / (nd - 1.0)
    s1 = S1.astype(np.float64)
    dead = S1 == 0
    s1[dead] = 1.0  # any non-zero value: these elements are replaced below
    num = nd * S2.astype(np.float64)
    den = s1 * s1
    ratio = num / den
    excess = ratio - 1.0
    sk = (k * excess).astype(np.float32)
    sk[dead] = np.float32(0.0)
    return sk


def flag(S1, sk, limits):
    lo, hi = np.float32(limits[0]), np.float32(limits[1])
    assert sk.dtype == np.float32
    return ((S1 == 0) | (sk < lo) | (sk > hi)).astype(np.uint8)


def voltage_stats(raw, tint, signed, scale=1.0, limits=None):
    """(power, sk, flags) of the contract; flags is None without limits."""
    S1, S2 = moments(raw, tint, signed)
    sk = spectral_kurtosis(S1, S2, tint)
    return scale_power(S1, scale), sk, None if limits is None else flag(S1, sk, limits)


# ---- shared test inputs (built once per process, never modified) -----------------------------------------------------
SCALING_SHAPE = (1, 2, 4, 2048, 1024)  # (B, A, C, T, tint): random uint8 window sums near 2^25.4, 26 significant bits
FOUR_SHAPE = (1, 4, 2, 8192, 4096)     # the four-behaviour cube, signed
FOUR_LIMITS = (0.75, 1.25)
_cache = {}


def random_voltages(shape):
    """Uniformly random full-range bytes (B, A, C, T, 2, 2), one cube per shape (read as uint8 or int8)."""
    if shape not in _cache:
        raw = np.random.default_rng(sum(shape)).integers(0, 256, tuple(shape) + (2, 2), dtype=np.uint8)
        raw.setflags(write=False)
        _cache[shape] = raw
    return _cache[shape]


def four_behaviours():
    """int8 cube of FOUR_SHAPE: antenna 0 Gaussian noise (sigma 20), 1 a constant 3+4i, 2 all zeros, 3 noise (sigma 10)
    whose first tenth of every window is multiplied by 5; rounded and clipped to int8."""
    if "four" not in _cache:
        B, A, C, T, tint = FOUR_SHAPE
        rng = np.random.default_rng(4)
        x = np.zeros((B, A, C, T, 2, 2), np.float64)
        x[:, 0] = 20.0 * rng.standard_normal((B, C, T, 2, 2))
        x[:, 1, ..., 0], x[:, 1, ..., 1] = 3.0, 4.0
        pulsed = 10.0 * rng.standard_normal((B, C, T // tint, tint, 2, 2))
        pulsed[:, :, :, :tint // 10] *= 5.0
        x[:, 3] = pulsed.reshape(B, C, T, 2, 2)
        raw = np.clip(np.rint(x), -128, 127).astype(np.int8)
        raw.setflags(write=False)
        _cache["four"] = raw
    return _cache["four"]
