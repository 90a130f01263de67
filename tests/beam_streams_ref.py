"""NumPy restatement of the beam-streams contract (bf_beam_streams, include/bf.h) and a seeded generator
of beams for its tests.

    beams (B, 2, C, T/16, 16, 2M) -> out (B, K, C, T, 2, 2)
    out[b, k, c, t, p, z] = beams[b, p, c, t/16, t%16, 2 m + z],  m = index[k]   (0 where m is outside [0, M))

a copy of bits; with `scale` the float32 beams are requantised like oracle.requantise.
"""
import numpy as np

import oracle as O

FORMS = ("i8", "f32", "f32q")
SCALE = 1 / 3  # the requantising form's scale: not a power of two, so the product rounds


def beam_streams(beams, index=None, scale=None):
    """The streams of `beams`; index None = every beam in order.  Entries outside [0, M) give zero streams."""
    beams = np.asarray(beams)
    B, P, C, NB, S, M2 = beams.shape
    assert P == 2 and S == 16 and M2 % 2 == 0
    M, T = M2 // 2, NB * S
    sel = np.arange(M) if index is None else np.asarray(index, np.int64)
    ok = (sel >= 0) & (sel < M)
    y = beams.reshape(B, 2, C, T, M, 2)[:, :, :, :, np.where(ok, sel, 0), :].transpose(0, 4, 2, 3, 1, 5)
    if scale is not None:
        assert beams.dtype == np.float32
        y = O.requantise(y, scale)
    y = np.ascontiguousarray(y)
    y[:, ~ok] = 0
    return y


def by_elements(beams, index=None):
    """The same by the element formula, one Python loop level per axis (small shapes only)."""
    B, _, C, NB, _, M2 = beams.shape
    M, T = M2 // 2, NB * 16
    sel = list(range(M)) if index is None else [int(m) for m in index]
    out = np.zeros((B, len(sel), C, T, 2, 2), beams.dtype)
    for b in range(B):
        for k, m in enumerate(sel):
            if not 0 <= m < M:
                continue
            for c in range(C):
                for t in range(T):
                    for p in range(2):
                        for z in range(2):
                            out[b, k, c, t, p, z] = beams[b, p, c, t // 16, t % 16, 2 * m + z]
    return out


F32_SPECIALS = np.array([0x7fc00000 | 0x1234, 0xffc0beef, 0x7f800001 | 0x2a00,  # NaNs with payloads (quiet, signalling)
                         0x7f800000, 0xff800000, 0x80000000, 0x00000001, 0x807fffff], np.uint32).view(np.float32)
F32_HALVES = np.array([0.5, 1.5, 2.5, -0.5, -1.5, 126.5, 127.5, -127.5, 1e30, -1e30], np.float32) / np.float32(SCALE)


def random_beams(B, C, T, M, int8, seed=0):
    """Seeded beams (B, 2, C, T/16, 16, 2M).  int8: every value of [-128, 127], with -128 and +-127 placed.  float32:
    Gaussian of rms 200 (so scale 1/3 both rounds and saturates) with NaNs that carry a payload, +-inf, -0.0,
    subnormals and rounding ties scattered at seeded positions."""
    rng = np.random.default_rng([seed, B, C, T, M, int(int8)])
    shape = (B, 2, C, T // 16, 16, 2 * M)
    n = int(np.prod(shape))
    if int8:
        y = rng.integers(-128, 128, n, dtype=np.int8)
        y[rng.permutation(n)[:3]] = (-128, 127, -127)
        return y.reshape(shape)
    y = (200 * rng.standard_normal(n)).astype(np.float32)
    special = np.concatenate([F32_SPECIALS, F32_HALVES])
    at = rng.permutation(n)[:min(n, 2 * special.size)]
    y.view(np.uint32)[at] = np.resize(special.view(np.uint32), at.size)
    return y.reshape(shape)


def as_bytes(a):
    return np.ascontiguousarray(a).view(np.uint8)
