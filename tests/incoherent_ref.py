"""NumPy restatement of the incoherent-beam contract (include/bf.h, bf_incoherent_beam):

    S[b][p][c][j]   = sum over antennas a with mask[a] != 0 (all when mask is None),
                      sum over t in [j*tint, (j+1)*tint) of x_re^2 + x_im^2                      (exact, int64)
    out[b][p][c][j] = float32(float64(S) * float64(float32(scale)))

With sum_pols the two polarisations are added into S before scaling.  S < 2^53 for every accepted shape, so the float64
conversion is exact and the output has one rounding (NumPy's float64 -> float32 cast rounds to nearest even).
"""
import numpy as np


def power_sums(raw, tint, signed, sum_pols=False, mask=None):
    """Exact int64 S of a (B, A, C, T, 2, 2) 8-bit cube: (B, 2, C, T // tint), or (B, 1, ...) with sum_pols."""
    raw = np.asarray(raw)
    B, A, C, T = raw.shape[:4]
    assert raw.shape[4:] == (2, 2) and raw.dtype.itemsize == 1 and T % tint == 0
    x = raw.view(np.int8 if signed else np.uint8)
    if mask is not None:
        x = x[:, np.asarray(mask) != 0]
    S = np.zeros((B, C, T, 2), np.int64)
    for a in range(x.shape[1]):  # antenna by antenna: no (B, A, C, T, 2, 2) int64 temporary
        v = x[:, a].astype(np.int64)
        S += v[..., 0] ** 2 + v[..., 1] ** 2
    S = S.reshape(B, C, T // tint, tint, 2).sum(axis=3)  # (B, C, J, 2)
    S = np.ascontiguousarray(S.transpose(0, 3, 1, 2))    # (B, 2, C, J)
    return S.sum(axis=1, keepdims=True) if sum_pols else S


def scale_sums(S, scale):
    assert int(np.max(S, initial=0)) < 2 ** 53
    return (S.astype(np.float64) * np.float64(np.float32(scale))).astype(np.float32)


def incoherent_beam(raw, tint, signed, sum_pols=False, scale=1.0, mask=None):
    return scale_sums(power_sums(raw, tint, signed, sum_pols, mask), scale)
