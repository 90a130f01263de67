"""NumPy restatement of the dedisperser contract (include/bf.h, bf_dedisperse):

    power (B, S, K, J, M) f32, ring (K, R, M) f32, lags (D, K) int32, N = B*J, n = b*J + j
    1. ring[k][(head + n) % R][m] = power[b][plane][k][j][m]                           (bits copied)
    2. acc[m][d][n] = sum over k of ring[k][(head + n - lag[d][k]) mod R][m]           (float64 sum of the f32 values)
       out[m][d][n] = float32(acc * float64(float32(scale)))
    lag = lags clamped into [0, R - N].

The sum is NumPy's float64 sum over the channel axis, in its order.  `tolerance` is the derived bound between two
float64 evaluations of the same sum in different orders.
"""
import numpy as np


def clamp_lags(lags, R, N):
    return np.clip(np.asarray(lags, np.int64), 0, R - N)


def append(power, ring, head, plane=0):
    """Step 1 on a copy of `ring`: the new ring."""
    power, ring = np.asarray(power), np.array(ring, np.float32)
    B, S, K, J, M = power.shape
    N, R = B * J, ring.shape[1]
    assert power.dtype == np.float32 and ring.shape == (K, R, M)
    assert R % N == 0 and 0 <= head < R and head % N == 0 and 0 <= plane < S
    ring[:, head:head + N] = power[:, plane].transpose(1, 0, 2, 3).reshape(K, N, M)
    return ring


def channel_sums(ring, lags, head, N):
    """Step 2's acc and the same sum of |x|: two float64 (M, D, N) arrays."""
    ring = np.asarray(ring)
    K, R, M = ring.shape
    lag = clamp_lags(lags, R, N)
    D = lag.shape[0]
    assert lag.shape == (D, K)
    slot = (head + np.arange(N)[None, None, :] - lag[:, :, None]) % R       # (D, K, N)
    x = ring[np.arange(K)[None, :, None], slot].astype(np.float64)          # (D, K, N, M)
    return x.sum(axis=1).transpose(2, 0, 1), np.abs(x).sum(axis=1).transpose(2, 0, 1)


def scale_sums(acc, scale):
    return (np.asarray(acc, np.float64) * np.float64(np.float32(scale))).astype(np.float32)


def dedisperse(power, ring, lags, head, plane=0, scale=1.0):
    """One call: (out (M, D, N) f32, the new ring)."""
    power = np.asarray(power)
    N = power.shape[0] * power.shape[3]
    new = append(power, ring, head, plane)
    acc, _ = channel_sums(new, lags, head, N)
    return scale_sums(acc, scale), new


def one_shot(stream, lags, scale=1.0):
    """The whole stream (K, Ntot, M) at once, zero before its first sample: out[m][d][t] = sum_k stream[k][t - lag]."""
    stream = np.asarray(stream, np.float32)
    K, Nt, M = stream.shape
    lag = np.asarray(lags, np.int64)
    assert lag.min() >= 0
    padded = np.concatenate([np.zeros((K, int(lag.max()), M), np.float32), stream], axis=1)
    t = int(lag.max()) + np.arange(Nt)[None, None, :] - lag[:, :, None]     # (D, K, Nt)
    x = padded[np.arange(K)[None, :, None], t].astype(np.float64)
    return scale_sums(x.sum(axis=1).transpose(2, 0, 1), scale)


def tolerance(ref_out, abs_sums, K, scale):
    """Bound on |got - ref_out| per element for general f32 values.  A float64 sum of K values, in any order, errs by
    at most K * 2^-53 * sum|x|; the kernel and this reference each stay within that, and the float32 rounding adds half
    an ulp to each: 2^-23 * |ref_out| + K * 2^-51 * scale * sum_k|x_k|.  `abs_sums` is channel_sums(...)[1]."""
    return (2.0 ** -23 * np.abs(np.asarray(ref_out, np.float64)) +
            K * 2.0 ** -51 * float(np.float32(scale)) * np.asarray(abs_sums, np.float64))
