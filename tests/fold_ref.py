"""NumPy restatement of the folder contract (include/bf.h, bf_fold):

    power (B, S, K, J, M) f32, beam (F), phase0 (F) and dphase (F) uint64, chan (F, K) uint64, N = B*J, n = b*J + j
    phi(f,k,n) = phase0[f] - chan[f][k] + n * dphase[f]                   (uint64, wraps mod 2^64)
    bin        = ((phi >> 32) * nbin) >> 32
    profile[f][s][k][bin] += float64(power[b][s][k][j][beam[f]]);  hits[f][k][bin] += 1

`fold` adds one call's partial sums (float64, each bin's samples in ascending n) to the prior accumulators, at the
touched elements only.  `tolerance` is the derived bound between two float64 evaluations of the same element.
"""
import numpy as np

MASK = (1 << 64) - 1


def u64(values):
    """Python ints (mod 2^64) as a uint64 array."""
    return np.array([int(v) & MASK for v in np.asarray(values, object).ravel()], np.uint64).reshape(np.shape(values))


def bins(phase0, dphase, chan, N, nbin):
    """The bin of every (f, k, n): int64 (F, K, N), in NumPy's wrapping uint64 arithmetic."""
    phase0, dphase, chan = (np.asarray(a, np.uint64) for a in (phase0, dphase, chan))
    F, K = chan.shape
    assert phase0.shape == (F,) and dphase.shape == (F,) and 1 <= nbin <= 4096
    with np.errstate(over="ignore"):
        n = np.arange(N, dtype=np.uint64)[None, None, :]
        phi = (phase0[:, None, None] - chan[:, :, None]) + n * dphase[:, None, None]
    return (((phi >> np.uint64(32)) * np.uint64(nbin)) >> np.uint64(32)).astype(np.int64)


def samples(power, beam):
    """x[f][s][k][n] = power[b][s][k][j][beam[f]]: f32 (F, S, K, N)."""
    power = np.asarray(power)
    B, S, K, J, M = power.shape
    assert power.dtype == np.float32
    return power.transpose(1, 2, 0, 3, 4).reshape(S, K, B * J, M)[..., np.asarray(beam, np.int64)].transpose(3, 0, 1, 2)


def partials(power, beam, phase0, dphase, chan, nbin):
    """One call's own sums: (partial f64 (F, S, K, nbin), abs f64 likewise: the sums of |x|, count int64 (F, K, nbin))."""
    x = samples(power, beam).astype(np.float64)
    F, S, K, N = x.shape
    b = bins(phase0, dphase, chan, N, nbin)
    flat = ((np.arange(F)[:, None, None] * K + np.arange(K)[None, :, None]) * nbin + b).ravel()
    size = F * K * nbin
    count = np.bincount(flat, minlength=size).reshape(F, K, nbin)
    partial, absx = np.empty((F, S, K, nbin)), np.empty((F, S, K, nbin))
    for s in range(S):  # bincount adds the weights of a bin in the order of the input: ascending n
        partial[:, s] = np.bincount(flat, weights=x[:, s].ravel(), minlength=size).reshape(F, K, nbin)
        absx[:, s] = np.bincount(flat, weights=np.abs(x[:, s]).ravel(), minlength=size).reshape(F, K, nbin)
    return partial, absx, count


def fold(power, beam, phase0, dphase, chan, nbin, profile, hits):
    """One call on copies of the accumulators: (profile, hits, partial, abs, count).  Elements with count 0 keep the
    prior's bits."""
    profile, hits = np.array(profile, np.float64), np.array(hits, np.uint32)
    partial, absx, count = partials(power, beam, phase0, dphase, chan, nbin)
    assert profile.shape == partial.shape and hits.shape == count.shape
    touched = np.broadcast_to((count > 0)[:, None], profile.shape)
    profile[touched] = profile[touched] + partial[touched]
    hits[count > 0] = (hits[count > 0].astype(np.int64) + count[count > 0]).astype(np.uint32)  # mod 2^32
    return profile, hits, partial, absx, count


def tolerance(pre, absx, count):
    """Bound on |got - ref| per element of profile for general f32 power.  An element takes t = count additions; a
    float64 evaluation in any order errs by at most t * 2^-53 * (|pre| + sum|x|); the kernel and this reference each stay
    within that: t * 2^-52 * (|pre| + sum|x|)."""
    return np.asarray(count, np.float64)[:, None] * 2.0 ** -52 * (np.abs(np.asarray(pre, np.float64)) + absx)
