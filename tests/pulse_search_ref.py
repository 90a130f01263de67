"""NumPy restatement of the pulse-search contract (include/bf.h, bf_pulse_search):

    series (M, D, N) f32, ring (M, D, R) f32, moments (M, D, P, 2) f64, widths (L) ascending, Wmax = widths[-1]
    1. ring[m][d][(head + n) % R] = series[m][d][n]                                           (bits copied)
    2. moments[m][d][slot] = (sum_n x, sum_n x*x), float64 sums of the f32 values
       S1, S2 = the sums over all P slots; cnt = n_blocks * N
    3. s_w[n] = sum_{i<w} ring[m][d][(head + n - i) mod R]                                    (float64)
       num = cnt * s_w[n] - w * S1;  den = w * (cnt * S2 - S1 * S1)
       snr_w[n] = den > 0 ? float32(num / sqrt(den)) : 0
    4. per sample the largest snr_w[n], ties to the smallest width index, from (-inf, index 0), strict comparisons
    5. peaks[m][d] = {bits of the row's best snr, its n, its width index, count of n with snr >= threshold}:
       larger snr, then smaller width index, then smaller n, from (-inf, n 0, index 0)
    6. best[m] = {bits of the beam's best peak snr, its d, n, width index}, ties to the smaller d

The boxcar sums are differences of NumPy's float64 cumulative sum over the row's window (the Wmax - 1 samples before
the block and the block); the moments are NumPy's float64 sums.

`tolerance` is a derived bound on |got - ref| of snr_w for general f32 input, between two float64 evaluations that
sum in different orders (the kernel and this file, or this file and a direct summation).  With u = 2^-53:
  * a float64 sum of t terms, in any order, errs by at most t * u * sum|x|.  A boxcar sum taken as the difference of
    two prefix sums of a window of t_s = N + Wmax - 1 samples errs by at most ds = 2 * t_s * u * A, A = the window's
    sum|x| (a direct sum of w terms is inside that).
  * the current block's moments err by at most N * u * (sum|x|, sum x^2) of the block; the other slots are the same
    stored bits for both evaluations; the sum over the P slots errs by at most P * u * (sum_p |m1_p|, sum_p m2_p):
    dS1 = u * (N * a1 + P * sum_p |m1_p|), dS2 = u * (N * m2 + P * sum_p m2_p), a1 = the block's sum|x|.
  * the arithmetic of num and den rounds each product and each difference once (or less, where a multiply-add is
    fused): dnum = cnt * ds + w * dS1 + 3u * (|cnt * s_w| + |w * S1|),
            dden = w * (cnt * dS2 + 2 |S1| dS1) + 3u * w * (cnt * S2 + S1^2).
  * to first order d(num / sqrt(den)) = dnum / sqrt(den) + |snr| * dden / (2 den), plus 2u * |snr| for the sqrt and
    the division.
Each of the two evaluations stays within that of the exact value, and the float32 rounding adds half an ulp to each:
    tol = 2^-23 * |ref| + 2 * (dnum / sqrt(den) + |ref| * dden / (2 den) + 2u * |ref|),   0 where den > 0 is false.
"""
import types

import numpy as np

U = 2.0 ** -53


def check(series, ring, moments, head, slot, n_blocks, widths):
    series, ring, moments = np.asarray(series), np.asarray(ring), np.asarray(moments)
    M, D, N = series.shape
    R, P = ring.shape[2], moments.shape[2]
    w = np.asarray(widths, np.int64)
    assert series.dtype == np.float32 and ring.dtype == np.float32 and moments.dtype == np.float64
    assert ring.shape == (M, D, R) and moments.shape == (M, D, P, 2)
    assert 1 <= w.size <= 16 and w[0] >= 1 and w[-1] <= 1024 and (np.diff(w) > 0).all()
    assert R % N == 0 and R >= N + w[-1] - 1 and 0 <= head < R and head % N == 0
    assert 1 <= P <= 64 and 0 <= slot < P and 1 <= n_blocks <= P
    return M, D, N, R, P, w


def append(series, ring, head):
    """Step 1 on a copy of `ring`."""
    new = np.array(ring, np.float32)
    new[:, :, head:head + series.shape[2]] = series
    return new


def block_moments(series, moments, slot):
    """Step 2 on a copy of `moments`."""
    x = np.asarray(series).astype(np.float64)
    new = np.array(moments, np.float64)
    new[:, :, slot, 0] = x.sum(axis=2)
    new[:, :, slot, 1] = (x * x).sum(axis=2)
    return new


def window(ring, head, N, Wmax):
    """The row's window after step 1, (M, D, N + Wmax - 1) f32: the Wmax - 1 samples before the block, then it."""
    R = ring.shape[2]
    return ring[:, :, (head - (Wmax - 1) + np.arange(N + Wmax - 1)) % R]


def boxcar_sums(win, widths, N):
    """s_w[n] (M, D, L, N) float64 as prefix differences."""
    Wmax = int(widths[-1])
    E = np.concatenate([np.zeros(win.shape[:2] + (1,)), np.cumsum(win.astype(np.float64), axis=2)], axis=2)
    top = Wmax + np.arange(N)
    return np.stack([E[:, :, top] - E[:, :, top - int(w)] for w in widths], axis=2)


def snr_of(s, S1, S2, cnt, widths):
    """Step 3 from the boxcar sums and the baseline: (snr_w (M, D, L, N) f32, num, den)."""
    w = np.asarray(widths, np.float64)[None, None, :]
    num = float(cnt) * s - (w * S1[:, :, None])[..., None]
    den = w * (float(cnt) * S2 - S1 * S1)[:, :, None]
    with np.errstate(invalid="ignore", divide="ignore", over="ignore"):
        ok = den > 0
        q = num / np.sqrt(np.where(ok, den, 1.0))[..., None]
        snr = np.where(ok[..., None], q.astype(np.float32), np.float32(0))
    return snr.astype(np.float32), num, den


def best_width(snr_w):
    """Step 4: (snr (M, D, N) f32, width_index (M, D, N) uint8)."""
    M, D, L, N = snr_w.shape
    best = np.full((M, D, N), -np.inf, np.float32)
    index = np.zeros((M, D, N), np.uint8)
    for i in range(L):
        with np.errstate(invalid="ignore"):
            better = snr_w[:, :, i] > best
        best = np.where(better, snr_w[:, :, i], best)
        index = np.where(better, np.uint8(i), index)
    return best, index


def peak_records(snr, index, threshold):
    """Step 5: int32 (M, D, 4).  `snr` holds no NaN (step 4 starts from -inf and compares strictly)."""
    M, D, N = snr.shape
    top = snr.max(axis=2)
    at_top = snr == top[..., None]
    idx = np.where(at_top, index, 255).min(axis=2)
    n = np.argmax(at_top & (index == idx[..., None]), axis=2)
    only_inf = np.isneginf(top)  # nothing beat the start (-inf, n 0, index 0)
    out = np.zeros((M, D, 4), np.int32)
    out[..., 0] = top.astype(np.float32).view(np.int32)
    out[..., 1] = np.where(only_inf, 0, n)
    out[..., 2] = np.where(only_inf, 0, idx)
    out[..., 3] = (snr >= np.float32(threshold)).sum(axis=2)
    return out


def best_records(peaks):
    """Step 6: int32 (M, 4)."""
    M = peaks.shape[0]
    s = np.ascontiguousarray(peaks[..., 0]).view(np.float32)
    d = np.argmax(s, axis=1)  # the first of equal maxima: the smaller d
    out = np.zeros((M, 4), np.int32)
    rows = np.arange(M)
    top = s[rows, d]
    only_inf = np.isneginf(top)
    out[:, 0] = top.view(np.int32)
    out[:, 1] = np.where(only_inf, 0, d)
    out[:, 2] = np.where(only_inf, 0, peaks[rows, d, 1])
    out[:, 3] = np.where(only_inf, 0, peaks[rows, d, 2])
    return out


def pulse_search(series, ring, moments, head, slot, n_blocks, widths, threshold):
    """One call.  A namespace: ring, moments (after the call), snr_w (M, D, L, N), snr, width_index, peaks, best, and
    what `tolerance` and the exactness checks need: s, num, den, S1, S2, cnt, win."""
    M, D, N, R, P, w = check(series, ring, moments, head, slot, n_blocks, widths)
    series = np.asarray(series)
    new_ring = append(series, ring, head)
    new_mom = block_moments(series, moments, slot)
    S1, S2 = new_mom[..., 0].sum(axis=2), new_mom[..., 1].sum(axis=2)
    cnt = n_blocks * N
    win = window(new_ring, head, N, int(w[-1]))
    s = boxcar_sums(win, w, N)
    snr_w, num, den = snr_of(s, S1, S2, cnt, w)
    snr, index = best_width(snr_w)
    peaks = peak_records(snr, index, threshold)
    return types.SimpleNamespace(ring=new_ring, moments=new_mom, snr_w=snr_w, snr=snr, width_index=index, peaks=peaks,
                                 best=best_records(peaks), s=s, num=num, den=den, S1=S1, S2=S2, cnt=cnt, win=win,
                                 widths=w, series=series)


def one_shot(stream, N, P, widths, threshold):
    """The whole stream (M, D, calls * N) at once, zero before its first sample, the baseline of call c the blocks
    max(0, c - P + 1) .. c: a list of per-call namespaces (snr_w, snr, width_index, peaks, best).  Boxcar sums and
    block sums come from the stream itself, no ring and no slots."""
    stream = np.asarray(stream, np.float32)
    M, D, Nt = stream.shape
    w = np.asarray(widths, np.int64)
    Wmax, calls = int(w[-1]), Nt // N
    assert Nt == calls * N
    x = stream.astype(np.float64)
    E = np.concatenate([np.zeros((M, D, Wmax)), np.cumsum(x, axis=2)], axis=2)   # E[Wmax + t] = sum of x[0 .. t]
    b1 = x.reshape(M, D, calls, N).sum(axis=3)
    b2 = (x * x).reshape(M, D, calls, N).sum(axis=3)
    out = []
    for c in range(calls):
        lo = max(0, c - P + 1)
        S1, S2 = b1[:, :, lo:c + 1].sum(axis=2), b2[:, :, lo:c + 1].sum(axis=2)
        top = Wmax + c * N + np.arange(N)
        s = np.stack([E[:, :, top] - E[:, :, top - int(wi)] for wi in w], axis=2)
        snr_w, _, _ = snr_of(s, S1, S2, (c + 1 - lo) * N, w)
        snr, index = best_width(snr_w)
        peaks = peak_records(snr, index, threshold)
        out.append(types.SimpleNamespace(snr_w=snr_w, snr=snr, width_index=index, peaks=peaks,
                                         best=best_records(peaks)))
    return out


def tolerance(ref, slot):
    """Bound on |got - ref.snr_w| per element, (M, D, L, N) float64 (module docstring); `ref` is what pulse_search
    returned."""
    N = ref.series.shape[2]
    P = ref.moments.shape[2]
    w = ref.widths.astype(np.float64)[None, None, :, None]
    x = ref.series.astype(np.float64)
    A = np.abs(ref.win.astype(np.float64)).sum(axis=2)[:, :, None, None]
    ds = 2.0 * ref.win.shape[2] * U * A
    dS1 = U * (N * np.abs(x).sum(axis=2) + P * np.abs(ref.moments[..., 0]).sum(axis=2))[:, :, None, None]
    dS2 = U * (N * (x * x).sum(axis=2) + P * np.abs(ref.moments[..., 1]).sum(axis=2))[:, :, None, None]
    S1, S2 = ref.S1[:, :, None, None], ref.S2[:, :, None, None]
    cnt = float(ref.cnt)
    dnum = cnt * ds + w * dS1 + 3 * U * (np.abs(cnt * ref.s) + np.abs(w * S1))
    dden = w * (cnt * dS2 + 2 * np.abs(S1) * dS1) + 3 * U * w * (cnt * np.abs(S2) + S1 * S1)
    den = ref.den[..., None]
    r = np.abs(ref.snr_w.astype(np.float64))
    with np.errstate(invalid="ignore", divide="ignore"):
        tol = 2.0 ** -23 * r + 2 * (dnum / np.sqrt(den) + r * dden / (2 * den) + 2 * U * r)
    return np.where(den > 0, tol, 0.0)
