"""NumPy restatement of the correlator's contract (include/bf.h, bf_correlate):

    x[a, p] = re + i*im of one sample; for the window b in [k*bint, (k+1)*bint), t in [j*tint, (j+1)*tint):
    S[k][c][j][bl(a1, a2)][p1][p2] = sum over the window of x[a1, p1] * conj(x[a2, p2])
        re = sum r1*r2 + i1*i2        im = sum i1*r2 - r1*i2                             (exact, int64, then int32)
    bl(a1, a2) = a1 (a1 + 1) / 2 + a2 for a1 >= a2, autos included.

The output has shape (B // bint, C, T // tint, A (A + 1) / 2, 2, 2, 2), the last axes (p1, p2, (re, im)).  One int64
einsum per (k, c) over the window's samples; the cast to int32 follows an assertion that every sum fits.
"""
import numpy as np


def n_baselines(A):
    return A * (A + 1) // 2


def full_sums(raw, tint, bint, signed):
    """Exact int64 (re, im), each (K, C, J, A, 2, A, 2) = [k, c, j, a1, p1, a2, p2], of a (B, A, C, T, 2, 2) 8-bit
    cube: every antenna pair in both orders."""
    raw = np.asarray(raw)
    B, A, C, T = raw.shape[:4]
    assert raw.shape[4:] == (2, 2) and raw.dtype.itemsize == 1 and T % tint == 0 and B % bint == 0
    assert bint == 1 or tint == T
    K, J = B // bint, T // tint
    x = raw.view(np.int8 if signed else np.uint8).reshape(K, bint, A, C, J, tint, 2, 2)
    re = np.empty((K, C, J, A, 2, A, 2), np.int64)
    im = np.empty_like(re)
    for k in range(K):
        for c in range(C):  # channel by channel: no whole-cube int64 temporary
            for j in range(J):
                v = x[k, :, :, c, j].astype(np.int64)                            # (bint, A, tint, p, z)
                v = v.transpose(1, 3, 0, 2, 4).reshape(2 * A, bint * tint, 2)    # rows (a, p), the window's samples
                r, i = v[..., 0], v[..., 1]
                m = np.concatenate([r, i], axis=1)                               # x . conj(y) = (r r' + i i')
                n = np.concatenate([i, -r], axis=1)                              #             + i (i r' - r i')
                re[k, c, j] = np.einsum("xn,yn->xy", m, m).reshape(A, 2, A, 2)
                im[k, c, j] = np.einsum("xn,yn->xy", n, m).reshape(A, 2, A, 2)
    return re, im


def visibilities(raw, tint, bint, signed):
    """The contract's int32 output (K, C, J, NBL, 2, 2, 2)."""
    re, im = full_sums(raw, tint, bint, signed)
    assert max(abs(int(re.min())), int(re.max()), abs(int(im.min())), int(im.max())) < 2 ** 31
    A = re.shape[3]
    a1, a2 = np.tril_indices(A)  # row-major lower triangle: position a1 (a1 + 1) / 2 + a2
    out = np.empty(re.shape[:3] + (n_baselines(A), 2, 2, 2), np.int32)
    out[..., 0] = re[:, :, :, a1, :, a2, :].transpose(1, 2, 3, 0, 4, 5)  # the advanced axes come first
    out[..., 1] = im[:, :, :, a1, :, a2, :].transpose(1, 2, 3, 0, 4, 5)
    return out


def accumulate(cubes, tint, bint, signed):
    """The contract's output after one plain call and accumulating calls over the further cubes: the int64 sum of
    their visibilities, asserted to fit, as int32."""
    total = sum(visibilities(raw, tint, bint, signed).astype(np.int64) for raw in cubes)
    assert int(np.abs(total).max()) < 2 ** 31
    return total.astype(np.int32)


# ---- shared test inputs (built once per process, never modified) -----------------------------------------------------
_cache = {}


def random_voltages(shape):
    """Uniformly random full-range bytes (B, A, C, T, 2, 2), one cube per shape (read as uint8 or int8)."""
    if shape not in _cache:
        raw = np.random.default_rng(sum(shape) + 7).integers(0, 256, tuple(shape) + (2, 2), dtype=np.uint8)
        raw.setflags(write=False)
        _cache[shape] = raw
    return _cache[shape]


def reference(shape, tint, bint, signed):
    """visibilities(random_voltages(shape), ...), computed once per process."""
    key = (shape, tint, bint, signed)
    if key not in _cache:
        out = visibilities(random_voltages(shape), tint, bint, signed)
        out.setflags(write=False)
        _cache[key] = out
    return _cache[key]
