"""NumPy restatement of the beam-detector contract (include/bf.h, bf_beam_detect):

    beams (B, 2, C, T/16, 16, 2M), the last axis (re, im) per beam; X = pol 0, Y = pol 1 of (b, c, t, m)
    I = Xr^2+Xi^2+Yr^2+Yi^2   Q = Xr^2+Xi^2-Yr^2-Yi^2   U = 2(XrYr+XiYi)   V = 2(XiYr-XrYi)
    acc[b][s][k][j][m] = sum over c in [k*fint, (k+1)*fint), t in [j*tint, (j+1)*tint) of the term s
    out                = float32(float64(acc) * float64(float32(scale)))

int8 beams: terms and sums in int64 (exact; |acc| < 2^53 for every accepted shape, so the float64 conversion is exact
and the output has one rounding).  f32 beams: terms and sums in float64 (the products of two f32 values are exact in
float64; the sums are NumPy's, in its order).  `tolerance` is the derived bound between two such float64 evaluations.
"""
import numpy as np

STOKES = "IQUV"


def stokes_sums(beams, tint, fint, iquv=True):
    """acc of a (B, 2, C, T/16, 16, 2M) int8 or float32 cube: (B, 4 or 1, C/fint, T/tint, M), int64 or float64."""
    beams = np.asarray(beams)
    B, P, C, nb, sb, M2 = beams.shape
    assert P == 2 and sb == 16 and M2 % 2 == 0 and beams.dtype in (np.int8, np.float32)
    T, M = nb * 16, M2 // 2
    assert T % tint == 0 and C % fint == 0
    wide = np.int64 if beams.dtype == np.int8 else np.float64
    v = beams.reshape(B, 2, C, T, M, 2)
    out = np.zeros((B, 4 if iquv else 1, C // fint, T // tint, M), wide)
    for c in range(C):  # channel by channel: no whole-cube wide temporary
        xr, xi = v[:, 0, c, :, :, 0].astype(wide), v[:, 0, c, :, :, 1].astype(wide)
        yr, yi = v[:, 1, c, :, :, 0].astype(wide), v[:, 1, c, :, :, 1].astype(wide)
        px, py = xr * xr + xi * xi, yr * yr + yi * yi
        terms = [px + py, px - py, 2 * (xr * yr + xi * yi), 2 * (xi * yr - xr * yi)] if iquv else [px + py]
        for s, term in enumerate(terms):
            out[:, s, c // fint] += term.reshape(B, T // tint, tint, M).sum(axis=2)
    return out


def scale_sums(S, scale):
    assert float(np.max(np.abs(S), initial=0)) < 2 ** 53
    return (S.astype(np.float64) * np.float64(np.float32(scale))).astype(np.float32)


def beam_detect(beams, tint, fint, iquv=True, scale=1.0):
    return scale_sums(stokes_sums(beams, tint, fint, iquv), scale)


def tolerance(ref_out, ref_sums, tint, fint, scale):
    """Bound on |got - ref_out| for f32 beams, per element.  The terms are exact in float64; a float64 sum of
    N = 4 * tint * fint of them, in any order, errs by at most N * 2^-53 * sum|term|, and sum|term| <= I of the same
    window for every Stokes parameter (2|XrYr| <= Xr^2 + Yr^2); the float32 rounding adds half an ulp.  The kernel and
    this reference each stay within that: 2^-23 * |ref_out| + N * 2^-51 * scale * I_ref.  `ref_sums` is stokes_sums of
    the same cube (its row 0 is I)."""
    n = 4 * tint * fint
    i_ref = np.asarray(ref_sums, np.float64)[:, :1]
    return 2.0 ** -23 * np.abs(np.asarray(ref_out, np.float64)) + n * 2.0 ** -51 * float(np.float32(scale)) * i_ref
