"""GPU: the pulse search (bf_pulse_search, csrc/bf_pulse_search.hip; beamforming.pulse_search) against the NumPy
restatement of its contract (pulse_search_ref.py): bit for bit on integer-valued series, within the derived bound
(pulse_search_ref.tolerance) on Gaussian series; the ring and the moments after the call bit for bit.

The C entry point takes the ring, `head`, the moments, `slot` and `n_blocks` explicitly, so one call on a randomly
prefilled ring and prefilled moments exercises wrapping: every shape runs at head = 0 (the history wraps to the ring's
end) and at head = R - N, and at (slot, n_blocks) = (0, 1) and (P - 1, P).  At (0, 1) the other slots are zero, as they
are at an operator's first call; at (P - 1, P) every slot holds the moments of a random block.

Shapes are (M, D, N, R, P, widths).  A row belongs to a group of G = 16, 32 or 64 lanes (the smallest that is at least
min(N, 64); wider while the workgroup's prefix arrays would not fit the LDS budget), a workgroup owns 256 / G rows, a
row is walked in tiles of T = min(N rounded up to G, 256) outputs, and a tile's window of T + Wmax - 1 samples is
scanned in chunks of G.  bf_last_kernel reports (G, T), and the grid asserts it.  Beyond the issue's list:
  G = 32, rows not a multiple of 8          (3, 3, 17, 34, 2, [1, 2, 18]): N one above 16; the window is a chunk + 2
  G = 32, a full group                      (1, 8, 32, 64, 2, [1, 32]): exactly one workgroup; the window is 63 = two
                                            chunks less one
  history one below / at / above G          (2, 9, 16, 32|48, 3, [1, 16] | [1, 17] | [1, 18]): the window is 31, 32 and
                                            33 samples: the last chunk of the scan full, or holding one sample
  the LDS budget widens G to 32             (2, 3, 16, 528, 2, [1, 512]): 16 groups of 16 + 512 float64 exceed 48 KiB
  ... and to 64                             (3, 3, 16, 1040, 2, [1, 1024]): N = 16 on whole waves, three quarters of a
                                            group's lanes hold no output
  N one below / at / above the tile         (1, 3, 255|256|257, .., 2, [1, 3, 200]): the second tile holds one output
"""
import functools

import numpy as np
import pytest

import dedisperse_ref
import pulse_search_ref as R
from dpdk_dc_sand_amd import _lib, accel
from dpdk_dc_sand_amd.beamforming import DedisperserTemplate, PulseSearchTemplate, candidates, dispersion_lags

pytestmark = pytest.mark.gpu

SENTINEL = 0x7fc0beef
TAIL = 4096
THRESHOLD = 1.0  # low, so that the counts are neither 0 nor N

POW2 = tuple(1 << i for i in range(8))
SIXTEEN = (1, 2, 3, 4, 6, 8, 12, 16, 24, 32, 48, 64, 80, 96, 112, 128)
# shape -> the (G, T) the launcher must pick
GRID = {
    (1, 1, 1, 1, 1, (1,)): (16, 16),
    (2, 3, 4, 12, 2, (1, 2, 3)): (16, 16),
    (3, 5, 16, 144, 4, POW2): (16, 16),
    (2, 2, 65, 130, 3, (1, 7, 64)): (64, 128),
    (1, 9, 130, 260, 2, (1, 2, 129)): (64, 192),
    (64, 33, 16, 32, 64, (1, 16)): (16, 16),
    (1, 2, 1024, 2048, 1, (1, 1024)): (64, 256),
    (4, 4, 128, 256, 8, SIXTEEN): (64, 128),
    # beyond the issue's list (module docstring)
    (3, 3, 17, 34, 2, (1, 2, 18)): (32, 32),
    (1, 8, 32, 64, 2, (1, 32)): (32, 32),
    (2, 9, 16, 32, 3, (1, 16)): (16, 16),
    (2, 9, 16, 32, 3, (1, 17)): (16, 16),
    (2, 9, 16, 48, 3, (1, 18)): (16, 16),
    (2, 3, 16, 528, 2, (1, 512)): (32, 32),
    (3, 3, 16, 1040, 2, (1, 1024)): (64, 64),
    (1, 3, 255, 510, 2, (1, 3, 200)): (64, 256),
    (1, 3, 256, 512, 2, (1, 3, 200)): (64, 256),
    (1, 3, 257, 514, 2, (1, 3, 200)): (64, 256),
}
SERIES_SHAPE = (4, 4, 128, 256, 8, SIXTEEN)  # PSEARCH_SERIES on and off; every other shape runs with it on


def ident(v):
    if isinstance(v, tuple) and v and isinstance(v[-1], tuple):
        return "x".join(map(str, v[:-1])) + "_w" + (str(len(v[-1])) + "to" + str(v[-1][-1]))
    return None


def bits(a):
    a = np.ascontiguousarray(a)
    return a.view({1: np.uint8, 4: np.uint32, 8: np.uint64}[a.dtype.itemsize])


@functools.lru_cache(maxsize=None)
def inputs(shape, fill, full):
    """(series, prefilled ring, prefilled moments) of a shape, never modified.  fill: "int" (integers below 2^8),
    "gauss" (Gaussian f32 of rms 1000) or "ties" (values in {0, 1}, row (0, 0) constant).  full: every moment slot holds
    a random block's moments (for n_blocks = P), else only slot 0 does (it is overwritten: n_blocks = 1)."""
    M, D, N, Rn, P, widths = shape
    rng = np.random.default_rng(sum(shape[:5]) + len(fill) + full)

    def draw(s):
        if fill == "int":
            return rng.integers(0, 1 << 8, s).astype(np.float32)
        if fill == "ties":
            return rng.integers(0, 2, s).astype(np.float32)
        return (1000 * rng.standard_normal(s)).astype(np.float32)
    series, ring, past = draw((M, D, N)), draw((M, D, Rn)), draw((M, D, P, N)).astype(np.float64)
    if fill == "ties":
        series[0, 0], ring[0, 0], past[0, 0] = 1, 1, 1
    moments = np.stack([past.sum(axis=3), (past * past).sum(axis=3)], axis=3)
    if not full:
        moments[:, :, 1:] = 0
    for a in (series, ring, moments):
        a.setflags(write=False)
    return series, ring, moments


def state(shape, at, base):
    M, D, N, Rn, P, widths = shape
    head = 0 if at == "head0" else Rn - N
    slot, n_blocks = (0, 1) if base == "first" else (P - 1, P)
    return head, slot, n_blocks


@functools.lru_cache(maxsize=None)
def reference(shape, fill, at, base, threshold=THRESHOLD):
    """pulse_search_ref.pulse_search of one call; shared, never modified."""
    head, slot, n_blocks = state(shape, at, base)
    series, ring, moments = inputs(shape, fill, base == "full")
    return R.pulse_search(series, ring, moments, head, slot, n_blocks, shape[5], threshold)


def padded(host, words=None):
    """A host uint32 image: `host`'s bits (or `words` sentinel words), then a tail of sentinels."""
    body = np.full(words, SENTINEL, np.uint32) if host is None else bits(host).view(np.uint32).ravel()
    return np.concatenate([body, np.full(TAIL, SENTINEL, np.uint32)])


def launch(context, queue, series, ring, moments, head, slot, n_blocks, widths, threshold=THRESHOLD, want_series=True):
    """bf_pulse_search on device copies, every buffer with a sentinel tail, every output prefilled with sentinels (the
    kernel assumes no zeroed output).  A dict of what was read back, tails checked and cut."""
    M, D, N = series.shape
    Rn, P = ring.shape[2], moments.shape[2]
    rows = M * D
    host = {"series": padded(series), "ring": padded(ring), "moments": padded(moments),
            "peaks": padded(None, rows * 4), "best": padded(None, M * 4)}
    if want_series:
        host["snr"] = padded(None, rows * N)
        host["width"] = padded(None, (rows * N + 3) // 4)
    dev = {}
    for k, h in host.items():
        dev[k] = accel.DeviceArray(context, h.shape, np.uint32)
        dev[k].set(queue, h)
    w = (_lib.c_int * len(widths))(*widths)
    _lib.call("bf_pulse_search", dev["series"].ptr, dev["ring"].ptr, dev["moments"].ptr, w,
              dev["snr"].ptr if want_series else None, dev["width"].ptr if want_series else None, dev["peaks"].ptr,
              dev["best"].ptr, M, D, N, Rn, head, P, slot, n_blocks, len(widths), threshold,
              _lib.PSEARCH_SERIES if want_series else 0, queue.handle)
    kernel = _lib.load().bf_last_kernel().decode()
    got = {k: dev[k].get(queue) for k in dev}
    for k, g in got.items():
        assert (g[-TAIL:] == SENTINEL).all(), f"{k}: the tail was written"
    out = {"kernel": kernel,
           "series": got["series"][:-TAIL].view(np.float32).reshape(M, D, N),
           "ring": got["ring"][:-TAIL].view(np.float32).reshape(M, D, Rn),
           "moments": got["moments"][:-TAIL].view(np.float64).reshape(M, D, P, 2),
           "peaks": got["peaks"][:-TAIL].view(np.int32).reshape(M, D, 4),
           "best": got["best"][:-TAIL].view(np.int32).reshape(M, 4)}
    if want_series:
        out["snr"] = got["snr"][:-TAIL].view(np.float32).reshape(M, D, N)
        width_bytes = got["width"][:-TAIL].view(np.uint8)
        assert (bits(width_bytes[rows * N:]) == np.frombuffer(np.uint32(SENTINEL).tobytes(), np.uint8)[
            np.arange(rows * N, width_bytes.size) % 4]).all(), "width_index: bytes past the end were written"
        out["width"] = width_bytes[:rows * N].reshape(M, D, N)
    return out


def check_exact(got, ref, series):
    """Every output bit for bit; the ring and the moments after the call; `series` untouched."""
    np.testing.assert_array_equal(bits(got["ring"]), bits(ref.ring))
    np.testing.assert_array_equal(bits(got["moments"]), bits(ref.moments))
    np.testing.assert_array_equal(bits(got["series"]), bits(series))
    if "snr" in got:
        np.testing.assert_array_equal(bits(got["snr"]), bits(ref.snr))
        np.testing.assert_array_equal(got["width"], ref.width_index)
    np.testing.assert_array_equal(got["peaks"], ref.peaks)
    np.testing.assert_array_equal(got["best"], ref.best)


def check_close(got, ref, slot, threshold=THRESHOLD):
    """Gaussian fill: the series within tolerance; the peak S/N within tolerance of the reference's maximum; the
    reference's S/N at the kernel's chosen (n, index) within tolerance of that maximum; the count between the
    reference's counts at threshold +- tolerance; best consistent with the kernel's own peaks.  A sample's tolerance is
    the largest of its widths' (the maximum of L values moves by at most the largest of their errors); comparing the
    reference at the kernel's choice with the reference's own maximum spends the bound twice (once from the kernel's
    value at its choice to the reference there, once from the kernel's maximum to the reference's)."""
    tol_w = R.tolerance(ref, slot)                      # (M, D, L, N)
    tol = tol_w.max(axis=2)                             # (M, D, N)
    M, D, N = ref.snr.shape
    ref64 = ref.snr.astype(np.float64)
    np.testing.assert_array_equal(bits(got["ring"]), bits(ref.ring))
    mom_tol = 2.0 ** -52 * N * np.stack([np.abs(ref.series.astype(np.float64)).sum(axis=2),
                                               (ref.series.astype(np.float64) ** 2).sum(axis=2)], axis=2)
    assert (np.abs(got["moments"][:, :, slot] - ref.moments[:, :, slot]) <= mom_tol).all()
    other = [p for p in range(ref.moments.shape[2]) if p != slot]
    np.testing.assert_array_equal(bits(got["moments"][:, :, other]), bits(ref.moments[:, :, other]))
    mi, di = np.meshgrid(np.arange(M), np.arange(D), indexing="ij")
    if "snr" in got:
        err = np.abs(got["snr"].astype(np.float64) - ref64)
        assert np.isfinite(got["snr"]).all() and (err <= tol).all(), (float((err / tol).max()), int((err > tol).sum()))
        # the chosen width: the reference's S/N at it is the reference's best to within twice the bound
        assert (got["width"] < ref.snr_w.shape[2]).all()
        at = np.take_along_axis(ref.snr_w, got["width"][:, :, None, :].astype(np.int64), axis=2)[:, :, 0]
        assert (ref64 - at.astype(np.float64) <= 2 * tol).all()
    peak = got["peaks"][..., 0].copy().view(np.float32).astype(np.float64)
    n, idx, count = got["peaks"][..., 1], got["peaks"][..., 2], got["peaks"][..., 3]
    assert (0 <= n).all() and (n < N).all() and (0 <= idx).all() and (idx < ref.snr_w.shape[2]).all()
    ref_top = ref64.max(axis=2)
    top_tol = tol[mi, di, ref64.argmax(axis=2)]
    assert (np.abs(peak - ref_top) <= np.maximum(top_tol, tol[mi, di, n])).all()
    ref_at = ref.snr_w[mi, di, idx, n].astype(np.float64)
    assert (ref_top - ref_at <= top_tol + tol_w[mi, di, idx, n]).all() and (ref_at <= ref_top).all()
    lo = (ref64 - tol >= threshold).sum(axis=2)
    hi = (ref64 + tol >= threshold).sum(axis=2)
    assert (lo <= count).all() and (count <= hi).all()
    np.testing.assert_array_equal(got["best"], R.best_records(got["peaks"]))


@pytest.mark.parametrize("shape", list(GRID), ids=ident)
@pytest.mark.parametrize("fill", ["int", "gauss"])
@pytest.mark.parametrize("at", ["head0", "headlast"])
@pytest.mark.parametrize("base", ["first", "full"])
def test_shape_grid(context, command_queue, shape, fill, at, base):
    M, D, N, Rn, P, widths = shape
    head, slot, n_blocks = state(shape, at, base)
    series, ring, moments = inputs(shape, fill, base == "full")
    ref = reference(shape, fill, at, base)
    if fill == "int":  # the contract's condition for bit-exactness, asserted on the CPU
        assert np.abs(ref.num).max() < 2 ** 53 and ref.den.max() < 2 ** 53
        assert N == 1 or (ref.den > 0).all()
    got = launch(context, command_queue, series, ring, moments, head, slot, n_blocks, widths)
    assert got["kernel"] == "pulse_search_kernel:g%d,t%d" % GRID[shape]
    if fill == "int":
        check_exact(got, ref, series)
    else:
        np.testing.assert_array_equal(bits(got["series"]), bits(series))
        check_close(got, ref, slot)


@pytest.mark.parametrize("fill", ["int", "gauss"])
def test_without_the_series_outputs(context, command_queue, fill):
    """(4, 4, 128, 256, 8, sixteen widths) without PSEARCH_SERIES: peaks and best as with it, and nothing else is
    written (snr and width_index are NULL; the ring and the moments change only where the contract says)."""
    shape = SERIES_SHAPE
    head, slot, n_blocks = state(shape, "headlast", "full")
    series, ring, moments = inputs(shape, fill, True)
    ref = reference(shape, fill, "headlast", "full")
    got = launch(context, command_queue, series, ring, moments, head, slot, n_blocks, shape[5], want_series=False)
    assert "snr" not in got
    if fill == "int":
        check_exact(got, ref, series)
    else:
        check_close(got, ref, slot)
    with_series = launch(context, command_queue, series, ring, moments, head, slot, n_blocks, shape[5])
    np.testing.assert_array_equal(got["peaks"], with_series["peaks"])
    np.testing.assert_array_equal(got["best"], with_series["best"])


@pytest.mark.parametrize("threshold", [0.0, 1.5])
def test_ties(context, command_queue, threshold):
    """Values in {0, 1} at (2, 4, 16, 32, 2, [1, 2, 4]), row (0, 0) constant (den = 0): bit for bit, the constant row's
    record (0.0, n 0, index 0, count N or 0), and the fill really has rows whose best S/N sits at several samples."""
    shape = (2, 4, 16, 32, 2, (1, 2, 4))
    series, ring, moments = inputs(shape, "ties", True)
    ref = R.pulse_search(series, ring, moments, 16, 1, 2, shape[5], threshold)
    assert (ref.den[0, 0] == 0).all() and ref.peaks[0, 0].tolist() == [0, 0, 0, 16 if threshold <= 0 else 0]
    assert ((ref.snr == ref.snr.max(axis=2, keepdims=True)).sum(axis=2) > 1).sum() >= 4
    got = launch(context, command_queue, series, ring, moments, 16, 1, 2, shape[5], threshold=threshold)
    check_exact(got, ref, series)


@pytest.mark.parametrize("shape", [(2, 3, 4, 12, 2, (1, 2, 3)), (3, 5, 16, 144, 4, POW2),
                                   (2, 2, 65, 130, 3, (1, 7, 64)), (1, 3, 257, 514, 2, (1, 3, 200))], ids=ident)
def test_writes_stay_in_bounds(context, command_queue, shape):
    """Every buffer with a 4096-word tail of 0x7fc0beef and every output prefilled with it (launch() checks the tails of
    all of them, the inputs' too): ring slots outside [head, head + N) are unchanged, moment slots other than `slot`
    are unchanged, `series` is unchanged, every output element was written (no sentinel is left), at a head in the
    middle of the ring."""
    M, D, N, Rn, P, widths = shape
    head, slot, n_blocks = N * ((Rn // N) // 2), P // 2, P
    series, ring, moments = inputs(shape, "int", True)
    ref = R.pulse_search(series, ring, moments, head, slot, n_blocks, widths, THRESHOLD)
    got = launch(context, command_queue, series, ring, moments, head, slot, n_blocks, widths)
    check_exact(got, ref, series)
    outside = np.ones(Rn, bool)
    outside[head:head + N] = False
    np.testing.assert_array_equal(bits(got["ring"][:, :, outside]), bits(ring[:, :, outside]))
    other = [p for p in range(P) if p != slot]
    np.testing.assert_array_equal(bits(got["moments"][:, :, other]), bits(moments[:, :, other]))
    assert not (bits(got["snr"]) == SENTINEL).any() and not (bits(got["peaks"]) == SENTINEL).any()


def test_nan_row(context, command_queue):
    """One NaN in row (1, 2) of (3, 5, 16, 144, 4, widths to 128): that row's S/N is 0 and its record (0.0, 0, 0, 0);
    every other row's outputs are bit-equal to the run without the NaN."""
    shape = (3, 5, 16, 144, 4, POW2)
    M, D, N, Rn, P, widths = shape
    head, slot, n_blocks = state(shape, "head0", "full")
    series, ring, moments = inputs(shape, "int", True)
    clean = launch(context, command_queue, series, ring, moments, head, slot, n_blocks, widths)
    dirty = series.copy()
    dirty[1, 2, 5] = np.nan
    got = launch(context, command_queue, dirty, ring, moments, head, slot, n_blocks, widths)
    ref = R.pulse_search(dirty, ring, moments, head, slot, n_blocks, widths, THRESHOLD)
    assert got["peaks"][1, 2].tolist() == [0, 0, 0, 0] and not got["snr"][1, 2].any() and not got["width"][1, 2].any()
    assert np.isnan(got["moments"][1, 2, slot]).all() and np.isnan(got["ring"][1, 2, head + 5])
    rows = np.ones((M, D), bool)
    rows[1, 2] = False
    for k in ("snr", "width", "peaks", "ring", "moments"):
        np.testing.assert_array_equal(bits(got[k][rows]), bits(clean[k][rows]))
    np.testing.assert_array_equal(got["peaks"], ref.peaks)
    np.testing.assert_array_equal(got["best"], ref.best)
    np.testing.assert_array_equal(bits(got["snr"]), bits(ref.snr))
    assert (got["best"][[0, 2]] == clean["best"][[0, 2]]).all()


def test_operator_over_calls(context, command_queue):
    """PulseSearch called 9 times at (2, 3, 8, 32, 4, [1, 2, 16]) with series=True: the ring wraps twice and the slots
    wrap twice; the concatenated series outputs and every call's records equal the one-shot reference of the
    concatenated input; head, slot, n_blocks and samples_seen advance as documented; after reset() a second run
    reproduces the first run's bytes."""
    M, D, N, Rn, P, calls = 2, 3, 8, 32, 4, 9
    widths = (1, 2, 16)
    rng = np.random.default_rng(12)
    stream = rng.integers(0, 1 << 8, (M, D, calls * N)).astype(np.float32)
    tmpl = PulseSearchTemplate(context, M, D, N, widths=widths, baseline_blocks=P, threshold=THRESHOLD, ring_length=Rn,
                               series=True)
    op = tmpl.instantiate(command_queue)
    op.ensure_all_bound()
    runs = []
    for _ in range(2):
        outs = []
        for c in range(calls):
            assert (op.head, op.slot, op.n_blocks, op.samples_seen) == (c * N % Rn, c % P, min(c, P), c * N)
            op.buffer("inSeries").set(command_queue, np.ascontiguousarray(stream[:, :, c * N:(c + 1) * N]))
            op()
            outs.append({k: op.buffer(k).get(command_queue) for k in ("outSnr", "outWidth", "outPeaks", "outBest")})
        runs.append(outs)
        assert op.samples_seen == calls * N > 2 * Rn and op.n_blocks == P and calls > 2 * P
        op.reset()
        assert (op.head, op.slot, op.n_blocks, op.samples_seen) == (0, 0, 0, 0)
    one = R.one_shot(stream, N, P, widths, THRESHOLD)
    for c in range(calls):
        np.testing.assert_array_equal(bits(runs[0][c]["outSnr"]), bits(one[c].snr))
        np.testing.assert_array_equal(runs[0][c]["outWidth"], one[c].width_index)
        np.testing.assert_array_equal(runs[0][c]["outPeaks"], one[c].peaks)
        np.testing.assert_array_equal(runs[0][c]["outBest"], one[c].best)
        for k in runs[0][c]:
            assert runs[0][c][k].tobytes() == runs[1][c][k].tobytes()
    assert np.concatenate([o["outSnr"] for o in runs[0]], axis=2).any()


def test_it_finds_the_pulse(context, command_queue):
    """Dedisperser -> PulseSearch bound on one queue (the slot bound, not copied) at K = 32 channels over 856-1712 MHz,
    M = 4 beams, N = 16 samples per call, 8 trials (DM 0, 0.5, ..., 3.5 at 76.6 us samples; latency 192 samples), widths
    (1, 2, 4, 8, 16), a baseline of 8 blocks.  The input is integer noise power (uniform in [0, 16) per channel), plus a
    dispersed pulse of width 4 and amplitude 8 per channel in beam 2 at trial 5, emitted at stream position 230: it
    ends at output sample 230 + 192 + 3 = 425, which is n = 9 of call 26.  Against the noise alone (sigma =
    sqrt(32 * 21.25) = 26) its boxcar S/N would be 4 * 32 * 8 / (2 * 26), near 20; the baseline of 128 samples includes
    the pulse itself, and the reference gives 9.6.  Every call's records equal the reference chain (dedisperse_ref,
    then pulse_search_ref) bit for bit; in call 26 outBest of beam 2 names trial 5, width index 2 and n = 9 -- asserted
    on the reference alone first -- and candidates() at the template's threshold returns that record for beam 2 and
    none for the other beams."""
    K, M, J, D, calls, P = 32, 4, 16, 8, 28, 8
    N, widths = J, (1, 2, 4, 8, 16)
    beam, trial, t0, width, amp = 2, 5, 230, 4, 8
    freqs = 856e6 + 856e6 * np.arange(K) / K
    lags, latency = dispersion_lags(0.5 * np.arange(D), freqs, 76.6e-6)
    assert latency == 192
    delay = latency - lags
    rng = np.random.default_rng(13)
    stream = rng.integers(0, 16, (K, calls * N, M)).astype(np.float32)
    for k in range(K):
        stream[k, t0 + delay[trial, k]:t0 + delay[trial, k] + width, beam] += amp
    power = stream.reshape(K, calls, 1, J, M).transpose(1, 2, 0, 3, 4)[:, :, None]    # (calls, B 1, S 1, K, J, M)
    power = np.ascontiguousarray(power)
    end = t0 + latency + width - 1
    hit, n_hit = end // N, end % N
    assert (hit, n_hit) == (26, 9) and hit < calls

    ded_t = DedisperserTemplate(context, 1, K, J, M, lags)
    ps_t = PulseSearchTemplate(context, M, D, N, widths=widths, baseline_blocks=P)
    assert ps_t.input_shape == ded_t.output_shape and ps_t.threshold == 6.0 and ps_t.ring_length == 32
    # the reference chain, and what it alone says about the pulse
    ring_d, head_d = np.zeros(ded_t.ring_shape, np.float32), 0
    ring_p, mom, head, slot, n_blocks = np.zeros(ps_t.ring_shape, np.float32), np.zeros(ps_t.moments_shape), 0, 0, 0
    refs = []
    for c in range(calls):
        series, ring_d = dedisperse_ref.dedisperse(power[c], ring_d, lags, head_d)
        head_d = (head_d + N) % ded_t.ring_length
        n_blocks = min(n_blocks + 1, P)
        r = R.pulse_search(series, ring_p, mom, head, slot, n_blocks, widths, ps_t.threshold)
        assert np.abs(r.num).max() < 2 ** 53 and r.den.max() < 2 ** 53
        ring_p, mom, head, slot = r.ring, r.moments, (head + N) % ps_t.ring_length, (slot + 1) % P
        refs.append(r)
    want = refs[hit].best[beam]
    assert want[1:].tolist() == [trial, n_hit, widths.index(width)]
    assert want[:1].view(np.float32)[0] > 8.0
    ref_cands = candidates(refs[hit].peaks, ps_t.threshold, hit * N)
    assert set(ref_cands["beam"]) == {beam} and trial in ref_cands["trial"]

    ded = ded_t.instantiate(command_queue)
    ps = ps_t.instantiate(command_queue)
    ded.ensure_all_bound()
    ps.bind(inSeries=ded.buffer("outData"))
    ps.ensure_all_bound()
    assert ps.buffer("inSeries") is ded.buffer("outData")
    for c in range(calls):
        before = ps.samples_seen
        ded.buffer("inPower").set(command_queue, power[c])
        ded()
        ps()
        peaks, best = ps.buffer("outPeaks").get(command_queue), ps.buffer("outBest").get(command_queue)
        np.testing.assert_array_equal(peaks, refs[c].peaks)
        np.testing.assert_array_equal(best, refs[c].best)
        if c == hit:
            assert best[beam].tolist() == want.tolist()
            found = candidates(peaks, ps_t.threshold, before)
            assert set(found["beam"]) == {beam}
            top = found[np.argmax(found["snr"])]
            assert (top["beam"], top["trial"], top["sample"], top["width_index"]) == (beam, trial, end, 2)
            assert top["snr"] == want[:1].view(np.float32)[0] and top["count"] >= 1
            np.testing.assert_array_equal(found, ref_cands)
