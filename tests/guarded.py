"""Guard-band harness: does a kernel write all and only its output, and read only its input?

For one call every buffer sits inside its own larger allocation

    [guard G][offset o][payload][guard G]          G = 64 KiB, o = 0 or the smallest alignment the entry point accepts

(the allocation base is at least 256-byte aligned, so the payload sits at exactly its minimum legal alignment when
o is that alignment).  The call is made twice, every byte of every allocation uploaded afresh before each:

             input allocations (guards and offset gap)      output allocations (whole allocation, payload included)
    run 1    0x00                                           0x5A
    run 2    0xFF (a NaN as f32, 255 or -1 as a sample)     0xA5

and `verdict` demands all of

    1. REPEAT  the output payloads of run 1 and run 2 are equal bit for bit (an element the kernel leaves unwritten keeps
               two different fills; a byte used from outside an input differs between the runs);
    2. ORACLE  the payload meets the case's oracle (the caller's check: bit-exact or the project's stated tolerance);
    3. GUARD   the output guards and the offset gap still hold their fill after both runs;
    4. INPUT   every input allocation, payload and guards, is byte-identical to what was uploaded;
    5. KERNEL  the kernel that ran (bf_last_kernel) is the one the case claims to cover.

The verdict is pure NumPy over host byte arrays (tests/test_guarded_host.py runs it over NumPy stand-ins for a kernel);
`DeviceExecutor` is the thin upload / launch / download wrapper for the GPU cases, `fused_ws` the guarded
bf_beamform_fused_ws call that tests/test_gpu_edges.py, tests/test_gpu_phase_domain.py and tests/test_gpu_plan_edges.py
share, and `beamform` the guarded bf_beamform call of tests/test_gpu_guarded.py and tests/test_gpu_plan_edges.py.

Limits: the harness never hands a kernel a pointer or size its header forbids and never depends on a fault.  An overrun
of up to G bytes on either side of a payload lands in memory the test owns and is reported; anything that strays
farther than 64 KiB from its buffer is out of this harness's reach.
"""
import ctypes

import numpy as np

G = 64 * 1024
IN_FILL = (0x00, 0xFF)
OUT_FILL = (0x5A, 0xA5)
REPEAT, ORACLE, GUARD, INPUT, KERNEL = "repeat", "oracle", "guard", "input", "kernel"


class Buf:
    """One buffer of a call.  Inputs carry their payload (any C-contiguous array); outputs a shape and dtype."""

    def __init__(self, name, kind, data=None, shape=None, dtype=None, offset=0):
        assert kind in ("in", "out") and offset >= 0
        self.name, self.kind, self.offset = name, kind, int(offset)
        if kind == "in":
            self.data = np.ascontiguousarray(data)
            self.shape, self.dtype = self.data.shape, self.data.dtype
        else:
            self.data = None
            self.shape, self.dtype = tuple(int(s) for s in shape), np.dtype(dtype)
        self.nbytes = int(np.prod(self.shape, dtype=np.int64)) * self.dtype.itemsize
        self.start = G + self.offset  # payload's first byte within the allocation
        self.total = self.start + self.nbytes + G

    def image(self, run):
        """The allocation's bytes as uploaded before run `run` (0 or 1)."""
        img = np.full(self.total, (IN_FILL if self.kind == "in" else OUT_FILL)[run], np.uint8)
        if self.kind == "in":
            img[self.start:self.start + self.nbytes] = self.data.reshape(-1).view(np.uint8)
        return img

    def payload(self, img):
        return img[self.start:self.start + self.nbytes].view(self.dtype).reshape(self.shape)


def inp(name, data, offset=0):
    return Buf(name, "in", data=data, offset=offset)


def out(name, shape, dtype, offset=0):
    return Buf(name, "out", shape=shape, dtype=dtype, offset=offset)


class GuardFailure(AssertionError):
    """The verdict's failures: `.checks` is the set of failed checks (REPEAT, ORACLE, GUARD, INPUT, KERNEL)."""

    def __init__(self, failures):
        self.failures = failures
        self.checks = {c for c, _ in failures}
        super().__init__("; ".join(f"[{c}] {msg}" for c, msg in failures))


def _where(mask, shape=None, limit=6):
    idx = np.flatnonzero(mask)
    shown = [int(i) if shape is None else tuple(int(v) for v in np.unravel_index(i, shape)) for i in idx[:limit]]
    return f"{idx.size} at {shown}{' ...' if idx.size > limit else ''}"


def verdict(bufs, before, after, oracle=None, kernels=None, expect_kernel=None):
    """before / after: per run (two of each) a dict name -> whole-allocation uint8 array, as uploaded and as downloaded.
    oracle(outputs) raises AssertionError when run 1's output payloads (dict name -> typed array) are wrong.
    kernels: the two runs' bf_last_kernel strings.  Returns the list of (check, message) failures."""
    failures = []
    for b in bufs:
        if b.kind == "out":
            p0 = after[0][b.name][b.start:b.start + b.nbytes]
            p1 = after[1][b.name][b.start:b.start + b.nbytes]
            if not np.array_equal(p0, p1):
                diff = (p0 != p1).reshape(-1, b.dtype.itemsize).any(axis=1)
                failures.append((REPEAT, f"{b.name}: runs differ in elements {_where(diff, b.shape)}"))
            for run in (0, 1):
                img, fill = after[run][b.name], OUT_FILL[run]
                lo, hi = img[:b.start] != fill, img[b.start + b.nbytes:] != fill
                if lo.any():
                    failures.append((GUARD, f"{b.name} run {run + 1}: bytes before the payload written, {_where(lo)} "
                                            f"(payload starts at {b.start})"))
                if hi.any():
                    failures.append((GUARD, f"{b.name} run {run + 1}: bytes past the payload written, "
                                            f"payload end + {_where(hi)}"))
        else:
            for run in (0, 1):
                bad = after[run][b.name] != before[run][b.name]
                if bad.any():
                    failures.append((INPUT, f"{b.name} run {run + 1}: input allocation modified, {_where(bad)} "
                                            f"(payload is [{b.start}, {b.start + b.nbytes}))"))
    if oracle is not None:
        try:
            oracle({b.name: b.payload(after[0][b.name]) for b in bufs if b.kind == "out"})
        except AssertionError as e:
            failures.append((ORACLE, str(e)[:600]))
    if expect_kernel is not None:
        for run in (0, 1):
            if kernels[run] != expect_kernel:
                failures.append((KERNEL, f"run {run + 1} launched {kernels[run]!r}, the case expects {expect_kernel!r}"))
                break
    return failures


def run_case(execute, bufs, launch, oracle=None, expect_kernel=None):
    """Two launches through `execute(bufs, images, launch) -> (images_after, kernel_name)`, then the verdict.
    Returns run 1's output payloads; raises GuardFailure."""
    assert len({b.name for b in bufs}) == len(bufs)
    before, after, kernels = [], [], []
    for run in (0, 1):
        images = {b.name: b.image(run) for b in bufs}
        got, kernel = execute(bufs, images, launch)
        before.append(images)
        after.append(got)
        kernels.append(kernel)
    failures = verdict(bufs, before, after, oracle, kernels, expect_kernel)
    if failures:
        raise GuardFailure(failures)
    return {b.name: b.payload(after[0][b.name]) for b in bufs if b.kind == "out"}


def host_execute(bufs, images, launch):
    """The executor of the self-test: `launch(mem)` is a NumPy stand-in for a kernel working on copies of the
    allocations, mem[name] = (whole-allocation uint8 array, payload start, payload bytes); it returns its name."""
    mem = {b.name: (images[b.name].copy(), b.start, b.nbytes) for b in bufs}
    kernel = launch(mem)
    return {name: m[0] for name, m in mem.items()}, kernel


class DeviceExecutor:
    """Upload every allocation, `launch(ptrs)` (ptrs[name] = the payload's device address; the caller makes the C-ABI
    call on `queue`), download every allocation whole."""

    def __init__(self, context, queue):
        from dpdk_dc_sand_amd import _lib
        self._lib, self.context, self.queue = _lib, context, queue

    def __call__(self, bufs, images, launch):
        lib = self._lib
        base = {}
        try:
            for b in bufs:
                base[b.name] = self.context.allocate_raw(b.total)
                assert base[b.name] % 256 == 0, "allocation base below 256-byte alignment"
                lib.call("bf_memcpy_h2d", base[b.name], images[b.name].ctypes.data, b.total, self.queue.handle)
            self.queue.finish()
            launch({b.name: base[b.name] + b.start for b in bufs})
            kernel = lib.load().bf_last_kernel().decode()
            self.queue.finish()
            got = {b.name: np.empty(b.total, np.uint8) for b in bufs}
            for b in bufs:
                lib.call("bf_memcpy_d2h", got[b.name].ctypes.data, base[b.name], b.total, self.queue.handle)
            self.queue.finish()
            return got, kernel
        finally:
            for p in base.values():
                lib.load().bf_free(ctypes.c_void_p(p))


def fused_ws(ex, c, raw, d, gains, out_dtype, oracle, Ctot, xeng_id, Ts, t0, batch_dt):
    """One guarded bf_beamform_fused_ws call of a case (the fields of fused_cases.Call: A M T B C flags expect scale
    workspace, and dch gains for the planner) in the band (Ctot, xeng_id, Ts) at steering times t0 + b batch_dt:
    guards, two fills, the expected kernel name, and the plan asked on the host == the kernel that ran.
    oracle(y) raises AssertionError on wrong beams.  Returns the beams."""
    import fused_cases as FC
    lib = ex._lib
    dch = d.shape[0]
    bufs = [inp("raw", raw, 16), inp("dv", d, 16), out("y", (c.B, 2, c.C, c.T // 16, 16, 2 * c.M), out_dtype, 16)]
    if gains is not None:
        bufs.append(inp("gains", gains, 4))
    ws_bytes = FC.workspace_bytes(c)
    if c.workspace:
        assert ws_bytes > 0, "the case expects a shape that uses the workspace"
        bufs.append(out("ws", (ws_bytes,), np.uint8, 16))

    def launch(p):
        lib.call("bf_beamform_fused_ws", p["raw"], p["dv"], dch, p.get("gains"), p["y"], c.B, c.C, c.T, c.A, c.M, Ctot,
                 xeng_id, Ts, t0, batch_dt, c.flags, c.scale, p.get("ws"), ws_bytes, ex.queue.handle)

    y = run_case(ex, bufs, launch, lambda outs: oracle(outs["y"]), c.expect)["y"]
    assert FC.planned_name(c) == lib.load().bf_last_kernel().decode()  # the plan, asked on the host, is what ran
    return y


def beamform(ex, A, M, NB, B, C, signed, expect, x_off, w_off=4, P=2):
    """One guarded bf_beamform call over random samples and a random table in [-1, 1), x and w at the given offsets
    from a 256-byte boundary, against oracle.complex_mult within the project's float tolerance.  Returns the beams."""
    import oracle as O
    from tolerance import assert_beams_allclose
    rng = np.random.default_rng(A * 7 + M + NB)
    x = rng.integers(0, 256, (B, P, C, NB, 16, A, 2), dtype=np.uint8)
    xv = x.view(np.int8) if signed else x
    w = rng.uniform(-1.0, 1.0, (B, P, C, 2 * A, 2 * M)).astype(np.float32)
    bufs = [inp("x", x, x_off), inp("w", w, w_off), out("y", (B, P, C, NB, 16, 2 * M), np.float32, 16)]

    def launch(p):
        ex._lib.call("bf_beamform", p["x"], p["w"], p["y"], B, P, C, NB, A, M, int(signed), ex.queue.handle)

    def oracle(outs):
        assert_beams_allclose(outs["y"], O.complex_mult(xv, w, signed=signed), xv, w, signed=signed)

    return run_case(ex, bufs, launch, oracle, expect)["y"]
