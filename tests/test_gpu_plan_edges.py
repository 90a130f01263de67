"""GPU: both sides of every kernel-selection threshold against the oracle (the edges of tests/plan_edges.py; that the
table is complete and the planner agrees with it is proved on the CPU by tests/test_plan_edges_host.py).

A kernel's last legal shape is where its padding, pulled-back last k-step, partial slab or LDS budget is tightest, and
its neighbour's first shape is where an off-by-one in the predicate sends a call to a kernel that cannot hold it.  Every
call of every edge runs bf_beamform_fused_ws under the guard-band harness (guards, two fills, the pinned kernel name,
the plan asked on the host == the kernel that ran) and must meet the suite's oracles: oracle.fused_beamform_int8 bit
for bit (oracle.requantise of the same kernel's float beams for BF_FUSED_INT8_VIA_F32), oracle.fused_beamform within
tolerance.assert_beams_allclose.  No tolerance of its own.  The bf_beamform edges (plan_edges.TABLE_EDGES) run through
guarded.beamform against oracle.complex_mult, both sample types."""
import numpy as np
import pytest

import edge_cases as EC
import guarded as gd
import oracle as O
import plan_edges as PE
from test_gpu_guarded import BDT, CTOT, T0, XENG
from tolerance import assert_beams_allclose

pytestmark = pytest.mark.gpu
TS = O.TS_MEERKAT
SIGNED, OUT_I8, VIA_F32 = PE.SIGNED, PE.OUT_I8, PE.VIA_F32
CALLS, TABLE_CALLS = PE.all_calls(), PE.table_calls()


@pytest.fixture(scope="module")
def ex(context, command_queue):
    return gd.DeviceExecutor(context, command_queue)


def inputs(c):
    """(raw bytes, delay models, weight table or None) of a call, from its shape alone: a via-f32 call and its float
    twin get the same."""
    rng = np.random.default_rng(c.A * 131 + c.M * 7 + c.T + c.C)
    raw = rng.integers(0, 256, (c.B, c.A, c.C, c.T, 2, 2), dtype=np.uint8)
    d = EC.random_delays(c.dch, c.M, c.A, c.A * 31 + c.M)
    gains = None
    if c.gains is not None:
        gains = (rng.uniform(0.25, 1.0, (c.M, c.A)) * PE.gain_cap(c)).astype(np.float32)
    return raw, d, gains


def run_float(ex, c, raw, d, gains):
    signed = bool(c.flags & SIGNED)
    rawv = raw.view(np.int8) if signed else raw

    def oracle(y):
        ref = O.fused_beamform(rawv, d, CTOT, xeng_id=XENG, t0=T0, batch_dt=BDT, signed=signed, gains=gains)
        w = O.fused_tables(d, c.B, c.C, CTOT, c.A, xeng_id=XENG, t0=T0, batch_dt=BDT, gains=gains)
        assert_beams_allclose(y, ref, O.reorder(rawv), w, signed=signed)

    return gd.fused_ws(ex, c, raw, d, gains, np.float32, oracle, CTOT, XENG, TS, T0, BDT)


def check_int8(y, ref):
    assert np.abs(ref.astype(int)).max() >= 4, "the reference is all but zero: the case checks nothing"
    np.testing.assert_array_equal(y, ref)


@pytest.mark.parametrize("c", [c for _, c in CALLS], ids=[i for i, _ in CALLS])
def test_fused_edge(ex, c):
    raw, d, gains = inputs(c)
    signed = bool(c.flags & SIGNED)
    if not c.flags & OUT_I8:
        run_float(ex, c, raw, d, gains)
    elif c.flags & VIA_F32:  # the contract: bf_requant of the float beams of the same kernel's float form
        ref = O.requantise(run_float(ex, PE.float_twin(c), raw, d, gains), c.scale)
        gd.fused_ws(ex, c, raw, d, gains, np.int8, lambda y: check_int8(y, ref), CTOT, XENG, TS, T0, BDT)
    else:
        ref = O.fused_beamform_int8(raw.view(np.int8) if signed else raw, d, CTOT, xeng_id=XENG, t0=T0, batch_dt=BDT,
                                    scale=c.scale, signed=signed, gains=gains)
        gd.fused_ws(ex, c, raw, d, gains, np.int8, lambda y: check_int8(y, ref), CTOT, XENG, TS, T0, BDT)


@pytest.mark.parametrize("s", [s for _, s in TABLE_CALLS], ids=[i for i, _ in TABLE_CALLS])
@pytest.mark.parametrize("signed", [False, True], ids=["u8", "s8"])
def test_beamform_edge(ex, s, signed):
    gd.beamform(ex, s.A, s.M, s.NB, s.B, s.C, signed, s.expect, s.x_off, s.w_off, P=s.P)
