"""CPU: the kernel-selection thresholds of tests/plan_edges.py against the host-side launch plan (bf_fused_plan).

  adjacency    : the two calls of every edge differ in exactly one argument, by one step of it
  names        : the plan gives each call its pinned kernel name, and the two plans differ in the edge's `differs`
  completeness : the planner is swept along A, M, T and C on every line of plan_edges.scans() (each mode -- float,
                 float-exact, via-f32, Q14 with and without an offered workspace, both sample types -- and each forced
                 path, at the settings the edges use); every handover from one kernel name to another that a sweep
                 finds must be in the edge table, at a point where the sweep found it.  A handover that recurs with
                 a period along an axis (full | partial slabs every 16 beams, whole 32-beam slabs every 32) is one
                 predicate and needs one edge.  A threshold added later without an edge fails here.
  refusals     : one step past every one-sided edge the call is refused in the existing words; bf_beamform refuses
                 one k-step past its last slab; the Q14 table generator refuses what its 32-bit stores cannot reach
"""
import ctypes

import pytest

import fused_cases as FC
import plan_edges as PE
from dpdk_dc_sand_amd import _lib

SIGNED, OUT_I8 = FC.SIGNED, FC.OUT_I8
FAKE = 0x10000  # an aligned address that is never dereferenced: each call below is refused before any launch
FIELDS = [f for f in FC.Call._fields if f != "expect"]


def plan(c):
    return _lib.fused_plan(c.B, c.C, c.T, c.A, c.M, c.dch, c.gains is not None, c.flags, c.scale, FC.workspace_bytes(c))


def needs_no_workspace(c):
    return FC.workspace_bytes(c._replace(workspace=True)) == 0


def test_the_table_holds_what_the_issue_counts():
    assert len(PE.EDGES) >= 100 and len({e.label for e in PE.EDGES}) == len(PE.EDGES)
    assert all(c.B <= 2 and c.T <= 272 and (c.C <= 3 or e.var in ("C", "M") and c.C in (8, 9))
               for e in PE.EDGES for c in (e.below, e.above) if c is not None)
    dchs = [e.below.dch == 1 for e in PE.EDGES]
    assert 0.25 < sum(dchs) / len(dchs) < 0.85  # delay_channels alternates between 1 and C


@pytest.mark.parametrize("e", PE.EDGES, ids=[e.label for e in PE.EDGES])
def test_adjacent_in_exactly_one_argument(e):
    if e.above is None:
        assert e.differs is None
        return
    lo, hi = e.below, e.above
    moved = {f for f in FIELDS if getattr(lo, f) != getattr(hi, f)}
    if "workspace" in moved and e.var != "ws":  # the side without one has nothing to be offered
        off = lo if not lo.workspace else hi
        assert needs_no_workspace(off), off
        moved.discard("workspace")
    if e.var in PE.ARG_STEP:
        assert moved == {e.var} and getattr(hi, e.var) - getattr(lo, e.var) == PE.ARG_STEP[e.var]
    elif e.var == "flags":
        assert moved == {"flags"} and bin(lo.flags ^ hi.flags).count("1") == 1
    elif e.var == "gains":
        assert moved == {"gains"} and (lo.gains is None) != (hi.gains is None)
    elif e.var == "dch":
        assert moved == {"dch"} and {lo.dch, hi.dch} == {1, lo.C} and lo.C > 1
    else:
        assert e.var == "ws" and moved == {"workspace"}


@pytest.mark.parametrize("e", PE.EDGES, ids=[e.label for e in PE.EDGES])
def test_pinned_names_and_the_field_that_differs(e):
    below = plan(e.below)
    assert below.kernel.decode() == e.below.expect
    if e.above is None:
        return
    above = plan(e.above)
    assert above.kernel.decode() == e.above.expect
    if e.differs is None:  # the kernel's own boundary: the plan must not move at all
        for f in ("kernel", "nslabs", "xcd_order", "uses_table", "lds_bytes"):
            assert getattr(below, f) == getattr(above, f), f
    else:
        assert getattr(below, e.differs) != getattr(above, e.differs), (e.differs, getattr(below, e.differs))
    assert (e.below.expect != e.above.expect) == (below.kernel != above.kernel)


def test_both_sample_types_on_every_32_beam_edge():
    """The unsigned correction is separate code in the 32-beam kernels: each of their edges has both sample types,
    but for the ring kernel, which takes int8 samples only (its uint8 neighbour is the signed | unsigned edge).
    uint8 samples of more than 363 antennas are admitted only with a weight table, so there the two differ in that."""
    def unsigned_unit(c):
        return c and c._replace(flags=c.flags & ~SIGNED, scale=0, gains=None, expect=c.expect.replace(":gain", ":unit"))

    signs = {}
    for e in PE.EDGES:
        names = [c.expect for c in (e.below, e.above) if c is not None]
        if any("w32" in n for n in names) and not any("w32r" in n for n in names):
            signs.setdefault((e.var, unsigned_unit(e.below), unsigned_unit(e.above)), set()).add(e.below.flags & SIGNED)
    assert len(signs) >= 14 and all(v == {0, SIGNED} for v in signs.values()), [k for k, v in signs.items() if len(v) < 2]


# ---- completeness ---------------------------------------------------------------------------------------------------
def sweep(flags, gains, offer, scale, fixed, var):
    """[(value, kernel name or None when refused)] along one argument."""
    out = []
    for v in PE.RANGES[var]:
        p = dict(fixed)
        p[var] = v
        n = ctypes.c_size_t(0)
        try:
            if offer:
                _lib.call("bf_fused_workspace_bytes", p["B"], p["C"], p["T"], p["A"], p["M"], flags, ctypes.byref(n))
            name = _lib.fused_plan(p["B"], p["C"], p["T"], p["A"], p["M"], 1, gains, flags, scale, n.value).kernel.decode()
        except _lib.BeamformerError:
            name = None
        out.append((v, name))
    return out


def test_every_handover_the_planner_makes_is_in_the_table():
    table, weighted = {}, set()
    for e in PE.EDGES:
        if e.above is not None and e.var in PE.ARG_STEP:
            key = (e.var, e.below.expect, e.above.expect)
            table.setdefault(key, set()).add((getattr(e.below, e.var), getattr(e.above, e.var)))
            if e.below.gains is not None and ":gain" in e.below.expect + e.above.expect:
                weighted.add(key)  # the weighted instantiations: the same thresholds (no line of their own)
    found = {}
    lines = PE.scans()
    assert len(lines) >= 50
    for label, flags, gains, offer, scale, fixed in lines:
        for var in PE.RANGES:
            run = sweep(flags, gains, offer, scale, fixed, var)
            for (v0, n0), (v1, n1) in zip(run, run[1:]):
                if n0 is not None and n1 is not None and n0 != n1:
                    found.setdefault((var, n0, n1), set()).add((v0, v1))
    assert len(found) >= 60
    missing = {k: sorted(v)[:3] for k, v in found.items() if not table.get(k, set()) & v}
    assert not missing, missing
    # and the table's own edges along A, M, T are handovers some sweep found (C moves no name on any line)
    unseen = [k for k in table if k[1] != k[2] and k not in found and k not in weighted]
    assert not unseen, unseen


# ---- refusals ---------------------------------------------------------------------------------------------------------
ONE_SIDED = [e for e in PE.EDGES if e.above is None]


@pytest.mark.parametrize("e", ONE_SIDED, ids=[e.label for e in ONE_SIDED])
def test_one_past_the_last_accepted_count_is_refused(e):
    c = e.below
    assert c.A in (1280, 2528)
    message = f"bf_beamform_fused: n_ants={c.A + 1} too large"
    with pytest.raises(_lib.BeamformerError) as err:
        _lib.fused_plan(c.B, c.C, c.T, c.A + 1, c.M, c.dch, c.gains is not None, c.flags, c.scale)
    assert err.value.status == -1 and err.value.message == message
    with pytest.raises(_lib.BeamformerError) as err:
        _lib.call("bf_beamform_fused_ws", FAKE, FAKE, c.dch, FAKE if c.gains is not None else None, FAKE, c.B, c.C, c.T,
                  c.A + 1, c.M, 8192, 0, 1e-9, 0.0, 0.0, c.flags, c.scale, None, 0, None)
    assert err.value.status == -1 and err.value.message == message


def test_bf_beamform_refuses_one_k_step_past_its_last_slab():
    last = dict(PE.table_calls())["lds-last:below"]
    assert last.A == 1280
    with pytest.raises(_lib.BeamformerError) as err:
        _lib.call("bf_beamform", FAKE, FAKE, FAKE, last.B, last.P, last.C, last.NB, last.A + 4, last.M, 0, None)
    assert err.value.status == -1
    assert err.value.message == "bf_beamform: n_ants=1284 too large for one coefficient slab"


def test_table_edges_are_adjacent_and_unique():
    labels = [label for label, _, _ in PE.TABLE_EDGES]
    assert len(set(labels)) == len(labels)
    for label, lo, hi in PE.TABLE_EDGES:
        if hi is None:
            continue
        moved = {f for f in PE.Shape._fields if f != "expect" and getattr(lo, f) != getattr(hi, f)}
        assert len(moved) == 1 and lo.expect != hi.expect, label
        f = moved.pop()
        # antenna rows come in fours (the ring and vec8 kernels); 192 | 200 keeps A % 8 == 0, the 16-byte row loads
        assert getattr(hi, f) - getattr(lo, f) in {"A": (4, 8), "NB": (1,), "C": (1,)}[f], label


Q14_RANGE = "q14 table: a run of {run} channel blocks of {words} words is beyond the generator's 32-bit store offsets"


@pytest.mark.parametrize("M,A,C,run", [
    (4096, 2048, 64, 64),   # 4 * M A * 64 = 2^31 exactly: the first run the stores cannot address
    (32768, 32767, 1, 1),   # M A < 2^31 (the entry point's own bound), one channel block of 4 GiB
    (4096, 4096, 40, 40),   # a short run: min(run, C) blocks count, not 64
])
def test_q14_table_refuses_what_its_32_bit_stores_cannot_reach(M, A, C, run):
    """q14_table_kernel stores through a buffer resource: 32-bit lane and scalar offsets from the run's first block,
    records below 2^31.  From 4 * words * min(64, C) = 2^31 on, stores would be dropped without a word; the launcher
    refuses.  (The accepted side of this boundary is a 2 GiB table and is not run.)"""
    with pytest.raises(_lib.BeamformerError) as err:
        _lib.call("bf_q14_coeffs", FAKE, 1, None, FAKE, 1, C, A, M, 8192, 0, 1e-9, 0.0, 0.0, None)
    assert err.value.status == -1 and err.value.message == Q14_RANGE.format(run=run, words=M * A)
