"""The fused beamformer's kernel-selection thresholds as data: for every shape predicate of csrc/bf_fused_plan.cpp the
last call one kernel takes and the first call its neighbour takes, importable without a GPU.

An Edge is two fused_cases.Calls that are adjacent in exactly one argument (A +- 1, M +- 1, T +- 16, C +- 1, one flag,
gains present or absent, delay_channels 1 or C, a workspace offered or not), each with the kernel name it must
report, and the plan field that must change between them (`differs`: kernel, nslabs, xcd_order, uses_table,
lds_bytes; None where the boundary is the kernel's own and no plan field moves).  A one-sided edge (above = None) is
the last shape a kernel accepts; the refusal beyond it is checked on the host.  tests/test_plan_edges_host.py holds the
planner to the names and proves by a scan (the lines of scans()) that no handover between two kernels is missing;
tests/test_gpu_plan_edges.py runs every call against the oracle.  Where a name disagrees, the value (or the planner) is
what is wrong, never the expectation.

A workspace that a shape has no use for (bf_fused_workspace_bytes == 0) cannot be offered, so on an edge that leaves
the table-driven kernels the side outside them carries workspace = False; the host test allows exactly that.
The bf_beamform launcher has no host plan: its edges (TABLE_EDGES) carry names derived by reading dispatch_table and
dispatch_vec of csrc/bf_beamform.hip; the guard-band harness's KERNEL check confirms them on the GPU."""
import math
from collections import namedtuple

import fused_cases as FC

SIGNED, OUT_I8, EXACT, VIA_F32, PATH = FC.SIGNED, FC.OUT_I8, FC.EXACT, FC.VIA_F32, FC.PATH
ITEM, GEN, WIDE, P2 = FC.ITEM, FC.GEN, FC.WIDE, "beamform_fused_wide_p2_kernel"
VITEM, VGEN = "beamform_fused_item_kernel:i8,", "beamform_fused_kernel:i8,"
I8ITEM, I8GEN, W32, W32T, W32R = FC.I8ITEM, "beamform_fused_i8_kernel:", "beamform_fused_i8_w32_kernel:", FC.W32T, FC.W32R

Edge = namedtuple("Edge", "label below above differs var")
EDGES = []
ARG_STEP = {"A": 1, "M": 1, "T": 16, "C": 1}


def gain_cap(c):
    """The bound on |gain| a case's weight table keeps: with int8 beams the caller owns the int32 bound
    A max|x| (|Wc| + |Ws|) < 2^31 (23171 per unit of gain); the largest power of two that keeps it for uint8 samples.
    A = 1248 -> 0.25, A = 2528 -> 0.125."""
    if not c.flags & OUT_I8 or c.flags & VIA_F32:
        return 1.0
    return min(1.0, 2.0 ** math.floor(math.log2(2.0 ** 31 / (c.A * 255 * 23171.0))))


def q14_scale(A, signed, gain):
    """A power-of-two output scale that puts the int8 beams' rms near 30 counts, so that little saturates: a beam
    component is a sum of 2A terms x w with w of rms gain / sqrt(2), x of rms 74 (int8) or 147 (uint8)."""
    rms = math.sqrt(A) * (74 if signed else 147) * gain
    return 2.0 ** round(math.log2(30 / rms))


def add(mode, var, vals, names, differs, sign="alt", path="auto", ws=False, gains=None, dch=None, exact="fe", B=2, C=3,
        **fixed):
    """One row -> its edges.  mode: f32 (one edge per letter of `exact`: f fast, e exact; {e} in the names), via
    (BF_FUSED_INT8_VIA_F32) or q14.  var / vals: the argument that moves and its two values (A M T C; flags: two
    extra flag words; gains: (None, seed); dch: (1, "C"); ws: (False, True)); vals[1] None: one-sided.
    sign: u, s, both, or alt (alternating with the table's length).  ws / gains / dch: a pair where the sides differ.
    dch None: alternating 1 and C."""
    d = dch if dch is not None else (1, "C")[len(EDGES) % 2]
    for e in (exact if mode == "f32" else "f"):
        for sg in ("us" if sign == "both" else sign if sign in ("u", "s") else "us"[len(EDGES) % 2]):
            signed = sg == "s"
            base = (SIGNED if signed else 0) | PATH[path]
            base |= {"f32": EXACT if e == "e" else 0, "via": OUT_I8 | VIA_F32, "q14": OUT_I8}[mode]
            calls = []
            for side in (0, 1):
                if vals[side] is None and var in ARG_STEP:
                    calls.append(None)
                    continue
                k = dict(fixed, B=B, C=C, flags=base, ws=ws, gains=gains, dch=d)
                if var == "flags":
                    k["flags"] = base | vals[side]
                else:
                    k[var] = vals[side]
                pick = {n: (v[side] if isinstance(v, tuple) else v) for n, v in k.items()}
                g = pick["gains"]
                scale = 1.0
                if mode == "via":
                    scale = 1 / 64
                elif mode == "q14":
                    probe = FC.Call(fixed.get("A", vals[0]), 1, 16, 1, 1, base, "", gains=g)
                    scale = q14_scale(probe.A, signed, 0.65 * gain_cap(probe) if g is not None else 1.0)
                calls.append(FC.Call(pick["A"], pick["M"], pick["T"], pick["B"], pick["C"], pick["flags"],
                                     names[side].format(e="exact" if e == "e" else "fast"),
                                     dch=pick["C"] if pick["dch"] == "C" else 1, gains=g, scale=scale,
                                     workspace=pick["ws"]))
            at = ",".join(f"{n}{v}" for n, v in fixed.items())
            tag = "-".join(x for x in (mode + ("x" if e == "e" else ""), path if path != "auto" else "",
                                       "ws" if ws else "", "g" if gains else "", sg + "8") if x)
            label = f"{tag}:{var}{vals[0]}|{vals[1]}@{at}"
            assert label not in {x.label for x in EDGES}, label
            EDGES.append(Edge(label, calls[0], calls[1], differs, var))


# ---- float beams ---------------------------------------------------------------------------------------------------
STAGED = ITEM + "nts2,full,{e},staged"
add("f32", "A", (64, 65), (STAGED, GEN + "nts2,{e}"), "kernel", M=16, T=64)
add("f32", "T", (256, 272), (STAGED, GEN + "nts2,{e}"), "kernel", A=64, M=16)
add("f32", "M", (7, 8), (ITEM + "nts1,partial,{e}", ITEM + "nts1,full,{e}"), "kernel", A=64, T=256)
add("f32", "M", (8, 9), (ITEM + "nts1,full,{e}", ITEM + "nts2,partial,{e}"), "lds_bytes", A=64, T=256)
add("f32", "M", (15, 16), (ITEM + "nts2,partial,{e}", STAGED), "lds_bytes", A=64, T=256)
add("f32", "M", (16, 17), (STAGED, ITEM + "nts2,partial,{e}"), "nslabs", A=64, T=256)
add("f32", "M", (31, 32), (ITEM + "nts2,partial,{e}", ITEM + "nts2,full,{e}"), "kernel", A=64, T=256)
add("f32", "M", (32, 33), (ITEM + "nts2,full,{e}", WIDE + "tw2,{e},unit,buf"), "kernel", A=64, T=256)
add("f32", "M", (32, 33), (ITEM + "nts2,full,{e}", ITEM + "nts2,partial,{e}"), "nslabs", path="item", A=64, T=256)
add("f32", "M", (8, 9), (GEN + "nts1,{e}", GEN + "nts2,{e}"), "lds_bytes", path="generic", A=64, T=256)
add("f32", "M", (23, 24), (GEN + "nts2,{e}", WIDE + "tw2,{e},unit,buf"), "kernel", A=65, T=64)
add("f32", "A", (15, 16), (ITEM + "nts1,partial,{e}", WIDE + "tw1,{e},unit,buf"), "kernel", path="wide", M=3, T=32)
add("f32", "A", (15, 16), (ITEM + "nts2,partial,{e}", WIDE + "tw2,{e},unit,buf"), "kernel", path="wide", M=20, T=32)
add("f32", "A", (15, 16), (STAGED, WIDE + "tw1,{e},unit,buf"), "kernel", path="wide", M=16, T=64)
add("f32", "M", (16, 17), (WIDE + "tw1,{e},unit,buf", WIDE + "tw2,{e},unit,buf"), "lds_bytes", path="wide", A=72, T=64)
# 32-beam slabs of 40 k-steps are exactly 160 KiB; one antenna more pads to 44 and takes 16-beam slabs
add("f32", "A", (640, 641), (WIDE + "tw2,{e},unit,buf", WIDE + "tw1,{e},unit,buf"), "nslabs", path="wide", B=1, C=2,
    M=20, T=32)
add("f32", "A", (640, 641), (GEN + "nts2,{e}", GEN + "nts1,{e}"), "nslabs", path="generic", B=1, C=2, M=9, T=32)
add("f32", "A", (1280, None), (GEN + "nts1,{e}", None), None, path="generic", B=1, C=2, M=9, T=32)
add("f32", "A", (1280, None), (WIDE + "tw1,{e},unit,buf", None), None, path="wide", B=1, C=2, M=20, T=32)
add("f32", "A", (64, 65), (ITEM + "nts2,full,{e}", WIDE + "tw2,{e},unit,buf"), "kernel", B=1, C=2, dch=1, M=32, T=256)
# the persistent kernel's predicate, one argument at a time around (A 256, T 256, M 32, delay_channels 1, no gains)
TW2 = WIDE + "tw2,fast,unit,buf"
PK = dict(exact="f", B=1, C=2, dch=1)
add("f32", "A", (255, 256), (TW2, P2), "kernel", M=32, T=256, **PK)
add("f32", "A", (256, 257), (P2, TW2), "kernel", M=32, T=256, **PK)
add("f32", "T", (240, 256), (TW2, P2), "kernel", A=256, M=32, **PK)
add("f32", "T", (256, 272), (P2, TW2), "kernel", A=256, M=32, **PK)
add("f32", "M", (31, 32), (TW2, P2), "kernel", A=256, T=256, **PK)
add("f32", "M", (32, 33), (P2, TW2), "kernel", A=256, T=256, **PK)
add("f32", "dch", (1, "C"), (P2, TW2), "kernel", exact="f", B=1, C=2, A=256, M=32, T=256)
add("f32", "gains", (None, 5), (P2, WIDE + "tw2,fast,gain,buf"), "kernel", A=256, M=32, T=256, **PK)

# ---- int8 beams requantised from float beams (BF_FUSED_INT8_VIA_F32) -----------------------------------------------
VFULL = VITEM + "nts2,full,fast,pow2"
add("via", "A", (64, 65), (VFULL, VGEN + "nts2,fast"), "kernel", M=16, T=64)
add("via", "T", (256, 272), (VFULL, VGEN + "nts2,fast"), "kernel", A=64, M=16)
add("via", "M", (7, 8), (VITEM + "nts1,partial,fast,pow2", VITEM + "nts1,full,fast,pow2"), "kernel", A=64, T=256)
add("via", "M", (8, 9), (VITEM + "nts1,full,fast,pow2", VITEM + "nts2,partial,fast,pow2"), "lds_bytes", A=64, T=256)
add("via", "M", (15, 16), (VITEM + "nts2,partial,fast,pow2", VFULL), "kernel", A=64, T=256)
add("via", "M", (16, 17), (VFULL, VITEM + "nts2,partial,fast,pow2"), "nslabs", A=64, T=256)
add("via", "M", (8, 9), (VGEN + "nts1,fast", VGEN + "nts2,fast"), "lds_bytes", path="generic", A=64, T=256)
add("via", "A", (640, 641), (VGEN + "nts2,fast", VGEN + "nts1,fast"), "nslabs", B=1, C=2, M=16, T=32)

# ---- int8 beams, the Q14 integer contract ---------------------------------------------------------------------------
BIG = dict(B=1, C=2)
A64P, AANYP = I8ITEM + "nts2,partial,a64,pow2", I8ITEM + "nts2,partial,aany,pow2"
add("q14", "A", (63, 64), (AANYP, A64P), "kernel", M=40, T=256)
add("q14", "A", (64, 65), (A64P, W32 + "unit"), "kernel", sign="both", M=40, T=64)
add("q14", "A", (64, 65), (A64P, W32T + "general,buf"), "kernel", sign="both", ws=(False, True), M=40, T=64)
add("q14", "T", (256, 272), (A64P, W32 + "unit"), "kernel", sign="both", A=64, M=40)
add("q14", "T", (256, 272), (A64P, W32T + "general,buf"), "kernel", sign="both", ws=(False, True), A=64, M=40)
add("q14", "A", (31, 32), (AANYP, W32 + "unit"), "kernel", sign="both", path="wide", M=40, T=64)
add("q14", "A", (31, 32), (AANYP, W32T + "general,buf"), "kernel", sign="both", path="wide", ws=(False, True), M=40, T=64)
add("q14", "A", (63, 64), (I8ITEM + "nts2,full,aany,pow2", I8ITEM + "nts2,full,a64,pow2"), "kernel", M=32, T=256, **BIG)
add("q14", "A", (64, 65), (I8ITEM + "nts2,full,a64,pow2", W32T + "general,buf"), "kernel", sign="both", ws=(False, True),
    M=32, T=256, **BIG)
add("q14", "A", (64, 65), (A64P, I8GEN + "nts2"), "kernel", path="item", M=40, T=64)
add("q14", "T", (256, 272), (A64P, I8GEN + "nts2"), "kernel", path="item", A=64, M=40)
add("q14", "M", (8, 9), (I8GEN + "nts1", I8GEN + "nts2"), "lds_bytes", path="generic", A=64, T=64)
# the table-driven kernels (a workspace offered)
STR = W32T + "straight,pow2"
add("q14", "A", (128, 129), (W32T + "general,buf", STR), "kernel", sign="both", ws=True, M=40, T=256, **BIG)
add("q14", "T", (128, 144), (W32T + "general,buf", STR), "kernel", sign="both", ws=True, A=256, M=40, **BIG)
add("q14", "T", (256, 272), (STR, W32T + "general,buf"), "kernel", sign="both", ws=True, A=256, M=40, **BIG)
add("q14", "A", (256, 257), (STR, W32 + "unit"), "uses_table", sign="both", ws=(True, False), M=40, T=256, **BIG)
add("q14", "ws", (False, True), (W32 + "unit", STR), "uses_table", sign="both", A=256, M=40, T=256, **BIG)
# the LDS-DMA ring: int8 samples, whole 32-beam slabs, T = 256, 8 table steps of more than 224 antennas
add("q14", "A", (224, 225), (STR, W32R + "pow2"), "kernel", sign="s", ws=True, M=32, T=256, **BIG)
add("q14", "A", (256, 257), (W32R + "pow2", W32 + "unit"), "uses_table", sign="s", ws=(True, False), M=32, T=256, **BIG)
add("q14", "M", (31, 32), (STR, W32R + "pow2"), "kernel", sign="s", ws=True, A=256, T=256, **BIG)
add("q14", "M", (32, 33), (W32R + "pow2", STR), "nslabs", sign="s", ws=True, A=256, T=256, **BIG)
add("q14", "T", (240, 256), (STR, W32R + "pow2"), "kernel", sign="s", ws=True, A=256, M=32, **BIG)
add("q14", "T", (256, 272), (W32R + "pow2", W32T + "general,buf"), "kernel", sign="s", ws=True, A=256, M=32, **BIG)
add("q14", "flags", (SIGNED, 0), (W32R + "pow2", STR), "kernel", sign="u", ws=True, A=256, M=32, T=256, **BIG)
# the limb image of 16 steps is the last that fits LDS: beyond 512 antennas the generic kernel.  uint8 samples of
# more than 363 antennas are admitted only with a weight table (the caller's bound)
add("q14", "A", (512, 513), (W32 + "unit", I8GEN + "nts2"), "kernel", sign="s", dch=1, M=40, T=32, **BIG)
add("q14", "A", (512, 513), (W32 + "gain", I8GEN + "nts2"), "kernel", sign="u", gains=7, dch=1, M=40, T=32, **BIG)
add("q14", "A", (1248, 1249), (I8GEN + "nts2", I8GEN + "nts1"), "nslabs", path="generic", gains=8, M=9, T=16, **BIG)
add("q14", "A", (2528, None), (I8GEN + "nts1", None), None, path="generic", gains=9, M=3, T=16, **BIG)
# the 16-column tile and slab boundaries of the beams on the a64 item kernel ...
I8F = {n: I8ITEM + n + ",a64,pow2" for n in ("nts1,partial", "nts1,full", "nts2,partial", "nts2,full")}
add("q14", "M", (7, 8), (I8F["nts1,partial"], I8F["nts1,full"]), "kernel", A=64, T=256)
add("q14", "M", (8, 9), (I8F["nts1,full"], I8F["nts2,partial"]), "lds_bytes", A=64, T=256)
add("q14", "M", (15, 16), (I8F["nts2,partial"], I8F["nts2,full"]), "kernel", A=64, T=256)
add("q14", "M", (16, 17), (I8F["nts2,full"], I8F["nts2,partial"]), "nslabs", A=64, T=256)
add("q14", "M", (32, 33), (I8F["nts2,full"], I8F["nts2,partial"]), "nslabs", A=64, T=256)
# ... and on the 32-beam kernel: within a slab no plan field moves; at 32 | 33 a second slab and the XCD slab order
add("q14", "M", (8, 9), (W32 + "unit", W32 + "unit"), None, sign="both", A=72, T=64)
add("q14", "M", (16, 17), (W32 + "unit", W32 + "unit"), None, sign="both", A=72, T=64)
add("q14", "M", (32, 33), (W32 + "unit", W32 + "unit"), "xcd_order", sign="both", A=72, T=64)
# the item kernels' XCD workgroup order, automatic: C % 8 == 0 and at least 8 beams
add("q14", "M", (7, 8), (I8F["nts1,partial"], I8F["nts1,full"]), "xcd_order", B=1, C=8, dch=1, A=64, T=64)
add("q14", "C", (8, 9), (I8F["nts1,full"], I8F["nts1,full"]), "xcd_order", B=1, dch=1, A=64, M=8, T=64)


def all_calls():
    """(id, Call) of every side of every edge."""
    return [(f"{e.label}:{side}", c) for e in EDGES for side, c in (("below", e.below), ("above", e.above))
            if c is not None]


def float_twin(c):
    """The float call whose beams a BF_FUSED_INT8_VIA_F32 call requantises: the same kernel's float form."""
    kind, tag = c.expect.split(":i8,")
    parts = tag.split(",")
    if kind.endswith("item_kernel"):
        name = ITEM + ",".join(parts[:-1]) + (",staged" if c.M == 16 else "")
    else:
        name = GEN + tag
    return c._replace(flags=c.flags & ~(OUT_I8 | VIA_F32), expect=name, scale=1.0)


# ---- the completeness scan -------------------------------------------------------------------------------------------
RANGES = {"A": range(1, 2601), "M": range(1, 131), "T": range(16, 529, 16), "C": range(1, 18)}
MODE_FLAGS = {"f32": 0, "f32x": EXACT, "via": OUT_I8 | VIA_F32 | SIGNED, "q14u": OUT_I8, "q14s": OUT_I8 | SIGNED}
FLOAT_LINES = {  # path -> the fixed settings its edges use (the variable's own value is replaced by the sweep)
    "auto": [dict(B=2, C=3, A=64, M=16, T=64), dict(B=2, C=3, A=64, M=16, T=256), dict(B=2, C=3, A=65, M=16, T=64),
             dict(B=1, C=2, A=256, M=32, T=256)],
    "item": [dict(B=2, C=3, A=64, M=16, T=256)],
    "generic": [dict(B=2, C=3, A=64, M=16, T=256), dict(B=1, C=2, A=640, M=9, T=32)],
    "wide": [dict(B=2, C=3, A=16, M=3, T=32), dict(B=1, C=2, A=640, M=20, T=32), dict(B=2, C=3, A=72, M=16, T=64)],
}
VIA_LINES = {p: [dict(B=2, C=3, A=64, M=16, T=64), dict(B=2, C=3, A=64, M=16, T=256)] for p in PATH}
Q14_LINES = {  # (path, workspace offered, gains) -> fixed settings
    ("auto", False, False): [dict(B=2, C=3, A=64, M=40, T=256), dict(B=2, C=3, A=72, M=9, T=64)],
    ("auto", True, False): [dict(B=2, C=3, A=64, M=40, T=256), dict(B=1, C=2, A=256, M=40, T=256),
                            dict(B=1, C=2, A=256, M=32, T=256)],
    ("item", False, False): [dict(B=2, C=3, A=64, M=40, T=256)],
    ("item", True, False): [dict(B=2, C=3, A=64, M=40, T=256)],
    ("generic", False, False): [dict(B=2, C=3, A=64, M=40, T=64)],
    ("generic", True, False): [dict(B=2, C=3, A=64, M=40, T=64)],
    ("generic", False, True): [dict(B=1, C=2, A=1248, M=9, T=16), dict(B=1, C=2, A=2528, M=3, T=16)],
    ("wide", False, False): [dict(B=2, C=3, A=64, M=40, T=256)],
    ("wide", True, False): [dict(B=2, C=3, A=64, M=40, T=256)],
}


def scans():
    """(label, flags, gains, workspace offered, scale, fixed settings): every line is swept along A, M, T and C."""
    out = []
    for mode in ("f32", "f32x", "via"):
        for path, lines in (VIA_LINES if mode == "via" else FLOAT_LINES).items():
            out += [(f"{mode},{path}", MODE_FLAGS[mode] | PATH[path], False, False, 1 / 64, f) for f in lines]
    for mode in ("q14u", "q14s"):
        for (path, ws, gains), lines in Q14_LINES.items():
            out += [(f"{mode},{path}{',ws' if ws else ''}{',gains' if gains else ''}", MODE_FLAGS[mode] | PATH[path],
                     gains, ws, 1 / 64, f) for f in lines]
    return out


# ---- bf_beamform: dispatch_table / dispatch_vec of csrc/bf_beamform.hip, read by hand ---------------------------------
# S = ceil(A / 16) k-steps, NT = ceil(M / 8) tiles; a slab of nts tiles holds S nts 2 KiB, 80 of them are LDS.
# Shape: A M NB B P C x_off w_off name.  An edge: (label, below, above); one-sided: above None.
RING, TABLE, OS = "beamform_table_ring_kernel:", "beamform_table_kernel:", "beamform_table_os_kernel"
PERSIST = "beamform_table_persist_kernel:nts2,r16,u8"
Shape = namedtuple("Shape", "A M NB B P C x_off w_off expect", defaults=(2, 1, 2, 2, 0, 4, None))


def sh(A, M, expect, **k):
    return Shape(A, M, expect=expect, **k)


ALIGNED = dict(NB=16, x_off=16, w_off=16)
TABLE_EDGES = [
    # the LDS cascade: the widest slab that fits
    ("lds-nts8|nts4", sh(160, 64, TABLE + "nts8,vec8"), sh(164, 64, RING + "nts4,r8,w8")),  # S 10 | 11: 160 | 176 KiB of 8 tiles
    ("lds-nts4|nts2", sh(320, 25, RING + "nts4,r4,w16"), sh(324, 25, RING + "nts2,r16,w8")),  # S 20 | 21
    ("lds-nts2|nts1", sh(640, 64, RING + "nts2,r8,w16"), sh(644, 64, RING + "nts1,r16,w8")),  # S 40 | 41
    ("lds-last", sh(1280, 64, RING + "nts1,r16,w16", C=1), None),  # S 80: exactly 160 KiB; A 1284 is refused (host test)
    # padded rings, Sp > S
    ("ring-r4-pad", sh(72, 64, RING + "nts8,r4,w16"), None),    # S 5 -> Sp 8
    ("ring-r8-pad", sh(136, 25, RING + "nts4,r8,w16"), None),   # S 9 -> Sp 16
    ("ring-none", sh(136, 64, TABLE + "nts8,vec8"), None),      # S 9 x 8 tiles: Sp 12 and 16 exceed LDS, no ring
    ("ring-r4-full", sh(264, 64, RING + "nts4,r4,w16"), None),  # S 17 -> Sp 20: exactly 160 KiB
    ("ring-r16-pad", sh(264, 9, RING + "nts2,r16,w16"), None),  # S 17 -> Sp 32
    ("rows-scalar", sh(258, 64, TABLE + "nts4,scalar"), None),  # A % 4 != 0 on long rows
    ("rows-w8", sh(68, 64, RING + "nts8,r4,w8"), None),         # A % 8 == 4: 8-byte loads though x is 16-byte aligned
    # long rows (S >= 16) take the widest slab of at most half of LDS
    ("half-lds", sh(240, 64, RING + "nts4,r8,w16"), sh(244, 64, RING + "nts2,r16,w8")),  # S 15 | 16
    # the output-stationary kernel: A % 64 == 0, 256 samples, 64 beams, 16-byte aligned x and w
    ("os-A", sh(192, 64, OS, **ALIGNED), sh(200, 64, RING + "nts4,r8,w16", **ALIGNED)),
    ("os-NB", sh(128, 64, RING + "nts8,r8,w16", **dict(ALIGNED, NB=15)), sh(128, 64, OS, **ALIGNED)),
    # the persistent kernel: at least 8 (b, p, c) items
    ("persist-items", sh(256, 12, RING + "nts2,r16,w16", B=1, P=1, C=7), sh(256, 12, PERSIST, B=1, P=1, C=8)),
]


def table_calls():
    return [(f"{label}:{side}", s) for label, lo, hi in TABLE_EDGES for side, s in (("below", lo), ("above", hi))
            if s is not None]
