"""The guard-band harness's verdict (tests/guarded.py) has teeth: NumPy stand-ins for a kernel, one correct and six
broken in one way each, run over host byte arrays; every broken one must be rejected by the check meant for it.  Also
the host side of bf_last_kernel (feature flag, prototype, "" on a fresh thread).  No GPU."""
import threading

import numpy as np
import pytest

import guarded as gd
from dpdk_dc_sand_amd import _lib

ROWS, COLS = 5, 7  # y[r][c] = 2 * x[r][c] + 1 as int16 of uint8: a stand-in "kernel" with a row structure
X = np.random.default_rng(7).integers(0, 256, (ROWS, COLS), dtype=np.uint8)
NAME = "standin_kernel:ok"


def bufs(x_off=0, y_off=0):
    return [gd.inp("x", X, offset=x_off), gd.out("y", (ROWS, COLS), np.int16, offset=y_off)]


def oracle(outs):
    np.testing.assert_array_equal(outs["y"], 2 * X.astype(np.int16) + 1)


def standin(fault=None):
    def launch(mem):
        (xa, xs, xn), (ya, ys, yn) = mem["x"], mem["y"]
        x = xa[xs:xs + xn].reshape(ROWS, COLS).astype(np.int16)
        y = 2 * x + 1
        if fault == "past_input":  # the byte after the input's payload leaks into the last result
            y[-1, -1] += np.int16(xa[xs + xn])
        yv = ya[ys:ys + yn].view(np.int16).reshape(ROWS, COLS)
        if fault == "skip_last":
            yv.reshape(-1)[:-1] = y.reshape(-1)[:-1]
        elif fault == "skip_row":
            yv[:2], yv[3:] = y[:2], y[3:]
        else:
            yv[...] = y
        if fault == "write_past":
            ya[ys + yn] = 0
        if fault == "write_before":
            ya[ys - 1] = 0
        if fault == "flip_input":
            xa[xs + 3] ^= 1
        return NAME
    return launch


@pytest.mark.parametrize("x_off,y_off", [(0, 0), (1, 2), (16, 8)])
def test_correct_standin_passes(x_off, y_off):
    outs = gd.run_case(gd.host_execute, bufs(x_off, y_off), standin(), oracle, NAME)
    oracle(outs)


@pytest.mark.parametrize("fault,check", [
    ("skip_last", gd.REPEAT), ("skip_row", gd.REPEAT), ("write_past", gd.GUARD), ("write_before", gd.GUARD),
    ("past_input", gd.REPEAT), ("flip_input", gd.INPUT)])
@pytest.mark.parametrize("y_off", [0, 2])
def test_broken_standin_is_rejected_by_its_check(fault, check, y_off):
    with pytest.raises(gd.GuardFailure) as e:
        gd.run_case(gd.host_execute, bufs(1, y_off), standin(fault), oracle, NAME)
    assert check in e.value.checks, e.value
    # a fault that leaves the results right is caught by its own check alone
    if fault in ("write_past", "write_before", "flip_input"):
        assert e.value.checks == {check}, e.value


def test_write_into_the_offset_gap_is_a_guard_failure():
    def launch(mem):
        name = standin()(mem)
        ya, ys, _ = mem["y"]
        ya[gd.G] = 0  # the first byte of the gap between the guard and an offset payload
        return name
    with pytest.raises(gd.GuardFailure) as e:
        gd.run_case(gd.host_execute, bufs(0, 4), launch, oracle, NAME)
    assert e.value.checks == {gd.GUARD}


def test_stale_but_correct_output_is_rejected():
    """What the harness exists for: a kernel that writes nothing, over a buffer that happens to hold the right answer
    from an earlier launch, passes an oracle comparison; here the payload is refilled, so it cannot."""
    with pytest.raises(gd.GuardFailure) as e:
        gd.run_case(gd.host_execute, bufs(), lambda mem: NAME, oracle, NAME)
    assert {gd.REPEAT, gd.ORACLE} <= e.value.checks


def test_wrong_result_and_wrong_kernel_name():
    def launch(mem):
        standin()(mem)
        ya, ys, _ = mem["y"]
        ya[ys] ^= 1
        return "standin_kernel:other"
    with pytest.raises(gd.GuardFailure) as e:
        gd.run_case(gd.host_execute, bufs(), launch, oracle, NAME)
    assert e.value.checks == {gd.ORACLE, gd.KERNEL}


def test_layout_and_fills():
    b = gd.out("y", (3,), np.float32, offset=4)
    assert (b.start, b.total) == (gd.G + 4, 2 * gd.G + 4 + 12)
    assert (b.image(0) == 0x5A).all() and (b.image(1) == 0xA5).all()
    i = gd.inp("x", np.arange(6, dtype=np.uint8), offset=8)
    img = i.image(1)
    assert (img[:gd.G + 8] == 0xFF).all() and (img[gd.G + 14:] == 0xFF).all()
    np.testing.assert_array_equal(i.payload(img), np.arange(6, dtype=np.uint8))
    assert np.isnan(np.full(4, 0xFF, np.uint8).view(np.float32)[0])


def test_last_kernel_feature_and_prototype():
    lib = _lib.load()
    assert lib.bf_has_feature(b"last_kernel") == 1
    assert lib.bf_has_feature(b"last") == 0
    assert lib.bf_abi_version() == 302
    res, args = _lib.PROTOTYPES["bf_last_kernel"]
    assert res is _lib.c_char_p and args == []


def test_last_kernel_is_empty_on_a_fresh_thread():
    got = []
    t = threading.Thread(target=lambda: got.append(_lib.load().bf_last_kernel()))
    t.start()
    t.join()
    assert got == [b""]


def test_refusals_leave_the_last_kernel_unchanged():
    lib = _lib.load()
    before = lib.bf_last_kernel()
    with pytest.raises(_lib.BeamformerError, match="misaligned"):
        _lib.call("bf_requant", (1 << 20) + 4, 1 << 20, 16, 1.0, None)
    assert lib.bf_last_kernel() == before
