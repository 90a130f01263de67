"""Multi-rank channel sharding on the GPU through libbf, on the one visible MI355X.

Two fresh child processes (ranks of a TCP rendezvous group of 2, no torch) share the GPU.  Rank 0 holds a full-band raw cube; the
channel scatter (dpdk_dc_sand_amd.shard) gives each rank its X-engine's contiguous channel slice; each rank beamforms
its slice with `FusedBeamformerTemplate(..., xeng_id=rank)` -- the reference's absolute-channel convention
`ichannel = c + C * xeng_id` (coeff_generator.py:49-53) -- and the beams are gathered back.  The gathered band must
equal the full-band oracle: int8 bit-exact, float32 within the stated tolerance.

`test_bench_multi_rank_rehearsal` runs bench.py itself under torch.distributed.run with two ranks on this GPU and
the host scatter backend (RCCL cannot put two ranks on one device); the driver's 8-GPU run uses the RCCL backend
(libbf bf_channel_scatter), whose one-rank form runs here.
"""
import json
import os
import socket
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

pytestmark = pytest.mark.gpu


def _free_port():
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    p = s.getsockname()[1]
    s.close()
    return p


def _rank_main(rank, world, port, out_dir):
    sys.path.insert(0, ROOT)
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    import oracle as O
    from dpdk_dc_sand_amd import accel
    from dpdk_dc_sand_amd.beamforming import FusedBeamformerTemplate
    from dpdk_dc_sand_amd.rendezvous import HostGroup
    from dpdk_dc_sand_amd.shard import gather_channel_slices, scatter_channel_slices

    group = HostGroup(rank, world, "127.0.0.1", port)
    try:
        B, A, M, T, C = 2, 64, 16, 256, 8
        Ctot = C * world
        ts = O.TS_MEERKAT
        bdt = T * 2 * Ctot * ts
        rng = np.random.default_rng(5)
        d = np.zeros((1, M, A, 4), np.float32)
        d[..., 0] = rng.uniform(0, 10 * ts, (M, A))
        d[..., 1] = rng.uniform(-1e-9, 1e-9, (M, A))
        d[..., 2] = rng.uniform(-np.pi, np.pi, (M, A))
        d[..., 3] = rng.uniform(-1, 1, (M, A))
        raw = rng.integers(-128, 128, (B, A, Ctot, T, 2, 2), dtype=np.int8) if rank == 0 else None
        mine = scatter_channel_slices(raw, (B, A, C, T, 2, 2), np.int8, group)

        ctx = accel.create_some_context(device=0)
        queue = ctx.create_command_queue()
        out = {}
        for name, kw in (("int8", dict(out_int8=True, out_scale=1 / 64)), ("f32", {})):
            op = FusedBeamformerTemplate(ctx, B, C, Ctot, T, A, M, xeng_id=rank, sample_period=ts, delay_channels=1,
                                         sample_signed=True, t0=1e-3, batch_dt=bdt, **kw).instantiate(queue)
            op.ensure_all_bound()
            op.buffer("inSamples").set(queue, mine)
            op.buffer("delay_vals").set(queue, d)
            op()
            out[name] = gather_channel_slices(op.buffer("outData").get(queue), group)
        if rank == 0:
            q_ref = O.fused_beamform_int8(raw, d, Ctot, t0=1e-3, batch_dt=bdt, scale=1 / 64, signed=True)
            y_ref = O.fused_beamform(raw, d, Ctot, t0=1e-3, batch_dt=bdt, signed=True)
            w = O.fused_tables(d, B, Ctot, Ctot, A, t0=1e-3, batch_dt=bdt)
            np.savez(os.path.join(out_dir, "result.npz"), q=out["int8"], q_ref=q_ref, y=out["f32"], y_ref=y_ref,
                     x=O.reorder(raw), w=w)
    finally:
        group.close()


def test_channel_sharded_hip_beamforming_matches_full_band(tmp_path):
    world = 2
    port = _free_port()
    env = dict(os.environ, PYTHONPATH=os.pathsep.join([ROOT, os.path.join(ROOT, "tests")]))
    code = ("import sys; sys.path.insert(0, %r); sys.path.insert(0, %r); import test_gpu_multi_rank as t; "
            "t._rank_main(int(sys.argv[1]), %d, %d, %r)") % (ROOT, os.path.join(ROOT, "tests"), world, port,
                                                               str(tmp_path))
    procs = [subprocess.Popen([sys.executable, "-c", code, str(r)], env=env, cwd=ROOT) for r in range(world)]
    try:
        rcs = [p.wait(timeout=110) for p in procs]
    finally:
        for p in procs:
            if p.poll() is None:
                p.kill()
    assert rcs == [0] * world, rcs
    from tolerance import assert_beams_allclose
    r = np.load(tmp_path / "result.npz")
    np.testing.assert_array_equal(r["q"], r["q_ref"])
    assert np.abs(r["q_ref"].astype(int)).max() >= 8
    assert_beams_allclose(r["y"], r["y_ref"], r["x"], r["w"], signed=True)


def test_bench_multi_rank_rehearsal(tmp_path):
    """bench.py --gpus 2 under torch.distributed.run: both ranks time their own channel shard (X-engines 0 and 1),
    the input arrives through the scatter (host backend here), and rank 0 prints one JSON line with the whole-job
    value, the scatter report and the config-4 channel-sharded secondary lines."""
    port = _free_port()
    cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node", "2", "--master-addr",
           "127.0.0.1", "--master-port", str(port), os.path.join(ROOT, "bench.py"), "--gpus", "2", "--steps", "4",
           "--warmup", "1", "--settle-ms", "0", "--scatter-backend", "host", "--workload", "cfg3", "--nbuf", "1",
           "--full"]
    r = subprocess.run(cmd, capture_output=True, text=True, timeout=110, cwd=ROOT)
    assert r.returncode == 0, r.stderr[-2000:]
    lines = [ln for ln in r.stdout.splitlines() if ln.strip().startswith("{")]
    assert len(lines) == 1, r.stdout
    line = json.loads(lines[0])
    assert line["n_gpus"] == 2 and line["scaling"] == "weak"
    assert line["scatter"]["backend"] == "host" and line["scatter"]["ranks"] == 2
    assert line["scatter"]["bytes_per_rank"] == 8 * 64 * 4096 * 256 * 4
    assert line["value"] > 0
    sec = line["secondary"]
    assert [s["workload"][:4] for s in sec] == ["cfg4", "cfg4"], sec
    assert all("error" not in s and s["n_gpus"] == 2 and s["value"] > 0 for s in sec), sec
    assert line["config"]["ranks_launched_by"].startswith("external")


def test_bench_gpus_two_without_launcher(tmp_path):
    """The driver's own command form, `python bench.py --gpus 2 ...` with no torch.distributed.run: bench.py starts
    its two ranks itself (both on this one GPU, host scatter backend since RCCL refuses two ranks on one device).
    Both ranks time their X-engine's shard and the config-4 secondaries; rank 0 prints the one line."""
    cmd = [sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "2", "--steps", "4", "--warmup", "1",
           "--settle-ms", "0", "--scatter-backend", "host", "--workload", "cfg3", "--nbuf", "1", "--full"]
    env = {k: v for k, v in os.environ.items() if k not in ("WORLD_SIZE", "RANK", "LOCAL_RANK")}
    r = subprocess.run(cmd, capture_output=True, text=True, timeout=110, cwd=ROOT, env=env)
    assert r.returncode == 0, r.stderr[-2000:]
    lines = [ln for ln in r.stdout.splitlines() if ln.strip().startswith("{")]
    assert len(lines) == 1, r.stdout
    line = json.loads(lines[0])
    assert line["n_gpus"] == 2 and line["config"]["ranks_launched_by"] == "bench.py"
    assert line["scatter"]["backend"] == "host" and line["scatter"]["ranks"] == 2
    assert len(line["per_rank_avg_launch_us"]) == 2 and all(t > 0 for t in line["per_rank_avg_launch_us"])
    sec = line["secondary"]
    assert [s["workload"][:4] for s in sec] == ["cfg4", "cfg4"], sec
    for s in sec:
        assert "error" not in s and s["n_gpus"] == 2 and s["value"] > 0, s
        assert len(s["per_rank_avg_launch_us"]) == 2 and all(t > 0 for t in s["per_rank_avg_launch_us"]), s


def test_bench_rccl_scatter_path_one_rank(tmp_path):
    """The RCCL side of the channel scatter on a one-GPU box: a one-rank libbf communicator runs bench.py's device
    path end to end -- band filled in HBM, the id hand-out, bf_channel_scatter, the received slice bound as the
    operator's input and timed.  (More ranks than GPUs is not an RCCL configuration; the N-rank run is the driver's
    multi-GPU node.)"""
    cmd = [sys.executable, os.path.join(ROOT, "bench.py"), "--steps", "3", "--warmup", "1", "--settle-ms", "0",
           "--scatter-backend", "rccl", "--scatter-at-one", "--workload", "cfg2", "--no-secondary", "--no-pmc",
           "--no-cpu-baseline", "--no-ceiling", "--no-rocprof"]
    env = dict(os.environ, MASTER_ADDR="127.0.0.1", MASTER_PORT=str(_free_port()))
    r = subprocess.run(cmd, capture_output=True, text=True, timeout=110, cwd=ROOT, env=env)
    assert r.returncode == 0, r.stderr[-2000:]
    lines = [ln for ln in r.stdout.splitlines() if ln.strip().startswith("{")]
    assert len(lines) == 1, r.stdout
    line = json.loads(lines[0])
    sc = line["scatter"]
    assert "error" not in sc, sc
    assert sc["backend"] == "rccl" and sc["ranks"] == 1 and "RCCL" in sc["collective"], sc
    assert line["scatter_ok"] is True and sc["verified"] is True, sc
    # three timed scatters + nothing else, all through ncclRecv (the self send/recv at one rank)
    assert sc["rccl_bytes_received_this_rank"] == 3 * sc["bytes_per_rank"], sc
    assert sc["bytes_per_rank"] == 8 * 64 * 4096 * 256 * 4 and sc["seconds"] > 0
    assert line["value"] > 0


def test_bench_rccl_scatter_two_ranks(tmp_path):
    """bench.py --gpus 2 over RCCL (one rank per GPU): the root's band is packed and sent to both ranks, and every
    rank's received slice is checksummed on its device and compared with the root's band slice [C r, C (r + 1)).

    The device count comes from libbf (the product's /opt/rocm HIP runtime) inside the test: a collection-time
    `torch.cuda.device_count()` would map torch's bundled HIP runtime into the test process first, and every later
    libbf load would then bind to it (test_hip_runtime_is_the_products)."""
    sys.path.insert(0, ROOT)
    from dpdk_dc_sand_amd import accel
    if accel.device_count() < 2:
        pytest.skip("the RCCL channel scatter across ranks needs two GPUs")
    port = _free_port()
    cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node", "2", "--master-addr",
           "127.0.0.1", "--master-port", str(port), os.path.join(ROOT, "bench.py"), "--gpus", "2", "--steps", "3",
           "--warmup", "1", "--settle-ms", "0", "--scatter-backend", "rccl", "--workload", "cfg2", "--no-secondary",
           "--no-pmc", "--no-cpu-baseline", "--no-ceiling", "--no-rocprof"]
    r = subprocess.run(cmd, capture_output=True, text=True, timeout=110, cwd=ROOT)
    assert r.returncode == 0, r.stderr[-2000:]
    lines = [ln for ln in r.stdout.splitlines() if ln.strip().startswith("{")]
    assert len(lines) == 1, r.stdout
    line = json.loads(lines[0])
    sc = line["scatter"]
    assert "error" not in sc and sc["backend"] == "rccl" and sc["ranks"] == 2, sc
    assert line["scatter_ok"] is True and sc["verified"] is True, sc
    assert [c["match"] for c in sc["checksums"]] == [True, True], sc


def test_channel_scatter_one_rank_comm():
    """libbf's communicator at one rank: the RCCL id, bf_comm_create, bf_comm_allreduce_max (an RCCL all-reduce) and
    bf_channel_scatter of a (B, A, C, T, 2, 2) band into a slice (the root's own 2-D pack) equal the numpy slice; the
    device RNG fill is deterministic."""
    sys.path.insert(0, ROOT)
    from dpdk_dc_sand_amd import _lib, accel
    from dpdk_dc_sand_amd.rendezvous import HostGroup
    from dpdk_dc_sand_amd.shard import ChannelScatter, host_checksum

    ctx = accel.create_some_context(device=0)
    q = ctx.create_command_queue()
    comm = ChannelScatter(HostGroup(0, 1), ctx)
    try:
        assert comm.allreduce_max(3.25) == 3.25
        B, A, C, T = 2, 3, 5, 32
        band = accel.DeviceArray(ctx, (B, A, C, T, 2, 2), np.uint8)
        _lib.call("bf_fill_random", band.ptr, band.nbytes, 7, q.handle)
        host = band.get(q)
        again = accel.DeviceArray(ctx, (B, A, C, T, 2, 2), np.uint8)
        _lib.call("bf_fill_random", again.ptr, again.nbytes, 7, q.handle)
        np.testing.assert_array_equal(again.get(q), host)
        assert len(np.unique(host)) > 200
        out = accel.DeviceArray(ctx, (B, A, C, T, 2, 2), np.uint8)
        out.set(q, np.zeros((B, A, C, T, 2, 2), np.uint8))
        assert comm.stats() == (0, 0)
        comm.scatter(band, out, B, A, C, T, q)
        np.testing.assert_array_equal(out.get(q), host)
        # the slice arrived through RCCL point-to-point: the root packs into staging and its own slice is a self
        # ncclSend/ncclRecv (bf_channel_scatter writes `slice` only through ncclRecv)
        assert comm.stats() == (host.nbytes, host.nbytes)
        ok, per_rank = comm.verify(band, out, B, A, C, T, q)
        assert ok and per_rank == [{"rank": 0, "checksum": f"{host_checksum(host):016x}", "match": True}]
        # a slice that differs from the band by one byte fails the check
        bad = host.copy()
        bad[1, 2, 3, 4, 1, 0] ^= 1
        out.set(q, bad)
        ok, per_rank = comm.verify(band, out, B, A, C, T, q)
        assert not ok and not per_rank[0]["match"]
    finally:
        comm.close()


def test_device_checksum_matches_restatement():
    """bf_checksum == shard.host_checksum, contiguous and for a strided (band, rank) region == the packed slice."""
    sys.path.insert(0, ROOT)
    from dpdk_dc_sand_amd import _lib, accel
    from dpdk_dc_sand_amd.shard import device_checksum, host_checksum, pack_channel_slices

    ctx = accel.create_some_context(device=0)
    q = ctx.create_command_queue()
    B, A, N, C, T = 3, 5, 4, 6, 48
    band = accel.DeviceArray(ctx, (B, A, N * C, T, 2, 2), np.uint8)
    _lib.call("bf_fill_random", band.ptr, band.nbytes, 11, q.handle)
    host = band.get(q)
    assert device_checksum(band, host.nbytes, 0, 1, q) == host_checksum(host)
    run = C * T * 4
    for r, part in enumerate(pack_channel_slices(host, N)):
        assert device_checksum(band.ptr + r * run, run, run * N, B * A, q) == host_checksum(part)
    big = accel.DeviceArray(ctx, (1 << 26,), np.uint8)  # 64 MiB: many workgroups, one atomic per wave
    _lib.call("bf_fill_random", big.ptr, big.nbytes, 3, q.handle)
    assert device_checksum(big, big.nbytes, 0, 1, q) == host_checksum(big.get(q))


@pytest.mark.parametrize("shape", [(8, 64, 4096, 256), (1, 2, 294912, 256)], ids=["2GiB-slice", "rows-over-256MiB"])
def test_channel_scatter_large_slices(shape):
    """bf_channel_scatter at one rank with slices RCCL's point-to-point cannot move in one message: a 2 GiB slice
    (RCCL 2.27.7's self ncclSend/ncclRecv of more than 1 GiB leaves every byte past 2^30 unwritten,
    profiles/r5_a_scatter_attribution.txt) and rows longer than the 256 MiB piece (sub-row segments).  The device
    checksums of every received slice must equal the band's."""
    sys.path.insert(0, ROOT)
    from dpdk_dc_sand_amd import _lib, accel
    from dpdk_dc_sand_amd.rendezvous import HostGroup
    from dpdk_dc_sand_amd.shard import ChannelScatter

    B, A, C, T = shape
    ctx = accel.create_some_context(device=0)
    q = ctx.create_command_queue()
    comm = ChannelScatter(HostGroup(0, 1), ctx)
    try:
        band = accel.DeviceArray(ctx, (B, A, C, T, 2, 2), np.uint8)
        _lib.call("bf_fill_random", band.ptr, band.nbytes, 13, q.handle)
        out = accel.DeviceArray(ctx, (B, A, C, T, 2, 2), np.uint8)
        _lib.call("bf_fill_random", out.ptr, out.nbytes, 17, q.handle)
        comm.scatter(band, out, B, A, C, T, q)
        ok, report = comm.verify(band, out, B, A, C, T, q)
        assert ok and report[0]["match"], report
        assert comm.stats() == (band.nbytes, band.nbytes)
    finally:
        comm.close()
