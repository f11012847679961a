"""bench.py's multi-GPU launch contract without a GPU, and the host transport of the C exchange.

  * `bench.py --gpus 2` started without a torchrun environment launches 2 ranks itself (one
    process per GPU), which rendezvous and report n_gpus = 2 (dry run: gloo, a CPU stand-in step);
  * a WORLD_SIZE that contradicts --gpus is refused (no 1-GPU line passed off as N GPUs);
  * backuwup_amd.comm.gloo_all_to_all, the host all-to-all handed to bw_comm_init_host in the
    multi-process GPU tests, delivers send[r] of every rank to rank r (world 2 and 4, gloo).
"""
import json
import os
import socket
import subprocess
import sys

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)


def _env(**kw):
    env = {k: v for k, v in os.environ.items() if k not in ("WORLD_SIZE", "RANK", "LOCAL_RANK", "MASTER_ADDR",
                                                           "MASTER_PORT")}
    env.update(kw)
    return env


@pytest.mark.parametrize("n", [2, 4])
def test_bench_gpus_n_launches_n_ranks(n):
    out = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", str(n), "--dry-run", "--no-power",
                          "--steps", "2", "--warmup", "1"], env=_env(), capture_output=True, text=True, timeout=300)
    assert out.returncode == 0, out.stderr[-3000:]
    lines = [l for l in out.stdout.splitlines() if l.startswith("{")]
    assert len(lines) == 1, out.stdout  # rank 0 prints the one line
    rec = json.loads(lines[0])
    assert rec["n_gpus"] == n and rec["dry_run"] is True and rec["value"] is None
    assert rec["config"]["parallelism"] == "dp%d" % n


def test_bench_rank_failure_exits_nonzero():
    """one rank of `bench.py --gpus 2` dies after warmup while its peer waits in the
    timing barrier; the launcher tears the survivor down and exits non-zero (no hang, no line)."""
    import time
    t0 = time.time()
    out = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "2", "--dry-run", "--no-power",
                          "--steps", "2", "--warmup", "1", "--dry-run-fail-rank", "1"], env=_env(),
                         capture_output=True, text=True, timeout=240)
    assert out.returncode != 0, out.stderr[-3000:]
    assert not [l for l in out.stdout.splitlines() if l.startswith("{")]
    assert time.time() - t0 < 200


def test_bench_refuses_world_mismatch():
    out = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "2", "--dry-run", "--no-power"],
                         env=_env(WORLD_SIZE="1", RANK="0", LOCAL_RANK="0"), capture_output=True, text=True,
                         timeout=120)
    assert out.returncode != 0
    assert "refusing" in out.stderr


def test_dump_outputs_is_exact_and_bounded(tmp_path):
    """--dump-outputs: every field of the blob record comes back bit for bit from the float arrays
    (the 64-bit gear hash from its halves); a batch past the row cap is a fixed sample, within 64 MB."""
    sys.path.insert(0, ROOT)
    import bench
    from backuwup_amd import BLOB_DTYPE
    rng = np.random.default_rng(7)
    n = 1000
    res = np.zeros(n, dtype=BLOB_DTYPE)
    res["file"] = np.arange(n) // 3
    res["offset"] = rng.integers(0, 1 << 44, n, dtype=np.uint64)
    res["length"] = rng.integers(1, 3 << 20, n, dtype=np.uint64)
    res["gear_hash"] = rng.integers(0, 1 << 64, n, dtype=np.uint64)
    res["gear_hash"][0] = 0xFFFFFFFFFFFFFFFF
    res["digest"] = rng.integers(0, 256, (n, 32), dtype=np.uint8)
    res["is_dup"] = rng.integers(0, 2, n, dtype=np.uint8)
    d = str(tmp_path / "whole")
    bench.dump_outputs(d, res, 0, 1)
    got = {f[:-4]: np.load(os.path.join(d, f)) for f in os.listdir(d)}
    assert sorted(got) == ["digest", "file", "gear_hash_hi", "gear_hash_lo", "is_dup", "length", "offset", "row"]
    assert all(a.dtype in (np.float32, np.float64) for a in got.values())
    assert np.array_equal(got["row"], np.arange(n))
    for f in ("file", "offset", "length", "digest", "is_dup"):
        assert np.array_equal(got[f].astype(BLOB_DTYPE[f].base), res[f]), f
    gear = (got["gear_hash_hi"].astype(np.uint64) << np.uint64(32)) | got["gear_hash_lo"].astype(np.uint64)
    assert np.array_equal(gear, res["gear_hash"])
    # past the cap: the same rows on every call, ascending, and under 64 MB on disk for the whole job
    big = np.zeros(bench.DUMP_MAX_ROWS + 5000, dtype=BLOB_DTYPE)
    big["offset"] = np.arange(len(big))
    sizes = []
    for k in ("a", "b"):
        d = str(tmp_path / k)
        bench.dump_outputs(d, big, 0, 1)
        sizes.append(sum(os.path.getsize(os.path.join(d, f)) for f in os.listdir(d)))
    rows = np.load(str(tmp_path / "a" / "row.npy"))
    assert len(rows) == bench.DUMP_MAX_ROWS and np.all(np.diff(rows) > 0)
    assert np.array_equal(rows, np.load(str(tmp_path / "b" / "row.npy")))
    assert np.array_equal(np.load(str(tmp_path / "a" / "offset.npy")), rows)
    assert sizes[0] == sizes[1] <= 64 * 1000 * 1000
    bench.dump_outputs(str(tmp_path / "r1"), res, 1, 2)  # a second rank's files carry its rank
    assert "rank1_digest.npy" in os.listdir(str(tmp_path / "r1"))


def test_bench_full_and_dump_options_parse():
    """--full and --dump-outputs are options of the one command line (dry run: nothing to dump)."""
    out = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--dry-run", "--full",
                          "--steps", "2", "--warmup", "1"], env=_env(), capture_output=True, text=True, timeout=120)
    assert out.returncode == 0, out.stderr[-3000:]
    rec = json.loads([l for l in out.stdout.splitlines() if l.startswith("{")][0])
    assert rec["steps"] == 2 and rec["ms_per_step"] > 0


def _a2a_worker(rank, world, port, q):
    import torch.distributed as dist
    from backuwup_amd.comm import gloo_all_to_all
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port))
    dist.init_process_group("gloo", rank=rank, world_size=world)
    try:
        b = 40
        send = np.zeros(world * b, dtype=np.uint8)
        for r in range(world):
            send[r * b:(r + 1) * b] = (rank * 16 + r) + np.arange(b, dtype=np.uint8)
        recv = np.zeros_like(send)
        gloo_all_to_all()(send, recv, b)
        q.put((rank, recv.tolist()))
    finally:
        dist.destroy_process_group()


@pytest.mark.parametrize("world", [2, 4])
def test_gloo_host_all_to_all(world):
    import torch.multiprocessing as mp
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    port = s.getsockname()[1]
    s.close()
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    procs = [ctx.Process(target=_a2a_worker, args=(r, world, port, q)) for r in range(world)]
    for p in procs:
        p.start()
    got = dict(q.get(timeout=120) for _ in range(world))
    for p in procs:
        p.join(timeout=60)
        assert p.exitcode == 0
    b = 40
    for r in range(world):
        recv = np.array(got[r], dtype=np.uint8)
        for src in range(world):
            assert recv[src * b:(src + 1) * b].tolist() == ((src * 16 + r) + np.arange(b, dtype=np.uint8)).tolist()
