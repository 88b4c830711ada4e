"""Multi-process path on CPU (gloo, world size 2): the pieces of bench.py that are
about ranks -- stream sharding (one subset per rank, no data-path collective),
max-over-ranks timing and whole-job aggregation.  The per-rank "hot path" here is
the oracle (this is a CPU test of the orchestration, not of the kernels)."""
import os
import socket
import subprocess
import sys
import textwrap
from pathlib import Path

ROOT = Path(__file__).resolve().parent.parent

WORKER = textwrap.dedent("""
    import os, sys, json, time
    sys.path.insert(0, {root!r}); sys.path.insert(0, {root!r} + "/tests")
    import numpy as np
    import torch, torch.distributed as dist
    import navtex_amd as nv, oracle_binding as ob, signals
    rank, world = int(os.environ["RANK"]), int(os.environ["WORLD_SIZE"])
    dist.init_process_group("gloo", rank=rank, world_size=world)
    S, frames = 3, 3                                   # streams per rank (weak scaling)
    bits = {{}}
    t0 = time.perf_counter()
    for s in range(S):
        gid = rank * S + s                             # same sharding rule as bench.py
        st, _ = signals.stream_params(nv, gid, nv.RATE_IN)
        iq = nv.synth_host(st, nv.RATE_IN, frames * nv.FRAME_IN)
        p = ob.Pipe(chain_mask=1, charlayer=False); p.push(iq)
        bits[gid] = p.bits(0)
    elapsed = time.perf_counter() - t0 + 0.01 * rank   # make the ranks differ
    dist.barrier()
    t = torch.tensor([elapsed], dtype=torch.float64)
    dist.all_reduce(t, op=dist.ReduceOp.MAX)
    gathered = [None] * world
    dist.all_gather_object(gathered, bits)
    if rank == 0:
        merged = {{}}
        for g in gathered: merged.update(g)
        print(json.dumps({{"max_elapsed": float(t.item()), "own_elapsed": elapsed, "ids": sorted(merged), "bits": merged,
                          "value": world * S * frames * nv.FRAME_IN / float(t.item())}}))
    dist.destroy_process_group()
""")


def free_port():
    with socket.socket() as s:
        s.bind(("127.0.0.1", 0))
        return s.getsockname()[1]


def test_two_ranks_shard_streams_without_collective(tmp_path, nv, oracle):
    import json
    import signals
    script = tmp_path / "worker.py"
    script.write_text(WORKER.format(root=str(ROOT)))
    env = dict(os.environ, MASTER_ADDR="127.0.0.1", OMP_NUM_THREADS="1")
    out = subprocess.run([sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node=2", "--master-addr", "127.0.0.1",
                          "--master-port", str(free_port()), str(script)], env=env, capture_output=True, text=True, timeout=600)
    assert out.returncode == 0, out.stderr[-2000:]
    line = [l for l in out.stdout.splitlines() if l.startswith("{")][-1]
    rec = json.loads(line)
    assert rec["ids"] == ["0", "1", "2", "3", "4", "5"] or rec["ids"] == [0, 1, 2, 3, 4, 5]
    assert rec["max_elapsed"] >= rec["own_elapsed"]          # MAX over ranks, not rank 0's own time
    # every global stream decodes exactly as a single-process run decodes it
    for gid in range(6):
        st, _ = signals.stream_params(nv, gid, nv.RATE_IN)
        p = oracle.Pipe(chain_mask=1, charlayer=False)
        p.push(nv.synth_host(st, nv.RATE_IN, 3 * nv.FRAME_IN))
        assert rec["bits"][str(gid)] == p.bits(0)
    # (all six are still inside the phasing preamble after 3 frames, so the bit strings
    # are shifted copies of one pattern; what matters is that each id was decoded by
    # exactly one rank and matches the single-process result above)
    assert len(rec["bits"]) == 6


RANKS_WORKER = textwrap.dedent("""
    import os, sys, json
    sys.path.insert(0, {root!r}); sys.path.insert(0, {root!r} + "/tests")
    import torch, torch.distributed as dist
    import bench
    rank, world = int(os.environ["RANK"]), int(os.environ["WORLD_SIZE"])
    dist.init_process_group("gloo", rank=rank, world_size=world)
    ranks = bench.Ranks(torch, dist, None, "gloo")
    ranks.sync()
    # rank 1's shard "fails": the verdict of the job is the minimum over ranks, the count the sum, the time the maximum
    ok = rank != 1
    parity = ranks.reduce(1.0 if ok else 0.0, "min") > 0.5
    checked = int(ranks.reduce(32.0, "sum"))
    elapsed = ranks.reduce(1.0 + rank, "max")
    line = {{"parity": parity, "parity_streams_checked": checked, "elapsed": elapsed}}
    bench.finish(line, parity, ranks, rank)      # prints on rank 0, exits 3 on EVERY rank
""")


def test_every_rank_checks_itself_and_the_job_fails_when_one_does(tmp_path):
    """bench.py's rank logic on gloo, world size 2: parity = MIN over ranks, streams checked = SUM, time = MAX; a rank
    whose shard differs from the oracle fails the whole job (exit status 3 on every rank, line still printed)."""
    import json
    script = tmp_path / "ranks_worker.py"
    script.write_text(RANKS_WORKER.format(root=str(ROOT)))
    env = dict(os.environ, MASTER_ADDR="127.0.0.1")
    out = subprocess.run([sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node=2", "--master-addr", "127.0.0.1",
                          "--master-port", str(free_port()), str(script)], env=env, capture_output=True, text=True, timeout=600)
    assert out.returncode != 0
    rec = json.loads([l for l in out.stdout.splitlines() if l.startswith("{")][-1])
    assert rec == {"parity": False, "parity_streams_checked": 64, "elapsed": 2.0}


def test_host_placement_helpers():
    """bench.py binds a rank to its GPU's NUMA node before any GPU call and sizes the host pools from its share of the
    cores; on a box without GPUs (here) it must leave the affinity alone and still give a sane thread count."""
    sys.path.insert(0, str(ROOT))
    import bench, fullsize
    before = os.sched_getaffinity(0)
    assert bench._parse_cpulist("0-3,8,10-11\n") == {0, 1, 2, 3, 8, 10, 11}
    old = os.environ.pop("NVX_HOST_THREADS", None)
    try:
        place = bench.place_rank(0, 8, 0)
        assert os.sched_getaffinity(0) <= before and 1 <= place["threads"] <= 16
        assert os.environ["NVX_HOST_THREADS"] == str(place["threads"])
    finally:
        os.sched_setaffinity(0, before)
        os.environ.pop("NVX_HOST_THREADS", None)
        if old is not None:
            os.environ["NVX_HOST_THREADS"] = old
    assert fullsize.spread(4096, 32)[0] == 0 and fullsize.spread(4096, 32)[-1] == 4095 and len(fullsize.spread(4096, 32)) == 32
    assert fullsize.spread(5, 32) == [0, 1, 2, 3, 4]


import pytest


@pytest.mark.gpu
def test_two_ranks_on_one_gpu_run_the_hip_path_and_check_their_own_shards(tmp_path):
    """The real bench.py with two processes (gloo for the three scalars it reduces; RCCL refuses two ranks on one
    device), both on GPU 0, each with its own shard of global stream ids: every rank verifies 32 streams of ITS shard
    against the oracle and the line carries the minimum."""
    import json
    env = dict(os.environ, MASTER_ADDR="127.0.0.1", NVX_BENCH_BACKEND="gloo", NVX_BENCH_DEVICE="0", HSA_ENABLE_IPC_MODE_LEGACY="0")
    out = subprocess.run([sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node=2", "--master-addr", "127.0.0.1",
                          "--master-port", str(free_port()), str(ROOT / "bench.py"), "--gpus", "2", "--full", "--streams", "96", "--frames", "6",
                          "--steps", "2", "--warmup", "1", "--no-cpu"], env=env, capture_output=True, text=True, timeout=900)
    assert out.returncode == 0, out.stderr[-3000:]
    rec = json.loads([l for l in out.stdout.splitlines() if l.startswith("{")][-1])
    assert rec["n_gpus"] == 2 and rec["parity"] is True and rec["parity_streams_checked"] == 64
    assert rec["demod"]["near_ties"] == 0 and rec["host_threads"] >= 1
    assert rec["config"]["streams_per_gpu"] == 96 and rec["scaling"] == "weak"


SELF_LAUNCH_WORKER = textwrap.dedent("""
    import json, os, sys
    rank, world = int(os.environ["RANK"]), int(os.environ["WORLD_SIZE"])
    print("chatter from rank", rank)                     # must not reach the parent's stdout
    if rank == 0:
        print(json.dumps({"n_gpus": world, "argv": sys.argv[1:], "master": os.environ.get("MASTER_ADDR")}), flush=True)
    sys.exit(int(os.environ.get("NVX_TEST_EXIT", "0")))
""")


@pytest.mark.parametrize("status", [0, 3])
def test_bench_launches_its_own_ranks_and_relays_line_and_status(tmp_path, status):
    """`python bench.py --gpus N` with no launcher around it: bench.self_launch starts the ranks as a child
    (torch.distributed.run), hands its own arguments on, relays exactly the child's JSON line on stdout and the child's
    failure as a non-zero exit status.  (The ranks here are a stand-in script: no GPU in this container.)"""
    import json
    worker = tmp_path / "worker.py"
    worker.write_text(SELF_LAUNCH_WORKER)
    driver = tmp_path / "driver.py"
    driver.write_text(textwrap.dedent(f"""
        import sys, argparse
        sys.path.insert(0, {str(ROOT)!r})
        import bench
        bench.self_launch(argparse.Namespace(gpus=2), script={str(worker)!r}, argv=["--gpus", "2", "--steps", "7"])
    """))
    env = {k: v for k, v in os.environ.items() if k not in ("RANK", "WORLD_SIZE", "LOCAL_RANK")}
    env["NVX_TEST_EXIT"] = str(status)
    out = subprocess.run([sys.executable, str(driver)], capture_output=True, text=True, timeout=600, env=env)
    assert (out.returncode == 0) == (status == 0), out.stderr[-2000:]
    assert len(out.stdout.splitlines()) == 1, out.stdout
    rec = json.loads(out.stdout)
    assert rec == {"n_gpus": 2, "argv": ["--gpus", "2", "--steps", "7"], "master": "127.0.0.1"}
    assert "chatter from rank" in out.stderr


def test_bench_multi_gpu_without_launcher_reaches_the_ranks():
    """The real bench.py, `--gpus 2`, no launcher: it no longer refuses -- it starts two ranks, and what stops them HERE is
    only that this container has no GPU (the product has no CPU path); the failure comes back as the exit status."""
    out = subprocess.run([sys.executable, str(ROOT / "bench.py"), "--gpus", "2", "--streams", "8", "--frames", "2", "--steps", "1", "--warmup", "0"],
                         capture_output=True, text=True, timeout=600,
                         env={k: v for k, v in os.environ.items() if k not in ("RANK", "WORLD_SIZE", "LOCAL_RANK")})
    if out.returncode == 0:                              # on a GPU box with two devices the run simply succeeds
        import json
        assert json.loads(out.stdout.splitlines()[-1])["n_gpus"] == 2
    else:
        assert "launching" in out.stderr and "--nproc-per-node=2" in out.stderr
        assert "torch.distributed.run (one process per GPU)" not in out.stderr


@pytest.mark.gpu
def test_plain_bench_gpus_2_runs_two_ranks_on_one_gpu():
    """the command the driver uses for N = 1 works unchanged for N = 2 -- `python bench.py --gpus 2` with no
    launcher around it (gloo for the scalars and device 0 for both ranks: RCCL refuses two ranks on one device)."""
    import json
    env = {k: v for k, v in os.environ.items() if k not in ("RANK", "WORLD_SIZE", "LOCAL_RANK", "LOCAL_WORLD_SIZE")}
    env.update(NVX_BENCH_BACKEND="gloo", NVX_BENCH_DEVICE="0", HSA_ENABLE_IPC_MODE_LEGACY="0")
    out = subprocess.run([sys.executable, str(ROOT / "bench.py"), "--gpus", "2", "--full", "--streams", "96", "--frames", "6", "--steps", "2", "--warmup", "1", "--no-cpu"],
                         env=env, capture_output=True, text=True, timeout=900)
    assert out.returncode == 0, out.stderr[-3000:]
    assert len(out.stdout.splitlines()) == 1
    rec = json.loads(out.stdout)
    assert rec["n_gpus"] == 2 and rec["parity"] is True and rec["parity_streams_checked"] == 64
    r = rec["ranks"]
    assert r["world_size_seen"] == 2 and r["backend"] == "gloo" and r["parity_streams_checked_per_rank"] == [32, 32]
    assert len(r["ms_per_step_per_rank"]) == 2 and r["ms_per_step_min"] <= r["ms_per_step_max"] <= rec["ms_per_step"] * 1.5
    assert r["device_per_rank"] == [0, 0]


@pytest.mark.gpu
def test_rccl_calls_of_the_multi_gpu_run_on_one_gpu():
    """The N > 1 path talks to RCCL (torch's "nccl" backend) for its barrier, MAX / MIN / SUM and the per-rank gathers, on
    device tensors.  No multi-GPU box has run it yet (SCALE_r01 / r02: skipped), so rehearse exactly those calls with a
    process group of ONE rank on the one GPU there is: NVX_BENCH_FORCE_DIST=1 under the launcher the driver uses."""
    import json
    env = {k: v for k, v in os.environ.items() if k not in ("RANK", "WORLD_SIZE", "LOCAL_RANK", "LOCAL_WORLD_SIZE")}
    env.update(NVX_BENCH_FORCE_DIST="1", HSA_ENABLE_IPC_MODE_LEGACY="0")
    out = subprocess.run([sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node=1", "--master-addr", "127.0.0.1",
                          "--master-port", str(free_port()), str(ROOT / "bench.py"), "--gpus", "1", "--full", "--streams", "96", "--frames", "6",
                          "--steps", "2", "--warmup", "1", "--no-cpu", "--no-legs", "--no-stage0-extra", "--verify", "32"],
                         env=env, capture_output=True, text=True, timeout=900)
    assert out.returncode == 0, out.stderr[-3000:]
    rec = json.loads([l for l in out.stdout.splitlines() if l.startswith("{")][-1])
    assert rec["n_gpus"] == 1 and rec["parity"] is True
    assert rec["ranks"]["backend"] == "rccl" and rec["ranks"]["world_size_seen"] == 1 and rec["ranks"]["parity_streams_checked_per_rank"] == [32]
