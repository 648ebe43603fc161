"""GPU: the multi-rank path on what one GPU can show.

  * libmcle's own RCCL communicator (csrc/comm.hip) with a world of one: id, init, counter all-reduce, destroy;
  * two PROCESSES sharing device 0, exchanging through gloo (RCCL refuses two ranks on one device), running the real
    fused pipelines through BatchedSimulationRunner: integer counters and every Result identical to the one-rank
    run (identical integer counters for any device count), with ONE reduction per SNR."""
import json
import os
import socket
import sys

import numpy as np
import pytest

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
pytestmark = pytest.mark.gpu


def _free_port():
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    port = s.getsockname()[1]
    s.close()
    return port


def test_native_rccl_communicator_single_rank(engine):
    from pyphysim_amd.distributed import NativeComm
    comm = NativeComm(engine, rank=0, world=1)
    try:
        assert engine.comm_info() == (0, 1)
        c = dict(n_realizations=7, n_skipped=1, sym_errors=123, sym_errors_sq=4567, bit_errors=89, bit_errors_sq=1011,
                 n_symbols=4096, n_bits=24576)
        # with a communicator -- even of one rank -- mcle_counters_allreduce runs k_counters_pack, the grouped in-place
        # SUM / MAX ncclAllReduce pair and k_counters_unpack (the early return for world == 1 left all of that
        # unexecuted on a one-GPU box); several blocks at once, values near 2^64 to catch a mis-typed reduction
        assert comm.allreduce_counters(c) == c
        rs = np.random.RandomState(4)
        n = 37
        host = rs.randint(0, 2 ** 63, size=(n, 8), dtype=np.uint64) * np.uint64(2) + np.uint64(1)
        cnt = engine.zeros(n, np.dtype((np.void, 64)))
        cnt.set(np.ascontiguousarray(host).view(np.dtype((np.void, 64))).reshape(n))
        engine.counters_allreduce(cnt, n)
        back = np.frombuffer(cnt.get().tobytes(), dtype=np.uint64).reshape(n, 8)
        assert np.array_equal(back, host)
        assert comm.allreduce_floats([1.5, -2.25]) == [1.5, -2.25]
        # integers travel through the uint64 counter reduction: exact beyond 2^53, negatives included
        big = [3, 1 << 40, (1 << 62) + 12345678901, -7, -(1 << 61) - 1, 0, (1 << 63) - 1, 5, 6, 7, 8, 9, 10]
        assert comm.broadcast_ints(big) == big
        with pytest.raises(Exception):
            engine.comm_init(b"\0" * 128, 0, 1)             # a context holds one communicator
    finally:
        comm.close()
    assert engine.comm_info() == (0, 1)
    # (every id drawn starts an RCCL bootstrap listener that lives until all ranks have joined: ids are only drawn
    # to be used -- NativeComm above consumed the one it drew)


def _native_worker(rank, world, port, out_path):
    """One rank of a NativeComm world on ITS OWN GPU: libmcle's RCCL communicator end to end."""
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port), RANK=str(rank), WORLD_SIZE=str(world),
                      LOCAL_RANK=str(rank), HSA_ENABLE_IPC_MODE_LEGACY="0")
    sys.path.insert(0, REPO)
    from pyphysim_amd.engine import Engine
    from pyphysim_amd.distributed import NativeComm
    eng = Engine(rank, "f32")
    comm = NativeComm(eng, rank=rank, world=world)
    try:
        c = dict(n_realizations=10 + rank, n_skipped=rank, sym_errors=100 * (rank + 1), sym_errors_sq=(1 << 60) + rank,
                 bit_errors=7, bit_errors_sq=9, n_symbols=4096 if rank == 0 else 0, n_bits=24576 if rank == 0 else 0)
        red = comm.allreduce_counters(c)
        ints = comm.broadcast_ints([(1 << 62) + 5, -3, 17] if rank == 0 else [0, 0, 0])
        fl = comm.allreduce_floats([1.0 + rank, 0.5])
        with open("%s.%d" % (out_path, rank), "w") as fh:
            json.dump({"red": red, "ints": ints, "fl": fl}, fh)
    finally:
        comm.close()
        eng.close()


@pytest.mark.timeout(600)
def test_native_rccl_communicator_two_ranks_on_two_gpus(tmp_path):
    """mcle_comm_init / mcle_counters_allreduce / mcle_allreduce_f64 with world = 2, one process per
    GPU (skipped on a one-GPU box: RCCL refuses two ranks on one device)."""
    from pyphysim_amd import _lib
    if _lib.device_count() < 2:
        pytest.skip("needs two GPUs")
    import torch.multiprocessing as mp
    out = str(tmp_path / "native2")
    mp.spawn(_native_worker, args=(2, _free_port(), out), nprocs=2, join=True)
    got = [json.load(open("%s.%d" % (out, r))) for r in range(2)]
    assert got[0] == got[1]
    assert got[0]["red"] == dict(n_realizations=21, n_skipped=1, sym_errors=300, sym_errors_sq=(1 << 61) + 1, bit_errors=14,
                                 bit_errors_sq=18, n_symbols=4096, n_bits=24576)
    assert got[0]["ints"] == [(1 << 62) + 5, -3, 17] and got[0]["fl"] == [3.0, 1.0]


def _worker(rank, world, port, out_path, which):
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port), RANK=str(rank), WORLD_SIZE=str(world),
                      LOCAL_RANK="0")
    sys.path.insert(0, REPO)
    import torch
    import torch.distributed as dist
    torch.cuda.set_device(0)
    if world > 1:
        dist.init_process_group("gloo", rank=rank, world_size=world)
    try:
        from pyphysim_amd import simulators
        if which == "mimo":
            sim = simulators.MimoOfdmSimulator([18.0, 25.0], M=64, rep_max=3000, batch_size=512 // world, seed=11,
                                               dtype="f32")
            names = ("ser", "ber", "symbol_errors", "bit_errors", "num_symbols", "num_skipped_reps")
        else:
            sim = simulators.IaSimulator([10.0, 20.0], M=16, NSymbs=100, solver="max_sinr", max_iterations=20,
                                         rep_max=4000, batch_size=1024 // world, seed=5, dtype="f32")
            names = ("ser", "ber", "symbol_errors", "sum_capacity", "ia_runned_iterations")
        sim.simulate()
        state = {n: [r.to_dict() for r in sim.results[n]] for n in names}
        with open("%s.%d" % (out_path, rank), "w") as fh:
            json.dump({"state": state, "reps": sim.runned_reps, "n_reductions": sim.n_reductions}, fh)
    finally:
        if world > 1:
            dist.destroy_process_group()


def _run(world, tmp_path, which):
    import torch.multiprocessing as mp
    out = str(tmp_path / ("%s%d" % (which, world)))
    mp.spawn(_worker, args=(world, _free_port(), out, which), nprocs=world, join=True)
    return [json.load(open("%s.%d" % (out, r))) for r in range(world)]


@pytest.mark.timeout(600)
def test_two_ranks_of_the_fused_config4_pipeline_equal_one_rank(tmp_path):
    one = _run(1, tmp_path, "mimo")[0]
    two = _run(2, tmp_path, "mimo")
    assert two[0]["state"] == two[1]["state"] == one["state"]
    assert two[0]["reps"] == one["reps"] == [3000, 3000]
    assert two[0]["n_reductions"] == 2                      # one all-reduce per SNR point


def _close(a, b):
    if isinstance(a, dict):
        return all(_close(a[k], b[k]) for k in a)
    if isinstance(a, float):
        return abs(a - b) <= 1e-9 * max(1.0, abs(b))
    return a == b


@pytest.mark.timeout(600)
def test_two_ranks_of_the_ia_pipeline_keep_the_capacity_results(tmp_path):
    """sum_capacity / ia_runned_iterations are carried with the counters, so sharding no
    longer divides a local sum by the global realization count."""
    one = _run(1, tmp_path, "ia")[0]
    two = _run(2, tmp_path, "ia")
    for name in ("ser", "ber", "symbol_errors", "ia_runned_iterations"):
        assert two[0]["state"][name] == one["state"][name], name
    for a, b in zip(two[0]["state"]["sum_capacity"], one["state"]["sum_capacity"]):
        assert _close(a, b), (a, b)                         # float sums: association differs, value does not
    cap = one["state"]["sum_capacity"][1]
    assert cap["num_updates"] == 4000 and 5.0 < cap["value"] / cap["total"] < 40.0


@pytest.mark.timeout(900)
def test_bench_under_the_drivers_launch_line_runs_the_rccl_allreduce():
    """`python -m torch.distributed.run --nproc-per-node 1 ... bench.py --gpus 1` (the driver's multi-GPU launch line with one
    rank): the RCCL process group comes up, the counter all-reduce runs inside every timed region, and the line says so --
    while a plain `python bench.py` run reports no exchange at all."""
    import json
    import subprocess
    import sys
    repo = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    common = ["--gpus", "1", "--steps", "2", "--warmup", "1", "--batch", "4096", "--full", "--no-cpu", "--pmc", "off",
              "--preroll-ms", "0", "--single-demod"]
    env = {k: v for k, v in os.environ.items() if k not in ("RANK", "LOCAL_RANK", "WORLD_SIZE", "MASTER_PORT")}
    env["HSA_ENABLE_IPC_MODE_LEGACY"] = "0"
    out = subprocess.run([sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node", "1",
                          "--master-addr", "127.0.0.1", "--master-port", "29541", os.path.join(repo, "bench.py")] + common,
                         env=env, capture_output=True, text=True, timeout=600)
    assert out.returncode == 0, out.stderr[-3000:]
    line = json.loads([l for l in out.stdout.splitlines() if l.startswith("{")][-1])
    assert line["rccl"]["process_group"] is True and line["rccl"]["backend"] == "nccl"
    assert line["rccl"]["rccl_world_size"] == 1 and line["rccl"]["allreduce_calls_in_timed_regions"] >= 1
    assert "RCCL" in line["config"]["exchange"] and line["n_gpus"] == 1 and line["value"] > 0
    # the timed exchange is the PRODUCT's: NativeComm -> mcle_counters_allreduce on the context stream (--comm auto)
    assert line["rccl"]["exchange_impl"].startswith("native") and line["rccl"]["native_comm"]["world"] == 1
    assert "mcle_counters_allreduce" in line["config"]["exchange"]
    # the strong leg: the configuration's literal total (config 4: 10^6) on the one rank
    st = line["strong"]
    assert st["total_realizations"] == 10 ** 6 and st["per_rank_realizations"] == [10 ** 6] and st["value"] > 1e6
    assert abs(st["efficiency"] - 1.0) < 1e-9 and st["ser"] > 0
    # the alternative exchange is still there and says so
    alt = subprocess.run([sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node", "1",
                          "--master-addr", "127.0.0.1", "--master-port", "29543", os.path.join(repo, "bench.py")] + common +
                         ["--comm", "torch", "--strong-reps", "0"], env=env, capture_output=True, text=True, timeout=600)
    assert alt.returncode == 0, alt.stderr[-3000:]
    a = json.loads([l for l in alt.stdout.splitlines() if l.startswith("{")][-1])
    assert a["rccl"]["exchange_impl"].startswith("torch") and "strong" not in a and a["ser"] == line["ser"]
    assert line["rccl"]["ranks"][0]["device"]
    plain = subprocess.run([sys.executable, os.path.join(repo, "bench.py")] + common, env=env, capture_output=True,
                           text=True, timeout=600)
    assert plain.returncode == 0, plain.stderr[-3000:]
    p = json.loads([l for l in plain.stdout.splitlines() if l.startswith("{")][-1])
    assert p["rccl"]["process_group"] is False and p["rccl"]["allreduce_calls_in_timed_regions"] == 0
    assert p["config"]["exchange"].startswith("none")
    # the integer counters behind both lines are the same realizations: same SER to the last digit
    assert p["ser"] == line["ser"]


@pytest.mark.timeout(900)
def test_bench_two_rank_code_path_on_one_gpu():
    """The N > 1 branch of bench.py -- disjoint contiguous ranges per rank, the all-reduce inside the timed region, the
    rank-0-alone leg (n1_value), per-rank devices and kernel times -- executed end to end with two ranks sharing the one GPU
    (gloo: RCCL refuses two ranks on a device; never a scaling figure).  The reduced counters must be those of the one-rank
    run over the same index range."""
    import json
    import subprocess
    import sys
    repo = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    env = {k: v for k, v in os.environ.items() if k not in ("RANK", "LOCAL_RANK", "WORLD_SIZE", "MASTER_PORT")}
    env["HSA_ENABLE_IPC_MODE_LEGACY"] = "0"
    common = ["--warmup", "1", "--batch", "4096", "--full", "--no-cpu", "--pmc", "off", "--preroll-ms", "0", "--single-demod"]
    two = subprocess.run([sys.executable, os.path.join(repo, "bench.py"), "--gpus", "2", "--steps", "2", "--dist-backend", "gloo",
                          "--share-gpus", "--strong-total", "20000", "--strong-reps", "2"] + common, env=env, capture_output=True, text=True, timeout=800)
    assert two.returncode == 0, two.stderr[-3000:]
    lines = [l for l in two.stdout.splitlines() if l.startswith("{")]
    assert len(lines) == 1                                                  # ONE JSON line, from rank 0
    t = json.loads(lines[0])
    assert t["n_gpus"] == 2 and t["rccl"]["rccl_world_size"] == 2 and t["rccl"]["backend"] == "gloo"
    assert t["config"]["rank_ranges"] == [[0, 8192], [8192, 16384]]
    assert [r["rank"] for r in t["rccl"]["ranks"]] == [0, 1] and all(r["device"] for r in t["rccl"]["ranks"])
    assert t["n1_value"] > 0 and t["kernel_ms_per_rank"]["min"] > 0 and t["kernel_ms_per_rank"]["max"] >= t["kernel_ms_per_rank"]["min"]
    assert t["rccl"]["allreduce_calls_in_timed_regions"] >= 2               # the two-rank region and the rank-0-alone region
    assert t["rccl"]["exchange_impl"].startswith("torch")                    # gloo: two ranks share one device, no RCCL
    st = t["strong"]                                                         # 20 000 realizations cut in two
    assert st["total_realizations"] == 20000 and st["per_rank_realizations"] == [10000, 10000]
    assert st["n1_value"] > 0 and st["value"] > 0 and 0.0 < st["efficiency"] < 2.0
    one = subprocess.run([sys.executable, os.path.join(repo, "bench.py"), "--gpus", "1", "--steps", "4"] + common, env=env,
                         capture_output=True, text=True, timeout=800)
    assert one.returncode == 0, one.stderr[-3000:]
    o = json.loads([l for l in one.stdout.splitlines() if l.startswith("{")][-1])
    assert o["config"]["rank_ranges"] == [[0, 16384]]
    assert o["ser"] == t["ser"] and o["ber"] == t["ber"]                      # same realizations, same integer counters


@pytest.mark.timeout(1500)
def test_bench_eight_rank_code_path_on_one_gpu():
    """the driver's N = 8 shape with REAL kernels on the one GPU these boxes have -- eight gloo ranks sharing
    the device, eight contiguous index ranges, the counter all-reduce inside the timed region, and the `strong` blocks of
    config 4 and config 5 cut in eight.  The reduced counters must be those of a ONE-rank job over the same index ranges (same
    SER / BER to the last digit, weak leg and both strong legs).  Never a scaling figure."""
    import json
    import subprocess
    import sys
    repo = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    env = {k: v for k, v in os.environ.items() if k not in ("RANK", "LOCAL_RANK", "WORLD_SIZE", "MASTER_PORT")}
    env["HSA_ENABLE_IPC_MODE_LEGACY"] = "0"
    common = ["--warmup", "1", "--full", "--no-cpu", "--pmc", "off", "--preroll-ms", "0", "--single-demod", "--dist-backend", "gloo",
              "--strong-total", "20001", "--strong-reps", "1"]
    eight = subprocess.run([sys.executable, os.path.join(repo, "bench.py"), "--gpus", "8", "--steps", "1", "--batch", "2048",
                            "--share-gpus"] + common, env=env, capture_output=True, text=True, timeout=1400)
    assert eight.returncode == 0, eight.stderr[-3000:]
    lines = [l for l in eight.stdout.splitlines() if l.startswith("{")]
    assert len(lines) == 1                                                  # ONE JSON line, from rank 0
    t = json.loads(lines[0])
    assert t["n_gpus"] == 8 and t["rccl"]["rccl_world_size"] == 8 and t["rccl"]["backend"] == "gloo"
    assert t["config"]["rank_ranges"] == [[2048 * r, 2048 * (r + 1)] for r in range(8)]
    assert [r["rank"] for r in t["rccl"]["ranks"]] == list(range(8))
    assert t["rccl"]["exchange_impl"].startswith("torch")                    # gloo: eight ranks on one device, no RCCL
    st, s5 = t["strong"], t["strong_c5"]
    assert st["total_realizations"] == 20001 and len(st["per_rank_realizations"]) == 8 and sum(st["per_rank_realizations"]) == 20001
    assert max(st["per_rank_realizations"]) - min(st["per_rank_realizations"]) <= 1          # 20001 = 8 x 2500 + 1: a ragged cut
    assert s5["config"] == "c5" and len(s5["per_rank_realizations"]) == 8 and sum(s5["per_rank_realizations"]) == s5["total_realizations"]
    # the same index ranges on ONE rank of a torch.distributed job (RANK / WORLD_SIZE set: the strong legs exist there too)
    env1 = dict(env, RANK="0", LOCAL_RANK="0", WORLD_SIZE="1", MASTER_ADDR="127.0.0.1", MASTER_PORT="29533")
    one = subprocess.run([sys.executable, os.path.join(repo, "bench.py"), "--gpus", "1", "--steps", "4", "--batch", "4096"] + common,
                         env=env1, capture_output=True, text=True, timeout=800)
    assert one.returncode == 0, one.stderr[-3000:]
    o = json.loads([l for l in one.stdout.splitlines() if l.startswith("{")][-1])
    assert o["config"]["rank_ranges"] == [[0, 16384]]
    assert o["ser"] == t["ser"] and o["ber"] == t["ber"]                      # weak leg: same realizations, same integer counters
    assert o["strong"]["ser"] == st["ser"] and o["strong_c5"]["ser"] == s5["ser"]   # strong legs: 8 shares = the whole
