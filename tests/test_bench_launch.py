"""bench.py's multi-rank launch (VERDICT r3 "next" 1): `--gpus N` from a plain
shell must run N rank processes itself, or fail; never a silent 1-rank line.

CPU tests run the launcher with `--launch-check` (the rendezvous alone, no GPU
work), from a plain shell and under torchrun; the GPU
test runs the real sharded bench with 2 ranks sharing the box's one GPU
through the library's host all-reduce transport (RCCL refuses one GPU twice)."""
import json
import os
import subprocess
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BENCH = os.path.join(ROOT, "bench.py")


def _env(**kw):
    env = {k: v for k, v in os.environ.items()
           if k not in ("WORLD_SIZE", "RANK", "LOCAL_RANK", "MASTER_ADDR", "MASTER_PORT")}
    env.update(kw)
    return env


def _json_lines(out):
    return [json.loads(l) for l in out.splitlines() if l.startswith("{")]


@pytest.mark.parametrize("n", [2, 3])
def test_gpus_n_spawns_n_ranks(n):
    p = subprocess.run([sys.executable, BENCH, "--gpus", str(n), "--launch-check"],
                       capture_output=True, text=True, timeout=240, env=_env())
    assert p.returncode == 0, p.stderr[-2000:]
    lines = _json_lines(p.stdout)
    assert len(lines) == 1, p.stdout  # rank 0 only
    assert lines[0]["n_gpus"] == n and lines[0]["ranks_counted"] == n


def test_torchrun_launch_runs_torch_free_workers():
    """The driver's N > 1 launch (`python -m torch.distributed.run ...
    bench.py --gpus N`): each torchrun rank joins gloo on the CPU only to
    publish rank 0's rendezvous port and runs its work in a child that never
    imports torch (tritd.rendezvous)."""
    import socket
    with socket.socket() as s:
        s.bind(("127.0.0.1", 0))
        port = s.getsockname()[1]
    p = subprocess.run([sys.executable, "-m", "torch.distributed.run", "--nnodes=1",
                        "--nproc-per-node", "2", "--master-addr", "127.0.0.1", "--master-port",
                        str(port), BENCH, "--gpus", "2", "--launch-check"],
                       capture_output=True, text=True, timeout=240, env=_env())
    assert p.returncode == 0, p.stderr[-3000:]
    lines = _json_lines(p.stdout)
    assert len(lines) == 1, p.stdout
    assert lines[0]["n_gpus"] == 2 and lines[0]["ranks_counted"] == 2
    assert lines[0]["torch_in_workers"] is False


def test_world_size_mismatch_fails_loudly():
    p = subprocess.run([sys.executable, BENCH, "--gpus", "2", "--launch-check"],
                       capture_output=True, text=True, timeout=120, env=_env(WORLD_SIZE="1"))
    assert p.returncode != 0
    assert "does not match WORLD_SIZE" in p.stderr


def test_single_gpu_needs_no_launcher():
    p = subprocess.run([sys.executable, BENCH, "--launch-check"], capture_output=True, text=True,
                       timeout=120, env=_env())
    assert p.returncode == 0, p.stderr[-2000:]
    assert _json_lines(p.stdout)[0]["n_gpus"] == 1


def _bench_module():
    import importlib.util
    spec = importlib.util.spec_from_file_location("tritd_bench", BENCH)
    m = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(m)
    return m


def test_dump_outputs_writes_a_fixed_sample_of_large_arrays(tmp_path):
    """--dump-outputs: small arrays whole, O and E above 16 MiB as the same
    2^21 column-major elements on every call, in the arrays' own precision."""
    import numpy as np
    b = _bench_module()
    rng = np.random.default_rng(5)
    n = (130, 129, 128)  # 130*129*128*8 B = 16.4 MiB: just above the whole-array limit
    res = dict(A=np.asfortranarray(rng.standard_normal((n[0], 2, 2))),
               B=np.asfortranarray(rng.standard_normal((2, n[1], 2))),
               C=np.asfortranarray(rng.standard_normal((2, 2, n[2]))),
               O=np.asfortranarray(rng.standard_normal(n)),
               E=np.asfortranarray(rng.standard_normal(n).astype(np.float32)),  # 8.2 MiB: whole
               errHist=rng.random(7), k=7)
    b.dump_outputs(str(tmp_path / "a"), res, 0, 1)
    b.dump_outputs(str(tmp_path / "b"), res, 0, 1)
    got = {f[:-4]: np.load(tmp_path / "a" / f) for f in os.listdir(tmp_path / "a")}
    assert sorted(got) == ["A", "B", "C", "E", "O", "errHist"]
    for k, v in got.items():
        assert v.dtype == res[k].dtype and v.dtype in (np.float32, np.float64)
        assert np.array_equal(v, np.load(tmp_path / "b" / (k + ".npy")))
    for k in ("A", "B", "C", "E", "errHist"):
        assert np.array_equal(got[k], res[k])
    idx = np.sort(np.random.default_rng(0).integers(0, res["O"].size, size=b.DUMP_SAMPLE))
    assert got["O"].shape == (b.DUMP_SAMPLE,)
    assert np.array_equal(got["O"], res["O"].ravel(order="F")[idx])
    assert sum(v.nbytes for v in got.values()) <= 64 << 20
    # N > 1: each rank names its shard
    b.dump_outputs(str(tmp_path / "c"), res, 1, 2)
    assert sorted(os.listdir(tmp_path / "c")) == sorted(k + "_rank1.npy" for k in got)


PLAIN_KEYS = {"metric", "value", "unit", "higher_is_better", "dtype", "ms_per_step", "steps",
              "warmup", "n_gpus", "config"}
FULL_ONLY_KEYS = {"rre_final", "k_final", "kernel_ms", "roofline", "cpu_baseline", "end_to_end",
                  "primitives", "config5", "per_rank", "placement_probe"}


@pytest.mark.gpu
def test_plain_bench_dumps_the_last_timed_step(tmp_path):
    """A plain run (no --full) prints the headline line only, and
    --dump-outputs holds what the session returns after warmup + steps
    iterations: the same arrays as a session run here on the same inputs for
    that many iterations, bit for bit (O and E of 129^3 * 8 B = 16.4 MiB, the
    smallest cube above the 16 MiB limit and an odd side, are dumped as the
    sample)."""
    import numpy as np
    import tritd
    n1, r, W, K = 129, 8, 5, 40  # the benchmark's default warm-up and steps
    out = tmp_path / "dump"
    p = subprocess.run([sys.executable, "-u", BENCH, "--n", str(n1), "--steps", str(K),
                        "--warmup", str(W), "--dump-outputs", str(out)],
                       capture_output=True, text=True, timeout=300, env=_env())
    assert p.returncode == 0, p.stderr[-4000:]
    lines = _json_lines(p.stdout)
    assert len(lines) == 1, p.stdout
    line = lines[0]
    assert PLAIN_KEYS <= set(line) and not (FULL_ONLY_KEYS & set(line)), sorted(line)
    assert line["full"] is False and line["steps"] == K and line["warmup"] == W
    assert line["unit"] == "iters/s" and line["higher_is_better"] is True and line["dtype"] == "f64"
    assert line["value"] > 0
    assert abs(line["ms_per_step"] * line["value"] - 1e3) < 1e-6 * 1e3
    got = {f[:-4]: np.load(out / f) for f in os.listdir(out)}
    assert sorted(got) == ["A", "B", "C", "E", "O", "errHist"]
    assert len(got["errHist"]) == W + K  # the state after the last timed step

    b = _bench_module()
    D, _, A0, B0, C0 = b.make_data(4, n1, n1, n1, r, (0, n1), want_L=False)
    from tritd import synth
    s = tritd.Session(r, dict(synth.TRAFFIC_OPTS, maxIter=100), A0, B0, C0, n1=n1, n2=n1, n3=n1,
                      D=D, device=0)
    s.run(W + K)
    s.sync()
    ref = s.get()
    s.close()
    for k in ("A", "B", "C", "errHist"):
        assert np.array_equal(got[k], ref[k]), k
    idx = np.sort(np.random.default_rng(0).integers(0, ref["O"].size, size=b.DUMP_SAMPLE))
    for k in ("O", "E"):
        assert got[k].dtype == np.float64
        assert np.array_equal(got[k], ref[k].ravel(order="F")[idx]), k
    assert all(np.isfinite(v).all() for v in got.values())


@pytest.mark.gpu
def test_plain_bench_outputs_repeat_and_steps_count(tmp_path):
    """Two plain runs with the same arguments dump identical arrays; --steps
    sets the number of timed iterations also past the solver's 100-iteration
    horizon (errHist has warmup + steps entries)."""
    import numpy as np
    W, K = 3, 110
    outs = []
    for name in ("a", "b"):
        out = tmp_path / name
        p = subprocess.run([sys.executable, "-u", BENCH, "--n", "40", "--steps", str(K),
                            "--warmup", str(W), "--dump-outputs", str(out)],
                           capture_output=True, text=True, timeout=300, env=_env())
        assert p.returncode == 0, p.stderr[-4000:]
        line = _json_lines(p.stdout)[0]
        assert line["steps"] == K and line["config"]["maxIter"] == W + K
        outs.append({f[:-4]: np.load(out / f) for f in os.listdir(out)})
    assert len(outs[0]["errHist"]) == W + K
    assert outs[0]["O"].shape == (40, 40, 40)  # small outputs are dumped whole
    for k in outs[0]:
        assert np.array_equal(outs[0][k], outs[1][k]), k


@pytest.mark.gpu
def test_bench_two_ranks_from_plain_shell():
    """The whole sharded bench, 2 ranks, started as `python3 bench.py --gpus 2`."""
    p = subprocess.run([sys.executable, "-u", BENCH, "--gpus", "2", "--comm", "host", "--full",
                        "--no-cpu", "--no-e2e", "--n", "64", "--steps", "4", "--warmup", "1"],
                       capture_output=True, text=True, timeout=600, env=_env())
    assert p.returncode == 0, p.stderr[-4000:]
    lines = _json_lines(p.stdout)
    assert len(lines) == 1, p.stdout
    line = lines[0]
    assert line["n_gpus"] == 2
    assert line["comm"] == {"transport": "host", "nranks": 2}
    assert line["hip_runtimes_mapped"] == 1 and "/opt/rocm" in line["hip_runtime"]
    assert line["value"] > 0 and line["rre_final"] < 1e-3
    # the per-rank breakdown: each rank's rows, iteration,
    # all-reduce and compute ms, two all-reduces per iteration
    pr = line["per_rank"]
    assert [p["rank"] for p in pr] == [0, 1] and sum(p["rows"] for p in pr) == 64
    for p in pr:
        assert p["allreduces_per_iteration"] == 2
        assert 0 < p["allreduce_ms"] < p["iteration_ms"]
        assert abs(p["compute_ms"] + p["allreduce_ms"] - p["iteration_ms"]) < 1e-9


@pytest.mark.gpu
def test_bench_two_ranks_under_torchrun():
    """The driver's own N > 1 command shape (`python -m torch.distributed.run
    --nnodes=1 --nproc-per-node N --master-addr 127.0.0.1 --master-port P
    bench.py --gpus N ...`), 2 ranks sharing the box's GPU over the host
    transport: torchrun's rank processes publish the rendezvous port over gloo
    and run the GPU work in torch-free workers; the line reports one HIP / HSA
    / RCCL copy each, from /opt/rocm, in rank 0's worker."""
    import socket
    with socket.socket() as s:
        s.bind(("127.0.0.1", 0))
        port = s.getsockname()[1]
    p = subprocess.run([sys.executable, "-m", "torch.distributed.run", "--nnodes=1",
                        "--nproc-per-node", "2", "--master-addr", "127.0.0.1", "--master-port",
                        str(port), BENCH, "--gpus", "2", "--comm", "host", "--full", "--no-cpu",
                        "--no-e2e", "--side", "64", "--steps", "4", "--warmup", "1"],
                       capture_output=True, text=True, timeout=600, env=_env())
    assert p.returncode == 0, p.stderr[-4000:]
    lines = _json_lines(p.stdout)
    assert len(lines) == 1, p.stdout
    line = lines[0]
    assert line["n_gpus"] == 2 and line["comm"] == {"transport": "host", "nranks": 2}
    assert line["value"] > 0 and line["rre_final"] < 1e-3
    st = line["runtime_stack"]
    assert all(len(v) == 1 and v[0].startswith("/opt/rocm") for v in st.values()), st
