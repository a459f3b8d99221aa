"""TriTD-ADMM benchmark: ADMM iterations/s + final RRE on the synthetic
512x512x512 r=8 fp64 workload (BASELINE.json configs[3] = SURVEY.md §8d
config 4, the default) or the 2048x2048x256 r=16 fp32 workload
(configs[4] = config 5, ``--config 5``).

    python bench.py [--gpus N] [--steps K] [--warmup W] [--config 2|3|4|5] [--algo admm|als]
                    [--dump-outputs DIR] [--full]
    python -m torch.distributed.run --nproc-per-node N ... bench.py --gpus N

A "step" is one ADMM iteration (triple_decomp_ADMM.m:31-66) over the whole
tensor, device-resident.  With N > 1 ranks the tensor is sharded along
mode 1 and the two per-iteration all-reduces run over RCCL
(strong scaling: the problem size is fixed).  `--gpus N` without a launcher
starts the N rank processes itself.  Rank 0 prints one JSON
line.

A plain run does what the headline figure needs and no more: it draws the
inputs, creates the session, runs W warm-up and K timed iterations, and prints
the line (iterations/s, ms_per_step, the workload).  `--dump-outputs DIR`
also writes what the session returns after the last timed iteration (A, B, C,
O, E, errHist) as DIR/<name>.npy.  Everything else is behind `--full`: the
HIP-event passes and the roofline, the rest of the 100-iteration solve and its
RRE, the per-rank breakdown, the end-to-end one-shot calls, the primitive
kernels, the config-5 leg, and the CPU baseline, which is the C restatement of
the MATLAB reference (oracle/tritd_ref.c, kind "port") timed on rank 0.
"""
import argparse
import json
import os
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.abspath(__file__))
PKG = os.path.join(ROOT, "triple-tensor-decomposition-with-admm_amd")
sys.path.insert(0, PKG)

import numpy as np  # noqa: E402

HBM_PEAK_GBS = 8000.0  # MI355X_MICROARCH.md: HBM3E 8.0 TB/s spec
F32_MFMA_PEAK_TFS = 157.3  # MI355X_MICROARCH.md: f32-input MFMA, dense
F64_MFMA_PEAK_TFS = 78.6  # MI355X_MICROARCH.md: f64 MFMA, dense
# SURVEY.md §8d workloads: (n1, n2, n3, r, dtype)
# (configs 2 and 3 are the reference's real-data experiments, run on
# synthetic stand-ins of their shapes: tritd.synth.sensor_like / video_like)
CONFIGS = {2: (54, 4, 1152, 5, "f64"), 3: (240, 320, 300, 5, "f64"),
           4: (512, 512, 512, 8, "f64"), 5: (2048, 2048, 256, 16, "f32")}
WORKLOADS = {
    2: "config 2: sensor-shaped stand-in 54x4x1152 r=5 fp64, 10%% entries zeroed, traffic opts "
       "(traffic_triple_comparison.m:27-50)",
    3: "config 3: Highway-shaped stand-in 240x320x300 r=5 fp64 video, video opts "
       "(video_triple_comparison.m:41-54)",
    4: "config 4: synthetic 512x512x512 fp64 r=8 low-rank + 5%% outliers (SURVEY.md 8d), traffic "
       "opts (traffic_triple_comparison.m:42-50)",
    5: "config 5: synthetic 2048x2048x256 fp32 r=16 low-rank + 5%% outliers (SURVEY.md 8d), "
       "traffic opts (traffic_triple_comparison.m:42-50)",
}


def ensure_built():
    """Rebuild libtritd.so when any source or header is newer than it, so a
    stale library is never benchmarked as HEAD.  (Compared with the sources
    themselves, not make's objects: a tree copied to a GPU box carries the
    library but not csrc/build/, and must not recompile there.)"""
    import glob
    csrc = os.path.join(PKG, "csrc")
    so = os.path.join(PKG, "tritd", "libtritd.so")
    srcs = [f for e in ("*.hip", "*.cpp", "*.h", "Makefile") for f in glob.glob(os.path.join(csrc, e))]
    srcs.append(os.path.join(ROOT, "include", "tritd.h"))
    if os.path.exists(so) and all(os.path.getmtime(f) <= os.path.getmtime(so) for f in srcs):
        return
    subprocess.run(["make", "-j8", "-C", csrc], check=True, stdout=subprocess.DEVNULL)


def cpu_baseline(D, r, opts, A0, B0, C0, iters, Lstar=None):
    """Time the C restatement of the reference on the host (BASELINE.md §3,
    SURVEY.md §8d): every core the process may use (OMP_NUM_THREADS if set,
    else the CPUs in this process's affinity mask), the CPU model recorded,
    the full solve (100 iterations at configs 1-4), and — given the clean
    tensor — the restatement's final RRE (traffic_triple_comparison.m:62-63,
    evaluate :194-199), so the line carries |RRE_gpu - RRE_cpu| from this box."""
    sys.path.insert(0, os.path.join(ROOT, "oracle"))
    try:
        if not os.path.exists(os.path.join(ROOT, "oracle", "build", "libtritd_ref.so")):
            subprocess.run(["make", "-C", os.path.join(ROOT, "oracle")], check=True,
                           stdout=subprocess.DEVNULL)
        import ctypes as C
        import tritd_ref
        lib = tritd_ref.load()
        env_t = int(os.environ.get("OMP_NUM_THREADS", "0") or 0)
        threads = env_t or len(os.sched_getaffinity(0))
        lib.tritd_ref_set_threads(threads)
        t0 = time.perf_counter()
        out = tritd_ref.admm(lib, D, r, opts, A0, B0, C0, max_iters=iters)
        dt = time.perf_counter() - t0
        k = out[6]
        prec = "fp32 (MATLAB single rules)" if D.dtype == np.float32 else "fp64"
        res = {"value": k / dt, "unit": "iters/s", "cores": threads,
               "threads_from": "OMP_NUM_THREADS" if env_t else "sched_getaffinity",
               "cpu_model": cpu_model(), "kind": "port", "iterations": k,
               "sample": "%d ADMM iterations of the same %dx%dx%d r=%d %s workload "
                         "(C restatement of triple_decomp_ADMM.m with its materialised "
                         "permutes/design matrices, GEMM and pinv; OpenMP; includes per-call "
                         "setup)" % (k, *D.shape, r, prec),
               "seconds": dt, "rre": None, "k": k, "errHist_final": float(out[4][-1])}
        if Lstar is not None:
            n1, n2, n3 = D.shape
            L = np.zeros((n1, n2, n3), order="F")
            p = lambda a: C.c_void_p(a.ctypes.data)  # noqa: E731
            A, B, Cc = (np.asfortranarray(x, dtype=np.float64) for x in out[:3])
            lib.tritd_ref_triple_product(p(A), p(B), p(Cc), n1, n2, n3, r, p(L))
            num = float(np.sum(np.square(L - Lstar)))
            res["rre"] = float(np.sqrt(num) / np.linalg.norm(Lstar))
        return res
    except Exception as e:  # the baseline is reported, never the product
        return {"value": None, "unit": "iters/s", "cores": 0, "kind": "port",
                "sample": "unavailable: %s" % e}


def end_to_end(tritd, D, r, opts, A0, B0, C0, device):
    """Wall time of one triple_decomp_ADMM(D, r, opts) call with maxIter = 100
    from host arrays to host arrays — what the reference's drivers time with
    tic/toc around the solver (traffic_triple_comparison.m:51,61; README.md:63):
    session creation (placement probe, D upload, tile-major conversion), the
    loop, and get (factors, O, E and errHist back to the host).  The one-shot
    call does not probe placements (TRITD_SESSION_PROBE is a session option);
    the same call with the probe forced (TRITD_PROBE=8) is timed beside it,
    interleaved, two calls each (min reported), so the probe's net effect on a
    one-shot solve stays visible."""
    o = dict(opts, maxIter=100)
    old = os.environ.get("TRITD_PROBE")
    times = {"default": [], "with_probe": []}
    k = None
    try:
        for rep in range(2):
            for label, val in (("default", old), ("with_probe", "8")):
                if val is None:
                    os.environ.pop("TRITD_PROBE", None)
                else:
                    os.environ["TRITD_PROBE"] = val
                t0 = time.perf_counter()
                out = tritd.triple_decomp_ADMM(D, r, o, A0, B0, C0, device=device,
                                               return_iters=True)
                times[label].append((time.perf_counter() - t0) * 1e3)
                k = out[-1]
                del out
    finally:
        if old is None:
            os.environ.pop("TRITD_PROBE", None)
        else:
            os.environ["TRITD_PROBE"] = old
    res = {"maxIter": 100, "k": k, "unit": "ms"}
    for label, t in times.items():
        res[label] = {"ms": min(t), "ms_each": [round(x, 2) for x in t]}
    res["ms"] = res["default"]["ms"]
    res["probe_net_ms"] = res["with_probe"]["ms"] - res["default"]["ms"]
    # where a one-shot call's time goes: the same steps
    # through a session, each timed — create (D over PCIe, tile-major layout),
    # the 100 device-resident iterations, get (fix-ups and layout on the
    # device, then O, E, factors and errHist back over PCIe) — and the bare
    # PCIe rate of one D-sized copy each way on this box
    from tritd import hip
    t0 = time.perf_counter()
    s = tritd.Session(r, o, A0, B0, C0, n1=D.shape[0], n2=D.shape[1], n3=D.shape[2], D=D,
                      device=device, probe=False)
    t1 = time.perf_counter()
    s.run(100)
    s.sync()
    t2 = time.perf_counter()
    out = s.get()
    t3 = time.perf_counter()
    s.close()
    del out
    Df = np.asfortranarray(D)
    buf = np.empty_like(Df)
    hip.synchronize()
    t4 = time.perf_counter()
    dev = hip.DeviceArray.from_host(Df)  # (includes the hipMalloc of 1 GB)
    hip.synchronize()
    t5 = time.perf_counter()
    dev.to_host(buf)  # (into pages the first touch must fault in)
    t6 = time.perf_counter()
    dev.free()
    del buf
    res["session_path"] = {"create_ms": (t1 - t0) * 1e3, "iterations_ms": (t2 - t1) * 1e3,
                           "get_ms": (t3 - t2) * 1e3,
                           "note": "tritd.Session(D host) / run(100) / get(): O, E, A, B, C, errHist"}
    res["pcie"] = {"bytes": int(D.nbytes), "h2d_GBs": D.nbytes / (t5 - t4) / 1e9,
                   "d2h_GBs": D.nbytes / (t6 - t5) / 1e9,
                   "note": "one hipMemcpy of D each way from pageable host memory"}
    return res


def latest_profile(name):
    """The newest profiles/round<N>/<name> (rounds of the driver), or None."""
    import glob
    import re
    best = None
    for f in glob.glob(os.path.join(ROOT, "profiles", "round*", name)):
        m = re.search(r"round(\d+)", f)
        if m and (best is None or int(m.group(1)) > best[0]):
            best = (int(m.group(1)), f)
    return best[1] if best else None


def pmc_mfma_util(config):
    """K2's MFMA utilisation from the committed rocprofv3 SQ pass
    (tools/pmc_summary.py --json -> profiles/round<N>/k2_mfma_util.json):
    SQ_VALU_MFMA_BUSY_CYCLES / (GRBM_GUI_ACTIVE / 8 XCDs x 1024 SIMDs)."""
    f = latest_profile("c5_k2_mfma_util.json" if config == 5 else "k2_mfma_util.json")
    if not f:
        return None, None
    with open(f) as fh:
        d = json.load(fh)
    return d.get("mfma_util"), os.path.relpath(f, ROOT)


def pmc_traffic(config):
    """HBM bytes per fused-update launch from the committed rocprofv3 PMC pass
    of the same workload (tools/pmc_traffic.py -> profiles/round<N>/k5_traffic.json,
    config 5: c5_k5_traffic.json), or None.  rocprofv3 cannot run inside the
    timed process, so the line cites the committed pass it copies."""
    f = latest_profile("c5_k5_traffic.json" if config == 5 else "k5_traffic.json")
    if not f:
        return None, None
    with open(f) as fh:
        d = json.load(fh)
    return d.get("bytes_per_launch"), os.path.relpath(f, ROOT)


def primitives(device, n=512, r=8, reps=10):
    """The API-level kernels north_star prices against the roofline — unfold
    (unfold.m:6-10, modes 2 and 3), soft_threshold (soft_threshold.m:2) at
    >= 80 % of HBM, and triple_product (triple_product.m:6, called by both
    drivers after the solve) on f64 MFMA — on device-resident n^3 fp64 arrays,
    timed with HIP events on the stream they are launched on (the null
    stream), through the HIP runtime libtritd is bound to (tritd.hip)."""
    import ctypes as C
    from tritd import hip
    from tritd._lib import check, lib
    hip.set_device(device)
    sp = C.c_void_p(0)
    N = n ** 3
    rng = np.random.default_rng(0)
    X = hip.DeviceArray.from_host(rng.standard_normal(N))
    Y = hip.DeviceArray(N * 8)
    p = lambda t: C.c_void_p(t.ptr)  # noqa: E731
    ev = hip.EventTimer(None)

    def timed(fn, warm=3):
        for _ in range(warm):
            fn()
        hip.synchronize()
        ev.start()
        for _ in range(reps):
            fn()
        return ev.stop() / reps

    out = {"shape": [n, n, n], "r": r, "reps": reps}

    def rec(name, ms, nbytes=None, flops=None):
        d = {"ms": ms}
        if nbytes is not None:
            d["algorithmic_bytes"] = nbytes
            d["GBs"] = nbytes / ms / 1e6
            d["hbm_frac"] = d["GBs"] / HBM_PEAK_GBS
        if flops is not None:
            d["TFs"] = flops / ms / 1e9
            d["mfma_frac"] = d["TFs"] / F64_MFMA_PEAK_TFS
        out[name] = d

    for mode in (2, 3):
        ms = timed(lambda: check(lib.tritd_dev_unfold_f64(p(X), n, n, n, mode, p(Y), sp)))
        rec("unfold_mode%d" % mode, ms, 2 * N * 8)
    ms = timed(lambda: check(lib.tritd_dev_soft_threshold_f64(p(X), N, C.c_double(0.5), p(Y), sp)))
    rec("soft_threshold", ms, 2 * N * 8)
    R = r * r
    A = hip.DeviceArray.from_host(rng.standard_normal(n * R))
    B = hip.DeviceArray.from_host(rng.standard_normal(R * n))
    Cc = hip.DeviceArray.from_host(rng.standard_normal(R * n))
    ms = timed(lambda: check(lib.tritd_dev_triple_product_f64(p(A), p(B), p(Cc), n, n, n, r, p(Y),
                                                             sp)))
    rec("triple_product", ms, N * 8, 2.0 * N * R)
    for t in (X, Y, A, B, Cc):
        t.free()
    return out


def listen_socket():
    """rank 0's rendezvous socket (tritd.rendezvous.StarGroup): bound to an
    ephemeral port on 127.0.0.1 and listening before any rank connects; the
    rank-0 worker inherits the descriptor, so the port is never re-bound."""
    import socket
    s = socket.socket(socket.AF_INET, socket.SOCK_STREAM)
    s.bind(("127.0.0.1", 0))
    s.listen(64)
    return s


def wait_all(procs):
    """Exit code 0 only if every process exits 0; the first failure stops the
    rest (a failed rank would leave the others in a collective)."""
    import signal
    rc = 0
    live = list(procs)
    while live:
        for p in list(live):
            c = p.poll()
            if c is None:
                continue
            live.remove(p)
            if c != 0 and rc == 0:
                rc = c if c > 0 else 1
                for q in live:
                    q.send_signal(signal.SIGTERM)
        time.sleep(0.05)
    return rc


def worker_cmd():
    return [sys.executable, os.path.abspath(__file__), "--worker"] + sys.argv[1:]


def spawn_ranks(n):
    """`--gpus N > 1` without a torch.distributed launcher around us: start
    the N rank workers ourselves, as CHILD processes (never an exec; this
    process has not touched the GPU), with torchrun's rank environment and
    the rendezvous port; rank 0 inherits the listening socket."""
    ls = listen_socket()
    port = ls.getsockname()[1]
    procs = []
    for r in range(n):
        env = dict(os.environ, RANK=str(r), LOCAL_RANK=str(r), WORLD_SIZE=str(n),
                   LOCAL_WORLD_SIZE=str(n), GROUP_RANK="0", TRITD_RDZV_PORT=str(port),
                   OMP_NUM_THREADS=os.environ.get("OMP_NUM_THREADS", "4"))
        fds = ()
        if r == 0:
            env["TRITD_RDZV_FD"] = str(ls.fileno())
            fds = (ls.fileno(),)
        procs.append(subprocess.Popen(worker_cmd(), env=env, pass_fds=fds))
    ls.close()
    return wait_all(procs)


def rank_parent():
    """A rank process started by torchrun (the driver's N > 1 launch): it
    joins a gloo group on the CPU only to publish rank 0's rendezvous port,
    then runs the rank's GPU work in a child worker that never imports torch
    (so libtritd binds /opt/rocm's HIP runtime and RCCL, the stack the GPU
    tests validate: VERDICT r5 next 3a), and exits with the worker's code.
    This process never touches the GPU and never execs."""
    import torch.distributed as tdist
    rank = int(os.environ["RANK"])
    tdist.init_process_group("gloo")
    ls = listen_socket() if rank == 0 else None
    port = [ls.getsockname()[1] if ls else None]
    tdist.broadcast_object_list(port, src=0)
    env = dict(os.environ, TRITD_RDZV_PORT=str(port[0]))
    fds = ()
    if ls is not None:
        env["TRITD_RDZV_FD"] = str(ls.fileno())
        fds = (ls.fileno(),)
    p = subprocess.Popen(worker_cmd(), env=env, pass_fds=fds)
    if ls is not None:
        ls.close()
    rc = wait_all([p])
    try:
        tdist.destroy_process_group()
    except Exception:
        pass
    return rc


def launch_check(args):
    """--launch-check: the rank plumbing alone (no GPU): every worker joins the
    rendezvous, the ranks count themselves with an all-reduce, rank 0 prints
    one JSON line.  CPU test of the `--gpus N` spawn and torchrun paths."""
    from tritd.rendezvous import StarGroup
    g = StarGroup.from_env(timeout=120)
    n = g.allreduce_sum([1.0])[0]
    torch_loaded = g.allgather("torch" in sys.modules)
    if g.rank == 0:
        print(json.dumps({"launch_check": True, "n_gpus": g.world, "ranks_counted": int(n),
                          "gpus_arg": args.gpus, "torch_in_workers": any(torch_loaded)}),
              flush=True)
    g.close()


def cpu_model():
    try:
        with open("/proc/cpuinfo") as f:
            for line in f:
                if line.startswith("model name"):
                    return line.split(":", 1)[1].strip()
    except OSError:
        pass
    return None


def make_data(config, n1, n2, n3, r, rows, want_L=True):
    """Synthetic inputs of `config`, rows = this rank's
    mode-1 range; returns (D, Lstar, A0, B0, C0) with D / Lstar of those rows
    (Lstar None unless wanted: a plain run never reads it)."""
    from tritd import synth
    i0, i1 = rows
    if config == 2:  # RRE against the complete readings (traffic_triple_comparison.m:62)
        d = synth.sensor_like(n1, n2, n3, r, missing=0.10, seed=0, init_seed=123)
        d["Lstar"] = d.pop("X")
    elif config == 3:  # RRE of the low-rank part against the frames
        d = synth.video_like(n1, n2, n3, r, seed=0, init_seed=123)
        d["Lstar"] = d.pop("X")
    elif CONFIGS[config][4] == "f32":  # config 5: rounded to single, this rank's rows only
        d = synth.low_rank_plus_outliers_f32(n1, n2, n3, r, p_out=0.05, seed=0, init_seed=123,
                                             rows=rows)
        return d["D"], d["Lstar"], d["A0"], d["B0"], d["C0"]
    else:
        d = synth.low_rank_plus_outliers(n1, n2, n3, r, p_out=0.05, seed=0, init_seed=123)
    D = np.asfortranarray(d["D"][i0:i1], dtype=np.float64)
    L = np.asfortranarray(d["Lstar"][i0:i1], dtype=np.float64) if want_L else None
    return D, L, d["A0"], d["B0"], d["C0"]


DUMP_SAMPLE = 1 << 21  # elements kept of an output too large to dump whole
DUMP_WHOLE_BYTES = 16 << 20  # O and E are dumped whole up to this size each


def dump_outputs(out_dir, res, rank, world):
    """--dump-outputs: what Session.get() returned after the last timed
    iteration, as <out_dir>/<name>.npy in the arrays' own precision (float32 or
    float64; `_rank<r>` appended to the name at N > 1, each rank writing its
    shard).  The factors and errHist are written whole; O and E are written
    whole up to 16 MiB each, otherwise as the elements (in column-major order)
    at 2^21 sorted indices drawn from numpy's default_rng(0): the same
    elements on every run of the same shape, 32 MiB at most for the pair."""
    os.makedirs(out_dir, exist_ok=True)
    sfx = "_rank%d" % rank if world > 1 else ""
    for name in ("A", "B", "C", "O", "E", "errHist"):
        a = np.asarray(res[name])
        if a.dtype not in (np.float32, np.float64):
            a = a.astype(np.float64)
        if name in ("O", "E") and a.nbytes > DUMP_WHOLE_BYTES:
            idx = np.sort(np.random.default_rng(0).integers(0, a.size, size=DUMP_SAMPLE))
            a = a.ravel(order="K")[idx]  # (O and E are column-major: a view, no copy)
        np.save(os.path.join(out_dir, name + sfx + ".npy"), a)


def run_case(config, K, W, group, comm, local_rank, n=None, r=None, host_comm=False, full=True,
             dump_dir=None):
    """One sharded (or single-GPU) run of `config`: W untimed warm-up
    iterations, K timed iterations between barriers (max over ranks), the
    outputs after the last of them written to `dump_dir` if given, and — with
    `full` — a K5 events pass, an events sample, then the untimed rest of the
    100-iteration solve and the driver's RRE.  Returns (result dict,
    (D, Lstar, A0, B0, C0)) — the data of this rank's rows, for the rank-0
    extras (Lstar None without `full`)."""
    import tritd
    from tritd import hip, synth
    from tritd.dist import shard_bounds
    world = group.world if group else 1
    rank = group.rank if group else 0
    n1, n2, n3, rr, dts = CONFIGS[config]
    if n is not None:
        n1 = n2 = n3 = n
    rr = r if r is not None else rr
    f32 = dts == "f32"
    npdt = np.float32 if f32 else np.float64
    maxIter = max(100, K + W)
    base_opts = synth.VIDEO_OPTS if config == 3 else synth.TRAFFIC_OPTS
    # up to the drivers' 100 iterations the stop test keeps their tol (it does
    # not fire there); a longer run iterates past it (tol 0: the test is still
    # computed every iteration, it only never stops the solve), so --steps
    # sets the number of timed iterations at any K
    opts = dict(base_opts, maxIter=maxIter, tol=base_opts["tol"] if K + W <= 100 else 0.0)
    i0, i1 = shard_bounds(n1, world, rank)
    D, Lstar, A0, B0, C0 = make_data(config, n1, n2, n3, rr, (i0, i1), want_L=full)

    def barrier():
        if group:
            group.barrier()

    # inputs resident in HBM before the timed region
    hip.set_device(local_rank)
    D_shard = hip.DeviceArray.from_host(np.asfortranarray(D, dtype=npdt))
    sess = tritd.Session(rr, opts, A0, B0, C0, n1=n1, n2=n2, n3=n3, i0=i0, i1=i1,
                         d_device_ptr=D_shard.ptr, ldD=i1 - i0, device=local_rank, comm=comm,
                         dtype=npdt)
    D_shard.free()
    sess.run(W)
    sess.sync()
    dense0, tiles_per_launch = sess.counters()

    def timed(k):
        barrier()
        hip.synchronize()
        t0 = time.perf_counter()
        sess.run(k)
        done, stopped = sess.sync()
        hip.synchronize()
        barrier()
        dt = time.perf_counter() - t0
        if group:
            dt = group.allreduce_max(dt)
        return dt, done, stopped

    # the timed region: K steps with no events (an event record is a stream
    # marker that widens the gap to the next kernel by several us: ~10 % of
    # config 2's iteration)
    sess.set_timing(False)
    dt, done, stopped = timed(K)
    if done != W + K or stopped:
        raise SystemExit("stop test fired inside the timed region (k=%d): timing invalid" % done)
    if dump_dir:
        dump_outputs(dump_dir, sess.get(), rank, world)
    out = {
        "value": K / dt, "ms_per_step": dt * 1e3 / K, "steps": K, "warmup": W, "dtype": dts,
        "n1": n1, "n2": n2, "n3": n3, "r": rr, "maxIter": maxIter, "opts": opts,
        "workload": (WORKLOADS[config] if n is None and r is None
                     else "config %d shape override: %dx%dx%d r=%d"
                     % (config, n1, n2, n3, rr)).replace("%%", "%"),
    }
    if not full:
        sess.close()
        return out, (D, Lstar, A0, B0, C0)
    dense1, _ = sess.counters()
    dense_per_launch = (dense1 - dense0) / K
    # K5's launch duration for the roofline: HIP events around K5 only, on
    # its stream, over a second timed pass of up to K steps
    K2n = max(1, min(K, maxIter - done))
    sess.set_timing("k5")
    dt_ev, done, stopped = timed(K2n)
    km = sess.kernel_ms()
    probe_ms, probe_pick = sess.probe()
    if stopped:
        raise SystemExit("stop test fired inside the K5 events pass (k=%d)" % done)
    # K2 and whole-iteration event timings: an untimed sample right after the
    # timed region (the solve continues; events around every kernel there)
    n_more = min(10, maxIter - done)
    ar_ms, ar_n = 0.0, 0
    if n_more > 0:
        sess.set_timing(True)
        sess.run(n_more)
        sess.sync()
        km2 = sess.kernel_ms()
        km["mode3"], km["iteration"] = km2["mode3"], km2["iteration"]
        ar_ms, ar_n = sess.comm_ms()
        sess.set_timing(False)
    # per-rank breakdown of that sample (N > 1): the all-reduces' ms (issue to
    # completion on the session stream, waiting for the slowest rank
    # included) and the rest of the iteration (this rank's compute)
    per_rank = None
    if group and world > 1:
        allv = group.allgather([rank, i1 - i0, km["iteration"], ar_ms, ar_n, km["fused_update"]])
        per_rank = [{"rank": int(v[0]), "rows": int(v[1]), "iteration_ms": float(v[2]),
                     "allreduce_ms": float(v[3]), "allreduces_per_iteration": int(v[4]),
                     "compute_ms": float(v[2] - v[3]), "fused_update_ms": float(v[5])}
                    for v in allv]
    # finish the solve (untimed) and report the driver RRE at the final k
    sess.run(maxIter - done)
    k_final, _ = sess.sync()
    L_shard = hip.DeviceArray.from_host(np.asfortranarray(Lstar, dtype=npdt))
    num, den = sess.rre_parts(L_shard.ptr, i1 - i0)
    L_shard.free()
    if group and world > 1:
        num, den = group.allreduce_sum([num, den])
    rre = float(np.sqrt(num / den))
    res = sess.get()
    errhist_final = float(res["errHist"][-1]) if len(res["errHist"]) else None

    # algorithmic bytes of the dominant kernel (fused update K5), per launch,
    # on this rank's shard: `streams` dense N-streams of s bytes
    # (fp64: D, Y_L read + Y_L, T written, Y_O rebuilt from Y_L and E; fp32:
    # D, Y_L, Y_O read + Y_L, Y_O, T written; O is rebuilt on demand), E in
    # compact form (`slots` 256 B slot accesses per 256-element tile: E^(k) and
    # E^(k-1) read + E^(k+1) written, or E read + written), whole tiles
    # (256 * s bytes) for the tiles stored densely, and W (R * n_local * n2 elements)
    s_b = 4 if f32 else 8
    nl = i1 - i0
    N_local = nl * n2 * n3
    tile_b = 256 * s_b
    streams, slots = sess.k5_profile()
    # (dense-E mode, sess.k5_profile() = (7, 0): every E access is a dense stream)
    k5_bytes = int(streams * N_local * s_b + slots * tiles_per_launch * 256
                   + (max(slots - 1, 0) * dense_per_launch * tile_b if slots else 0)
                   + rr * rr * nl * n2 * s_b)
    # flops: L(ij,t) = sum_k (Ah*Bh)(ij,k) Ch(t,k) and W = T x3 Ch, 2 N R each
    k5_flops = 4.0 * N_local * rr * rr
    k5_ms = km["fused_update"]
    gbs = k5_bytes / (k5_ms * 1e-3) / 1e9 if k5_ms > 0 else None
    tfs = k5_flops / (k5_ms * 1e-3) / 1e12 if k5_ms > 0 else None
    # the committed PMC pass is of the 1-GPU launch (a shard moves 1/N of it)
    # (committed PMC passes exist for configs 4 and 5 at their default shapes)
    pmc_ok = world == 1 and config in (4, 5) and n is None and r is None
    traffic, traffic_src = pmc_traffic(config) if pmc_ok else (None, None)
    if f32:  # config 5 is MFMA-bound
        roof = {"bound": "mfma", "achieved": tfs, "peak": F32_MFMA_PEAK_TFS, "unit": "TFLOP/s",
                "frac": (tfs / F32_MFMA_PEAK_TFS) if tfs else None,
                "hbm_achieved_GBs": gbs, "hbm_frac": (gbs / HBM_PEAK_GBS) if gbs else None,
                "algorithmic_flops_per_launch": k5_flops}
    else:
        roof = {"bound": "hbm", "achieved": gbs, "peak": HBM_PEAK_GBS, "unit": "GB/s",
                "frac": (gbs / HBM_PEAK_GBS) if gbs else None,
                "mfma_achieved_TFs": tfs}
    roof.update({"kernel": "k5_fused (fused ADMM update + L + W)", "traffic": traffic,
                 "dense_streams": streams, "slot_accesses_per_tile": slots,
                 "traffic_source": traffic_src, "algorithmic_bytes_per_launch": k5_bytes,
                 "e_dense_tiles_per_launch": dense_per_launch,
                 "e_tiles_per_launch": tiles_per_launch})
    # K2 (the mode-3 MTTKRP, X3*H' of :93): the RPAS GEMM north_star prices
    # against the MFMA peak; 2 * N_local * R flops per launch
    k2_ms = km["mode3"]
    k2_flops = 2.0 * N_local * rr * rr
    k2_tfs = k2_flops / (k2_ms * 1e-3) / 1e12 if k2_ms > 0 else None
    k2_peak = F32_MFMA_PEAK_TFS if f32 else F64_MFMA_PEAK_TFS
    pmc_util, pmc_src = pmc_mfma_util(config) if pmc_ok else (None, None)
    roof["mfma_gemm"] = {"kernel": "k_m3_cp (mode-3 MTTKRP, X3*H' of triple_decomp_ADMM.m:93)",
                         "achieved": k2_tfs, "peak": k2_peak, "unit": "TFLOP/s",
                         "frac": (k2_tfs / k2_peak) if k2_tfs else None,
                         "algorithmic_flops_per_launch": k2_flops, "ms": k2_ms,
                         "pmc_mfma_util": pmc_util, "pmc_source": pmc_src}
    sess.close()
    out.update({
        "per_rank": per_rank, "rre_final": rre, "k_final": k_final,
        "errHist_final": errhist_final,
        "kernel_ms": {"fused_update": k5_ms, "mode3_mttkrp": km["mode3"],
                      "iteration_events": km["iteration"], "samples": km["samples"],
                      "k5_events_pass": {"steps": K2n, "ms_per_step": dt_ev * 1e3 / K2n,
                                         "note": "a second timed pass with HIP events "
                                                 "around K5 only (value is the pass "
                                                 "without events)"}},
        "roofline": roof,
        "placement_probe": {"ms": [round(m, 4) for m in probe_ms], "picked": probe_pick},
    })
    return out, (D, Lstar, A0, B0, C0)


def c5_reference():
    """The committed 100-iteration class-single restatement of config 5
    (tests/golden/c5_horizon.npz, tests/golden/make_c5_horizon.py), or None."""
    f = os.path.join(ROOT, "tests", "golden", "c5_horizon.npz")
    if not os.path.exists(f):
        return None
    z = np.load(f)
    return {"k": int(z["k"]), "rre": float(z["rre"]), "errHist_final": float(z["errHist"][-1]),
            "source": os.path.relpath(f, ROOT)}


def config5_summary(d):
    """The keys that place config 5 beside the config-4 line, plus its RRE
    against the committed full-horizon CPU restatement."""
    roof = d["roofline"]
    out = {"workload": d["workload"], "value": d["value"], "unit": "iters/s",
           "ms_per_step": d["ms_per_step"], "steps": d["steps"], "warmup": d["warmup"],
           "dtype": d["dtype"], "rre_final": d["rre_final"], "k_final": d["k_final"],
           "errHist_final": d["errHist_final"],
           "fused_update_ms": d["kernel_ms"]["fused_update"],
           "mode3_mttkrp_ms": d["kernel_ms"]["mode3_mttkrp"],
           "roofline": {k: roof.get(k) for k in ("bound", "achieved", "peak", "unit", "frac",
                                                 "kernel", "traffic", "traffic_source",
                                                 "algorithmic_flops_per_launch")},
           "mode3_mfma_frac": roof.get("mfma_gemm", {}).get("frac"),
           "per_rank": d["per_rank"]}
    ref = c5_reference()
    if ref is not None and d["maxIter"] == 100:
        out["cpu_restatement"] = ref
        out["rre_vs_cpu"] = abs(d["rre_final"] - ref["rre"])
        out["rre_bound"] = 1e-6 + 2e-5 * ref["rre"]
        out["k_matches_cpu"] = d["k_final"] == ref["k"]
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--gpus", type=int, default=1)
    ap.add_argument("--steps", type=int, default=40)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--config", type=int, default=4, choices=sorted(CONFIGS))
    ap.add_argument("--n", "--side", dest="n", type=int, default=None,
                    help="config 4: cube side override (--side under torchrun, whose own "
                         "parser takes --n for an abbreviation of its options)")
    ap.add_argument("--r", type=int, default=None)
    ap.add_argument("--dump-outputs", metavar="DIR", default=None,
                    help="write the outputs after the last timed step (A, B, C, O, E, errHist) "
                         "as DIR/<name>.npy; O and E as a fixed seeded sample when large")
    ap.add_argument("--full", action="store_true",
                    help="also run what the headline figure does not need: HIP-event passes and "
                         "roofline, the rest of the solve and its RRE, end-to-end calls, primitive "
                         "kernels, the config-5 leg and the CPU baseline (each with its --no-* "
                         "switch)")
    # the full 100-iteration solve at configs 1-4 (one
    # iteration at config 5, reported per iteration)
    ap.add_argument("--cpu-iters", type=int, default=None)
    ap.add_argument("--no-cpu", action="store_true")
    ap.add_argument("--no-e2e", action="store_true", help="skip the end-to-end one-shot calls")
    ap.add_argument("--no-prims", action="store_true", help="skip the primitive kernels")
    ap.add_argument("--no-c5", action="store_true",
                    help="skip the config-5 leg of the default (config 4) line")
    ap.add_argument("--c5-steps", type=int, default=10, help="timed iterations of the config-5 leg")
    ap.add_argument("--comm", default="rccl", choices=("rccl", "host"),
                    help="N > 1: libtritd's RCCL communicator (default), or the host all-reduce "
                         "transport over the rendezvous sockets (correctness rehearsal with ranks "
                         "sharing a GPU)")
    # --algo als: triple_decomp_ALS.m on the config-4 workload
    ap.add_argument("--algo", default="admm", choices=("admm", "als"))
    ap.add_argument("--launch-check", action="store_true",
                    help="test the N-rank launch only (rendezvous, no GPU work)")
    ap.add_argument("--worker", action="store_true", help=argparse.SUPPRESS)
    args = ap.parse_args()
    if args.gpus < 1:
        raise SystemExit("--gpus must be >= 1")
    if "WORLD_SIZE" not in os.environ and args.gpus > 1:
        # never a silent one-rank run of an N-GPU request
        return spawn_ranks(args.gpus)
    world = int(os.environ.get("WORLD_SIZE", "1"))
    if world != args.gpus:
        raise SystemExit("--gpus %d does not match WORLD_SIZE %d" % (args.gpus, world))
    if world > 1 and not args.worker:
        return rank_parent()  # started by torchrun: GPU work in a torch-free child
    if args.launch_check:
        return launch_check(args)
    if args.algo == "als":
        if world > 1:
            raise SystemExit("--algo als runs on one GPU")
        return bench_als(args)

    rank = int(os.environ.get("RANK", "0"))
    local_rank = int(os.environ.get("LOCAL_RANK", "0"))
    host_comm = args.comm == "host"
    group = None
    if world > 1:
        from tritd.rendezvous import StarGroup
        group = StarGroup.from_env()

    # one rank checks / rebuilds the library, the others wait for it (ranks
    # building concurrently would race on the same objects)
    if local_rank == 0:
        ensure_built()
    if group:
        group.barrier()
    import tritd
    from tritd import hip
    from tritd._lib import HIP_RUNTIME, hip_runtimes, runtime_stack

    comm = None
    if world > 1:
        from tritd.rendezvous import make_comm, make_host_comm
        if host_comm:
            # rehearsal of the N > 1 path on fewer GPUs than ranks (the
            # timing is not a scaling number)
            local_rank = local_rank % max(tritd.device_count(), 1)
            comm = make_host_comm(group, local_rank)
        else:
            comm = make_comm(group, local_rank)
    # what the library's communicator itself reports (RCCL: ncclCommCount)
    comm_info = comm.info() if comm is not None else (1, 0, "none")
    if comm is not None and comm_info[0] != world:
        raise SystemExit("communicator reports %d ranks, WORLD_SIZE is %d" % (comm_info[0], world))

    main_res, data = run_case(args.config, args.steps, args.warmup, group, comm, local_rank,
                              n=args.n, r=args.r, host_comm=host_comm, full=args.full,
                              dump_dir=args.dump_outputs)
    D, Lstar, A0, B0, C0 = data
    extras = args.full and rank == 0 and world == 1
    e2e = None
    if extras and not args.no_e2e:
        e2e = end_to_end(tritd, D, main_res["r"], main_res["opts"], A0, B0, C0, local_rank)
    prims = None
    if extras and not args.no_prims:
        prims = primitives(local_rank)
    cpu = None
    if extras and not args.no_cpu:
        f32 = CONFIGS[args.config][4] == "f32"
        iters = args.cpu_iters if args.cpu_iters is not None else (1 if f32 else 100)
        cpu = cpu_baseline(D, main_res["r"], main_res["opts"], A0, B0, C0, iters,
                           Lstar=None if f32 else Lstar)
    del D, Lstar, data

    # the north_star's second headline configuration in the same line (VERDICT
    # r4 next 5, r5 next 3b): a bounded config-5 run on the same ranks and
    # communicator, after the config-4 session has released its device memory
    c5 = None
    if args.full and args.config == 4 and args.n is None and args.r is None and not args.no_c5:
        d5, _ = run_case(5, args.c5_steps, 2, group, comm, local_rank, host_comm=host_comm)
        c5 = config5_summary(d5)

    if rank == 0:
        line = {
            "metric": "ADMM iters/sec + final RRE, 512^3 r=8 tensor at 1/2/4/8 MI355X",
            "value": main_res["value"],
            "unit": "iters/s",
            "n_gpus": world,
            "steps": main_res["steps"],
            "warmup": main_res["warmup"],
            "ms_per_step": main_res["ms_per_step"],
            "higher_is_better": True,
            "scaling": "strong",
            "vs_baseline": None,
            "dtype": main_res["dtype"],
            "data": "synthetic",
            "config": {"workload": main_res["workload"],
                       "n1": main_res["n1"], "n2": main_res["n2"], "n3": main_res["n3"],
                       "r": main_res["r"], "maxIter": main_res["maxIter"],
                       "tol": main_res["opts"]["tol"],
                       "parallelism": "mode1-shard x%d" % world
                                      + (" (host all-reduce rehearsal: not a scaling number)"
                                         if host_comm and world > 1 else "")},
            "comm": {"transport": comm_info[2], "nranks": comm_info[0]},
            # the libamdhip64 libtritd ran on (/opt/rocm's: no rank imports torch)
            "hip_runtime": HIP_RUNTIME,
            "hip_runtimes_mapped": len(hip_runtimes()),
            # HIP / HSA / RCCL copies mapped in rank 0 (one each, /opt/rocm)
            "runtime_stack": runtime_stack(),
            "rccl_nranks": comm_info[0] if comm_info[2] == "rccl" else None,
            "full": args.full,
        }
    if rank == 0 and args.full:
        line.update({
            # N > 1: per rank, from an events sample after the timed region
            "per_rank": main_res["per_rank"],
            "rre_final": main_res["rre_final"],
            # |RRE_gpu - RRE_cpu| on this box
            "rre_vs_cpu": (abs(main_res["rre_final"] - cpu["rre"])
                           if cpu and cpu.get("rre") is not None else None),
            "k_final": main_res["k_final"],
            "errHist_final": main_res["errHist_final"],
            "kernel_ms": main_res["kernel_ms"],
            "roofline": main_res["roofline"],
            "cpu_baseline": cpu,
            # candidate tensor pools timed with K5's access pattern at session
            # creation (rank 0), the fastest kept
            "placement_probe": main_res["placement_probe"],
            # one whole triple_decomp_ADMM call (maxIter=100), host arrays in and out,
            # timed like the drivers' tic/toc (traffic_triple_comparison.m:51,61)
            "end_to_end": e2e,
            # unfold / soft_threshold / triple_product on 512^3 fp64, device-resident
            "primitives": prims,
            # config 5 (2048x2048x256 fp32 r=16) on the same ranks, a bounded run
            "config5": c5,
        })
    if rank == 0:
        print(json.dumps(line), flush=True)

    if comm is not None:
        comm.close()
    if group is not None:
        group.close()


def cpu_baseline_als(X, r, A0, B0, C0, iters):
    """The numpy restatement of triple_decomp_ALS.m (oracle/tritd_oracle.py) on
    a bounded sample of iterations (BLAS threads of numpy)."""
    sys.path.insert(0, os.path.join(ROOT, "oracle"))
    try:
        import tritd_oracle as orc
        t0 = time.perf_counter()
        *_, k = orc.triple_decomp_ALS(X, r, dict(maxIter=iters, tol=0.0), A0, B0, C0,
                                      printer=lambda s: None)
        dt = time.perf_counter() - t0
        return {"value": k / dt, "unit": "iters/s",
                "cores": int(os.environ.get("OMP_NUM_THREADS", "0")) or (os.cpu_count() or 1),
                "kind": "port",
                "sample": "%d ALS iterations of the same %dx%dx%d r=%d fp64 workload (numpy "
                          "restatement of triple_decomp_ALS.m: buildF/G/H design matrices, "
                          "unfold permutes, GEMM, SVD pinv)" % (k, *X.shape, r),
                "seconds": dt}
    except Exception as e:  # the baseline is reported, never the product
        return {"value": None, "unit": "iters/s", "cores": 0, "kind": "port",
                "sample": "unavailable: %s" % e}


def bench_als(args):
    """ALS iterations/s (triple_decomp_ALS.m:14-39) on the config-4 tensor,
    one GPU, X resident in HBM.  Roofline on the fused fit kernel (L + error +
    W = X x3 C^; 4 N R flops on f64 MFMA, N*8 B read)."""
    if int(os.environ.get("WORLD_SIZE", "1")) > 1:
        raise SystemExit("--algo als runs on one GPU")
    ensure_built()
    import tritd
    from tritd import hip, synth
    n1, n2, n3, r, _ = CONFIGS[4]
    if args.n is not None:
        n1 = n2 = n3 = args.n
    r = args.r if args.r is not None else r
    K, W = args.steps, args.warmup
    data = synth.low_rank_plus_outliers(n1, n2, n3, r, p_out=0.05, seed=0, init_seed=123)
    X = data["D"]
    Xd = hip.DeviceArray.from_host(np.asfortranarray(X))
    opts = dict(maxIter=K + W, tol=0.0)  # tol 0: the stop test never fires in the timed region
    s = tritd.AlsSession(r, opts, data["A0"], data["B0"], data["C0"], n1=n1, n2=n2, n3=n3,
                         x_device_ptr=Xd.ptr, ldX=n1, quiet=True)
    Xd.free()
    s.run(W)
    s.sync()
    s.set_timing(True)
    hip.synchronize()
    t0 = time.perf_counter()
    s.run(K)
    done, stopped = s.sync()
    hip.synchronize()
    dt = time.perf_counter() - t0
    km = s.kernel_ms()
    res = s.get()
    if args.dump_outputs:  # an ALS solve returns the factors and errHist
        os.makedirs(args.dump_outputs, exist_ok=True)
        for name in ("A", "B", "C", "errHist"):
            np.save(os.path.join(args.dump_outputs, name + ".npy"), res[name])
    N = n1 * n2 * n3
    fit_flops = 4.0 * N * r * r
    fit_bytes = N * 8 + r * r * n1 * n2 * 8
    tfs = fit_flops / (km["fit"] * 1e-3) / 1e12 if km["fit"] > 0 else None
    cpu = None
    if args.full and not args.no_cpu:
        cpu = cpu_baseline_als(X, r, data["A0"], data["B0"], data["C0"], args.cpu_iters or 3)
    line = {
        "metric": "ALS iters/sec (triple_decomp_ALS.m), 512^3 r=8",
        "value": K / dt, "unit": "iters/s", "n_gpus": 1, "steps": K, "warmup": W,
        "ms_per_step": dt * 1e3 / K, "higher_is_better": True, "scaling": "strong",
        "vs_baseline": None, "dtype": "f64", "data": "synthetic",
        "config": {"workload": "triple_decomp_ALS on config 4: synthetic %dx%dx%d fp64 r=%d "
                               "low-rank + 5%% outliers" % (n1, n2, n3, r),
                   "n1": n1, "n2": n2, "n3": n3, "r": r, "parallelism": "mode1-shard x1"},
        "errHist_final": float(res["errHist"][-1]), "k_final": res["k"],
        "kernel_ms": {"fit": km["fit"], "mode3_mttkrp": km["mode3"],
                      "iteration_events": km["iteration"], "samples": km["samples"]},
        "roofline": {"bound": "mfma", "achieved": tfs, "peak": 78.6, "unit": "TFLOP/s",
                     "frac": tfs / 78.6 if tfs else None, "traffic": None,
                     "kernel": "k_als_fit (triple product + error + W)",
                     "algorithmic_flops_per_launch": fit_flops,
                     "hbm_achieved_GBs": fit_bytes / (km["fit"] * 1e-3) / 1e9 if km["fit"] else None},
        "cpu_baseline": cpu,
    }
    print(json.dumps(line), flush=True)
    s.close()


if __name__ == "__main__":
    sys.exit(main() or 0)
