"""The library's own multi-rank schedule with real ranks on one GPU.

RCCL refuses one GPU twice in a communicator, so these tests give libtritd a
host transport (tritd_comm_create_host: each all-reduce drains the session
stream and runs torch.distributed over gloo on a host copy).  Everything else
is the code path `bench.py --gpus N` runs: the sharded iterate_fused
schedule of solver.cpp (two all-reduces per iteration, K5's norm partials in
red1's tail sized to the largest shard, the stop test deferred behind the
next iteration's speculative M1 .. M2), agree_counts at session creation, and
for ALS the als.cpp schedule.  Shards are uneven and straddle 16 rows (n1 = 33
on 2 ranks: 17 | 16; n1 = 49 on 3 ranks: 17 | 16 | 16), so the ranks launch
different K5 grids.  Results must match the oracle's unsharded solve
(triple_decomp_ADMM.m:15-68) at the tolerances of test_gpu_parity.py.

With the spec key `full_device` a rank takes its shard the way
include/tritd.h describes the multi-GPU call — D(i0,0,0) of the whole device
tensor, ldD = n1 — and reports its rre_parts against L*(i0,0,0); the parent
checks that the parts sum to the whole.
"""
import os
import socket

import numpy as np
import pytest

from conftest import ORACLE, PKG, load_golden, rel

pytestmark = pytest.mark.gpu


def _case(n1, stop, disp=False):
    from tritd import synth
    d = synth.low_rank_plus_outliers(n1, 10, 8, 2, seed=5, init_seed=9)
    opts = dict(synth.TRAFFIC_OPTS, maxIter=30, tol=0.2 if stop else 1e-5, disp=int(disp))
    return d, opts


def _worker(rank, world, spec, outdir):
    import sys
    for p in (PKG, ORACLE):
        sys.path.insert(0, p)
    import tritd
    from tritd.dist import shard_bounds
    if spec.get("rdzv"):  # bench.py's torch-free path (tritd.rendezvous)
        from tritd.rendezvous import StarGroup, make_host_comm as rz_host_comm
        # rank 0 binds its own port and publishes it through a file (a port
        # probed by the parent and bound later can be taken in between)
        pf = os.path.join(outdir, "rdzv_port")
        if rank == 0:
            ls = socket.socket()
            ls.bind(("127.0.0.1", 0))
            ls.listen(world)
            with open(pf + ".tmp", "w") as f:
                f.write(str(ls.getsockname()[1]))
            os.replace(pf + ".tmp", pf)
            group = StarGroup(0, world, 0, listen_fd=ls.detach(), timeout=120)
        else:
            import time
            t0 = time.monotonic()
            while not os.path.exists(pf):
                if time.monotonic() - t0 > 120:
                    raise TimeoutError("rank 0 did not publish its port")
                time.sleep(0.05)
            with open(pf) as f:
                group = StarGroup(rank, world, int(f.read()), timeout=120)
        dist = None
    else:
        import datetime
        import torch.distributed as dist
        from tritd.dist import make_host_comm
        # a file store: no TCP port to race for
        dist.init_process_group("gloo", init_method="file://" + os.path.join(outdir, "gloo_store"),
                                rank=rank, world_size=world, timeout=datetime.timedelta(seconds=120))
    kind = spec["kind"]
    if "golden" in spec:
        z = load_golden(spec["golden"])
        D = z["D"] if kind == "admm" else z["X"]
        r, opts, A0, B0, C0 = int(z["r"]), z["opts"], z["A0"], z["B0"], z["C0"]
    else:
        d, opts = _case(spec["n1"], spec["stop"], spec.get("disp", False))
        D, r, A0, B0, C0 = d["D"], 2, d["A0"], d["B0"], d["C0"]
    n1, n2, n3 = D.shape
    i0, i1 = shard_bounds(n1, world, rank)
    comm = rz_host_comm(group, 0) if dist is None else make_host_comm(dist, rank, world, 0)
    Dl = np.asfortranarray(D[i0:i1])
    dLstar = None
    if spec.get("full_device"):
        # the natural multi-GPU call of include/tritd.h: every rank holds the
        # WHOLE D (and L*) on the device and hands its session D(i0,0,0) with
        # ldD = n1 (odd i0: a pointer that is only element-aligned)
        from tritd import hip
        assert kind == "admm" and "golden" not in spec
        dD = hip.DeviceArray.from_host(np.asfortranarray(D))
        dLstar = hip.DeviceArray.from_host(np.asfortranarray(d["Lstar"]))
        s = tritd.Session(r, opts, A0, B0, C0, n1=n1, n2=n2, n3=n3, i0=i0, i1=i1,
                          d_device_ptr=dD.ptr + 8 * i0, ldD=n1, device=0, comm=comm, probe=False)
        dD.free()
    elif kind == "admm":
        s = tritd.Session(r, opts, A0, B0, C0, n1=n1, n2=n2, n3=n3, i0=i0, i1=i1, D=Dl, device=0,
                          comm=comm, probe=False)
    else:
        s = tritd.AlsSession(r, opts, A0, B0, C0, n1=n1, n2=n2, n3=n3, i0=i0, i1=i1, X=Dl,
                             device=0, comm=comm)
    s.run(int(opts["maxIter"]))
    s.sync()
    res = s.get()
    if dLstar is not None:  # this rank's part of the driver's RRE against L*(i0,0,0), ldX = n1
        res["num"], res["den"] = s.rre_parts(dLstar.ptr + 8 * i0, n1)
        dLstar.free()
    s.close()
    comm.close()
    np.savez(os.path.join(outdir, f"rank{rank}.npz"), i0=i0, i1=i1,
             **{k: v for k, v in res.items() if k != "k"}, k=res["k"])
    if dist is None:
        group.barrier()
        group.close()
        return
    dist.barrier()
    dist.destroy_process_group()


def _run(tmp_path, world, spec):
    # stdlib spawn (not torch.multiprocessing): the ranks import torch for
    # gloo, this test process does not (it stays on /opt/rocm's HIP runtime)
    import multiprocessing as mp
    ctx = mp.get_context("spawn")
    ps = [ctx.Process(target=_worker, args=(q, world, spec, str(tmp_path))) for q in range(world)]
    for p in ps:
        p.start()
    for p in ps:
        p.join(150)
    for p in ps:
        if p.is_alive():
            p.terminate()
            p.join()
    assert all(p.exitcode == 0 for p in ps), [p.exitcode for p in ps]
    return [np.load(tmp_path / f"rank{q}.npz") for q in range(world)]


def _assemble(zs, shapeA, shapeO=None):
    A = np.zeros(shapeA, order="F")
    O = E = None
    if shapeO is not None:
        O = np.zeros(shapeO, order="F")
        E = np.zeros(shapeO, order="F")
    for z in zs:
        i0, i1 = int(z["i0"]), int(z["i1"])
        A[i0:i1] = z["A"][i0:i1]
        if O is not None:
            O[i0:i1], E[i0:i1] = z["O"], z["E"]
    return A, O, E


@pytest.mark.timeout(240)
@pytest.mark.parametrize("world,n1,stop,disp", [(2, 33, False, False), (2, 33, True, True),
                                                (3, 49, False, False), (3, 49, True, False)])
def test_library_schedule_uneven_ranks_match_oracle(tmp_path, world, n1, stop, disp):
    import tritd_oracle as orc
    d, opts = _case(n1, stop, disp)
    rA, rB, rC, rO, reh, rE, rk, _ = orc.triple_decomp_ADMM(d["D"], 2, opts, d["A0"], d["B0"],
                                                            d["C0"], printer=lambda s: None)
    assert (rk < 30) == stop
    zs = _run(tmp_path, world, dict(kind="admm", n1=n1, stop=stop, disp=disp))
    for z in zs:
        assert int(z["k"]) == rk
        np.testing.assert_allclose(z["errHist"], reh, rtol=1e-8, atol=1e-13)
        assert rel(z["B"], rB) < 1e-8 and rel(z["C"], rC) < 1e-8
    A, O, E = _assemble(zs, rA.shape, rO.shape)
    assert rel(A, rA) < 1e-8 and rel(O, rO) < 1e-9 and rel(E, rE) < 1e-9


@pytest.mark.timeout(240)
@pytest.mark.parametrize("world,n1", [(2, 33), (3, 49)])
def test_ranks_on_the_whole_device_tensor_and_sharded_rre_parts(tmp_path, world, n1):
    """Every rank creates its session from D(i0,0,0) of the whole device
    tensor with ldD = n1 (i0 = 17, 33: odd) and calls rre_parts on
    L*(i0,0,0) with ldX = n1, over the torch-free rendezvous transport (the
    device-pointer entry points want one HIP runtime in the process).  The
    solve matches the oracle as above, and the ranks' num and den sum to the
    float64 restatement on the assembled factors at the tolerances of
    tests/test_gpu_session_boundary.py (boundary_cases.rre_reference).
    Measured on an MI355X: both sums equal the restatement to the last bit in
    either world (num tolerance 3.9e-12 and 1.5e-12)."""
    import boundary_cases as bc
    import tritd_oracle as orc
    d, opts = _case(n1, False)
    rA, rB, rC, rO, reh, rE, rk, _ = orc.triple_decomp_ADMM(d["D"], 2, opts, d["A0"], d["B0"],
                                                            d["C0"], printer=lambda s: None)
    zs = _run(tmp_path, world, dict(kind="admm", n1=n1, stop=False, rdzv=True, full_device=True))
    assert [int(z["i0"]) for z in zs][1:] == [17, 33][:world - 1]
    for z in zs:
        assert int(z["k"]) == rk
        np.testing.assert_allclose(z["errHist"], reh, rtol=1e-8, atol=1e-13)
        assert rel(z["B"], rB) < 1e-8 and rel(z["C"], rC) < 1e-8
        np.testing.assert_array_equal(z["B"], zs[0]["B"])
        np.testing.assert_array_equal(z["C"], zs[0]["C"])
    A, O, E = _assemble(zs, rA.shape, rO.shape)
    assert rel(A, rA) < 1e-8 and rel(O, rO) < 1e-9 and rel(E, rE) < 1e-9
    L = orc.triple_product(A, zs[0]["B"], zs[0]["C"])
    num_ref, den_ref, rtol_num, rtol_den = bc.rre_reference(L, d["Lstar"])
    num, den = sum(float(z["num"]) for z in zs), sum(float(z["den"]) for z in zs)
    print("  sharded rre_parts world=%d: num %.17g (ref %.17g) dev %.1e of %.1e | den dev %.1e of %.1e"
          % (world, num, num_ref, abs(num - num_ref) / num_ref, rtol_num,
             abs(den - den_ref) / den_ref, rtol_den), flush=True)
    assert all(float(z["num"]) > 0 and float(z["den"]) > 0 for z in zs)
    assert abs(num - num_ref) <= rtol_num * num_ref
    assert abs(den - den_ref) <= rtol_den * den_ref


@pytest.mark.timeout(240)
@pytest.mark.parametrize("name", ["g17x16x20_r8", "g12x10x8_r2_stop"])
def test_library_schedule_world2_matches_golden(tmp_path, name):
    g = load_golden(name)
    zs = _run(tmp_path, 2, dict(kind="admm", golden=name))
    for z in zs:
        assert int(z["k"]) == g["k"]
        np.testing.assert_allclose(z["errHist"], g["errHist"], rtol=1e-8, atol=1e-13)
        assert rel(z["B"], g["B"]) < 1e-8 and rel(z["C"], g["C"]) < 1e-8
    A, O, E = _assemble(zs, g["A"].shape, g["O"].shape)
    assert rel(A, g["A"]) < 1e-8 and rel(O, g["O"]) < 1e-9 and rel(E, g["E"]) < 1e-9


@pytest.mark.timeout(240)
def test_als_library_schedule_world2_matches_golden(tmp_path):
    name = "als20x24x18_r5_stop"
    g = load_golden(name)
    zs = _run(tmp_path, 2, dict(kind="als", golden=name))
    for z in zs:
        assert int(z["k"]) == g["k"]
        np.testing.assert_allclose(z["errHist"], g["errHist"], rtol=1e-9, atol=1e-14)
        assert rel(z["B"], g["B"]) < 1e-8 and rel(z["C"], g["C"]) < 1e-8
    A, _, _ = _assemble(zs, g["A"].shape)
    assert rel(A, g["A"]) < 1e-8


@pytest.mark.timeout(240)
def test_rendezvous_host_transport_world2_matches_golden(tmp_path):
    """bench.py's torch-free rank path (tritd.rendezvous.StarGroup, VERDICT r5
    next 3a): two ranks on the box's GPU, the host all-reduce transport over
    the rendezvous sockets, against a golden (triple_decomp_ADMM.m:15-68)."""
    name = "g17x16x20_r8"
    g = load_golden(name)
    zs = _run(tmp_path, 2, dict(kind="admm", golden=name, rdzv=True))
    for z in zs:
        assert int(z["k"]) == g["k"]
        np.testing.assert_allclose(z["errHist"], g["errHist"], rtol=1e-8, atol=1e-13)
        assert rel(z["B"], g["B"]) < 1e-8 and rel(z["C"], g["C"]) < 1e-8
    A, O, E = _assemble(zs, g["A"].shape, g["O"].shape)
    assert rel(A, g["A"]) < 1e-8 and rel(O, g["O"]) < 1e-9 and rel(E, g["E"]) < 1e-9


@pytest.mark.timeout(240)
@pytest.mark.parametrize("name", ["g30_r3", "g12x10x8_r2_stop"])
def test_rccl_one_rank_through_rendezvous_matches_golden(name):
    """The RCCL transport as bench.py's ranks create it — unique id through
    tritd.rendezvous, no torch in the process, /opt/rocm's HIP / HSA / RCCL —
    with one rank (the box has one GPU): the sharded schedule with real
    ncclAllReduce calls on the session stream, against a golden."""
    import tritd
    from tritd._lib import runtime_stack
    from tritd.rendezvous import StarGroup, make_comm
    g = load_golden(name)
    comm = make_comm(StarGroup(0, 1, 0), 0)
    assert comm.info() == (1, 0, "rccl")
    n1, n2, n3 = g["D"].shape
    s = tritd.Session(int(g["r"]), g["opts"], g["A0"], g["B0"], g["C0"], n1=n1, n2=n2, n3=n3,
                      i0=0, i1=n1, D=np.asfortranarray(g["D"]), device=0, comm=comm, probe=False)
    s.run(int(g["opts"]["maxIter"]))
    s.sync()
    res = s.get()
    s.close()
    comm.close()
    assert int(res["k"]) == g["k"]
    np.testing.assert_allclose(res["errHist"], g["errHist"], rtol=1e-8, atol=1e-13)
    assert rel(res["A"], g["A"]) < 1e-8 and rel(res["B"], g["B"]) < 1e-8
    assert rel(res["C"], g["C"]) < 1e-8
    assert rel(res["O"], g["O"]) < 1e-9 and rel(res["E"], g["E"]) < 1e-9
    st = runtime_stack()
    assert "torch" not in __import__("sys").modules
    assert all(len(v) == 1 and v[0].startswith("/opt/rocm") for v in st.values()), st
