"""GPU tests of the run-time time step on partitioned levels: in-process groups of two and three parts on this one GPU, the
one-rank RCCL form and the multi-process HIP IPC form each against ONE solver that holds the whole level, bit for bit, under
"local" and "global" at tse.RANK_CFL; the group's agreement rule; no all-reduce under a local mode; the torch path
(PartitionedCycle).  Everything here runs its ranks on ONE GPU: never run on more than one GPU."""
import os
import subprocess
import sys

import numpy as np
import pytest

import free_stream_emulator as fse
import time_step_emulator as tse

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CASES, K, CFL = tse.GPU_CASES, tse.GPU_CYCLES, tse.RANK_CFL
MODES = ("local", "global")
REF = (0.25, -0.125, 0.375)


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.int64)


def _same(got, want, what):
    assert np.array_equal(_bits(got), _bits(want)), f"{what}: max |difference| {np.abs(np.asarray(got) - np.asarray(want)).max():.3e}"


def _levels(case):
    import mgcfd
    mesh = mgcfd.Mesh("input.dat", fse.case_input(case), fse.case_duplicate(case))
    levels = [mesh.level(l) for l in range(mesh.num_levels)]
    for L in levels:
        if np.size(L["coords"]) == 0:                         # (a single-level fvcorr input has no .coords file)
            L["coords"] = None
    return mesh, levels, mesh.variant


def _parts(levels, n):
    from mgcfd.partition import rcb_partition
    c = levels[0].get("coords")
    if c is None:
        return (np.arange(levels[0]["nel"]) * n) // levels[0]["nel"]
    return rcb_partition(np.asarray(c).reshape(-1, 3), n)


def _group(levels, variant, part0):
    import mgcfd
    from mgcfd.partition import partition_hierarchy
    H = partition_hierarchy(levels, part0)
    solvers = []
    for h in H:
        lv, owned, keys = h.solver_args()
        solvers.append(mgcfd.Solver.from_arrays(lv, variant, n_owned=owned, order_keys=keys))
    g = mgcfd.Group(solvers)
    for h, s in zip(H, solvers):
        for l in range(len(levels)):
            s.rank_set_halo(l, h.levels[l])
            s.rank_set_wall_slots(l, h.levels[l])
    for l in range(len(levels)):
        g.exchange(l)
    return H, solvers, g


@pytest.mark.parametrize("n_parts", [2, 3])
@pytest.mark.parametrize("case", CASES)
def test_group_equals_one_solver(case, n_parts, oracle):
    """Group.set_time_step, Group.cycles(loads=True), then Group.sweeps on level 0: owned nodes of every level and the loads
    history bitwise the one-solver run's — itself the emulator's —, under local, then (state kept) global steps."""
    import mgcfd
    mesh, levels, variant = _levels(case)
    whole = mgcfd.Solver.from_arrays(levels, variant)
    H, solvers, g = _group(levels, variant, _parts(levels, n_parts))
    em = tse.TimeStepOracle(oracle, case)
    for mode in MODES:
        whole.set_time_step(mode, CFL)
        g.set_time_step(mode, CFL)
        em.set_time_step(mode, CFL)
        assert all(s.time_step_control() == (mode, CFL) for s in solvers)
        want_rms, want = whole.run_cycles(K, loads=True, ref_point=REF)
        assert em.cycles(K)[0] == 0
        _same(whole.get(0, "variables"), em.variables(0), f"{case} {mode}: the one solver against the emulator")
        rms, hist = g.cycles(K, loads=True, ref_point=REF)
        _same(hist, want, f"{case} {mode} {n_parts} parts: loads history")
        assert np.allclose(rms, want_rms, rtol=1e-12, atol=0)
        whole.smooth(0, fse.SWEEPS)
        assert em.sweeps(0, fse.SWEEPS) == 0
        _same(whole.get(0, "variables"), em.variables(0), f"{case} {mode}: sweeps of the one solver against the emulator")
        g.sweeps(0, fse.SWEEPS)
        g.synchronize()
        for h, s in zip(H, solvers):
            for l in range(len(levels)):
                P = h.levels[l]
                _same(s.get(l, "variables")[:P.n_owned], whole.get(l, "variables")[P.global_ids[:P.n_owned]],
                      f"{case} {mode} {n_parts} parts: rank {h.rank} level {l}")
                _same(s.get(l, "step_factors")[:P.n_owned], whole.get(l, "step_factors")[P.global_ids[:P.n_owned]],
                      f"{case} {mode} {n_parts} parts: step factors, rank {h.rank} level {l}")
    em.close()
    g.close()
    for s in solvers:
        s.close()
    whole.close()
    mesh.close()


def test_group_refuses_ranks_that_disagree():
    import mgcfd
    mesh, levels, variant = _levels("m6_2lvl")
    H, solvers, g = _group(levels, variant, _parts(levels, 3))
    g.set_time_step("local", CFL)
    g.cycles(1)
    for mode, cfl in (("global", CFL), ("local", 0.5)):      # another mode; the same mode at another CFL number
        solvers[1].set_time_step(mode, cfl)
        for call in (lambda: g.cycles(1), lambda: g.cycles(1, loads=True), lambda: g.sweeps(0, 1), lambda: g.sweeps_rms(0, 1),
                     lambda: g.surface_loads(0)):
            with pytest.raises(mgcfd.MgcfdError) as e:
                call()
            assert e.value.code == 1 and "rank 1" in str(e.value) and "time step" in str(e.value)
    for mode, cfl in ((9, 0.5), ("local", 0.0), ("local", float("nan"))):
        with pytest.raises(mgcfd.MgcfdError) as e:
            g.set_time_step(mode, cfl)
        assert e.value.code == 1
    assert solvers[0].time_step_control() == ("local", CFL) and solvers[1].time_step_control() == ("local", 0.5)
    solvers[1].set_time_step("local", CFL)
    g.cycles(1)                                               # in line again
    g.close()
    for s in solvers:
        s.close()
    mesh.close()


@pytest.mark.parametrize("graph", [0, 1])
@pytest.mark.parametrize("case", ["m6_2lvl", "fvcorr_1lvl"])
def test_one_rank_rccl_sweeps(case, graph):
    """mgcfd_rank_sweeps on an RCCL communicator of the one rank this box offers, with and without sweep graphs: sweeps under
    local, the setter (the rank's graphs go), sweeps under global — the plain solver's bits."""
    import mgcfd
    from mgcfd.partition import partition_level
    mesh, levels, variant = _levels(case)
    L = levels[0]
    n = fse.SWEEPS
    ref = mgcfd.Solver.from_arrays([L], variant)
    want = {}
    for mode in MODES:
        ref.set_time_step(mode, CFL)
        ref.smooth(0, n)
        want[mode] = (ref.get(0, "variables"), ref.get(0, "step_factors"))
    ref.close()
    P = partition_level(L, np.zeros(L["nel"], dtype=np.int64))[0]
    s = mgcfd.Solver.from_arrays([P.level], variant, n_owned=[P.n_owned])
    s.rank_attach_rccl(0, 1, mgcfd.rccl_unique_id())
    s.rank_set_halo(0, P)
    s.set_option("graph", graph)
    s.rank_exchange(0)
    replayed = 0
    for mode in MODES:
        s.set_time_step(mode, CFL)
        assert s.rank_graph_status(0)["graphs"] == 0, "the setter drops the rank's sweep graphs"
        s.rank_sweeps(0, n)
        _same(s.get(0, "variables")[:P.n_owned], want[mode][0][P.global_ids[:P.n_owned]], f"{case} {mode} graph={graph}")
        _same(s.get(0, "step_factors")[:P.n_owned], want[mode][1][P.global_ids[:P.n_owned]], f"{case} {mode} graph={graph}: step factors")
        st = s.rank_graph_status(0)
        if graph:
            assert not st["capture_refused"], st
            assert st["graphs"] >= 1 and st["sweeps_replayed"] > replayed, (mode, st, replayed)      # captured again, and replayed
            replayed = st["sweeps_replayed"]
    s.rank_detach()
    s.close()
    mesh.close()


def test_one_rank_rccl_cycles():
    """mgcfd_rank_cycles under local and global steps equals mgcfd_run_cycles."""
    import mgcfd
    from mgcfd.partition import partition_hierarchy
    mesh, levels, variant = _levels("m6_3lvl")
    whole = mgcfd.Solver.from_arrays(levels, variant)
    H = partition_hierarchy(levels, np.zeros(levels[0]["nel"], dtype=np.int64))
    lv, owned, keys = H[0].solver_args()
    s = mgcfd.Solver.from_arrays(lv, variant, n_owned=owned, order_keys=keys)
    s.rank_attach_rccl(0, 1, mgcfd.rccl_unique_id())
    for l in range(len(levels)):
        s.rank_set_halo(l, H[0].levels[l])
        s.rank_exchange(l)
    for mode in MODES:
        whole.set_time_step(mode, CFL)
        s.set_time_step(mode, CFL)
        want_rms = whole.run_cycles(K)
        rms = s.rank_cycles(K)
        for l in range(len(levels)):
            _same(s.get(l, "variables"), whole.get(l, "variables")[H[0].levels[l].global_ids], f"{mode}: level {l}")
        assert np.allclose(rms, want_rms, rtol=1e-12, atol=0.0)
    s.rank_detach()
    s.close()
    whole.close()
    mesh.close()


@pytest.mark.parametrize("ranks,lattice,sweeps,mesh,extra", [
    (2, 16, 6, "m6wing", ["--time-step", "local"]),
    (2, 16, 6, "m6wing", ["--time-step", "global"]),
    (3, 20, 7, "m6wing", ["--time-step", "local", "--fused"]),
    (3, 20, 7, "fvcorr", ["--time-step", "global"]),          # fvcorr under a global step: the all-reduce through the flags
    (2, 30, 5, "tet", ["--time-step", "local", "--one-by-one"]),
    # no rank holds every rank's export: a global step would have no all-reduce to go through (MGCFD_ERR_ARG, "needs the
    # all-reduce"); a local step asks for none
    (3, 20, 7, "m6wing", ["--time-step", "local", "--strips", "--neighbours-only"]),
])
def test_ranks_in_different_processes(ranks, lattice, sweeps, mesh, extra):
    """tools/ipc_ranks_check.py: `ranks` PROCESSES on this one GPU exchanging through HIP IPC, each comparing its owned nodes
    and its ghosts with the unpartitioned level under the same time-step policy, bit for bit; no wait may have given up."""
    r = subprocess.run([sys.executable, os.path.join(ROOT, "tools", "ipc_ranks_check.py"), "--ranks", str(ranks), "--lattice", str(lattice),
                        "--sweeps", str(sweeps), "--mesh", mesh, "--cfl", repr(CFL)] + extra, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    assert r.stdout.count("owned equal, ghosts equal, waits that gave up: 0") == ranks
    if "--neighbours-only" in extra:
        assert f"attached 1 of {ranks - 1} other ranks" in r.stdout      # the end slabs hold one export each


@pytest.mark.parametrize("fused", [False, True])
def test_torch_path_skips_the_all_reduce_under_a_local_mode(fused):
    """mgcfd.distributed.PartitionedCycle on three parts of this GPU (threads for ranks, in-process copies for the messages,
    as tests/test_gpu_parity.py drives it): K cycles under "local" never call the all-reduce hook, K more under "global" call it
    once per sweep and rank; every level's owned nodes equal mgcfd_run_cycles on the whole hierarchy, bit for bit."""
    import threading
    import mgcfd
    import torch
    from mgcfd.distributed import HipSolverAdapter, PartitionedCycle
    from mgcfd.partition import partition_hierarchy
    n_parts = 3
    dev = torch.device("cuda", 0)
    mesh, levels, variant = _levels("m6_3lvl")
    whole = mgcfd.Solver.from_arrays(levels, variant)
    H = partition_hierarchy(levels, _parts(levels, n_parts))
    tstream = torch.cuda.Stream()
    solvers, cyclers, calls = [], [], []
    barrier = threading.Barrier(n_parts)

    def exchange(cy, level):
        barrier.wait()
        for peer, buf in cy.buf_recv[level].items():
            buf.copy_(cyclers[peer].buf_send[level][cy.h.rank])
        barrier.wait()

    def allreduce_min(cy, level):
        calls.append((cy.h.rank, level))
        barrier.wait()
        if cy.h.rank == 0:
            m = torch.stack([c.s.min_tensor(level) for c in cyclers]).min(dim=0).values
            for c in cyclers:
                c.s.min_tensor(level).copy_(m)
        barrier.wait()

    for h in H:
        lv, owned, keys = h.solver_args()
        s = mgcfd.Solver.from_arrays(lv, variant, n_owned=owned, order_keys=keys)
        s.set_stream(tstream.cuda_stream)
        solvers.append(s)
        cyclers.append(PartitionedCycle(HipSolverAdapter(s, dev), h, None, exchange=exchange, allreduce_min=allreduce_min,
                                        make_buffer=lambda n: torch.empty(max(n, 1), dtype=torch.float64, device=dev), fused=fused))
    sweeps_per_cycle = len(levels) + max(0, len(levels) - 2)
    for mode in MODES:
        for s in solvers + [whole]:
            s.set_time_step(mode, CFL)
        whole.run_cycles(K)
        del calls[:]
        errors = []

        def run(cy):
            try:
                torch.cuda.set_device(0)
                torch.cuda.set_stream(tstream)
                for _ in range(K):
                    cy.cycle()
            except Exception as e:                               # pragma: no cover
                errors.append(e)
                barrier.abort()

        threads = [threading.Thread(target=run, args=(c,)) for c in cyclers]
        for th in threads:
            th.start()
        for th in threads:
            th.join()
        assert not errors, errors
        assert len(calls) == (0 if mode == "local" else K * sweeps_per_cycle * n_parts), (mode, len(calls))
        for h, s in zip(H, solvers):
            for l, P in enumerate(h.levels):
                _same(s.get(l, "variables")[:P.n_owned], whole.get(l, "variables")[P.global_ids[:P.n_owned]], f"{mode} fused={fused}: rank {h.rank} level {l}")
    for s in solvers:
        s.close()
    whole.close()
    mesh.close()
