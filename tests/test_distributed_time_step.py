"""mgcfd.distributed.set_time_step_all with two gloo ranks on the CPU: every rank ends up with RANK 0's time-step mode and
CFL number, bit for bit, whatever it passed itself, and the ranks' runs agree with one solver.  As in
tests/test_distributed_free_stream.py the per-rank solver is a stand-in built on the oracle (the emulator of
tests/time_step_emulator.py); the product passes a mgcfd.api.Solver to the very same helper."""
import os
import socket
import sys

import numpy as np
import pytest
import torch.distributed as dist
import torch.multiprocessing as mp

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CASE = "m6_2lvl"
CYCLES = 3
LEGS = [("local", 0.8), ("global", 1.5), ("local_legacy", 0.1 + 0.2)]      # (0.30000000000000004: every bit must travel)


class OracleSolver:
    """What the helper needs of mgcfd.api.Solver: set_time_step(mode, cfl)."""

    def __init__(self, oracle, tse):
        self.em = tse.TimeStepOracle(oracle, CASE)
        self.calls = []

    def set_time_step(self, mode="reference", cfl=0.5):
        self.calls.append((mode, cfl))
        self.em.set_time_step(mode, cfl)


def _free_port():
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    port = s.getsockname()[1]
    s.close()
    return port


def _worker(rank, world, port, out_dir):
    for p in ("mg-cfd-app-plain_amd", "oracle", "tests"):
        sys.path.insert(0, os.path.join(ROOT, p))
    import oracle_py
    import time_step_emulator as tse
    from mgcfd.distributed import set_time_step_all
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port))
    dist.init_process_group("gloo", rank=rank, world_size=world)
    solver = OracleSolver(oracle_py, tse)
    rms = []
    for k, leg in enumerate(LEGS):
        # rank 0 names the policy; the other ranks name nothing, or something else that must be ignored
        mine = leg if rank == 0 else ((None, None) if k == 0 else ("global", 9.0))
        got = set_time_step_all(solver, mine[0], mine[1], dist=dist)
        assert got == leg, (rank, got, leg)
        rc, r = solver.em.cycles(CYCLES)
        assert rc == 0
        rms.append(r)
    assert solver.calls == LEGS, solver.calls
    np.save(os.path.join(out_dir, f"vars_{rank}.npy"), solver.em.variables(0))
    np.save(os.path.join(out_dir, f"rms_{rank}.npy"), np.concatenate(rms))
    dist.barrier()
    dist.destroy_process_group()


@pytest.mark.timeout(300)
def test_two_gloo_ranks_take_rank_zeros_time_step(tmp_path, oracle):
    import time_step_emulator as tse
    from mgcfd.distributed import set_time_step_all
    mp.spawn(_worker, args=(2, _free_port(), str(tmp_path)), nprocs=2, join=True)
    one = OracleSolver(oracle, tse)                          # one solver, no process group: the helper only sets it
    rms = []
    for leg in LEGS:
        assert set_time_step_all(one, leg[0], leg[1]) == leg
        rc, r = one.em.cycles(CYCLES)
        assert rc == 0
        rms.append(r)
    bits = lambda a: np.ascontiguousarray(a, dtype=np.float64).view(np.int64)
    for r in range(2):
        assert np.array_equal(bits(np.load(tmp_path / f"vars_{r}.npy")), bits(one.em.variables(0)))
        assert np.array_equal(bits(np.load(tmp_path / f"rms_{r}.npy")), bits(np.concatenate(rms)))
    with pytest.raises(ValueError):
        set_time_step_all(one, "implicit", 0.5)
