"""mgcfd.distributed.set_free_stream_all with two gloo ranks on the CPU: every rank ends up with RANK 0's free stream, bit
for bit, whatever it passed itself, and the ranks' runs agree with one solver.  As in tests/test_distributed_gloo.py the
per-rank solver is a stand-in built on the oracle (the composed V-cycle of tests/free_stream_emulator.py); the product
passes a mgcfd.api.Solver to the very same helper."""
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


class OracleSolver:
    """What the helper needs of mgcfd.api.Solver: set_free_stream(mach, alpha_deg, reinitialise)."""

    def __init__(self, oracle, fse):
        self.fse = fse
        self.co = fse.ComposedOracle(oracle, CASE)
        self.calls = []

    def set_free_stream(self, mach, alpha_deg, reinitialise=True):
        self.calls.append((mach, alpha_deg, reinitialise))
        self.co.set_far_field(self.fse.free_stream_constants(mach, alpha_deg), reinitialise)


def _free_port():
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    port = s.getsockname()[1]
    s.close()
    return port


def _worker(rank, world, port, pairs, out_dir):
    for p in ("mg-cfd-app-plain_amd", "oracle", "tests"):
        sys.path.insert(0, os.path.join(ROOT, p))
    import free_stream_emulator as fse
    import oracle_py
    from mgcfd.distributed import set_free_stream_all
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port))
    dist.init_process_group("gloo", rank=rank, world_size=world)
    solver = OracleSolver(oracle_py, fse)
    rms = []
    for k, pair in enumerate(pairs):
        # rank 0 names the free stream; the other ranks name nothing, or something else that must be ignored
        mine = pair if rank == 0 else ((None, None) if k == 0 else (9.0, -45.0))
        got = set_free_stream_all(solver, mine[0], mine[1], reinitialise=(k == 0) if rank == 0 else True, dist=dist)
        assert got == pair, (rank, got, pair)
        rc, r = solver.co.cycles(CYCLES)
        assert rc == 0
        rms.append(r)
    assert solver.calls == [(pairs[0][0], pairs[0][1], True), (pairs[1][0], pairs[1][1], False)], solver.calls
    np.save(os.path.join(out_dir, f"vars_{rank}.npy"), solver.co.variables(0))
    np.save(os.path.join(out_dir, f"ff_{rank}.npy"), solver.co.ff17)
    np.save(os.path.join(out_dir, f"rms_{rank}.npy"), np.concatenate(rms))
    dist.barrier()
    dist.destroy_process_group()


@pytest.mark.timeout(300)
def test_two_gloo_ranks_take_rank_zeros_free_stream(tmp_path, oracle):
    import free_stream_emulator as fse
    from mgcfd.distributed import set_free_stream_all
    pairs = list(fse.GPU_PAIRS)
    mp.spawn(_worker, args=(2, _free_port(), pairs, str(tmp_path)), nprocs=2, join=True)
    # one solver, no process group: the helper only sets it
    one = OracleSolver(oracle, fse)
    rms = []
    for k, pair in enumerate(pairs):
        assert set_free_stream_all(one, pair[0], pair[1], reinitialise=(k == 0)) == pair
        rc, r = one.co.cycles(CYCLES)
        assert rc == 0
        rms.append(r)
    bits = lambda a: np.ascontiguousarray(a, dtype=np.float64).view(np.int64)
    for r in range(2):
        assert np.array_equal(bits(np.load(tmp_path / f"ff_{r}.npy")), bits(fse.free_stream_constants(*pairs[-1])))
        assert np.array_equal(bits(np.load(tmp_path / f"vars_{r}.npy")), bits(one.co.variables(0)))
        assert np.array_equal(bits(np.load(tmp_path / f"rms_{r}.npy")), bits(np.concatenate(rms)))
