"""Child process of tests/test_gpu_free_stream_ranks.py: what has to run in a process of its own, because a process group
is made for it (backend "nccl").

  python free_stream_children.py nccl_helper OUT.npy      a one-rank RCCL process group through distributed.set_free_stream_all
"""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in ("mg-cfd-app-plain_amd", "oracle", "tests"):
    sys.path.insert(0, os.path.join(ROOT, p))

import free_stream_emulator as fse     # noqa: E402

CASE = "m6_2lvl"


def nccl_helper(out):
    """set_free_stream_all under backend "nccl" (RCCL takes device tensors only), one rank: the far field it leaves."""
    import socket
    import torch
    import torch.distributed as dist
    import mgcfd
    from mgcfd.distributed import set_free_stream_all
    sock = socket.socket(); sock.bind(("127.0.0.1", 0)); port = sock.getsockname()[1]; sock.close()
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port))
    torch.cuda.set_device(0)
    dist.init_process_group("nccl", rank=0, world_size=1, device_id=torch.device("cuda", 0))
    mesh = mgcfd.Mesh("input.dat", fse.case_input(CASE), fse.case_duplicate(CASE))
    s = mgcfd.Solver.from_mesh(mesh)
    pair = fse.GPU_PAIRS[0]
    assert set_free_stream_all(s, pair[0], pair[1], reinitialise=True, dist=dist) == pair
    assert s.free_stream() == pair
    np.save(out, s.far_field())
    s.close()
    mesh.close()
    dist.barrier()
    dist.destroy_process_group()


if __name__ == "__main__":
    {"nccl_helper": nccl_helper}[sys.argv[1]](sys.argv[2])
