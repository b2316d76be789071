"""Host-side checks of who frees what in the library: solver.cpp destroys nothing by hand — device memory goes through
DeviceOwner and the handles through the unique_ptr aliases of csrc/device_owner.hpp — and the introspection call the GPU
tests count with is part of the ABI."""
import os
import re

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "mg-cfd-app-plain_amd", "csrc")
BY_HAND = ("hipFree(", "hipEventDestroy(", "hipStreamDestroy(", "hipGraphExecDestroy(", "hipMalloc(", "hipExtMallocWithFlags(",
           "hipIpcCloseMemHandle(")


def _code_lines(path):
    with open(path) as f:
        return [(n, line) for n, line in enumerate(f, 1)]


def test_solver_cpp_frees_nothing_by_hand():
    hits = [(n, line.strip()) for n, line in _code_lines(os.path.join(CSRC, "solver.cpp")) if any(t in line for t in BY_HAND)]
    # the one exception: the warm-up thread's hipFree(nullptr), which only wakes the runtime
    assert len(hits) == 1 and "hipFree(nullptr)" in hits[0][1] and "g_warm" in hits[0][1], hits
    text = open(os.path.join(CSRC, "solver.cpp")).read()
    for gone in ("in_block", "block_bytes", "g_comms", "~RankLoads", "dev_alloc", "dev_upload"):
        assert gone not in text, gone


def test_the_owner_header_destroys_each_kind_in_one_place():
    text = open(os.path.join(CSRC, "device_owner.hpp")).read()
    for call in ("hipEventDestroy(", "hipStreamDestroy(", "hipGraphExecDestroy(", "hipIpcCloseMemHandle("):
        assert text.count(call) == 1, call
    assert len(re.findall(r"struct \w+ \{ void operator\(\)", text)) == 4         # the deleters


def test_the_solver_destructor_only_synchronises():
    text = open(os.path.join(CSRC, "solver.cpp")).read()
    body = text[text.index("mgcfd_solver::~mgcfd_solver()"):]
    body = body[body.index("{") + 1:body.index("\n}\n")]
    assert len([l for l in body.splitlines() if l.strip()]) <= 6, body


def test_live_device_resources_is_exported():
    import mgcfd
    assert "mgcfd_live_device_resources" in mgcfd.EXPORTED_SYMBOLS
    header = open(os.path.join(ROOT, "include", "mgcfd.h")).read()
    assert "int mgcfd_live_device_resources(int64_t out[3]);" in header
    assert callable(mgcfd.live_device_resources)
