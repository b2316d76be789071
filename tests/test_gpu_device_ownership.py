"""GPU tests of who frees what: every solver, halo exchange and group gives back exactly what it took on the device, counted
by the library itself (mgcfd.live_device_resources: allocations, bytes, handles — no tolerance, the figures are integers
the library keeps); replacing a level's halo exchange frees the old one; a refused mgcfd_rank_set_halo changes nothing; a
solver created after one that was destroyed while attached is a rank of nothing.  All on the golden m6_2lvl mesh (336 nodes,
two levels), its ranks on this one GPU."""
import ctypes as C
import gc
import types

import numpy as np
import pytest

import free_stream_emulator as fse

pytestmark = pytest.mark.gpu

CASE = "m6_2lvl"
ERR_ARG = 1


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.int64)


def _live():
    import mgcfd
    gc.collect()                        # (a solver another test dropped without close() goes now, not in the middle of this one)
    return mgcfd.live_device_resources()


@pytest.fixture(scope="module")
def case():
    """The mesh, its levels as arrays and its two parts — read and partitioned once, never changed."""
    import mgcfd
    from mgcfd.partition import partition_hierarchy, rcb_partition
    mesh = mgcfd.Mesh("input.dat", fse.case_input(CASE), fse.case_duplicate(CASE))
    levels = [mesh.level(l) for l in range(mesh.num_levels)]
    H = partition_hierarchy(levels, rcb_partition(np.asarray(levels[0]["coords"]).reshape(-1, 3), 2))
    yield types.SimpleNamespace(mesh=mesh, levels=levels, variant=mesh.variant, H=H)
    mesh.close()


def _rank_solvers(case):
    import mgcfd
    solvers = []
    for h in case.H:
        lv, owned, keys = h.solver_args()
        solvers.append(mgcfd.Solver.from_arrays(lv, case.variant, n_owned=owned, order_keys=keys))
    return solvers


def _group(case, exchange=True):
    import mgcfd
    solvers = _rank_solvers(case)
    g = mgcfd.Group(solvers)
    for h, s in zip(case.H, solvers):
        for l in range(len(case.levels)):
            s.rank_set_halo(l, h.levels[l])
    if exchange:
        for l in range(len(case.levels)):
            g.exchange(l)
    return solvers, g


def _raw_set_halo(s, level, peers, send, recv):
    """mgcfd_rank_set_halo as given (Solver.rank_set_halo sorts the peers): the return code."""
    n = len(peers)
    keep = [np.ascontiguousarray(a, dtype=np.int64) for a in list(send) + list(recv)]
    pa = (C.c_int * n)(*peers)
    sc = (C.c_int64 * n)(*[len(a) for a in keep[:n]])
    rc = (C.c_int64 * n)(*[len(a) for a in keep[n:]])
    sp = (C.c_void_p * n)(*[a.ctypes.data for a in keep[:n]])
    rp = (C.c_void_p * n)(*[a.ctypes.data for a in keep[n:]])
    return s.lib.mgcfd_rank_set_halo(s.handle, level, n, pa, sc, sp, rc, rp)


def test_one_solver_leaves_nothing_alive(case):
    import mgcfd
    base = _live()
    s = mgcfd.Solver.from_mesh(case.mesh)
    alive = mgcfd.live_device_resources()
    print("baseline", base, "with one solver", alive)
    assert alive["allocations"] - base["allocations"] >= 4 * len(case.levels) and alive["handles"] > base["handles"]
    s.run_cycles(2, loads=True)
    s.close()
    assert _live() == base


def test_a_group_leaves_nothing_alive(case):
    base = _live()
    solvers, g = _group(case)
    g.cycles(2)
    g.sweeps(0, 4)                      # (four sweeps: a host thread per rank; direct mode and the minima's words are in place)
    g.synchronize()
    assert solvers[0].rank_info()["transport"] == "in-process group"
    g.close()
    for s in solvers:
        s.close()
    assert _live() == base


@pytest.mark.parametrize("option,value", [("flux_variant", 1 << 2), ("exact", 0)])
def test_arrays_an_option_uploads_later_go_too(case, option, value):
    import mgcfd
    base = _live()
    s = mgcfd.Solver.from_mesh(case.mesh)
    before = mgcfd.live_device_resources()
    s.set_option(option, value)
    s.run_cycles(1)
    after = mgcfd.live_device_resources()
    print(option, value, "allocations", before["allocations"], "->", after["allocations"])
    assert after["allocations"] > before["allocations"], "the option uploaded nothing: the case tests nothing"
    s.close()
    assert _live() == base


def test_replacing_an_exchange_frees_the_old_one(case):
    import mgcfd
    base = _live()
    s, other = _rank_solvers(case)
    other.close()
    s.rank_attach_plain(0, 2)
    P = case.H[0].levels[0]
    s.rank_set_halo(0, P)
    noted = mgcfd.live_device_resources()
    for _ in range(20):
        s.rank_set_halo(0, P)
    assert mgcfd.live_device_resources() == noted
    assert s.rank_halo_info(0)["nodes_sent"] == sum(len(v) for v in P.send.values())
    s.close()
    assert _live() == base

    # ... and not under a group that has swept: its ranks hold addresses into the exchange
    solvers, g = _group(case)
    g.sweeps(0, 1)
    g.synchronize()
    noted = mgcfd.live_device_resources()
    with pytest.raises(mgcfd.MgcfdError) as e:
        solvers[0].rank_set_halo(0, P)
    assert e.value.code == ERR_ARG and "group" in str(e.value)
    assert mgcfd.live_device_resources() == noted
    g.sweeps(0, 1)                      # (the exchange is still the group's)
    g.synchronize()
    g.close()
    for r in solvers:
        r.close()
    assert _live() == base


def test_a_refused_set_halo_changes_nothing(case):
    import mgcfd
    base = _live()
    P = case.H[0].levels[0]
    peers = sorted(set(P.send) | set(P.recv))
    assert peers == [1]
    results = []
    for spoil in (True, False):
        solvers, g = _group(case, exchange=False)
        s = solvers[0]
        if spoil:
            noted = mgcfd.live_device_resources()
            ghost = np.array(P.send[1], dtype=np.int64)
            ghost[-1] = P.n_owned                                           # a ghost in a send list
            assert _raw_set_halo(s, 0, [1], [ghost], [P.recv[1]]) == ERR_ARG
            assert "owned" in s.lib.mgcfd_last_error().decode()
            empty = np.zeros(0, np.int64)
            assert _raw_set_halo(s, 0, [1, 0], [P.send[1], empty], [P.recv[1], empty]) == ERR_ARG      # descending peers
            assert "ascending" in s.lib.mgcfd_last_error().decode()
            assert mgcfd.live_device_resources() == noted
        for l in range(len(case.levels)):
            g.exchange(l)
        g.sweeps(0, 2)
        g.synchronize()
        results.append([r.get(0, "variables")[:h.levels[0].n_owned] for h, r in zip(case.H, solvers)])
        g.close()
        for r in solvers:
            r.close()
    for r, (got, want) in enumerate(zip(*results)):
        assert np.array_equal(_bits(got), _bits(want)), f"rank {r}: the sweeps after the refused calls differ from a fresh solver's"
    assert _live() == base


def test_a_solver_made_after_an_undetached_one_is_no_rank(case):
    """(mgcfd_rank_exchange on a level without halo lists says so before it asks what the solver is a rank of; the call that
    asks first, mgcfd_rank_set_halo, is the one whose message is checked.)"""
    import mgcfd
    base = _live()
    solvers, g = _group(case)
    for s in solvers:
        s.close()                       # (no rank_detach, and the group is still there)
    fresh = [s for _ in range(4) for s in _rank_solvers(case)]
    assert len(fresh) == 8
    for k, s in enumerate(fresh):
        info = s.rank_info()
        assert info["transport"] == "none" and info["ranks"] == 1, info
        with pytest.raises(mgcfd.MgcfdError) as e:
            s.rank_set_halo(0, case.H[k % 2].levels[0])
        assert e.value.code == ERR_ARG and "not a rank of anything" in str(e.value)
        with pytest.raises(mgcfd.MgcfdError) as e:
            s.rank_exchange(0)
        assert e.value.code == ERR_ARG
    g.close()
    for s in fresh:
        s.close()
    assert _live() == base
