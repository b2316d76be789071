"""GPU tests of the run-time free stream (mgcfd_set_free_stream and what goes with it) on ONE solver: cold and warm starts
against the composed oracle (tests/free_stream_emulator.py), bit for bit; captured graphs after a change; the per-kernel
entry points; the surface loads' p_inf; the fast mode.  Groups, ranks and the drop-in binary: tests/test_gpu_free_stream_ranks.py.

Every case of fse.GPU_CASES runs at every pair of fse.GPU_PAIRS; tests/test_host_free_stream.py asserts on the CPU that the
composed oracle stays valid for each of these combinations."""
import ctypes as C
import itertools

import numpy as np
import pytest

import free_stream_emulator as fse
import surface_loads_emulator as emu
from conftest import perturbed_state

pytestmark = pytest.mark.gpu

CASES, PAIRS, K = fse.GPU_CASES, fse.GPU_PAIRS, fse.GPU_CYCLES
REF = (0.25, -0.125, 0.375)
REL_RUN = 1e-10          # tests/test_gpu_order_free.py: level `variables` after whole cycles, max |difference| / max |value|
RMS_FAST = 1e-9          # ... and its RMS tolerance


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.int64)


def _same(got, want, what):
    assert np.array_equal(_bits(got), _bits(want)), f"{what}: max |difference| {np.abs(np.asarray(got) - np.asarray(want)).max():.3e}"


def _solver(case, graph=0, timing=0, exact=1):
    import mgcfd
    mesh = mgcfd.Mesh("input.dat", fse.case_input(case), fse.case_duplicate(case))
    s = mgcfd.Solver.from_mesh(mesh)
    s.set_option("graph", graph)
    s.set_option("timing", timing)
    s.set_option("exact", exact)
    return mesh, s


def _oracle_history(oracle, case, legs):
    """legs = [(pair, reinitialise, cycles), ...]: the composed oracle driven through them one cycle at a time; returns per
    leg the list of (level-0 variables, rms) after each of its cycles, and the final state of every level."""
    co = fse.ComposedOracle(oracle, case, fse.free_stream_constants(*legs[0][0]))
    out = []
    for pair, reinit, cycles in legs:
        co.set_far_field(fse.free_stream_constants(*pair), reinitialise=reinit)
        leg = []
        for _ in range(cycles):
            rc, rms = co.cycles(1)
            assert rc == 0
            leg.append((co.variables(0), rms[0]))
        out.append(leg)
    final = [co.variables(l) for l in range(co.n)]
    co.close()
    return out, final


@pytest.mark.parametrize("case", CASES)
def test_cold_start_at_each_pair(case, oracle):
    """Level-0 `variables` after k = 1..3 cycles bitwise the composed oracle's, the RMS history within the tolerance
    tests/test_gpu_parity.py uses (rtol 1e-12), under graph in {0, 1} x timing in {0, 4}.  The first run of a solver is a
    cold start of a fresh solver; the later ones re-initialise a solver that has run (at another pair, with its graphs)."""
    want = {pair: _oracle_history(oracle, case, [(pair, True, K)])[0][0] for pair in PAIRS}
    for graph, timing in itertools.product((0, 1), (0, 4)):
        mesh, s = _solver(case, graph, timing)
        for pair in PAIRS:
            for k in range(1, K + 1):
                s.set_free_stream(*pair, reinitialise=True)
                assert s.free_stream() == pair
                _same(s.far_field(), fse.free_stream_constants(*pair), "far_field()")
                rms = s.run_cycles(k)
                what = f"{case} {pair} graph={graph} timing={timing} k={k}"
                _same(s.get(0, "variables"), want[pair][k - 1][0], what)
                want_rms = np.array([w[1] for w in want[pair][:k]])
                print(what, "rms", rms, "want", want_rms)
                assert np.allclose(rms, want_rms, rtol=1e-12, atol=0), what
        s.close()
        mesh.close()


@pytest.mark.parametrize("case", CASES)
def test_default_pair_changes_nothing(case, oracle):
    import mgcfd
    runs = []
    for call in (False, True):
        for graph in (0, 1):
            mesh, s = _solver(case, graph)
            _same(s.far_field(), fse.oracle_default_ff17(oracle), "a fresh solver's far field")
            assert s.free_stream() == (1.2, 0.0)
            if call:
                s.set_free_stream(1.2, 0.0, True)
                _same(s.far_field(), fse.oracle_default_ff17(oracle), "far field after set_free_stream(1.2, 0.0)")
            rms, hist = s.run_cycles(K, loads=True, ref_point=REF)
            runs.append((rms, hist, [s.get(l, "variables") for l in range(s.num_levels)]))
            s.close()
            mesh.close()
    # runs = (never called, graph 0), (never called, graph 1), (called, graph 0), (called, graph 1)
    _same(runs[2][0], runs[0][0], "RMS, graph = 0")
    _same(runs[3][0], runs[1][0], "RMS, graph = 1")
    for rms, hist, state in runs[1:]:
        assert np.allclose(rms, runs[0][0], rtol=1e-12, atol=0)
        _same(hist, runs[0][1], "loads history")
        for l, v in enumerate(state):
            _same(v, runs[0][2][l], f"level {l}")
    _same(mgcfd.free_stream_constants(1.2, 0.0), fse.oracle_default_ff17(oracle), "constants")


@pytest.mark.parametrize("case", CASES)
def test_warm_start(case, oracle):
    """K cycles at pair A, set_free_stream(B, reinitialise=False), K cycles: every level bitwise the composed oracle driven
    the same way; and from the default free stream of a solver nobody set."""
    for a, b in ((PAIRS[0], PAIRS[1]), (PAIRS[1], PAIRS[0]), (fse.DEFAULT, PAIRS[0])):
        legs, final = _oracle_history(oracle, case, [(a, True, K), (b, False, K)])
        mesh, s = _solver(case)
        if a != fse.DEFAULT:
            s.set_free_stream(*a, reinitialise=True)
        rms_a = s.run_cycles(K)
        _same(s.get(0, "variables"), legs[0][-1][0], f"{case}: after the first leg at {a}")
        s.set_free_stream(*b, reinitialise=False)
        _same(s.get(0, "variables"), legs[0][-1][0], f"{case}: the state is kept by a warm set_free_stream")
        rms_b = s.run_cycles(K)
        for l in range(s.num_levels):
            _same(s.get(l, "variables"), final[l], f"{case}: {a} -> {b}, level {l}")
        assert np.allclose(rms_a, [w[1] for w in legs[0]], rtol=1e-12, atol=0)
        assert np.allclose(rms_b, [w[1] for w in legs[1]], rtol=1e-12, atol=0)
        s.close()
        mesh.close()


@pytest.mark.parametrize("case", CASES)
def test_graphs_are_captured_again_after_a_change(case):
    """graph = 1: cycles at A, set B (warm), cycles again — bitwise the same sequence with graph = 0; the same for sweeps
    (mgcfd_smooth's sweep graphs) and for the cycles that record loads.  A replay of what was captured at A would carry A's
    far field and p_inf."""
    a, b = PAIRS
    out = {}
    for graph in (0, 1):
        mesh, s = _solver(case, graph)
        s.set_free_stream(*a)
        r1, h1 = s.run_cycles(1, loads=True, ref_point=REF)          # (the cycle that records loads is a graph of its own)
        r2 = s.run_cycles(K - 1)
        s.set_free_stream(*b, reinitialise=False)
        r3, h3 = s.run_cycles(1, loads=True, ref_point=REF)
        r4 = s.run_cycles(K - 1)
        state = [s.get(l, "variables") for l in range(s.num_levels)]
        # sweeps of level 0 alone (mgcfd_smooth's sweep graphs), fse.SWEEPS at A from its far field, then as many at B
        s.set_free_stream(*a)
        s.smooth(0, fse.SWEEPS)
        s.set_free_stream(*b, reinitialise=False)
        s.smooth(0, fse.SWEEPS)
        out[graph] = ([r1, r2, r3, r4, h1, h3], state + [s.get(0, "variables")])
        s.close()
        mesh.close()
    for k, (x, y) in enumerate(zip(out[0][0], out[1][0])):
        _same(y, x, f"{case}: {'RMS' if k < 4 else 'loads'} history {k}")      # (a replay runs the launches the eager cycle runs)
    for l, (x, y) in enumerate(zip(out[0][1], out[1][1])):
        _same(y, x, f"{case}: state {l}")


@pytest.mark.parametrize("case", CASES)
def test_per_kernel_entry_points_follow_the_change(case, oracle):
    """compute_wall_flux_edge (the far-field faces) and compute_fluxes against the oracle's loops given the same 17 values."""
    lib = oracle.load()
    for pair in PAIRS:
        co = fse.ComposedOracle(oracle, case, fse.free_stream_constants(*pair))
        mesh, s = _solver(case)
        s.set_free_stream(*pair)
        for l in range(s.num_levels):
            L = co.oc.levels[l]
            q = perturbed_state(L.nel, co.ff17[:5], seed=40 + l)
            s.set(l, "variables", q)
            want = np.zeros((L.nel, 5))
            lib.ora_compute_wall_flux_edge(L.wall_start, L.n_wall, L.edges, oracle.ptr(q), oracle.ptr(want), C.byref(co.ff))
            s.zero_fluxes(l)
            s.compute_wall_flux_edge(l)
            _same(s.get(l, "fluxes"), want, f"{case} {pair} level {l}: compute_wall_flux_edge")
            if L.n_wall > 0:
                assert np.any(want != 0.0)
            want = np.zeros((L.nel, 5))
            lib.ora_compute_flux_edge(L.internal_start, L.n_internal, L.edges, oracle.ptr(q), oracle.ptr(want))
            lib.ora_compute_boundary_flux_edge(L.boundary_start, L.n_boundary, L.edges, oracle.ptr(q), oracle.ptr(want))
            lib.ora_compute_wall_flux_edge(L.wall_start, L.n_wall, L.edges, oracle.ptr(q), oracle.ptr(want), C.byref(co.ff))
            s.zero_fluxes(l)
            s.compute_fluxes(l)
            _same(s.get(l, "fluxes"), want, f"{case} {pair} level {l}: compute_fluxes")
        s.close()
        mesh.close()
        co.close()


@pytest.mark.parametrize("case", CASES)
def test_loads_follow_the_change(case, oracle):
    """surface_loads and the run_cycles(loads=True) history equal the emulator with the NEW far_field(): p_inf follows."""
    a, b = PAIRS
    legs, _ = _oracle_history(oracle, case, [(a, True, K), (b, False, K)])
    mesh, s = _solver(case)
    d = mesh.level(0)
    walls = s.get_edges(0, d["n_edges"])[d["boundary_start"]:d["boundary_start"] + d["n_boundary"]]
    p_inf = []
    for pair, leg in zip((a, b), legs):
        s.set_free_stream(*pair, reinitialise=(pair == a))
        ff = s.far_field()
        p_inf.append(emu.pressure(ff[:5])[0])
        _, hist = s.run_cycles(K, loads=True, ref_point=REF)
        want = np.array([emu.surface_loads(v, walls, d["coords"], ff, REF) for v, _ in leg])
        _same(hist, want, f"{case} {pair}: loads history")
        _same(s.surface_loads(0, REF), want[-1], f"{case} {pair}: surface_loads")
    s.close()
    mesh.close()


def test_load_coefficients_turn_with_alpha():
    import mgcfd
    f = np.array([0.3, -0.7, 0.11, 0.5, -0.25, 0.125])
    S, c = 0.7532, 0.64607
    got = {}
    for pair in PAIRS + [fse.DEFAULT]:
        ff = mgcfd.free_stream_constants(*pair)
        got[pair] = mgcfd.load_coefficients(ff, f, S, c)
        # the header's formula: q = 0.5 rho |V|^2, alpha = atan2(Vy, Vx)
        rho, v = ff[0], ff[1:4] / ff[0]
        q = 0.5 * rho * (v[0] * v[0] + v[1] * v[1] + v[2] * v[2])
        al = np.arctan2(v[1], v[0])
        want = np.array([(f[0] * np.cos(al) + f[1] * np.sin(al)) / (q * S), (-f[0] * np.sin(al) + f[1] * np.cos(al)) / (q * S),
                         f[2] / (q * S), f[3] / (q * S * c), f[4] / (q * S * c), f[5] / (q * S * c)])
        assert np.allclose(got[pair], want, rtol=1e-14, atol=0), pair
        assert np.allclose(got[pair], emu.coefficients(ff, f, S, c), rtol=1e-14, atol=0)
        assert np.isclose(np.degrees(al), pair[1], rtol=1e-12, atol=1e-15)
    assert got[PAIRS[0]][1] != got[PAIRS[1]][1] and got[PAIRS[0]][0] != got[fse.DEFAULT][0]


@pytest.mark.parametrize("case", CASES)
def test_fast_mode_after_a_change(case):
    """exact = 0 after a change of free stream (cold, then warm) against the exact run at the same pairs, within the bound
    tests/test_gpu_order_free.py applies to whole cycles: 1e-10 of the largest value per level, RMS rtol 1e-9."""
    a, b = PAIRS
    out = {}
    for exact in (1, 0):
        mesh, s = _solver(case, exact=exact)
        s.set_free_stream(*a)
        r1 = s.run_cycles(K)
        v1 = [s.get(l, "variables") for l in range(s.num_levels)]
        s.set_free_stream(*b, reinitialise=False)
        r2 = s.run_cycles(K)
        v2 = [s.get(l, "variables") for l in range(s.num_levels)]
        out[exact] = (r1, v1, r2, v2)
        s.close()
        mesh.close()
    for leg in (0, 2):
        assert np.allclose(out[0][leg], out[1][leg], rtol=RMS_FAST, atol=0)
        for l, (got, want) in enumerate(zip(out[0][leg + 1], out[1][leg + 1])):
            rel = np.abs(got - want).max() / max(np.abs(want).max(), 1e-300)
            print(case, "leg", leg // 2, "level", l, "rel", rel)
            assert rel <= REL_RUN, f"{case} leg {leg // 2} level {l}: {rel:.3e}"


def test_setter_refuses_a_sweep_under_way():
    """Between mgcfd_sweep_stage 0 and the last stage (or after mgcfd_sweep_flux0) the buffers hold half a sweep of the old
    free stream: the setter returns MGCFD_ERR_ARG and changes nothing; once the sweep has ended it works as ever."""
    import mgcfd
    mesh, s = _solver("m6_2lvl")
    ref_mesh, ref = _solver("m6_2lvl")
    s.set_free_stream(*PAIRS[0])
    ref.set_free_stream(*PAIRS[0])
    s.sweep_begin(0)
    s.sweep_stage(0, 0, partials=False)
    for reinit in (True, False):
        with pytest.raises(mgcfd.MgcfdError) as e:
            s.set_free_stream(*PAIRS[1], reinitialise=reinit)
        assert e.value.code == 1 and "sweep is under way" in str(e.value)
    assert s.free_stream() == PAIRS[0]
    s.sweep_stage(0, 1, partials=False)
    s.sweep_stage(0, 2, partials=False)
    ref.smooth(0, 1)
    _same(s.get(0, "variables"), ref.get(0, "variables"), "the sweep the refused calls interrupted")
    s.sweep_begin(0)
    s.sweep_flux0(0)
    with pytest.raises(mgcfd.MgcfdError) as e:
        s.set_free_stream(*PAIRS[1])
    assert e.value.code == 1
    s.sweep_end(0)
    ref.smooth(0, 1)
    _same(s.get(0, "variables"), ref.get(0, "variables"), "the second sweep")
    for t in (s, ref):
        t.set_free_stream(*PAIRS[1])
        t.run_cycles(1)
    _same(s.get(0, "variables"), ref.get(0, "variables"), "a cycle after the change")
    s.close(); ref.close()
    mesh.close(); ref_mesh.close()


def test_setter_argument_errors_and_polar():
    import mgcfd
    mesh, s = _solver("m6_2lvl")
    for mach, alpha in ((0.0, 0.0), (1.2, 90.0), (float("nan"), 1.0)):
        with pytest.raises(mgcfd.MgcfdError) as e:
            s.set_free_stream(mach, alpha)
        assert e.value.code == 1
    assert s.free_stream() == (1.2, 0.0)                     # a refused call changes nothing
    alphas, mach = fse.POLAR_ALPHAS, fse.POLAR_MACH
    assert mach == 0.8 and alphas[-1] == 3.0
    for warm in (True, False):
        pol = s.polar(alphas, K, mach=0.8, warm_start=warm, ref_point=REF, ref_area=0.75, ref_length=0.6)
        assert [p["alpha"] for p in pol] == alphas and all(p["mach"] == 0.8 for p in pol)
        # the same loop by hand on another solver
        mesh2, t = _solver("m6_2lvl")
        for k, (al, p) in enumerate(zip(alphas, pol)):
            t.set_free_stream(0.8, al, reinitialise=(k == 0 or not warm))
            rms, hist = t.run_cycles(K, loads=True, ref_point=REF)
            _same(p["rms"], rms, "polar RMS")
            _same(p["loads"], hist, "polar loads")
            _same(p["coefficients"], mgcfd.load_coefficients(mgcfd.free_stream_constants(0.8, al), hist[-1], 0.75, 0.6), "polar coefficients")
        t.close()
        mesh2.close()
    assert s.free_stream() == (0.8, 3.0)
    pol = s.polar([1.0], 1)                                   # mach=None keeps the solver's
    assert pol[0]["mach"] == 0.8
    s.close()
    mesh.close()
