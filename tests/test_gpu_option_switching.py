"""GPU tests of switching one optional-physics setting on and off under another: dual time stepping, the JST dissipation, FAS
multigrid and the viscous terms share level 0's numbering for the ordered RMS sum (held while any of them is on) and the decision
whether a level runs fused stages and graphs.  Every ordered pair (A, B) of the four on lattice B of tests/fas_emulator.py under
local steps at CFL 1.0: A on, B on, A off must leave exactly the solver on which only B was ever switched on — what the library
holds on the device (counted before any launch, so a wrong release shows as a count and not as a fault), then the bits of two cycles —
and B off must leave a solver that was never touched.  The settings are the emulators' own for lattice B; tests/test_host_fas.py,
test_host_jst.py, test_host_dual_time.py and test_host_viscous.py assert that each single-option run stays valid."""
import itertools

import numpy as np
import pytest

import dual_time_emulator as dte
import fas_emulator as fe
import free_stream_emulator as fse
import viscous_emulator as ve

pytestmark = pytest.mark.gpu

MODE, CFL = "local", 1.0
CYCLES = 2
OPTIONS = ("dual_time", "jst", "fas", "viscous")


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.int64)


def _same(got, want, what):
    assert np.array_equal(_bits(got), _bits(want)), f"{what}: max |difference| {np.abs(np.asarray(got) - np.asarray(want)).max():.3e}"


def _live():
    import mgcfd
    r = mgcfd.live_device_resources()
    return np.array([r["allocations"], r["bytes"], r["handles"]], dtype=np.int64)


@pytest.fixture(scope="module")
def case(tmp_path_factory):
    return fe.write_lattice("B", tmp_path_factory.mktemp("switching_lattice"))


@pytest.fixture(scope="module")
def switches(oracle, case):
    """{option: (on, off)}, each a function of the solver."""
    dt = dte.pick_dt(oracle, case, MODE, CFL)
    return {"dual_time": (lambda s: s.set_dual_time(dt), lambda s: s.set_dual_time(0.0)),
            "jst": (lambda s: s.set_jst(), lambda s: s.set_jst(levels=0)),
            "fas": (lambda s: s.set_fas(True), lambda s: s.set_fas(False)),
            "viscous": (lambda s: s.set_viscous(ve.GPU_MU["B"], wall=False), lambda s: s.set_viscous(0.0, levels=0))}


class _Tracked:
    """A solver and what the library holds on the device for it: the counters are the process's, so every call that may change
    them goes through ``do`` and is booked to this solver."""

    def __init__(self, case):
        import mgcfd
        before = _live()
        self.mesh = mgcfd.Mesh("input.dat", fse.case_input(case), fse.case_duplicate(case))
        self.s = mgcfd.Solver.from_mesh(self.mesh)
        self.s.set_time_step(MODE, CFL)
        self.held = _live() - before

    def do(self, f):
        before = _live()
        out = f(self.s)
        self.held = self.held + _live() - before
        return out

    def close(self):
        self.s.close()
        self.mesh.close()


@pytest.fixture(scope="module")
def kept(case, switches):
    """What an option still holds after on and off again with nothing run in between.  Dual time, FAS and the viscous terms release
    what they allocated; the JST dissipation keeps its seven arrays of level 0 (include/mgcfd.h: allocated by the first enabling
    call), one allocation of at least 7 x 8 bytes per node, and nothing else."""
    out = {}
    for name, (on, off) in switches.items():
        t = _Tracked(case)
        start = t.held
        t.do(on)
        t.do(off)
        out[name] = t.held - start
        if name == "jst":
            assert out[name][0] == 1 and out[name][1] >= 7 * 8 * t.s.nel(0) and out[name][2] == 0
        else:
            assert not out[name].any(), (name, out[name])
        t.close()
    return out


def _compare_runs(a, b, what):
    rms_a, rms_b = a.do(lambda s: s.run_cycles(CYCLES)), b.do(lambda s: s.run_cycles(CYCLES))
    print(what, "rms", rms_a, rms_b)
    assert np.all(np.isfinite(rms_a)) and rms_a.any()
    _same(rms_a, rms_b, f"{what}: RMS history")
    for l in range(a.s.num_levels):
        _same(a.s.get(l, "variables"), b.s.get(l, "variables"), f"{what}: variables, level {l}")
    assert a.s.pending_invalid_state()[0] == 0 and b.s.pending_invalid_state()[0] == 0


@pytest.mark.parametrize("first,second", list(itertools.permutations(OPTIONS, 2)), ids=lambda v: v)
def test_on_on_off(first, second, case, switches, kept):
    (a_on, a_off), (b_on, b_off) = switches[first], switches[second]
    both, only_b, never = _Tracked(case), _Tracked(case), _Tracked(case)
    assert np.array_equal(both.held, only_b.held) and np.array_equal(both.held, never.held)
    # A on, B on, A off, nothing run in between: what only B holds (and what A keeps once it has been on), before any launch
    both.do(a_on); both.do(b_on); both.do(a_off)
    only_b.do(b_on)
    print(first, second, "held", both.held, only_b.held, never.held, "kept", kept[first], kept[second])
    assert np.array_equal(both.held, only_b.held + kept[first]), "after A on, B on, A off the library holds what B alone holds"
    assert only_b.held[0] > never.held[0], "B holds something"
    _compare_runs(both, only_b, f"{second} after {first} on and off")
    # B off: a solver that was never touched, in what it holds and in what it computes from the same state
    both.do(b_off)
    never.do(lambda s: s.run_cycles(CYCLES))                 # (the cycle driver's own arrays: made by the first run)
    assert np.array_equal(both.held, never.held + kept[first] + kept[second]), "after B off the library holds what an untouched solver holds"
    for l in range(never.s.num_levels):
        never.s.set(l, "variables", both.s.get(l, "variables"))
    _compare_runs(both, never, f"{first} and {second} off again")
    for t in (both, only_b, never):
        t.close()
