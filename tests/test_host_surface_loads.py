"""CPU tests of the surface loads: the host-only coefficient call against its formula, the numpy emulator (the GPU tests'
yardstick) against an exactly rounded sum, and the driver's --output-loads / --loads-reference command line."""
import math
import os
import subprocess

import numpy as np
import pytest

import surface_loads_emulator as emu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden")
EXE = os.path.join(ROOT, "mg-cfd-app-plain_amd", "csrc", "euler3d_gpu_double")


@pytest.fixture(scope="module")
def mgcfd_mod():
    import mgcfd
    if not os.path.exists(mgcfd.LIB_PATH) or not os.path.exists(EXE):
        import __graft_entry__
        __graft_entry__.build()
    return mgcfd


def _ff17(oracle):
    ff = oracle.farfield()
    return np.concatenate([np.array(ff.var), np.array(ff.fc_mx), np.array(ff.fc_my), np.array(ff.fc_mz), np.array(ff.fc_de)])


def _rotated(ff17, deg):
    """The same free stream at another angle of attack in the x-y plane (cfd_loops.h:85-104)."""
    out = ff17.copy()
    speed = math.hypot(ff17[1], ff17[2])
    a = math.radians(deg)
    out[1], out[2] = speed * math.cos(a), speed * math.sin(a)
    return out


def test_the_three_entry_points_are_bound(mgcfd_mod):
    for name in ("mgcfd_surface_loads", "mgcfd_run_cycles_loads", "mgcfd_load_coefficients"):
        assert name in mgcfd_mod.EXPORTED_SYMBOLS
    assert mgcfd_mod.load_library().mgcfd_abi_version() == 1


@pytest.mark.parametrize("deg", [0.0, 3.06, -7.5, 30.0])
def test_load_coefficients_match_the_formula(mgcfd_mod, oracle, deg):
    ff = _rotated(_ff17(oracle), deg)
    rng = np.random.default_rng(5)
    loads = rng.normal(size=(8, 6)) * np.array([1e-2, 3e-2, 1e-3, 2e-3, 5e-3, 1e-2])
    for S, c in [(1.0, 1.0), (0.7532, 0.64607), (12.5, 3.0)]:
        got = mgcfd_mod.load_coefficients(ff, loads, S, c)
        assert got.shape == loads.shape
        for k in range(len(loads)):
            want = emu.coefficients(ff, loads[k], S, c)
            scale = np.abs(want).max()
            assert np.abs(got[k] - want).max() <= 1e-14 * scale, (S, c, got[k], want)
    # the default reference values are 1 and 1
    assert np.array_equal(mgcfd_mod.load_coefficients(ff, loads[0]), mgcfd_mod.load_coefficients(ff, loads[0], 1.0, 1.0))


def test_load_coefficients_reject_a_bad_reference(mgcfd_mod, oracle):
    ff = _ff17(oracle)
    for S, c in [(0.0, 1.0), (1.0, -2.0), (float("nan"), 1.0), (1.0, float("inf"))]:
        with pytest.raises(mgcfd_mod.MgcfdError) as e:
            mgcfd_mod.load_coefficients(ff, np.ones(6), S, c)
        assert e.value.code == 1 and "reference area" in str(e.value)


@pytest.mark.parametrize("n", [1, 255, 256, 257, 5000, 65536, 65537, 200000])
def test_emulator_tree_agrees_with_an_exact_sum(n):
    rng = np.random.default_rng(n)
    terms = rng.uniform(0.25, 1.75, size=(n, 6)) * np.array([1.0, -3.0, 1e-3, 7.0, -1e4, 0.5])
    got = emu.reduce_loads(terms)
    for c in range(6):
        want = math.fsum(terms[:, c])
        assert abs(got[c] - want) <= 1e-12 * abs(want), (n, c)


def test_emulator_tree_pairs_operands_by_halving_strides():
    # one chunk: v[64] and v[192] meet at s = 128 before their sum meets v[0] at s = 64; added one by one in index
    # order, each 1e-16 would be lost against 1.0
    v = np.zeros((256, 6))
    v[0, :] = 1.0
    v[64, :] = 1e-16
    v[192, :] = 1e-16
    got = emu.reduce_loads(v)
    assert np.array_equal(got, np.full(6, 1.0 + (1e-16 + 1e-16)))
    assert got[0] != (1.0 + 1e-16) + 1e-16
    assert np.array_equal(emu.reduce_loads(np.zeros((0, 6))), np.zeros(6))


@pytest.mark.parametrize("value", ["", "1,1,0,0", "1,1,0,0,0,0", "a,1,0,0,0", "1,,0,0,0", "0,1,0,0,0", "1,-1,0,0,0",
                                   "1,1,0,0,nan", "1,1,0,0,inf", "1,1,0,0,0x", " 1,1,0,0,0", "1;1;0;0;0"])
def test_driver_rejects_a_malformed_loads_reference(mgcfd_mod, value):
    r = subprocess.run([EXE, "--output-loads", f"--loads-reference={value}", "-i", "input.dat", "-d",
                        os.path.join(GOLDEN, "m6_2lvl", "input")], capture_output=True, text=True, timeout=60)
    assert r.returncode == 1
    assert "--loads-reference" in r.stderr and "expected S,c,x,y,z" in r.stderr
    assert r.stdout == ""


def test_driver_accepts_a_well_formed_loads_reference(mgcfd_mod):
    # parsed, then the run stops at the missing input file as any run would
    r = subprocess.run([EXE, "--output-loads", "--loads-reference=0.7532,0.64607,0.25,-1e-3,2E+0"], capture_output=True,
                       text=True, timeout=60)
    assert r.returncode == 1 and "ERROR: input_file not set" in r.stdout
    assert "--loads-reference" not in r.stderr


def test_driver_refuses_output_loads_on_several_gpus(mgcfd_mod):
    r = subprocess.run([EXE, "--output-loads", "--gpus", "2", "-i", "input.dat", "-d", os.path.join(GOLDEN, "m6_2lvl", "input"),
                        "-g", "1"], capture_output=True, text=True, timeout=60)
    assert r.returncode == 1
    assert "--output-loads runs on one GPU only" in r.stderr
    # refused right after parsing: no input read, no device or solver set up, nothing printed
    assert r.stdout == "" and "[euler3d_gpu_double]" not in r.stderr and "Could not open" not in r.stderr


def test_driver_help_lists_the_loads_flags(mgcfd_mod):
    r = subprocess.run([EXE, "--help"], capture_output=True, text=True, timeout=60)
    assert r.returncode == 1
    assert "--output-loads" in r.stderr and "--loads-reference=S,c,x,y,z" in r.stderr
