"""euler3d_gpu_double's options, case by case against what the driver did before its flags and config keys were gathered into one
table (csrc/main.cpp, kOptions): exit status, stdout, stderr and the resulting Config, byte for byte.

tests/driver_config_dump.cpp includes main.cpp whole and runs what the driver runs before it touches a file or a device
(parse_arguments, then check_combinations), then prints every field of Config.  tests/golden/driver_options/cases.json holds
the cases: argv, the config files to write (relative paths, so that no temporary path reaches the output), the status, stderr,
what stdout holds before the Config, and the fields of the Config that differ from "defaults", the Config of an empty command
line (a member that would be empty is left out).  It was recorded once from the driver as it was before the table, with this helper; the cases that trip a rule of main()
from that driver's own binary.  It is never to be regenerated from the code under test.

Every option is there from each of its sources with an accepted and a refused value; every kind of number and every range
with the values about its bounds, a non-integer, nan, inf, the empty string, a leading space and trailing junk; every name of
every enumerated option; the optional values in every form; the config flags; every rule between options, the order of the
rules, the order of the arguments about -c, the input_file_directory rewrite, getopt's abbreviations and messages, the help
text and the lines a config file's reader ignores."""
import json
import os
import subprocess
from concurrent.futures import ThreadPoolExecutor

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "mg-cfd-app-plain_amd", "csrc")
HIPCC = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
HOSTFLAGS = "-O3 -std=c++17 -fPIC -fno-fast-math -ffp-contract=off -Wall -Wextra -Wno-unused-parameter".split()   # csrc/Makefile

with open(os.path.join(ROOT, "tests", "golden", "driver_options", "cases.json")) as f:
    FIXTURE = json.load(f)


@pytest.fixture(scope="module")
def helper(tmp_path_factory):
    """The helper, built as csrc/Makefile builds the driver: compiled alone, then linked against build/multi_gpu.o and the library."""
    for need in ("build/multi_gpu.o", "libmgcfd_hip.so"):
        assert os.path.exists(os.path.join(CSRC, need)), f"{need} is missing: build() makes it"
    d = tmp_path_factory.mktemp("driver_options")
    obj, exe = str(d / "driver_config_dump.o"), str(d / "driver_config_dump")
    for cmd in ([HIPCC] + HOSTFLAGS + [f"-I{ROOT}/include", f"-I{CSRC}", "-c", os.path.join(ROOT, "tests", "driver_config_dump.cpp"), "-o", obj],
                [HIPCC, "-o", exe, obj, os.path.join(CSRC, "build", "multi_gpu.o"), f"-L{CSRC}", "-lmgcfd_hip", f"-Wl,-rpath,{CSRC}"]):
        r = subprocess.run(cmd, capture_output=True, text=True, timeout=600)
        assert r.returncode == 0, r.stderr[-3000:]
    return exe


def _run(exe, case, where):
    """One case in a process of its own (getopt's state is global) and a directory of its own; argv[0] is the driver's name."""
    os.makedirs(where)
    for rel, text in case.get("files", {}).items():
        path = os.path.join(where, rel)
        os.makedirs(os.path.dirname(path), exist_ok=True)
        with open(path, "w", newline="") as f:
            f.write(text)
    r = subprocess.run(["euler3d_gpu_double"] + case["argv"], executable=exe, capture_output=True, text=True, cwd=where, timeout=60)
    return r.returncode, r.stdout, r.stderr


def _expected_stdout(case):
    lines = []
    for line in FIXTURE["defaults"]:
        name = line.split("=", 1)[0]
        lines.append(f"{name}={case['config'][name]}" if name in case.get("config", {}) else line)
    return case.get("stdout_head", "") + "".join(line + "\n" for line in lines)


def test_the_fixture_covers_every_name_of_the_table():
    """Every --name and every key that main.cpp's table holds stands in a case, accepted once and (with a value) refused once."""
    import re
    table = open(os.path.join(CSRC, "main.cpp")).read()
    table = table[table.index("const Option kOptions[] = {"):table.index("constexpr int kFirstOptionCode")]
    entries = re.findall(r'^    \{("[\w-]+"|nullptr), (?:\'\w\'|0), ("\w+"|nullptr), (\w+), ([\w:]+(?:\(\w+)?)', table, re.M)
    assert len(entries) > 75, len(entries)
    cases = FIXTURE["cases"]
    never_refused = ("Read::String", "Read::Int", "Read::Ignored", "by(set_config_filepath")
    for cli, key, has_arg, read in entries:
        if cli != "nullptr":
            flag = "--" + cli.strip('"')
            mine = [c for c in cases if any(a == flag or a.startswith(flag + "=") for a in c["argv"])]
            assert any(c["status"] == 0 and "stderr" not in c for c in mine) or flag == "--help", flag
            assert has_arg == "kNoArg" or read in never_refused or any(c["status"] == 1 for c in mine), flag
        if key != "nullptr":
            start = key.strip('"') + " ="
            mine = [c for c in cases if any(line.startswith(start) for text in c.get("files", {}).values() for line in text.split("\n"))]
            assert any(c["status"] == 0 and "stderr" not in c for c in mine), key
            assert has_arg == "kNoArg" or read in never_refused or any("stderr" in c or "stdout_head" in c for c in mine), key


def test_every_case_gives_what_the_driver_gave_before_the_table(helper, tmp_path):
    cases = FIXTURE["cases"]
    assert len(cases) > 500
    with ThreadPoolExecutor(max_workers=min(8, os.cpu_count() or 1)) as pool:
        got = list(pool.map(lambda kc: _run(helper, kc[1], str(tmp_path / str(kc[0]))), enumerate(cases)))
    wrong = []
    for case, (status, stdout, stderr) in zip(cases, got):
        if (status, stdout, stderr) != (case["status"], _expected_stdout(case), case.get("stderr", "")):
            wrong.append((case["argv"], case.get("files"), "status", status, case["status"], "stderr", stderr, case.get("stderr", ""),
                          "stdout", [l for l in stdout.split("\n") if l not in _expected_stdout(case).split("\n")],
                          [l for l in _expected_stdout(case).split("\n") if l not in stdout.split("\n")]))
    assert not wrong, f"{len(wrong)} of {len(cases)} cases differ; the first: {wrong[:3]}"
