"""The wide path's group programs (policy-server_amd/csrc/groupvm.hpp: the script VM and the wide
jump code) alone on the host. tests/script_check.cpp compiles each script for the wide path, runs
it for every vector of member results in heap blocks of exactly the sizes the planner gives the
device, and compares each run with the host interpreter; it runs as a plain executable under
AddressSanitizer and UBSan (no Python in that process). The scripts are the expressions of
rhai_cases.VALID and 3 seeds x 60 scripts of fuzz._script over the members a, b, c, and, one input
file per family, the Unicode sweeps of script_unicode_cases.py over the member a (the case tables by
value, the closure code points alone in their contexts, Final_Sigma contexts, trim)."""
import os
import random
import re
import shutil
import subprocess

import pytest

import script_unicode_cases
from fuzz import _script
from rhai_cases import VALID

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "policy-server_amd", "csrc")
CXX = shutil.which("g++") or shutil.which("clang++") or "/opt/rocm/llvm/bin/clang++"
MEMBERS = ["a", "b", "c"]
SEEDS = (9000, 9001, 9002)


def scripts():
    rows = [expr for expr, _ in VALID]
    for seed in SEEDS:
        rng = random.Random(seed)
        rows += [_script(rng, MEMBERS) for _ in range(60)]
    return rows


@pytest.fixture(scope="module")
def script_check(tmp_path_factory):
    exe = tmp_path_factory.mktemp("script_check") / "script_check"
    subprocess.run([CXX, "-O1", "-g", "-std=c++17", "-Wall", "-Wextra", "-Werror", "-fsanitize=address,undefined",
                    "-fno-sanitize-recover=undefined", "-D__HIP_PLATFORM_AMD__", "-I", CSRC, "-o", str(exe),
                    os.path.join(ROOT, "tests", "script_check.cpp"), os.path.join(CSRC, "expr.cpp"),
                    os.path.join(CSRC, "knobs.cpp")], check=True)
    return exe


def run_script_check(exe, src, rows, members):
    with open(src, "wb") as f:
        f.write(b"%d\n" % len(rows))
        for expr in rows:
            body = expr.encode()
            f.write(b"%d %d\n%s\n" % (len(members), len(body), " ".join(members).encode()))
            f.write(body + b"\n")
    # (out-of-bounds accesses and undefined behaviour are the point; the leak check at exit needs
    # ptrace rights a test runner may lack)
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=0")
    env.pop("KW_GROUP_FORM", None)  # the form is the compiler's own choice for the wide path
    out = subprocess.run([str(exe), str(src)], check=False, capture_output=True, text=True, env=env)
    assert out.returncode == 0, out.stdout[-3000:] + out.stderr[-3000:]
    m = re.search(r"scripts (\d+) vm (\d+) wide (\d+) refused (\d+) runs (\d+) failures (\d+)", out.stdout)
    assert m, out.stdout[-3000:]
    n, vm, wide, refused, runs, failures = map(int, m.groups())
    print(out.stdout.strip())
    assert failures == 0 and n == len(rows)
    assert 2 * vm >= n, "fewer than half of the scripts reached the script VM"
    assert runs == (vm + wide) * (1 << len(members))
    return vm, wide, refused


def test_script_check_under_sanitizers(script_check, tmp_path):
    run_script_check(script_check, tmp_path / "scripts.bin", scripts(), MEMBERS)


@pytest.mark.parametrize("family", list(script_unicode_cases.FAMILIES))
def test_unicode_sweeps_under_sanitizers(script_check, tmp_path, family):
    """Every script of the family compiles to the script form and, for both answers of member a,
    the VM with the script's own char table agrees with the host interpreter (which maps through
    the whole tables)."""
    rows = script_unicode_cases.scripts(family)
    vm, wide, refused = run_script_check(script_check, tmp_path / "scripts.bin", rows, ["a"])
    assert vm == len(rows) and wide == 0 and refused == 0
