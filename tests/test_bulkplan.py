"""The bulk path's arithmetic (policy-server_amd/csrc/bulkplan.hpp, the header bulk.cpp runs) on the
host: the chunk boundaries equal the ones recorded from the loop the header replaced
(tests/golden/bulk_chunks.txt) and keep their properties, the row slabs of an unchunked pass are
the given ones and keep theirs, and the packed placement of a chunk's ranges stays inside the
slot-size estimate: tests/bulkplan_check.cpp."""
import os
import shutil
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CXX = shutil.which("g++") or shutil.which("clang++") or "/opt/rocm/llvm/bin/clang++"


def test_chunk_bounds_and_packed_placement(tmp_path):
    exe = tmp_path / "bulkplan_check"
    subprocess.run([CXX, "-O2", "-std=c++17", "-Wall", "-Wextra", "-Werror", "-I", os.path.join(ROOT, "policy-server_amd", "csrc"),
                    "-o", str(exe), os.path.join(ROOT, "tests", "bulkplan_check.cpp")], check=True)
    out = subprocess.run([str(exe), os.path.join(ROOT, "tests", "golden", "bulk_chunks.txt")], check=False,
                         capture_output=True, text=True)
    assert out.returncode == 0, out.stdout + out.stderr
    assert "cases 361 " in out.stdout and "failures 0" in out.stdout
