"""The index table of tile_frame's gather (csrc/eaqhm_ls_gather.h) on the CPU: tests/gather_table_check.cpp includes the
header as plain C++ and compares, for every Kc of the three-weight classes and every entry of every lower tile of the
stacked system, the table's byte offset and conjugation flag with the rule written out per entry (plain and packed tile
layout; padding must land on the zero cell, everything else inside the 3 npair tiles)."""
import os
import shutil
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "eaqhm-analysis-and-synthesis-in-python_amd", "csrc")


def test_table_matches_the_rule_per_entry(tmp_path):
    cxx = next((c for c in (shutil.which("c++"), shutil.which("g++"), shutil.which("clang++"),
                            os.environ.get("HIPCC"), "/opt/rocm/bin/hipcc") if c and os.path.exists(c)), None)
    assert cxx, "no C++ compiler"
    exe = str(tmp_path / "gather_table_check")
    subprocess.run([cxx, "-x", "c++", "-std=c++17", "-O1", "-I", CSRC, "-o", exe,
                    os.path.join(ROOT, "tests", "gather_table_check.cpp")], check=True)
    r = subprocess.run([exe], capture_output=True, text=True)
    print(r.stdout)
    assert r.returncode == 0 and r.stdout.strip().endswith(", 0 wrong"), r.stdout[-2000:]
