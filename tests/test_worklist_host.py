"""The work lists of the fused renderer (csrc/render_worklist.hpp) on the host: tests/worklist_host_main.cpp is built as a stand-alone program with the
address and undefined-behaviour sanitizers and checks, for every policy, ray counts 1 .. 4096, 1 / 4 / 8 tiles per ray, plain and pair launches, 8 and 256
waves per XCD: every (ray, tile) exactly once, a ray's items in order and contiguous, every ray on the XCD the chunking gives it, sampling on the first
item only, and the closed-form ticket decode equal to the builder."""
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _build(tmp_path, extra):
    exe = str(tmp_path / "worklist_host")
    cmd = ["g++", "-std=c++17", "-O1", "-g", "-Wall", "-Wextra", "-I", os.path.join(ROOT, "avatarcraft_amd", "csrc"),
           os.path.join(ROOT, "tests", "worklist_host_main.cpp"), "-o", exe] + extra
    return exe, subprocess.run(cmd, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)


def test_worklist_properties(tmp_path):
    if shutil.which("g++") is None:
        pytest.fail("g++ not found: the work-list builder is checked as a host program")
    exe, r = _build(tmp_path, ["-fsanitize=address,undefined", "-fno-sanitize-recover=all"])
    if r.returncode != 0:                      # a compiler without the sanitizer runtimes still checks the properties
        exe, r = _build(tmp_path, [])
    assert r.returncode == 0, r.stdout
    assert "warning" not in r.stdout, r.stdout
    r = subprocess.run([exe], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, timeout=300)
    print(r.stdout)
    assert r.returncode == 0, r.stdout[-4000:]
    lines = r.stdout.strip().splitlines()
    assert lines[-1] == "ok"
    assert sum(l.startswith("policy ") for l in lines) == 9          # every policy of the header
