"""The weight-prefetch plan of the one-launch MLP sweeps (csrc/gemm_chain_prefetch.h: pf_thread / pf_line, the functions the kernel of
csrc/gemm_chain.hip calls to decide which 4 bytes each thread requests) - proven on the CPU, because an out-of-range request on
the device would be a memory fault.

tests/chain_prefetch_plan_main.cpp is a stand-alone host program (its own main, nothing loaded into Python) compiled with
-fsanitize=address,undefined.  For every instantiated chain shape, 1 - 3 strips per panel and grids of 1, 7, 8, 9, 210, 256 and 775
blocks it runs the kernel's loop for every thread of every block against heap buffers of exactly the packed streams' sizes
(nk x NW x ntg x 2048 bytes per unit) and asserts that the blocks of one XCD touch every 128-byte line of every unit exactly
once and that no request reaches past its unit's buffer."""
from __future__ import annotations

import os
import shutil
import subprocess

from conftest import ROOT


def _host_compiler():
    for cand in (os.environ.get("CXX"), "c++", "g++", "clang++", "/opt/rocm/llvm/bin/clang++"):
        if cand and shutil.which(cand):
            return shutil.which(cand)
    raise AssertionError("no host C++ compiler found")


def test_prefetch_plan_covers_every_line_once_and_stays_inside(tmp_path):
    exe = str(tmp_path / "chain_prefetch_plan")
    base = ["-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
            "-I", os.path.join(ROOT, "aimnetcentral_amd", "csrc"), os.path.join(ROOT, "tests", "chain_prefetch_plan_main.cpp"), "-o", exe]
    # The sanitizer runtimes are linked statically, so the program starts in whatever environment the suite runs in (a dynamically
    # linked runtime insists on being the first library loaded).  clang links them statically by default; g++ needs the flags.
    cxx = _host_compiler()
    r = subprocess.run([cxx, "-static-libasan", "-static-libubsan", *base], capture_output=True, text=True)
    if r.returncode != 0:
        r = subprocess.run([cxx, *base], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    r = subprocess.run([exe], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "chain prefetch plan ok" in r.stdout
