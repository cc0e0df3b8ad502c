"""The plan of one evaluation (csrc/eval_plan.h: eval_validate, eval_plan, layout_plan - the functions aimnet_engine_eval calls to
decide which launch does which job) - proven on the CPU, because the invariants it has to keep ("exactly one launch reduces the
energies", "exactly one writes the charges", "the reverse-pair lookup runs once, before the force gather", "no two live lists share
a buffer") used to be carried by mutable flags inside eval and could only be observed on a GPU.

tests/eval_plan_main.cpp is a stand-alone host program (its own main, nothing loaded into Python) compiled with
-fsanitize=address,undefined.  It walks the product of the request shapes with a pairwise sample of the engine switches and size
predicates (see its header for the list and for why the sample), skips what eval's own checks reject, and asserts those
invariants on every plan - and that the walk reached every branch of every decision."""
from __future__ import annotations

import os
import subprocess

from conftest import ROOT
from test_chain_prefetch_plan import _host_compiler


def test_eval_plan_keeps_its_invariants(tmp_path):
    exe = str(tmp_path / "eval_plan")
    base = ["-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
            "-I", os.path.join(ROOT, "aimnetcentral_amd", "csrc"), os.path.join(ROOT, "tests", "eval_plan_main.cpp"), "-o", exe]
    # (static sanitizer runtimes: see tests/test_chain_prefetch_plan.py)
    cxx = _host_compiler()
    r = subprocess.run([cxx, "-static-libasan", "-static-libubsan", *base], capture_output=True, text=True)
    if r.returncode != 0:
        r = subprocess.run([cxx, *base], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    r = subprocess.run([exe], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "eval plan ok" in r.stdout
