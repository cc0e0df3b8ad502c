"""The checks and the plan of the two tangent entry points (csrc/tangent_plan.h: tangent_validate, tangent_plan - the functions
aimnet_engine_hvp and aimnet_engine_charge_response call before anything is launched) - proven on the CPU.  "Rejected before
anything is launched, status untouched" used to be a property of statement order inside two long bodies, observable on a GPU only.

tests/tangent_plan_main.cpp is a stand-alone host program (its own main, nothing loaded into Python) compiled with
-fsanitize=address,undefined.  It walks the product of the request shapes (see its header), holds every reject to the table of
the inline checks it replaces - same entry prefix, same message, same order of precedence - asserts the invariants the layout and
the stages rely on for every plan, and that the walk reached every reject and every plan branch."""
from __future__ import annotations

import os
import subprocess

from conftest import ROOT
from test_chain_prefetch_plan import _host_compiler


def test_tangent_plan_keeps_its_checks_and_invariants(tmp_path):
    exe = str(tmp_path / "tangent_plan")
    base = ["-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
            "-I", os.path.join(ROOT, "aimnetcentral_amd", "csrc"), os.path.join(ROOT, "tests", "tangent_plan_main.cpp"), "-o", exe]
    # (static sanitizer runtimes: see tests/test_chain_prefetch_plan.py)
    cxx = _host_compiler()
    r = subprocess.run([cxx, "-static-libasan", "-static-libubsan", *base], capture_output=True, text=True)
    if r.returncode != 0:
        r = subprocess.run([cxx, *base], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    r = subprocess.run([exe], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "tangent plan ok" in r.stdout
