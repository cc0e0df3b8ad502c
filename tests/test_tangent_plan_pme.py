"""tangent_validate / tangent_plan of csrc/tangent_plan.h with TangentRequest.pme_tangent, through a stand-alone program
(tests/pme_tangent_plan_main.cpp) built with the address and undefined-behaviour sanitizers: unarmed, the refusal of
AIMNET_COULOMB_PME and the plan are what they were, word for word; armed, every reject and the `pme` branch (with `lr_list`, its
mesh slices in bounds) are reached.  CPU only."""
from __future__ import annotations

import os
import subprocess

from test_chain_prefetch_plan import _host_compiler

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_tangent_plan_with_an_armed_mesh(tmp_path):
    exe = str(tmp_path / "pme_tangent_plan")
    base = ["-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
            "-I", os.path.join(ROOT, "aimnetcentral_amd", "csrc"), os.path.join(ROOT, "tests", "pme_tangent_plan_main.cpp"), "-o", exe]
    cxx = _host_compiler()  # (static sanitizer runtimes: see tests/test_chain_prefetch_plan.py)
    r = subprocess.run([cxx, "-static-libasan", "-static-libubsan", *base], capture_output=True, text=True)
    if r.returncode != 0:
        r = subprocess.run([cxx, *base], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    r = subprocess.run([exe], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "pme tangent plan ok" in r.stdout


def test_the_refusal_text_in_the_header_is_todays():
    """The unarmed message is also what tests/test_gpu_hvp_ewald.py::test_rejections and tests/test_host_driver.py match on."""
    src = open(os.path.join(ROOT, "aimnetcentral_amd", "csrc", "tangent_plan.h")).read()
    assert '"hvp: the analytic tangent sweep does not cover particle-mesh Ewald (use the exact Ewald sum or DSF, or "' in src
    assert "r.coulomb == AIMNET_COULOMB_PME && !r.pme_tangent" in src
