"""tangent_validate / tangent_plan of csrc/tangent_plan.h with TangentRequest.d3_tangent, through a stand-alone program
(tests/d3_tangent_plan_main.cpp) built with the address and undefined-behaviour sanitizers: unarmed, the two limits of the
finite-difference dispersion block and the plan are what they were, word for word; armed, the two limits are lifted, every other
refusal keeps its words, `d3_analytic` is planned and the block's buffers shrink by at least the replicas.  CPU only."""
from __future__ import annotations

import os
import subprocess

from test_chain_prefetch_plan import _host_compiler

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_tangent_plan_with_an_armed_dispersion_block(tmp_path):
    exe = str(tmp_path / "d3_tangent_plan")
    base = ["-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
            "-I", os.path.join(ROOT, "aimnetcentral_amd", "csrc"), os.path.join(ROOT, "tests", "d3_tangent_plan_main.cpp"), "-o", exe]
    cxx = _host_compiler()  # (static sanitizer runtimes: see tests/test_chain_prefetch_plan.py)
    r = subprocess.run([cxx, "-static-libasan", "-static-libubsan", *base], capture_output=True, text=True)
    if r.returncode != 0:
        r = subprocess.run([cxx, *base], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    r = subprocess.run([exe], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "d3 tangent plan ok" in r.stdout


def test_the_layout_mirrored_by_the_program_is_the_one_in_hvp_hip():
    """The program restates the bytes tangent_layout gives the block; the lines it restates are held here, so that a change of the
    layout is a change of the program too."""
    src = open(os.path.join(ROOT, "aimnetcentral_amd", "csrc", "hvp.hip")).read()
    assert "if (P.d3_analytic) {" in src and "} else if (P.d3_block) {" in src
    assert "W.d3t_cn = c.take<float4>(kn), W.d3t_g = c.take<float4>(kn);" in src
    assert "W.d3c_idx = c.take<int>(cn * cap_d3), W.d3c_shift = c.take<int>(cn * cap_d3), W.d3c_cnt = c.take<int>(cn);" in src
    hdr = open(os.path.join(ROOT, "aimnetcentral_amd", "csrc", "tangent_plan.h")).read()
    assert "const int k_max = d3_fd ? 16383 : 65535;" in hdr and "const bool d3_fd = d3 && !r.d3_tangent;" in hdr
