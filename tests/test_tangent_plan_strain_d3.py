"""tangent_validate / tangent_plan of csrc/tangent_plan.h with TangentRequest.strain_d3 (what aimnet_engine_set_strain_terms names),
through a stand-alone program (tests/strain_d3_plan_main.cpp) built with the address and undefined-behaviour sanitizers: with the bit
clear every verdict and message is what it was; with the bit set and the dispersion block unarmed, the new message; with both, the
request is accepted where the same request without the term is, `d3_strain` is planned and nothing sized moves.  CPU only."""
from __future__ import annotations

import os
import subprocess

from test_chain_prefetch_plan import _host_compiler

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_tangent_plan_with_the_dispersion_block_under_strain(tmp_path):
    exe = str(tmp_path / "strain_d3_plan")
    base = ["-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
            "-I", os.path.join(ROOT, "aimnetcentral_amd", "csrc"), os.path.join(ROOT, "tests", "strain_d3_plan_main.cpp"), "-o", exe]
    cxx = _host_compiler()  # (static sanitizer runtimes: see tests/test_chain_prefetch_plan.py)
    r = subprocess.run([cxx, "-static-libasan", "-static-libubsan", *base], capture_output=True, text=True)
    if r.returncode != 0:
        r = subprocess.run([cxx, *base], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    r = subprocess.run([exe], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "strain d3 plan ok" in r.stdout


def test_the_refusals_the_program_names_are_the_ones_in_the_header():
    hdr = open(os.path.join(ROOT, "aimnetcentral_amd", "csrc", "tangent_plan.h")).read()
    assert '"hvp: strain tangent: the DFT-D3 block is not carried under strain (options.dftd3 = 0)"' in hdr
    assert "carried under strain by its analytic tangent only" in hdr and "(aimnet_engine_set_dftd3_tangent(e, 1))" in hdr
    assert "P.d3_strain = P.strain && P.d3_analytic && r.strain_d3;" in hdr
    pub = open(os.path.join(ROOT, "include", "aimnet_hip.h")).read()
    assert "#define AIMNET_STRAIN_TERM_DFTD3 1u" in pub and "#define AIMNET_ABI_VERSION 12" in pub
