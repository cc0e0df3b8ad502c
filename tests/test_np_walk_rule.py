"""The host's copy of "does this evaluation build a long-range list" (aimnetcentral_amd/capacity.py, builds_lr_list) against the
engine's own decision (csrc/eval_plan.h: plan_np_walk, eval_validate, eval_plan).  If the two disagreed the host would send
max_nb_lr = 0 for a list the engine wants to build, and the engine would reject the call ("non-periodic DSF Coulomb needs
max_nb_lr > 0") - or the host would pay for a buffer nobody fills.

tests/np_walk_rule_main.cpp is a stand-alone host program (its own main, nothing loaded into Python) compiled with
-fsanitize=address,undefined.  It prints the engine's side for every request without caller-supplied lists; bbox_applies(N, n_mol) is
an input on both sides (N = 1500 or 1499 atoms in one molecule)."""
from __future__ import annotations

import os
import subprocess

from conftest import ROOT
from test_chain_prefetch_plan import _host_compiler

from aimnetcentral_amd import capacity


def test_host_rule_agrees_with_the_plan(tmp_path):
    exe = str(tmp_path / "np_walk_rule")
    base = ["-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
            "-I", os.path.join(ROOT, "aimnetcentral_amd", "csrc"), os.path.join(ROOT, "tests", "np_walk_rule_main.cpp"), "-o", exe]
    # (static sanitizer runtimes: see tests/test_chain_prefetch_plan.py)
    cxx = _host_compiler()
    r = subprocess.run([cxx, "-static-libasan", "-static-libubsan", *base], capture_output=True, text=True)
    if r.returncode != 0:
        r = subprocess.run([cxx, *base], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    r = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stdout + r.stderr
    lines = r.stdout.strip().splitlines()
    assert lines[-1] == "np walk rule: 256 lines"  # (2 x 3 + 2 periodic-only methods) x 2^4 switches x 2 capacities
    sent = 0
    for line in lines[:-1]:
        fields, verdict, msg = (part.strip() for part in line.split("|", 2))
        pbc, coulomb, bbox_ok, np_walk, d3, same, max_nb_lr = (int(x) for x in fields.split())
        accepted, built = (int(x) for x in verdict.split())
        host = capacity.builds_lr_list(1500 if bbox_ok else 1499, 1, bool(pbc), False, coulomb, bool(np_walk), bool(d3), bool(same))
        if (max_nb_lr > 0) != host:
            continue  # not what the host sends for this request
        sent += 1
        assert host == bool(built), line
        assert accepted or "max_nb_lr" not in msg, line
    assert sent == 128
