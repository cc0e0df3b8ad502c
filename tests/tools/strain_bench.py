"""Strain derivatives of periodic cells, timed: the six Voigt strains in ONE armed tangent sweep (AIMNet2Calculator.strain_response:
dF/d strain and d stress/d strain), beside what a user had before it - a 4-point central difference of eval(forces, stress) over
strained cells, 24 evaluations - and an unarmed 16-direction hessian_vector_product on the same cells (the form everybody else runs:
compare it between two builds with `--unarmed-only`, which needs nothing of the feature).  The 324-atom and 2 304-atom cells of
tests/tools/pme_hvp_bench.py, DSF Coulomb at the default cutoff.  HIP events on one device in one process, the operators interleaved
call by call, `--warmup` calls dropped, median / min / max of `--calls` (the spread of a row is its max - min).  Not gated.
Record: profiles/strain_tangent.md."""
from __future__ import annotations

import argparse
import os
import statistics
import sys
import warnings

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

FD_STEP = 1e-3  # relative strain step of the difference quotient (fp32 forces: the noise / kink trade-off of calculator._fd_hvp)


def voigt_strains():
    e = np.zeros((6, 3, 3), np.float32)
    for I, (a, b) in enumerate(((0, 0), (1, 1), (2, 2), (1, 2), (0, 2), (0, 1))):
        e[I, a, b] += 0.5
        e[I, b, a] += 0.5
    return e


def fd_strain_response(calc, data, strains, h=FD_STEP):
    """(dF/dt [K,N,3], d stress/dt [K,3,3]) by the 4-point central difference of eval(forces, stress): 4 K evaluations."""
    x, cell = np.asarray(data["coord"], np.float64), np.asarray(data["cell"], np.float64)
    dF, dS = [], []
    for eps in strains.astype(np.float64):
        r = {}
        for k in (1, -1, 2, -2):
            s = np.eye(3) + k * h * eps
            r[k] = calc(dict(data, coord=(x @ s).astype(np.float32), cell=(cell @ s).astype(np.float32)), forces=True, stress=True)
        dF.append((8.0 * (r[1]["forces"] - r[-1]["forces"]) - (r[2]["forces"] - r[-2]["forces"])) / (12.0 * h))
        dS.append((8.0 * (r[1]["stress"] - r[-1]["stress"]) - (r[2]["stress"] - r[-2]["stress"])) / (12.0 * h))
    return torch.stack(dF), torch.stack(dS)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--calls", type=int, default=7)
    ap.add_argument("--sizes", default="324,2304")
    ap.add_argument("--unarmed-only", action="store_true", help="the 16-direction hvp alone (runs on a build without the feature)")
    a = ap.parse_args()
    from pme_hvp_bench import small_cell, supercell

    from aimnetcentral_amd import AIMNet2Calculator, loader

    calc = AIMNet2Calculator(loader.synthetic_spec(0), device="cuda:0")
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        calc.set_lrcoulomb_method("dsf")
    g = np.load(os.path.join(ROOT, "tests", "golden", "pbc96_dsf15.npz"))
    ca, za, cella = small_cell(5, 12, 6.0)
    cells = {324: supercell(ca, za, cella, (3, 3, 3), 3), 2304: supercell(g["coord"], g["numbers"], g["cell"], (6, 2, 2), 3)}
    eps = voigt_strains()
    for n in (int(s) for s in a.sizes.split(",")):
        data = cells[n]
        assert len(data["numbers"]) == n
        v = torch.from_numpy(np.random.default_rng(4).standard_normal((16, n, 3)).astype(np.float32)).cuda()
        ops = {"unarmed hvp, 16 directions": lambda: calc.hessian_vector_product(data, v)}
        if not a.unarmed_only:
            ops["armed sweep, 6 strains"] = lambda: calc.strain_response(data, eps)
            ops["eval differences, 24 evaluations"] = lambda: fd_strain_response(calc, data, eps)
        times, out = {k: [] for k in ops}, {}
        for it in range(a.warmup + a.calls):
            for name, op in ops.items():
                t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                t0.record()
                out[name] = op()
                t1.record()
                torch.cuda.synchronize()
                if it >= a.warmup:
                    times[name].append(t0.elapsed_time(t1))
        for name, t in times.items():
            med = statistics.median(t)
            print(f"{n:5d} atoms  {name:34s} median {med:9.3f} ms  min {min(t):9.3f}  max {max(t):9.3f}  spread {max(t) - min(t):7.3f}  "
                  f"({a.calls} calls)", flush=True)
        if not a.unarmed_only:
            sw, (dF, dS) = out["armed sweep, 6 strains"], out["eval differences, 24 evaluations"]
            print(f"{n:5d} atoms  max|dF/de sweep - differences| = {(sw['force_derivative'] - dF).abs().max().item():.3e} on "
                  f"{sw['force_derivative'].abs().max().item():.3e};  max|d stress/de sweep - differences| = "
                  f"{(sw['stress_derivative'] - dS).abs().max().item():.3e} on {sw['stress_derivative'].abs().max().item():.3e}", flush=True)


if __name__ == "__main__":
    main()
