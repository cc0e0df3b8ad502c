"""The DFT-D3 block under strain, timed on the 324- and 2 304-atom cells of tests/tools/strain_bench.py with the external term at 15 A
(AIMNet2Calculator on synthetic weights, DSF Coulomb at the default cutoff, set_dftd3_hessian("analytic")):
  (i)   the armed sweep of the six Voigt strains with the term (AIMNet2Calculator.strain_response),
  (ii)  the same sweep of a calculator without the term,
  (iii) 24 evaluations of eval(forces, stress) with the term: the 4-point central difference a user would otherwise take,
  (iv)  a 6-direction hessian_vector_product with the term through the analytic block, no strain, and (v) the same without the term
        - (iv) - (v) is the unarmed analytic block at the same K, for comparison with (i) - (ii), the block's cost under strain.
HIP events on one device in one process, the operators interleaved call by call, `--warmup` calls dropped, median / min / max of
`--calls`.  Not gated.  Record: profiles/strain_d3.md."""
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


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--calls", type=int, default=7)
    ap.add_argument("--sizes", default="324,2304")
    a = ap.parse_args()
    from pme_hvp_bench import small_cell, supercell
    from strain_bench import fd_strain_response, voigt_strains

    from aimnetcentral_amd import AIMNet2Calculator, loader

    gd, tab = (np.load(os.path.join(ROOT, "tests", "golden", f + ".npz")) for f in ("dftd3", "dftd3_subset"))
    spec = loader.synthetic_spec(0)
    spec.metadata = dict(spec.metadata, needs_dispersion=True, d3_params={k: float(gd[k]) for k in ("s6", "s8", "a1", "a2")})
    with_d3 = AIMNet2Calculator(spec, device="cuda:0", dftd3_data={k: tab[k] for k in ("c6ab", "cn_ref", "rcov", "r4r2")})
    without = AIMNet2Calculator(loader.synthetic_spec(0), device="cuda:0")
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        with_d3.set_lrcoulomb_method("dsf")
        without.set_lrcoulomb_method("dsf")
    with_d3.set_dftd3_hessian("analytic")
    g = np.load(os.path.join(ROOT, "tests", "golden", "pbc96_dsf15.npz"))
    ca, za, cella = small_cell(5, 12, 6.0)
    cells = {324: supercell(ca, za, cella, (3, 3, 3), 3), 2304: supercell(g["coord"], g["numbers"], g["cell"], (6, 2, 2), 3)}
    eps = voigt_strains()
    for n in (int(s) for s in a.sizes.split(",")):
        data = cells[n]
        assert len(data["numbers"]) == n
        v = torch.from_numpy(np.random.default_rng(4).standard_normal((6, n, 3)).astype(np.float32)).cuda()
        ops = {"(i) armed sweep, 6 strains, D3": lambda: with_d3.strain_response(data, eps),
               "(ii) armed sweep, 6 strains, no D3": lambda: without.strain_response(data, eps),
               "(iii) eval differences, 24 evaluations, D3": lambda: fd_strain_response(with_d3, data, eps),
               "(iv) hvp, 6 directions, D3 analytic": lambda: with_d3.hessian_vector_product(data, v),
               "(v) hvp, 6 directions, no D3": lambda: without.hessian_vector_product(data, v)}
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
        med = {}
        for name, t in times.items():
            med[name] = statistics.median(t)
            print(f"{n:5d} atoms  {name:44s} median {med[name]:9.3f} ms  min {min(t):9.3f}  max {max(t):9.3f}  spread {max(t) - min(t):7.3f}  "
                  f"({a.calls} calls)", flush=True)
        k = list(ops)
        print(f"{n:5d} atoms  block under strain (i) - (ii) = {med[k[0]] - med[k[1]]:.3f} ms;  analytic block without strain (iv) - (v) = "
              f"{med[k[3]] - med[k[4]]:.3f} ms;  (iii) / (i) = {med[k[2]] / med[k[0]]:.1f}", flush=True)
        sw, (dF, dS) = out[k[0]], out[k[2]]
        print(f"{n:5d} atoms  max|dF/de sweep - differences| = {(sw['force_derivative'] - dF).abs().max().item():.3e} on "
              f"{sw['force_derivative'].abs().max().item():.3e};  max|d stress/de sweep - differences| = "
              f"{(sw['stress_derivative'] - dS).abs().max().item():.3e} on {sw['stress_derivative'].abs().max().item():.3e}", flush=True)


if __name__ == "__main__":
    main()
