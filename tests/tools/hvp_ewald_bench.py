"""Dense Hessian of the 96-atom periodic fixture (pbc96_dsf15, 288 directions) with Ewald summation: the analytic tangent sweep
against differences of the analytic forces (`hvp_method = "fd"`, the path this method took before the sweep carried it).  HIP
events, 5 warm-up calls, median of 10, the two operators interleaved.  `--once analytic|fd`: one warmed call of one operator and
nothing else (for a kernel trace of that call).  Record: profiles/r7_hvp_ewald.md."""
from __future__ import annotations

import argparse
import os
import statistics
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--once", choices=("analytic", "fd"))
    ap.add_argument("--accuracy", type=float, default=1e-6)
    a = ap.parse_args()
    from aimnetcentral_amd import AIMNet2Calculator, loader

    g = np.load(os.path.join(ROOT, "tests", "golden", "pbc96_dsf15.npz"))
    calc = AIMNet2Calculator(loader.synthetic_spec(0), device="cuda:0")
    calc.set_lrcoulomb_method("ewald", ewald_accuracy=a.accuracy)
    data = dict(coord=g["coord"], numbers=g["numbers"], charge=0.0, cell=g["cell"])
    eye = torch.eye(288, device="cuda").view(288, 96, 3)

    def run(method):
        calc.hvp_method = method
        return calc.hessian_vector_product(data, eye)

    if a.once:
        run(a.once)
        torch.cuda.synchronize()
        run(a.once)
        torch.cuda.synchronize()
        return
    times = {"analytic": [], "fd": []}
    for it in range(15):
        for method in ("analytic", "fd"):
            t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            t0.record()
            h = run(method)
            t1.record()
            torch.cuda.synchronize()
            if it >= 5:
                times[method].append(t0.elapsed_time(t1))
    ha, hf = run("analytic").view(288, 288), run("fd").view(288, 288)
    for m, t in times.items():
        print(f"{m:9s} median {statistics.median(t):9.3f} ms  min {min(t):9.3f}  max {max(t):9.3f}  (10 calls, 288 directions, 96 atoms)")
    print(f"max|H_analytic - H_fd| = {(ha - hf).abs().max().item():.3e} on max|H| = {ha.abs().max().item():.3e};  "
          f"asymmetry analytic {(ha - ha.T).abs().max().item():.3e}, fd {(hf - hf.T).abs().max().item():.3e}")
    print("status[7] (k entries) =", int(calc.engine.last_status[7]))


if __name__ == "__main__":
    main()
