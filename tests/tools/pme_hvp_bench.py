"""Hessian-vector products of periodic cells with the three operators a "pme" user can choose from: the armed mesh sweep
(set_pme_hessian("analytic")), the exact-Ewald sweep (set_lrcoulomb_method("ewald")) and differences of the analytic forces with the
mesh method (the default for "pme": four force evaluations per direction).  One direction and 16 directions on the 324-atom cell
(cell A of tests/test_gpu_hvp_ewald.py, 3 x 3 x 3) and a 2 304-atom cell (pbc96_dsf15, 6 x 2 x 2).  HIP events on one device in one
process, the operators interleaved call by call, `--warmup` calls dropped, median / min / max of `--calls`.  Not gated.
Record: profiles/pme_hessian.md."""
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


def small_cell(seed, n, L, dmin=0.95):
    """`small_cell` of tests/test_gpu_hvp_ewald.py"""
    rng = np.random.default_rng(seed)
    cell = np.diag([L, 1.1 * L, 0.9 * L]); cell[1, 0] = 0.8; cell[2, 0] = -0.6; cell[2, 1] = 0.5
    inv, pts = np.linalg.inv(cell), []
    while len(pts) < n:
        x = rng.random(3) @ cell
        if all(np.linalg.norm(((x - p) @ inv - np.rint((x - p) @ inv)) @ cell) >= dmin for p in pts):
            pts.append(x)
    z = rng.choice([1, 6, 7, 8], size=n, p=[0.5, 0.3, 0.1, 0.1])
    return np.array(pts, np.float32), z.astype(np.int64), cell.astype(np.float32)


def supercell(coord, numbers, cell, reps, seed):
    shifts = np.array([(i, j, k) for i in range(reps[0]) for j in range(reps[1]) for k in range(reps[2])], dtype=np.float64)
    x = (coord[None].astype(np.float64) + (shifts @ cell.astype(np.float64))[:, None]).reshape(-1, 3)
    x = (x + np.random.default_rng(seed).normal(0.0, 0.02, x.shape)).astype(np.float32)
    return dict(coord=x, numbers=np.tile(numbers, len(shifts)), charge=0.0, cell=(np.array(reps)[:, None] * cell).astype(np.float32))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--accuracy", type=float, default=1e-6)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--calls", type=int, default=7)
    ap.add_argument("--sizes", default="324,2304")
    a = ap.parse_args()
    from aimnetcentral_amd import AIMNet2Calculator, loader

    def calculator(method, armed):
        calc = AIMNet2Calculator(loader.synthetic_spec(0), device="cuda:0")
        with warnings.catch_warnings():
            warnings.simplefilter("ignore")
            calc.set_lrcoulomb_method(method, ewald_accuracy=a.accuracy)
        if armed:
            calc.set_pme_hessian("analytic")
        return calc

    ops = {"pme sweep": calculator("pme", True), "ewald sweep": calculator("ewald", False), "pme fd": calculator("pme", False)}
    g = np.load(os.path.join(ROOT, "tests", "golden", "pbc96_dsf15.npz"))
    ca, za, cella = small_cell(5, 12, 6.0)
    cells = {324: supercell(ca, za, cella, (3, 3, 3), 3), 2304: supercell(g["coord"], g["numbers"], g["cell"], (6, 2, 2), 3)}
    for n in (int(s) for s in a.sizes.split(",")):
        data = cells[n]
        assert len(data["numbers"]) == n
        for K in (1, 16):
            v = torch.from_numpy(np.random.default_rng(4).standard_normal((K, n, 3)).astype(np.float32)).cuda()
            times = {k: [] for k in ops}
            out = {}
            for it in range(a.warmup + a.calls):
                for name, calc in ops.items():
                    t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                    t0.record()
                    out[name] = calc.hessian_vector_product(data, v)
                    t1.record()
                    torch.cuda.synchronize()
                    if it >= a.warmup:
                        times[name].append(t0.elapsed_time(t1))
            for name, t in times.items():
                med = statistics.median(t)
                print(f"{n:5d} atoms  K = {K:2d}  {name:12s} median {med:9.3f} ms  min {min(t):9.3f}  max {max(t):9.3f}  "
                      f"per direction {med / K:9.3f} ms  ({a.calls} calls)", flush=True)
            ref = out["ewald sweep"]
            for name in ("pme sweep", "pme fd"):
                print(f"{n:5d} atoms  K = {K:2d}  max|{name} - ewald sweep| = {(out[name] - ref).abs().max().item():.3e} on "
                      f"max|Hv| = {ref.abs().max().item():.3e}", flush=True)
        print(f"{n:5d} atoms  status[7]: mesh points {int(ops['pme sweep'].engine.last_status[7])}, "
              f"k entries {int(ops['ewald sweep'].engine.last_status[7])}", flush=True)


if __name__ == "__main__":
    main()
