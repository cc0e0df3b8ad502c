"""Hessian-vector products with the external DFT-D3 term, the dispersion block armed (HipEngine.hvp(..., d3_tangent=True): the
analytic tangent of csrc/d3.hip) against unarmed (the 4-point central difference over four displaced copies of the D3 list per
direction - the launches of every build before the switch existed).  One direction and 16 directions on the 324-atom cell and the
2 304-atom cell of tests/tools/pme_hvp_bench.py (DSF Coulomb at 15 A, D3 at 15 A), and the dense Hessian (120 unit directions) of a
40-atom molecule.  HIP events on one device in one process, the two operators in ABBA order within every round, `--warmup` rounds
dropped, median / min / max of 2 x `--rounds` calls each.  Then the error of both blocks against the fp64 yardstick
(tests/d3_tangent_yardstick.py) on het27 / par12: the armed block alone, and the unarmed block as armed block + (unarmed sweep -
armed sweep) - the two sweeps share every other launch bit for bit.  Not gated.  Record: profiles/d3_hessian.md."""
from __future__ import annotations

import argparse
import ctypes as C
import os
import statistics
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

from pme_hvp_bench import small_cell, supercell  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--rounds", type=int, default=4)
    ap.add_argument("--sizes", default="324,2304")
    a = ap.parse_args()
    from aimnetcentral_amd import _lib, capacity, loader, workloads
    from aimnetcentral_amd.engine import HipEngine

    import d3_cases as D
    import d3_tangent_yardstick as Y

    eng = HipEngine(loader.synthetic_spec(0), "cuda:0")
    eng.set_dftd3_tables(D.tables())
    par = D.par(15.0)
    dev = eng.device

    def tens(x, dt=torch.float32):
        return torch.as_tensor(np.asarray(x)).to(dt).to(dev)

    def timed(label, args, kw, K, v):
        times = {True: [], False: []}
        out = {}
        for it in range(a.warmup + a.rounds):
            for armed in (True, False, False, True):
                t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                t0.record()
                out[armed] = eng.hvp(*args, v, dftd3=par, d3_tangent=armed, **kw)["hv"]
                t1.record()
                torch.cuda.synchronize()
                if it >= a.warmup:
                    times[armed].append(t0.elapsed_time(t1))
        med = {k: statistics.median(t) for k, t in times.items()}
        for armed, name in ((True, "armed"), (False, "unarmed")):
            t = times[armed]
            print(f"{label}  K = {K:3d}  {name:8s} median {med[armed]:9.3f} ms  min {min(t):9.3f}  max {max(t):9.3f}  per direction "
                  f"{med[armed] / K:8.4f} ms  ({len(t)} calls)", flush=True)
        print(f"{label}  K = {K:3d}  armed / unarmed = {med[True] / med[False]:.3f}   max|armed - unarmed| = "
              f"{(out[True] - out[False]).abs().max().item():.3e} on max|Hv| = {out[False].abs().max().item():.3e}", flush=True)

    g = np.load(os.path.join(ROOT, "tests", "golden", "pbc96_dsf15.npz"))
    ca, za, cella = small_cell(5, 12, 6.0)
    cells = {324: supercell(ca, za, cella, (3, 3, 3), 3), 2304: supercell(g["coord"], g["numbers"], g["cell"], (6, 2, 2), 3)}
    for n in (int(s) for s in a.sizes.split(",")):
        d = cells[n]
        args = (tens(d["coord"]), tens(d["numbers"], torch.int32), torch.zeros(n, dtype=torch.int32, device=dev), tens([0.0]))
        kw = dict(cell=tens(d["cell"]), coulomb="dsf", dsf_rc=15.0)
        for K in (1, 16):
            v = tens(np.random.default_rng(4).standard_normal((K, n, 3)))
            timed(f"{n:5d} atoms", args, kw, K, v)
        # bytes of one more direction, as the split of the sweeps sees them
        opt = eng.fill_options(capacity.Request("hvp", n, 1, True, _lib.COULOMB_DSF, 15.0, 0.2, 1e-6, par))
        per = {}
        for armed in (0, 1):
            eng.lib.aimnet_engine_set_dftd3_tangent(eng._h, armed)
            per[armed] = [int(eng.lib.aimnet_engine_hvp_workspace_bytes(eng._h, n, 1, K, C.byref(opt))) for K in (1, 2)]
        eng.lib.aimnet_engine_set_dftd3_tangent(eng._h, 0)
        print(f"{n:5d} atoms  max_nb_d3 {int(opt.max_nb_d3)}  workspace per direction and atom: unarmed {(per[0][1] - per[0][0]) / n:.0f} B, "
              f"armed {(per[1][1] - per[1][0]) / n:.0f} B", flush=True)

    c40, z40 = workloads.random_organic(40, np.random.Generator(np.random.PCG64(5)))
    args = (tens(c40), tens(z40, torch.int32), torch.zeros(40, dtype=torch.int32, device=dev), tens([0.0]))
    timed("   40 atoms", args, dict(coulomb="simple"), 120, tens(np.eye(120).reshape(120, 40, 3)))

    # error of both blocks against the yardstick
    c = D.case("het27")
    V = Y.directions(c, 3)
    ref = Y.yardstick(c, "par12", V)
    top = np.abs(ref).max()
    p12 = D.get_par("par12")
    args = (tens(c.coord), tens(c.numbers, torch.int32), tens(c.mol, torch.int32), tens(c.charge))
    kw = dict(cell=tens(c.cell), coulomb="none", dftd3=p12)
    alone = eng.hvp(*args, tens(V), d3_tangent=True, _d3_block_only=True, **kw)["hv"].cpu().numpy().astype(np.float64)
    armed = eng.hvp(*args, tens(V), d3_tangent=True, **kw)["hv"].cpu().numpy().astype(np.float64)
    unarmed = eng.hvp(*args, tens(V), **kw)["hv"].cpu().numpy().astype(np.float64)
    print(f"het27 / par12, 3 random directions, max|H_d3 v| = {top:.3e} eV/A^2: armed block {np.abs(alone - ref).max():.3e} "
          f"({np.abs(alone - ref).max() / top:.2e} of max), unarmed block {np.abs(alone + (unarmed - armed) - ref).max():.3e} "
          f"({np.abs(alone + (unarmed - armed) - ref).max() / top:.2e} of max); max|sweep without the block| = "
          f"{np.abs(armed - alone).max():.3e}", flush=True)


if __name__ == "__main__":
    main()
