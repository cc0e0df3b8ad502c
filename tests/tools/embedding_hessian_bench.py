"""Cost of the electrostatic embedding in the analytic Hessian sweep: the dense Hessian of the 40-atom fixture (120 unit directions,
HipEngine.hvp, coulomb "simple") without an embedding and with M = 64, 10^4 and 10^5 point charges, with and without the mixed
block ext_hv.  The numbers of profiles/embedding_hessian.md.

    python tests/tools/embedding_hessian_bench.py [--bare-only] [--rounds R] > embedding_hessian_bench.json

Every figure is a host clock around n calls that end in a device synchronise, after a warm-up call of the same shape
(tests/tools/hvp_bench.py::timed); the variants are timed in turn, R rounds of them, and the median and the spread (min - max) over
the rounds are reported.  --bare-only times the unarmed path alone: the script then runs in a checkout without the feature too,
which is how the parent commit's figure is taken in the same job, alternating with this one."""
import argparse
import json
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path[:0] = [ROOT, HERE]
from aimnetcentral_amd import loader  # noqa: E402
from aimnetcentral_amd.engine import HipEngine  # noqa: E402
from hvp_bench import timed  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--bare-only", action="store_true")
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--calls", type=int, default=20)
    a = ap.parse_args()
    g = np.load(os.path.join(os.path.dirname(HERE), "golden", "hvp40.npz"))
    n = len(g["numbers"])
    t = lambda v, dt=torch.float32: torch.as_tensor(np.asarray(v)).to(dt).cuda()  # noqa: E731
    eng = HipEngine(loader.synthetic_spec(0), "cuda:0")
    args = (t(g["coord"]), t(g["numbers"], torch.int32), torch.zeros(n, dtype=torch.int32, device="cuda"), t([0.0]))
    eye = torch.eye(3 * n, device="cuda").view(3 * n, n, 3)
    variants = {"bare": lambda: eng.hvp(*args, eye, coulomb="simple")}
    if not a.bare_only:
        sys.path.insert(0, os.path.dirname(HERE))
        from embedding_yardstick import sites  # M point charges 2.5 - 8 A outside the molecule

        for M in (64, 10_000, 100_000):
            X, Q = sites(g["coord"], M)
            for ext in (False, True):
                e = dict(ext_coord=t(X), ext_charge=t(Q), want_ext_hv=ext)
                variants[f"M={M}" + (" + ext_hv" if ext else "")] = lambda e=e: eng.hvp(*args, eye, coulomb="simple", embedding=e)
    times = {k: [] for k in variants}
    for _ in range(a.rounds):
        for k, fn in variants.items():
            times[k].append(timed(fn, a.calls))
    res = {k: {"median_ms": float(np.median(v)), "min_ms": float(min(v)), "max_ms": float(max(v))} for k, v in times.items()}
    print(json.dumps({"tree": ROOT, "directions": 3 * n, "atoms": n, "rounds": a.rounds, "calls_per_round": a.calls, "hessian_ms": res}, indent=1))


if __name__ == "__main__":
    main()
