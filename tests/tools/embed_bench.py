"""Cost of the electrostatic embedding (csrc/embed.hip): the time an evaluation with forces gains from M point charges per
molecule, on taxol (113 atoms, tests/golden/taxol.npz) and on a shard of 128 x 50-atom molecules.

Device events around synchronised regions of `--reps` evaluations, one warm-up region, the median of five regions; the embedded
and the plain evaluation alternate inside one call.  With `--plain-only` only the plain evaluation is timed (five regions, their
median and spread): run it once on this build and once with AIMNET_HIP_LIB naming another build of the library to compare the two.
The field pass's own time and pair rate come from the engine's family timer (set_profiling) on an evaluation without the site pass.

    python tests/tools/embed_bench.py [--sites 1000 20000 200000] [--reps 20] [--plain-only]
"""
from __future__ import annotations

import argparse
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)

from aimnetcentral_amd import loader, workloads  # noqa: E402
from aimnetcentral_amd.engine import HipEngine  # noqa: E402


def region_ms(fn, reps):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    a.record()
    for _ in range(reps):
        fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b) / reps


def shell_sites(coord, mol, n_mol, M, rng):
    """M sites per molecule on shells 2.5 - 8 A outside the molecule (the construction of the test fixture)."""
    X, em = [], []
    for m in range(n_mol):
        x = coord[mol == m].astype(np.float64)
        c = x.mean(0)
        R = np.linalg.norm(x - c, axis=1).max()
        d = rng.standard_normal((M, 3))
        d /= np.linalg.norm(d, axis=1, keepdims=True)
        X.append((c + d * (R + rng.uniform(2.5, 8.0, M))[:, None]).astype(np.float32))
        em.append(np.full(M, m, np.int32))
    return np.concatenate(X), rng.uniform(-0.8, 0.8, M * n_mol).astype(np.float32), np.concatenate(em)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sites", type=int, nargs="*", default=[1000, 20000, 200000])
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--plain-only", action="store_true")
    a = ap.parse_args()
    dev = torch.device("cuda:0")
    eng = HipEngine(loader.synthetic_spec(0, cold=True), dev)
    g = np.load(os.path.join(ROOT, "tests", "golden", "taxol.npz"))
    c50, z50, m50, q50 = workloads.random_batch(128, 50, 50, seed=1)
    cases = {"taxol": (g["coord"].astype(np.float32), g["numbers"], np.zeros(113, np.int64), np.zeros(1, np.float32)),
             "128x50": (c50, z50, m50, q50)}
    rng = np.random.default_rng(5)
    for name, (c, z, mol, q) in cases.items():
        n_mol = len(q)
        args = [torch.from_numpy(np.ascontiguousarray(v)).to(dev) for v in (c, z, mol, q)]
        plain = lambda: eng.eval(*args, forces=True, coulomb="simple", sync=False)  # noqa: E731
        region_ms(plain, a.reps)
        if a.plain_only:
            t = [region_ms(plain, a.reps) for _ in range(5)]
            print(json.dumps({"case": name, "sites": 0, "lib": os.environ.get("AIMNET_HIP_LIB", "in-tree"), "plain_ms": float(np.median(t)),
                              "spread_ms": float(max(t) - min(t))}))
            continue
        for M in a.sites:
            X, Q, em = shell_sites(c, mol, n_mol, M, rng)
            e = dict(ext_coord=torch.from_numpy(X).to(dev), ext_charge=torch.from_numpy(Q).to(dev),
                     ext_mol_idx=torch.from_numpy(em).to(dev), want_ext_forces=True)
            emb = lambda: eng.eval(*args, forces=True, coulomb="simple", sync=False, embedding=e)  # noqa: E731
            region_ms(emb, a.reps)
            tp, te = [], []
            for _ in range(5):  # alternate the two
                tp.append(region_ms(plain, a.reps))
                te.append(region_ms(emb, a.reps))
            # the field pass alone: no site pass requested, the "coulomb" family of the engine's timer gains field + seed pass
            e_field = {k: v for k, v in e.items() if k != "want_ext_forces"}
            field = lambda: eng.eval(*args, forces=True, coulomb="simple", sync=False, embedding=e_field)  # noqa: E731
            eng.set_profiling(2)
            region_ms(field, a.reps)
            coul_emb = eng.read_profile()["coulomb"] / a.reps
            region_ms(plain, a.reps)
            coul_plain = eng.read_profile()["coulomb"] / a.reps
            eng.set_profiling(0)
            pairs = float(len(z)) * M  # every atom against the M sites of its molecule
            print(json.dumps({"case": name, "sites_per_mol": M, "plain_ms": float(np.median(tp)), "embedded_ms": float(np.median(te)),
                              "added_ms": float(np.median(te) - np.median(tp)), "spread_plain_ms": float(max(tp) - min(tp)),
                              "field_pass_ms": coul_emb - coul_plain,
                              "field_pass_pairs_per_s": pairs / max(1e-9, (coul_emb - coul_plain) * 1e-3)}))
            del e


if __name__ == "__main__":
    main()
