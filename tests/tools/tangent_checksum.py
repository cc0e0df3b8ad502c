"""Checksums of the two tangent entry points (every output of `HipEngine.hvp` and `HipEngine.charge_response` as raw bytes) and their
workspace sizes: equal across two builds of the library when a change to the host code of csrc/hvp.hip leaves every launch as it
was.  One line per case, so two runs compare with diff.  AIMNET_HIP_LIB=<the other build's libaimnet_hip.so> python tests/tools/tangent_checksum.py"""
import ctypes as C
import hashlib
import os
import sys

import numpy as np
import torch

ROOT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "..")
sys.path.insert(0, ROOT)
from aimnetcentral_amd import _lib, capacity, loader  # noqa: E402
from aimnetcentral_amd.engine import HipEngine  # noqa: E402


def golden(name):
    return np.load(os.path.join(ROOT, "tests", "golden", name + ".npz"))


def t(a, dt=torch.float32):
    return torch.as_tensor(np.asarray(a)).to(dt).to("cuda:0")


def sha(res):
    return {k: hashlib.sha1(v.cpu().numpy().tobytes()).hexdigest()[:12] for k, v in sorted(res.items())}


def args_of(eng, coord, numbers, mol=None, charge=(0.0,), mult=None):
    q = np.atleast_1d(np.asarray(charge, dtype=np.float32))
    if eng.nq == 2:  # (alpha, beta) of every molecule
        mt = np.ones_like(q) if mult is None else np.atleast_1d(np.asarray(mult, dtype=np.float32))
        q = np.stack([0.5 * q + 0.5 * (mt - 1), 0.5 * q - 0.5 * (mt - 1)], -1)
    mol = np.zeros(len(numbers), dtype=np.int64) if mol is None else mol
    return t(coord), t(numbers, torch.int32), t(mol, torch.int32), t(q)


def directions(k, n, seed):
    return t(np.random.default_rng(seed).standard_normal((k, n, 3)).astype(np.float32))


def main():
    eng = HipEngine(loader.synthetic_spec(0), "cuda:0")
    nse = HipEngine(loader.synthetic_spec(0, num_charge_channels=2), "cuda:0")
    gd, tab = golden("dftd3"), golden("dftd3_subset")
    d3 = dict(s6=float(gd["s6"]), s8=float(gd["s8"]), a1=float(gd["a1"]), a2=float(gd["a2"]), cutoff=15.0, smoothing_fraction=0.2)
    eng.set_dftd3_tables({k: tab[k] for k in ("c6ab", "cn_ref", "rcov", "r4r2")})

    g = golden("hvp40")
    a40, eye = args_of(eng, g["coord"], g["numbers"]), torch.eye(120, device="cuda:0").view(120, 40, 3).contiguous()
    p = golden("pbc96_dsf8_wrapped")
    a96, cell96, v96 = args_of(eng, p["coord"], p["numbers"]), t(p["cell"]), directions(3, 96, 11)
    s = golden("nse")
    ab5 = args_of(nse, s["b5_coord"], s["b5_numbers"], s["b5_mol_idx"], s["b5_charge"], s["b5_mult"])
    vb5 = directions(3, len(s["b5_numbers"]), 12)
    x = golden("taxol")
    n_taxol = len(x["numbers"])

    cases = (
        ("hvp hvp40 simple", lambda: eng.hvp(*a40, eye)),
        ("hvp hvp40 dsf8", lambda: eng.hvp(*a40, eye, coulomb="dsf", dsf_rc=8.0)),
        ("hvp hvp40 simple + forces", lambda: eng.hvp(*a40, eye, want_forces=True)),
        ("hvp pbc96 dsf8", lambda: eng.hvp(*a96, v96, cell=cell96, coulomb="dsf", dsf_rc=8.0, dsf_alpha=0.25, want_forces=True)),
        ("hvp pbc96 ewald", lambda: eng.hvp(*a96, v96, cell=cell96, coulomb="ewald", ewald_accuracy=1e-6, want_forces=True)),
        ("hvp nse b5", lambda: nse.hvp(*ab5, vb5, want_forces=True)),
        ("hvp hvp40 simple + d3", lambda: eng.hvp(*a40, eye, dftd3=d3, want_forces=True)),
        ("charge_response hvp40 dipole", lambda: eng.charge_response(*a40, eye)),
        ("charge_response pbc96", lambda: eng.charge_response(*a96, v96, cell=cell96)),
        ("charge_response nse b5 dspin", lambda: nse.charge_response(*ab5, vb5)),
    )
    for name, run in cases:
        print(f"{name}: {sha(run())}")

    def request(n, periodic, method, rc, dftd3=None):
        return capacity.Request("hvp", n, 1, periodic, method, rc, dftd3=dftd3)

    e96 = capacity.ewald_list_cutoff([abs(np.linalg.det(p["cell"].astype(np.float64)))], [96], 1e-6)
    for name, n, rq in (("40 atoms", 40, request(40, False, _lib.COULOMB_SIMPLE, 15.0)),
                        ("96 atoms periodic ewald", 96, request(96, True, _lib.COULOMB_EWALD, e96)),
                        ("taxol dsf + d3", n_taxol, request(n_taxol, False, _lib.COULOMB_DSF, 15.0, d3))):
        opt = eng.fill_options(rq)
        for entry in ("hvp", "charge_response"):
            f = getattr(eng.lib, f"aimnet_engine_{entry}_workspace_bytes")
            print(f"workspace bytes, {entry}, {name}: " + ", ".join(f"K={k}: {int(f(eng._h, n, 1, k, C.byref(opt)))}" for k in (1, 2, 120)))


if __name__ == "__main__":
    main()
