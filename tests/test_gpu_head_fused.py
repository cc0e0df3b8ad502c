"""The fused energy head (csrc/gemm_head.hip: 256 -> 128 -> 128 -> 1, forward and backward in one launch, 64 atoms per block) at its
block edges, in both operand forms.

The default engines take the exact-fp32 path up to 256 rows, so the other modules reach a ragged or an exactly full block of the
head only by chance.  Here the split kernels are forced onto every size (gemm_bf3 = 2) with the fp16x2 (gemm_h2 = 1) and the bf16x3
(gemm_h2 = 0) operands, on batches of N = 3, 63, 64, 65, 128 and 129 atoms: one ragged block, exactly one block, one block plus one
row, two blocks, two blocks plus one row.

* The head's forward is the same instruction sequence with and without the backward (only the last wait of its second GEMM and the
  early return differ): the per-atom energies and the energies of an energy-only request and of a forces request are bitwise equal.
* Against the oracle, the gate of the randomised sweep (test_gpu_fuzz._compare, imported: reference gates + the fp32 oracle's own
  distance from fp64) - these are the inputs it was written for, random_batch molecules, at sizes it did not reach.
(Rows of the adjoint buffer beyond the batch are not looked at: the backward reuses that buffer.)"""
from __future__ import annotations

import numpy as np
import pytest
import torch

import test_gpu_fuzz as Z
from aimnetcentral_amd import workloads
from oracle import aimnet2_oracle as O

pytestmark = pytest.mark.gpu

SHAPES = [(1, 3), (3, 21), (2, 32), (5, 13), (4, 32), (3, 43)]  # (molecules, atoms each): N = 3, 63, 64, 65, 128, 129
CASES = [(s, h2, False) for s in SHAPES for h2 in (1, 0)] + [(s, h2, True) for s in ((2, 32), (5, 13)) for h2 in (1, 0)]

_refs: dict = {}  # (shape, nse) -> (case, fp32 oracle result, fp64 oracle result): computed once, shared by both operand forms


def _case_and_refs(shape, nse, orc, orc64):
    if (shape, nse) not in _refs:
        n_mol, k = shape
        c, z, mol, q = workloads.random_batch(n_mol, k, k, seed=100 * n_mol + k)
        mult = (1.0 + np.arange(n_mol) % 3).astype(np.float32)  # open-shell family: mixed multiplicities
        okw = dict(coulomb="simple", **({"mult": mult} if nse else {}))
        label = f"fused head: {n_mol} x {k} atoms, nse={nse}"
        case = (c, z, mol, q, mult, nse, dict(coulomb="simple"), okw, None, label)
        ref = O.evaluate(orc, c, z, q, mol, return_intermediates=True, **okw)
        ref64 = O.evaluate(orc64, c, z, q, mol, return_intermediates=True, **dict(okw, forces=False, stress=False))
        _refs[(shape, nse)] = (case, ref, ref64)
    return _refs[(shape, nse)]


@pytest.mark.parametrize("shape,h2,nse", CASES, ids=[f"{s[0]}x{s[1]}-{'h2' if h else 'bf3'}{'-nse' if n else ''}" for s, h, n in CASES])
def test_fused_head_at_block_edges(shape, h2, nse, hip_engine, hip_engine_nse, oracle32, oracle32_nse, oracle64, oracle64_nse):
    eng, orc, orc64 = (hip_engine_nse, oracle32_nse, oracle64_nse) if nse else (hip_engine, oracle32, oracle64)
    case, ref, ref64 = _case_and_refs(shape, nse, orc, orc64)
    c, z, mol, q, mult = case[:5]
    n, dev = len(z), eng.device
    charge = np.stack([0.5 * q + 0.5 * (mult - 1.0), 0.5 * q - 0.5 * (mult - 1.0)], axis=-1).astype(np.float32) if nse else q
    assert n == shape[0] * shape[1] and eng.get_option("head_fused") == 1
    try:
        eng.set_option("gemm_bf3", 2)
        eng.set_option("gemm_h2", h2)
        r = eng.eval(torch.from_numpy(c).to(dev), torch.from_numpy(z).to(dev), torch.from_numpy(mol).to(dev), torch.from_numpy(charge).to(dev),
                     forces=False, coulomb="simple")
        e_atom_fwd = eng.debug_view("e_atom")[:n].cpu().numpy().copy()
        energy_fwd = r["energy"].cpu().numpy().copy()
        res = Z.run_case(eng, case)  # the same batch with forces
        e_atom = eng.debug_view("e_atom")[:n].cpu().numpy().copy()
    finally:
        eng.set_option("gemm_bf3", 1)
        eng.set_option("gemm_h2", 1)
    assert np.isfinite(e_atom).all()
    assert e_atom_fwd.tobytes() == e_atom.tobytes(), f"{case[-1]}: e_atom differs between energy-only and forces"
    assert energy_fwd.tobytes() == res["energy"].tobytes(), f"{case[-1]}: energy differs between energy-only and forces"
    Z._compare(res, ref, ref64, mol, case[-1], nse)
