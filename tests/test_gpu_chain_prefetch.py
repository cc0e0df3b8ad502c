"""Engine option "chain_prefetch" (csrc/gemm_chain.hip, plan in csrc/gemm_chain_prefetch.h): at kernel entry the blocks of a one-launch
MLP sweep that share an XCD request the sweep's packed weight stream into their L2.  The requests deliver nothing the kernel
reads, so every output must be BITWISE the same: one-launch sweep with the requests (option 1: where they pay; 2: on every
grid), without them (0), and the per-layer launches of csrc/gemm_h2.hip - GELU' of every layer, the last layer's output, the
input adjoint of the backward sweep (pass 0 in both variants).

The row counts are chosen for the block-rank arithmetic of the plan and the panel forms, not for any workload:
    1     one block, one live row
    16    one full strip
    129   9 one-strip blocks: XCD 0 holds two blocks, the others one
    4097  first size with two-strip panels: 129 blocks, ragged last panel
    8193  first size with three-strip panels
That no request leaves its buffer is proven on the CPU (tests/test_chain_prefetch_plan.py), never probed here."""
from __future__ import annotations

import ctypes as C

import numpy as np
import pytest
import torch

from aimnetcentral_amd import _lib, workloads

pytestmark = pytest.mark.gpu

LAYER_DIMS = [[704, 512, 380, 258], [733, 512, 380, 258], [733, 512, 380, 380, 256]]  # synthetic_spec(0) = the shipped architecture


def pad32(n):
    return (n + 31) // 32 * 32


def _split2(eng, x, mode=1):
    m, k = x.shape
    out = torch.zeros(m, 2 * pad32(k), dtype=torch.int16, device=x.device)
    st = torch.cuda.current_stream(x.device).cuda_stream
    assert eng.lib.aimnet_debug_split_h2(x.data_ptr(), k, m, k, out.data_ptr(), 2 * pad32(k), mode, st) == 0, _lib.last_error()
    return out


def _ptrs(ts):
    return (C.c_void_p * len(ts))(*[t.data_ptr() if t is not None else None for t in ts])


# (label, chain, chain_prefetch): 1 issues the requests on grids where they pay (from about 1 700 rows), 2 on every grid - the small
# row counts below are there for the plan's arithmetic and need the requests issued
VARIANTS = (("per-layer", 0, 0), ("chain", 1, 0), ("chain+prefetch", 1, 1), ("chain+prefetch forced", 1, 2))


def _sweeps(eng, p, M, seed):
    """forward and backward sweep(s) of pass p on the same inputs, once per variant -> {label: {name: tensor}}"""
    dev = eng.device
    st = torch.cuda.current_stream(dev).cuda_stream
    d = LAYER_DIMS[p]
    nl, kp = len(d) - 1, [pad32(v) for v in d]
    g = torch.Generator(device="cpu").manual_seed(seed)
    numbers = torch.tensor([1, 6, 7, 8], dtype=torch.int32)[torch.randint(0, 4, (M,), generator=g)].to(dev)
    x2 = _split2(eng, torch.randn(M, d[0], generator=g).to(dev))
    zbar2 = _split2(eng, torch.randn(M, d[nl], generator=g).to(dev))
    out, D_ref = {}, None
    try:
        for label, chain, pf in VARIANTS:
            eng.set_option("chain_prefetch", pf)
            H = [torch.zeros(M, kp[l + 1], device=dev) for l in range(nl)]
            D = [torch.zeros(M, kp[l + 1], device=dev) for l in range(nl)]
            rc = eng.lib.aimnet_engine_debug_mlp_sweep(eng._h, p, 0, chain, 0, x2.data_ptr(), M, numbers.data_ptr(), _ptrs(H), _ptrs(D), None, None, st)
            assert rc == 0, _lib.last_error()
            if D_ref is None:
                D_ref = D  # every backward sweep reads the same chain-rule factors
            res = {"out": H[nl - 1]}
            for l in range(nl):
                if l < nl - 1 or p == 2:  # (the last layer of passes 0 / 1 is linear: no GELU')
                    res[f"D{l}"] = D[l]
            for flag in ((1, 0) if p == 0 else (0,)):
                zb = [torch.zeros(M * 2 * max(kp), dtype=torch.int16, device=dev) for _ in range(2)]
                zb[0][: M * 2 * kp[nl]] = zbar2.view(-1)  # dense rows, row stride 2 * k_out of the last layer
                which = C.c_int(-1)
                rc = eng.lib.aimnet_engine_debug_mlp_sweep(eng._h, p, 1, chain, flag, zb[0].data_ptr(), M, numbers.data_ptr(), None, _ptrs(D_ref), _ptrs(zb),
                                                           C.byref(which), st)
                assert rc == 0, _lib.last_error()
                xbar = zb[which.value].view(torch.float32)[: M * kp[0]].view(M, kp[0]).clone()
                res[f"xbar{flag}"] = xbar[:, 256:] if flag else xbar
            torch.cuda.synchronize()
            out[label] = res
    finally:
        eng.set_option("chain_prefetch", 1)
    return out


@pytest.mark.parametrize("M", [1, 16, 129, 4097, 8193])
@pytest.mark.parametrize("p", [0, 1, 2])
def test_sweeps_bitwise_equal_with_and_without_prefetch(hip_engine, p, M):
    assert hip_engine.get_option("chain_prefetch") == 1  # the default
    out = _sweeps(hip_engine, p, M, seed=31 * p + M)
    ref = out["per-layer"]
    for label in ("chain", "chain+prefetch", "chain+prefetch forced"):
        assert out[label].keys() == ref.keys()
        for key, want in ref.items():
            got = out[label][key]
            assert torch.equal(want, got), f"{label}: {key}"
            assert torch.isfinite(got).all(), f"{label}: {key}"
    for key in ref:
        if key.startswith("xbar"):
            assert ref[key].abs().max() > 0, key


def test_evaluation_bitwise_equal(hip_engine):
    """energy, forces, charges and stress of a periodic DSF evaluation of a 288-atom cell with and without the prefetch.
    At 288 rows the default (option 1) issues no requests, so the options compared are 0 and 2 (requests forced).  The default at
    sizes where it does issue them is covered by the sweep cases at M = 4097 and 8193 above, not by a whole evaluation here."""
    eng, dev = hip_engine, hip_engine.device
    c, z, cell = workloads.glucose_supercell((3, 1, 1))
    rng = np.random.default_rng(5)
    c = torch.from_numpy((c + rng.normal(0, 0.02, c.shape)).astype(np.float32)).to(dev)
    z = torch.from_numpy(z).to(dev)
    cell = torch.from_numpy(cell.astype(np.float32)).to(dev)
    assert eng.get_option("gemm_chain") == 1
    res = {}
    try:
        for mode in (0, 2):  # (288 rows: below the size from which option 1 issues the requests)
            eng.set_option("chain_prefetch", mode)
            r = eng.eval(c, z, torch.zeros(len(z), dtype=torch.int64, device=dev), torch.zeros(1, device=dev), cell=cell, forces=True, stress=True,
                         coulomb="dsf", dsf_rc=15.0)
            res[mode] = {k: v.clone() for k, v in r.items()}
    finally:
        eng.set_option("chain_prefetch", 1)
    for k in ("energy", "forces", "charges", "stress"):
        assert torch.equal(res[0][k], res[2][k]), k
        assert torch.isfinite(res[2][k]).all(), k
