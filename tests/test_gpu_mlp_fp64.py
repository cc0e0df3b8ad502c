"""The MLP sweeps of large systems (aimnet_engine_debug_mlp_sweep: the one-launch csrc/gemm_chain.hip and the per-layer
csrc/gemm_h2.hip launches) against an fp64 MLP built from the oracle's copy of the weights - not against each other, as
test_gpu_chain.py does.

Every pass of the single- and two-channel engines, both sweep forms, at 300 / 5 000 / 10 080 / 12 400 rows (panel heights 16 /
32 / 48, ragged last panels, more panels than CUs).  Forward: the last output (fp32, and the split form where the sweep writes
one) and GELU' of every hidden layer; backward: the input adjoint J^T zbar for a random adjoint of the last pre-activation,
both pass-0 variants.  Pass 0 draws its element numbers from every finite row of the embedding table: the engine folds those
256 input columns into a per-element bias table (engine.hip, emb_bias0), the fp64 MLP takes them as input columns.

Gate: no worse than fp32 arithmetic - the same MLP in fp32 torch on the CPU, measured against fp64, is the yardstick:
kernel rms error <= 2 x, max error <= 4 x the yardstick's."""
from __future__ import annotations

import ctypes as C

import numpy as np
import pytest
import torch

from aimnetcentral_amd import _lib

pytestmark = pytest.mark.gpu

RMS_RATIO, MAX_RATIO = 2.0, 4.0


def pad32(n):
    return (n + 31) // 32 * 32


def _split2(eng, x):
    m, k = x.shape
    out = torch.zeros(m, 2 * pad32(k), dtype=torch.int16, device=x.device)
    st = torch.cuda.current_stream(x.device).cuda_stream
    assert eng.lib.aimnet_debug_split_h2(x.data_ptr(), k, m, k, out.data_ptr(), 2 * pad32(k), 1, st) == 0, _lib.last_error()
    return out


def _unsplit2(c2, n):
    m = c2.shape[0]
    v = c2.reshape(m, -1)[:, : 2 * pad32(n)].reshape(m, pad32(n) // 32, 2, 32).view(torch.float16).double()
    sign = torch.where(torch.arange(pad32(n) // 32, device=c2.device) % 2 == 1, -1.0, 1.0).double().view(1, -1, 1)
    return (v[:, :, 0] + sign * v[:, :, 1] / 4096.0).reshape(m, pad32(n))[:, :n]


def _ptrs(ts):
    return (C.c_void_p * len(ts))(*[t.data_ptr() if t is not None else None for t in ts])


def _gelu_grad(z):
    cdf = 0.5 * (1 + torch.erf(z / 2**0.5))
    return cdf + z * torch.exp(-0.5 * z * z) / (2 * torch.pi) ** 0.5


def _mlp(x, layers, last_linear):
    """-> (output, pre-activations)"""
    zs = []
    h = x
    for i, (w, b) in enumerate(layers):
        z = h @ w.T + b
        zs.append(z)
        h = z if (last_linear and i == len(layers) - 1) else torch.nn.functional.gelu(z)
    return h, zs


def _mlp_adjoint(zbar, layers, zs):
    """J^T zbar for zbar = adjoint of the last pre-activation"""
    g = zbar
    for l in range(len(layers) - 1, -1, -1):
        hb = g @ layers[l][0]
        g = hb * _gelu_grad(zs[l - 1]) if l > 0 else hb
    return g


def _err(got, ref):
    d = (got - ref).double()
    return d.pow(2).mean().sqrt().item(), d.abs().max().item()


def _check_weights(eng, oracle, p):
    """the fixture pair holds the same weights: the engine's spec (zero-padded to pad32 on upload, no column permutation) and
    the oracle's state dict"""
    sp = eng.spec
    layers = oracle.mlps[p]
    dims = [layers[0][0].shape[1]] + [w.shape[0] for w, _ in layers]
    assert list(sp.mlp_dims[p]) == dims
    for l, (w, b) in enumerate(layers):
        assert np.array_equal(np.asarray(sp.weights[f"mlps.{p}.{2 * l}.weight"], np.float64), w.numpy())
        assert np.array_equal(np.asarray(sp.weights[f"mlps.{p}.{2 * l}.bias"], np.float64), b.numpy())
    afv = oracle.afv.numpy()
    rows = np.nonzero(np.isfinite(afv).all(1))[0]
    assert np.array_equal(np.asarray(sp.weights["afv.weight"], np.float64)[rows], afv[rows])
    return dims, bool(sp.last_linear[p]), rows


ENGINES = [("hip_engine", "oracle64"), ("hip_engine_nse", "oracle64_nse")]


@pytest.mark.parametrize("M", [300, 5000, 10080, 12400])
@pytest.mark.parametrize("p", [0, 1, 2])
@pytest.mark.parametrize("which", ENGINES, ids=["nq1", "nq2"])
def test_mlp_sweeps_match_fp64(request, which, p, M):
    eng = request.getfixturevalue(which[0])
    oracle = request.getfixturevalue(which[1])
    dev, st = eng.device, torch.cuda.current_stream(eng.device).cuda_stream
    dims, last_linear, rows = _check_weights(eng, oracle, p)
    nl, kp = len(dims) - 1, [pad32(v) for v in dims]
    layers64 = [(w.to(dev), b.to(dev)) for w, b in oracle.mlps[p]]
    layers32 = [(w.float(), b.float()) for w, b in oracle.mlps[p]]

    g = torch.Generator().manual_seed(1000 * p + M + 7 * dims[-1])
    x = torch.randn(M, dims[0], generator=g)
    numbers = torch.from_numpy(rows.astype(np.int32))[torch.randint(0, len(rows), (M,), generator=g)]
    if p == 0:
        x[:, :256] = oracle.afv[numbers.long()].float()  # the embedding block (the engine reads its bias table instead)
    zbar = torch.randn(M, dims[-1], generator=g)

    # fp64 reference and fp32 CPU yardstick
    out64, zs64 = _mlp(x.double().to(dev), layers64, last_linear)
    out32, zs32 = _mlp(x, layers32, last_linear)
    xbar64 = _mlp_adjoint(zbar.double().to(dev), layers64, zs64)
    xbar32 = _mlp_adjoint(zbar, layers32, zs32)
    d64 = [_gelu_grad(z) for z in zs64]
    d32 = [_gelu_grad(z) for z in zs32]

    x2, zbar2 = _split2(eng, x.to(dev)), _split2(eng, zbar.to(dev))
    num_d = numbers.to(dev)
    report = []

    def gate(what, got, ref64, ref32):
        rk, mk = _err(got, ref64)
        ry, my = _err(ref32.to(dev), ref64)
        report.append(f"{what}: rms {rk:.2e} ({rk / ry:.2f} x fp32) max {mk:.2e} ({mk / my:.2f} x fp32)")
        assert torch.isfinite(got).all(), what
        assert rk <= RMS_RATIO * ry and mk <= MAX_RATIO * my, report[-1]

    for chain in (0, 1):
        for flag in ((0, 1) if not last_linear else (0,)):  # flag 1: the last output in split form (the fused head's input)
            H = [torch.zeros(M, kp[l + 1], device=dev) for l in range(nl)]
            D = [torch.zeros(M, kp[l + 1], device=dev) for l in range(nl)]
            rc = eng.lib.aimnet_engine_debug_mlp_sweep(eng._h, p, 0, chain, flag, x2.data_ptr(), M, num_d.data_ptr(), _ptrs(H), _ptrs(D),
                                                       None, None, st)
            assert rc == 0, _lib.last_error()
            torch.cuda.synchronize()
            last = _unsplit2(H[nl - 1].view(torch.int16), dims[-1]) if flag else H[nl - 1][:, : dims[-1]]
            gate(f"chain {chain} out{' (split)' if flag else ''}", last, out64, out32)
            if flag == 0:
                for l in range(nl):
                    if l < nl - 1 or not last_linear:
                        gate(f"chain {chain} GELU' {l}", D[l][:, : dims[l + 1]], d64[l], d32[l])
                Dfwd = D
        for flag in ((1, 0) if p == 0 else (0,)):  # pass 0: flag 1 forms only the conv columns 256.. of xbar
            zb = [torch.zeros(M * 2 * max(kp), dtype=torch.int16, device=dev) for _ in range(2)]
            zb[0][: M * 2 * kp[nl]] = zbar2.view(-1)  # dense rows, row stride 2 * k_out of the last layer
            which_buf = C.c_int(-1)
            rc = eng.lib.aimnet_engine_debug_mlp_sweep(eng._h, p, 1, chain, flag, zb[0].data_ptr(), M, num_d.data_ptr(), None, _ptrs(Dfwd),
                                                       _ptrs(zb), C.byref(which_buf), st)
            assert rc == 0, _lib.last_error()
            torch.cuda.synchronize()
            xbar = zb[which_buf.value].view(torch.float32)[: M * kp[0]].view(M, kp[0])
            c0 = 256 if flag else 0
            gate(f"chain {chain} xbar[{c0}:]", xbar[:, c0 : dims[0]], xbar64[:, c0:], xbar32[:, c0:])
    print(f"{which[0]} pass {p} M {M}:\n  " + "\n  ".join(report))
