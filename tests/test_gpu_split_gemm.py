"""The split-operand MLP GEMMs of large systems against fp64: csrc/gemm_h2.hip (fp16x2 operands, the default) and
csrc/gemm_bf3a.hip (bf16x3 operands, the fallback when an activation leaves fp16's range), through their debug entry points.

- the split itself, bit for bit against a numpy model of the rounding and of the sign conventions (gemm_h2_common.h)
- every tile id x epilogue x fp32 / split output x accumulator-sign form (alt 0 / 1 / 2), at the edges of M, N and K, against an
  fp64 product: max and relative-rms gates, GELU' against the fp64 formula, and guard bands around every output (extra rows,
  ldc > N, sentinel bits) plus the engine's dense row layout (ldc2 == 2N), where a stray store lands in the next row
- both ring depths of gemm_h2 (2: more than CUs / 2 tiles, 4: fewer; 3 in a child process with AIMNET_H2_DEEP=3)
- the accumulation bias that the two interleaved accumulator sets cancel
- negative controls: corrupted operands must be rejected by the same gates."""
from __future__ import annotations

import os
import subprocess
import sys

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

TILES = [0, 452, 432, 422, 223, 224, 234, 851]
TILE_TM = {452: 160, 432: 96, 422: 64, 223: 128, 224: 128, 234: 192, 851: 80}  # block tile rows (gemm_split.h kSplitCands)
MAX_ERR, RMS_REL = 5e-5, 1e-6  # the gate of the exact-fp32 / bf16x3 siblings (test_gpu_ops.py); relative rms of mean |z|
SENT16 = 0x7E5B  # sentinel of the guard bands (a NaN as fp16, an odd bit pattern in every other reading)
SENT32 = 0x7FC0DEAD


def pad32(n):
    return (n + 31) // 32 * 32


def _lib():
    from aimnetcentral_amd import _lib

    return _lib.load(), _lib


def _stream():
    return torch.cuda.current_stream(torch.device("cuda:0")).cuda_stream


# ---- split helpers (layouts of include/aimnet_hip.h) ----------------------------------------------------------------------
def split2(x, mode):
    """h2 split of fp32 x [m][k] (mode 0 plain, 1 activation, 2 weight) -> int16 [m][2 pad32(k)]"""
    lib, L = _lib()
    m, k = x.shape
    out = torch.empty(m, 2 * pad32(k), dtype=torch.int16, device=x.device)
    assert lib.aimnet_debug_split_h2(x.data_ptr(), k, m, k, out.data_ptr(), 2 * pad32(k), mode, _stream()) == 0, L.last_error()
    return out


def split3(x, neg=1 << 30):
    """bf3 split of fp32 x [m][k]; k-blocks from `neg` on negated, -2: every odd block -> int16 [m][3 pad32(k)]"""
    lib, L = _lib()
    m, k = x.shape
    out = torch.empty(m, 3 * pad32(k), dtype=torch.int16, device=x.device)
    assert lib.aimnet_debug_split_bf3(x.data_ptr(), k, m, k, out.data_ptr(), 3 * pad32(k), neg, _stream()) == 0, L.last_error()
    return out


def unsplit2(c2, n):
    """h2 activation form (lo of odd k-blocks negated) -> fp64 [m][n]"""
    m = c2.shape[0]
    v = c2.reshape(m, -1)[:, : 2 * pad32(n)].reshape(m, pad32(n) // 32, 2, 32).view(torch.float16).double()
    sign = torch.where(torch.arange(pad32(n) // 32, device=c2.device) % 2 == 1, -1.0, 1.0).double().view(1, -1, 1)
    return (v[:, :, 0] + sign * v[:, :, 1] / 4096.0).reshape(m, pad32(n))[:, :n]


def unsplit3(c3, n):
    """bf3 form (planes sum to the value) -> fp64 [m][n]"""
    m = c3.shape[0]
    v = c3.reshape(m, -1)[:, : 3 * pad32(n)].reshape(m, pad32(n) // 32, 3, 32).to(torch.int32) << 16
    return v.view(torch.float32).double().sum(dim=2).reshape(m, pad32(n))[:, :n]


def h2_model(x: np.ndarray, mode: int):
    """numpy model of the h2 split: hi = fp16_rne(x), lo = fp16_rne((x - hi) * +-4096) in fp32; mode 1 negates the scale of
    the odd k-blocks, mode 2 flips the sign bit of hi in the odd k-blocks (zeros included).  -> (hi, lo) uint16 [m][pad32(k)]"""
    m, k = x.shape
    xp = np.zeros((m, pad32(k)), np.float32)
    xp[:, :k] = x
    odd = (np.arange(pad32(k)) // 32) % 2 == 1
    hi = xp.astype(np.float16)
    sc = np.where(odd & (mode == 1), np.float32(-4096.0), np.float32(4096.0)).astype(np.float32)
    with np.errstate(over="ignore"):
        lo = ((xp - hi.astype(np.float32)) * sc).astype(np.float32).astype(np.float16)
    hb = hi.view(np.uint16).copy()
    if mode == 2:
        hb[:, odd] ^= 0x8000
    return hb, lo.view(np.uint16)


def _planes2(s2, k):
    m = s2.shape[0]
    v = s2.cpu().numpy().view(np.uint16).reshape(m, pad32(k) // 32, 2, 32)
    return v[:, :, 0, :].reshape(m, -1), v[:, :, 1, :].reshape(m, -1)


# ---- 1. split exactness ------------------------------------------------------------------------------------------------------
def _split_inputs(m, k, seed):
    g = torch.Generator().manual_seed(seed)
    mag = torch.logspace(-6, np.log10(6e4), k, dtype=torch.float64)[torch.randperm(k, generator=g)]
    x = (torch.randn(m, k, generator=g, dtype=torch.float64).sign() * mag * torch.rand(m, k, generator=g, dtype=torch.float64).add(0.5))
    x = x.clamp(-65000, 65000).float()
    x[0, :6] = torch.tensor([0.0, -0.0, 1.0, -1.0, 65504.0, -6e-8])
    x[1, 32:38] = torch.tensor([0.0, -0.0, 2.0**-14, 2.0**-24, 1 + 2.0**-11, 1 + 2.0**-11 + 2.0**-23])  # (an odd k-block)
    return x


@pytest.mark.parametrize("mode", [0, 1, 2])
def test_h2_split_is_the_rne_model(mode):
    """aimnet_debug_split_h2 == the numpy model bit for bit in every sign mode; the pad columns of the last block are zero in
    both planes; and hi + lo / 4096 holds x to 2^-23 |x| where lo is a normal fp16 number and fits (|x| in [2^-13, 32768))."""
    m, k = 67, 733
    x = _split_inputs(m, k, 11 + mode)
    s2 = split2(x.cuda(), mode)
    torch.cuda.synchronize()
    hi, lo = _planes2(s2, k)
    mhi, mlo = h2_model(x.numpy(), mode)
    bad = np.argwhere((hi != mhi) | (lo != mlo))
    assert bad.size == 0, f"{len(bad)} elements differ from the model, first (row, col) {bad[:4].tolist()}"
    # pad columns 733..735 (block 22, even): zero bits in both planes
    assert not hi[:, k:].any() and not lo[:, k:].any()
    # accuracy of the pair (signs undone)
    odd = (np.arange(pad32(k)) // 32) % 2 == 1
    h = hi.view(np.float16).astype(np.float64)
    lv = lo.view(np.float16).astype(np.float64) / 4096.0
    if mode == 1:
        lv[:, odd] *= -1
    if mode == 2:
        h[:, odd] *= -1
    xv = x.double().numpy()
    err = np.abs(xv - (h + lv)[:, :k])
    sel = (np.abs(xv) >= 2.0**-13) & (np.abs(xv) < 32768)
    assert sel.sum() > 10000
    assert (err[sel] <= 2.0**-23 * np.abs(xv[sel])).all(), float((err[sel] / np.abs(xv[sel])).max() / 2.0**-24)
    # below 2^-13 hi / lo underflow gradually: absolute error of lo's subnormal spacing
    tiny = np.abs(xv) < 2.0**-13
    assert (err[tiny] <= 2.0**-37).all()


def test_h2_split_bound_is_tight():
    """The pair's error reaches 2^-23 |x| (not 2^-24: |x - hi| <= 2^-11 |x| leaves 13 significant bits for the 11 of lo), and
    the scaled residual of |x| >= 32768 can round to inf - the reason the range check stops there (gemm_h2_common.h)."""
    x = np.array([[1 + 2.0**-11 + 2.0**-23, 32784.0, 32767.0, 32768.0 + 15.0]], np.float32)
    hi, lo = h2_model(x, 0)
    s2 = split2(torch.from_numpy(np.ascontiguousarray(x)).cuda(), 0)
    torch.cuda.synchronize()
    ghi, glo = _planes2(s2, x.shape[1])
    assert (ghi[:, :4] == hi[:, :4]).all() and (glo[:, :4] == lo[:, :4]).all()
    v = ghi[0, :4].view(np.float16).astype(np.float64) + glo[0, :4].view(np.float16).astype(np.float64) / 4096
    assert abs(v[0] - float(x[0, 0])) == pytest.approx(2.0**-23, rel=1e-6)
    assert np.isinf(glo[0, 1:2].view(np.float16)).all()  # 32784 = 32768 + 16: hi 32768, residual 16 * 4096 = 65536
    assert np.isfinite(glo[0, [0, 2, 3]].view(np.float16)).all()


def test_bf3_split_odd_blocks_negated_is_exact():
    """neg_from_block = -2 (the form of gemm_bf3a.hip's alt = 1 weights): every odd k-block negated, the planes still sum to x
    exactly and plane 0 is the round-to-nearest-even bf16 of x."""
    m, k = 65, 733
    x = _split_inputs(m, k, 99)
    s3 = split3(x.cuda(), -2)
    torch.cuda.synchronize()
    planes = (s3.view(m, pad32(k) // 32, 3, 32).to(torch.int32) << 16).view(torch.float32).cpu()
    sign = torch.where(torch.arange(pad32(k) // 32) % 2 == 1, -1.0, 1.0).double().view(1, -1, 1)
    val = (planes.double().sum(dim=2) * sign).reshape(m, pad32(k))
    assert torch.equal(val[:, :k], x.double())
    assert torch.equal(val[:, k:], torch.zeros(m, pad32(k) - k, dtype=torch.float64))
    p0 = (planes[:, :, 0, :].double() * sign).reshape(m, pad32(k))[:, :k]
    assert torch.equal(p0, x.to(torch.bfloat16).double())


# ---- 2. tile-by-tile fp64 tests ---------------------------------------------------------------------------------------------
class Operands:
    """A [mmax][K], Bt [N][K] and bias in every form a launch can take, their fp64 product computed once"""

    def __init__(self, mmax, N, K, seed, pos=False):
        g = torch.Generator().manual_seed(seed)
        dev = torch.device("cuda:0")
        if pos:
            A, Bt = torch.rand(mmax, K, generator=g), torch.rand(N, K, generator=g) * 0.05
        else:
            A, Bt = torch.randn(mmax, K, generator=g), torch.randn(N, K, generator=g) * 0.1
        self.N, self.K = N, K
        self.A, self.Bt = A.to(dev), Bt.to(dev)
        self.bias = torch.randn(N, generator=g).to(dev)
        self.Dm = torch.rand(mmax, N, generator=g).to(dev)  # the epilogue-3 input
        self.z = self.A.double() @ self.Bt.double().T
        # one k-block wider, junk in front: the alt = 2 form (operand starting on an odd k-block, as mlp_gemm3 with k0)
        junk = lambda r: torch.randn(r, 32, generator=g).to(dev) * 7.0  # noqa: E731
        self.Aw, self.Bw = torch.cat([junk(mmax), self.A], 1), torch.cat([junk(N), self.Bt], 1)
        self._cache = {}

    def forms(self, kern, alt, wrong=False, drop_lo=False):
        """(A ptr tensor, lda, Bt tensor, ldb, element offset of the first block) for alt 0 / 1 / 2; wrong: weights in the
        plain form whatever alt says (sign error on odd k-blocks); drop_lo: the lo / minor planes zeroed"""
        key = (kern, alt, wrong, drop_lo)
        if key not in self._cache:
            w = 2 if kern == "h2" else 3
            A, B = (self.Aw, self.Bw) if alt == 2 else (self.A, self.Bt)
            if kern == "h2":
                a = split2(A, 0 if alt == 0 else 1)
                b = split2(B, 0 if (alt == 0 or wrong) else 2)
            else:
                a = split3(A)
                b = split3(B, 1 << 30 if (alt == 0 or wrong) else -2)
            if drop_lo:
                for t in (a, b):
                    t.view(t.shape[0], -1, w, 32)[:, :, 1:, :] = 0
            off = 32 * w if alt == 2 else 0
            self._cache[key] = (a, a.shape[1], b, b.shape[1], off)
        return self._cache[key]

    def want(self, M, epi):
        z = self.z[:M]
        if epi == 0:
            return z, None
        zb = z + self.bias.double()
        if epi == 1:
            return zb, None
        if epi == 2:
            cdf = 0.5 * (1 + torch.erf(zb / 2**0.5))
            return zb * cdf, cdf + zb * torch.exp(-0.5 * zb * zb) / (2 * torch.pi) ** 0.5
        return z * self.Dm[:M].double(), None


def run_gemm(kern, ops: Operands, cfg, epi, out, M, alt, dense=False, **form_kw):
    """One launch into sentinel-filled buffers with guard rows and ldc > N.  -> (result fp64 [M][N], D, guard violations)
    dense: the split output with ldc2 == 2N / ldc3 == 3N (the engine's layout; guard rows below only)."""
    lib, L = _lib()
    dev = torch.device("cuda:0")
    N, K = ops.N, ops.K
    w = 2 if kern == "h2" else 3
    GR = 3  # guard rows
    ldc = N + 12  # (N % 4 == 0: rows stay 16-byte aligned)
    C = torch.full((M + GR, ldc), SENT32, dtype=torch.int32, device=dev)
    D = torch.full((M + GR, ldc), SENT32, dtype=torch.int32, device=dev)
    if epi == 3:
        D[:M, :N] = ops.Dm[:M].view(torch.int32)
    ldo = w * N if dense else w * pad32(N) + 32 * w * 2
    C2 = torch.full((M + GR, ldo), SENT16, dtype=torch.int16, device=dev)
    D0, C20, C0 = D.clone(), C2.clone(), C.clone()
    a, lda, b, ldb, off = ops.forms(kern, alt, **form_kw)
    fn = lib.aimnet_debug_gemm_h2 if kern == "h2" else lib.aimnet_debug_gemm_bf3a
    rc = fn(cfg, epi, int(out), a.data_ptr() + 2 * off, lda, b.data_ptr() + 2 * off, ldb, M, N, K, ops.bias.data_ptr(),
            C.data_ptr(), C2.data_ptr(), ldo, D.data_ptr(), ldc, alt, _stream())
    assert rc == 0, L.last_error()
    torch.cuda.synchronize()
    viol = []
    inside = torch.zeros(M + GR, ldc, dtype=torch.bool, device=dev)
    inside[:M, :N] = True
    if out:
        ins2 = torch.zeros(M + GR, ldo, dtype=torch.bool, device=dev)
        ins2[:M, : w * N] = True
        if (C2 != C20)[~ins2].any():
            r, c = torch.nonzero((C2 != C20) & ~ins2)[0].tolist()
            viol.append(f"split output written outside [M, N] ({int(((C2 != C20) & ~ins2).sum())} elements, first row {r} col {c})")
        res = (unsplit2 if kern == "h2" else unsplit3)(C2[:M], N)
        if not torch.equal(C, C0):
            viol.append("fp32 C written in split-output mode")
    else:
        if (C != C0)[~inside].any():
            viol.append(f"C written outside [M, N] ({int(((C != C0) & ~inside).sum())} elements)")
        res = C[:M, :N].view(torch.float32).double()
    if epi == 2:
        if (D != D0)[~inside].any():
            viol.append("D written outside [M, N]")
    elif not torch.equal(D, D0):
        viol.append(f"D changed by epilogue {epi}")  # epilogue 3: an input, bitwise unchanged; 0 / 1: untouched
    return res, D[:M, :N].view(torch.float32).double(), viol


def gate(res, ref):
    """(max |err|, rms err / mean |ref|)"""
    d = res - ref
    return d.abs().max().item(), d.pow(2).mean().sqrt().item() / max(ref.abs().mean().item(), 1e-30)


def check_case(kern, ops, cfg, epi, out, M, alt, dense=False):
    res, D, viol = run_gemm(kern, ops, cfg, epi, out, M, alt, dense)
    tag = f"{kern} tile {cfg} epi {epi} out {int(out)} M {M} N {ops.N} K {ops.K} alt {alt}{' ldc2=2N' if dense else ''}"
    assert not viol, f"{tag}: {viol}"
    want, want_d = ops.want(M, epi)
    mx, rms = gate(res, want)
    assert torch.isfinite(res).all() and mx < MAX_ERR and rms < RMS_REL, f"{tag}: max {mx:.2e} rms {rms:.2e}"
    if want_d is not None:
        dd = (D - want_d).abs().max().item()
        assert dd < MAX_ERR, f"{tag}: GELU' max {dd:.2e}"
    return mx, rms


# (N, K) with the tile-pair edge N % 96 == 64 next to the layer widths; N = 100: fp32 output only (split output needs N % 32 == 0)
NK = [(64, 32), (160, 736), (128, 96), (384, 64), (512, 736), (100, 96)]


def _ms(cfg):
    tm = TILE_TM.get(cfg, 160)
    return [1, 17, tm, tm + 1, 2500]


def _tile_sweep(kern, N, K, seed, tiles=TILES, alts=(0, 1, 2)):
    ops = Operands(2500, N, K, seed)
    worst = [0.0, 0.0]
    for cfg in tiles:
        for M in _ms(cfg):
            for alt in alts:
                for epi, out in ((0, False), (1, False), (2, False), (3, False), (2, True), (3, True)):
                    if out and N % 32:
                        continue
                    mx, rms = check_case(kern, ops, cfg, epi, out, M, alt)
                    worst = [max(worst[0], mx), max(worst[1], rms)]
                if N % 32 == 0:  # the engine's dense split-output rows: a stray store lands in the next row
                    for epi in (2, 3):
                        check_case(kern, ops, cfg, epi, True, M, alt, dense=True)
    return worst


@pytest.mark.parametrize("N,K", NK)
@pytest.mark.parametrize("kern", ["h2", "bf3a"])
def test_split_gemm_tiles_match_fp64(kern, N, K):
    """every tile x epilogue x output form x alt at M = 1, 17, one tile, one tile + 1, 2 500 (ring depth 4 on gemm_h2)"""
    mx, rms = _tile_sweep(kern, N, K, seed=N * 7 + K)
    print(f"{kern} N={N} K={K}: worst max {mx:.2e} rms {rms:.2e}")


@pytest.mark.parametrize("kern", ["h2", "bf3a"])
def test_split_gemm_tiles_large_grid(kern):
    """M = 10 080, N = 512, K = 736: more than CUs / 2 tiles for every tile id (gemm_h2 ring depth 2)"""
    ops = Operands(10080, 512, 736, seed=10080)
    for cfg in TILES:
        check_case(kern, ops, cfg, 0, False, 10080, 1)
        check_case(kern, ops, cfg, 2, True, 10080, 1, dense=True)
        check_case(kern, ops, cfg, 3, True, 10080, 2)


def _depth3_main():
    """child-process body of test_h2_ring_depth_3 (AIMNET_H2_DEEP is read once per process)"""
    for N, K in ((160, 736), (64, 32), (512, 736)):
        _tile_sweep("h2", N, K, seed=3 * N + K, alts=(1, 2))
    print("DEPTH3_OK")


def test_h2_ring_depth_3():
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    code = ("import sys; sys.path[:0] = [%r, %r]; import test_gpu_split_gemm as t; t._depth3_main()"
            % (root, os.path.join(root, "tests")))
    env = dict(os.environ, AIMNET_H2_DEEP="3")
    r = subprocess.run([sys.executable, "-c", code], env=env, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0 and "DEPTH3_OK" in r.stdout, (r.returncode, r.stdout[-2000:], r.stderr[-4000:])


# ---- 3. accumulation bias ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kern", ["h2", "bf3a"])
def test_accumulation_bias_cancels(kern):
    """all-positive operands (a one-signed truncation of the matrix pipe would not average out): |mean err| / mean |z| of the
    engine form (alt = 1) <= 1.5e-8.  The plain-weight form (alt = 0, one accumulator sign) on the same data: bf3a -1.8e-8
    against -4.6e-9 with the two sets - the cancellation is asserted; h2 +6.1e-9 against +6.6e-9 - its fp16 hi x hi products
    carry no measurable truncation bias of their own, so only the absolute gate applies."""
    ops = Operands(10080, 512, 736, seed=77, pos=True)
    bias = {}
    for alt in (0, 1):
        res, _, viol = run_gemm(kern, ops, 0, 0, False, 10080, alt)
        assert not viol
        bias[alt] = (res - ops.z).mean().item() / ops.z.abs().mean().item()
    print(f"{kern}: relative mean error alt 0 {bias[0]:+.2e}, alt 1 {bias[1]:+.2e}")
    assert abs(bias[1]) <= 1.5e-8, bias
    if kern == "bf3a":
        assert abs(bias[1]) < 0.5 * abs(bias[0]), bias


# ---- 4. negative controls: the gates above reject corrupted operands ---------------------------------------------------------
@pytest.mark.parametrize("kern", ["h2", "bf3a"])
def test_gates_reject_dropped_lo_planes(kern):
    """lo planes zeroed (the cross terms dropped): the result is the fp16 / bf16 product, far outside the rms gate"""
    ops = Operands(2500, 512, 736, seed=5)
    for alt in (1, 2):
        res, _, viol = run_gemm(kern, ops, 0, 0, False, 2500, alt, drop_lo=True)
        assert not viol
        mx, rms = gate(res, ops.want(2500, 0)[0])
        assert rms > 10 * RMS_REL, (alt, mx, rms)


@pytest.mark.parametrize("kern", ["h2", "bf3a"])
def test_gates_reject_wrong_weight_signs(kern):
    """plain weights under alt = 1 / 2 (sign error on the odd k-blocks): fails the max gate"""
    ops = Operands(500, 160, 96, seed=6)
    for alt in (1, 2):
        res, _, viol = run_gemm(kern, ops, 0, 0, False, 500, alt, wrong=True)
        assert not viol
        mx, rms = gate(res, ops.want(500, 0)[0])
        assert mx > 1e3 * MAX_ERR, (alt, mx, rms)
