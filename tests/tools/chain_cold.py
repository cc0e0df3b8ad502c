#!/usr/bin/env python
"""The six one-launch MLP sweeps of the default path (csrc/gemm_chain.hip) timed in isolation with their operands HOT and COLD.

tests/tools/chain_sweep.py repeats one launch back to back: weights, input rows and GELU' are cache-resident there, while in a
step ~2.5 GB pass through the 4 MiB L2s and the 256 MiB Infinity Cache between two uses of a chain's weights.  This tool times
single launches (HIP events around one aimnet_engine_debug_mlp_sweep call, median of REPS) in three states:

  hot           back to back
  all cold      before every timed launch a scratch buffer of EVICT_MIB (>= 512) MiB is read and written
  weights cold  the same eviction, then a plain reduction over the sweep's input rows and (backward) its GELU' buffers brings
                those back on-die: what is still cold is the weight stream (and the lines the sweep writes)

for engine option chain_prefetch = 0 and 1.  Of the gap hot -> all cold, "weights cold" shows what the weights cause; the rest
belongs to the block-private operands.  Prints a markdown table (profiles/r7_chain_cold.md).

Env: M (rows, default 10080), REPS (default 25), EVICT_MIB (default 768), PREFETCH ("0,1"; "-1": leave the option alone - a library
without it, through AIMNET_HIP_LIB)."""
import ctypes as C
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", ".."))
from aimnetcentral_amd import _lib, loader  # noqa: E402
from aimnetcentral_amd.engine import HipEngine  # noqa: E402

M = int(os.environ.get("M", 10080))
REPS = max(20, int(os.environ.get("REPS", 25)))
EVICT_MIB = max(512, int(os.environ.get("EVICT_MIB", 768)))
PREFETCH = [int(v) for v in os.environ.get("PREFETCH", "0,1").split(",")]
LAYER_DIMS = [[704, 512, 380, 258], [733, 512, 380, 258], [733, 512, 380, 380, 256]]  # synthetic_spec(0)

eng = HipEngine(loader.synthetic_spec(0), "cuda:0")
lib, dev = eng.lib, eng.device
stream = torch.cuda.current_stream(dev).cuda_stream
scratch = torch.zeros(EVICT_MIB * (1 << 20) // 4, dtype=torch.float32, device=dev)
head_fused = eng.get_option("head_fused") != 0


def pad32(n):
    return (n + 31) // 32 * 32


def split2(x):
    m, k = x.shape
    out = torch.zeros(m, 2 * pad32(k), dtype=torch.int16, device=dev)
    assert lib.aimnet_debug_split_h2(x.data_ptr(), k, m, k, out.data_ptr(), 2 * pad32(k), 1, stream) == 0, _lib.last_error()
    return out


def ptrs(ts):
    return (C.c_void_p * len(ts))(*[t.data_ptr() if t is not None else None for t in ts])


def evict():
    scratch.add_(1.0)  # reads and writes every line of the buffer


def touch(ts):
    for t in ts:
        t.view(-1).view(torch.int32).sum()  # a plain reduction: the rows come back on-die


def time_one(launch, before):
    ts = []
    for _ in range(REPS):
        before()
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        launch()
        e1.record()
        e1.synchronize()
        ts.append(e0.elapsed_time(e1) * 1e3)
    return statistics.median(ts)


def sweeps():
    """(name, launch, refill, operands to bring back for "weights cold") of the six sweeps of the default path"""
    numbers = torch.tensor([1, 6, 7, 8], dtype=torch.int32, device=dev)[torch.randint(0, 4, (M,), device=dev)]
    out = []
    for p in (0, 1, 2):
        d = LAYER_DIMS[p]
        nl, kp = len(d) - 1, [pad32(v) for v in d]
        torch.manual_seed(p)
        x2 = split2(torch.randn(M, d[0], device=dev))
        H = [torch.zeros(M, kp[l + 1], device=dev) for l in range(nl)]
        D = [torch.zeros(M, kp[l + 1], device=dev) for l in range(nl)]
        split_last = 1 if (p == 2 and head_fused) else 0  # the fused energy head reads the last output in split form

        def fwd(p=p, x2=x2, H=H, D=D, split_last=split_last):
            rc = lib.aimnet_engine_debug_mlp_sweep(eng._h, p, 0, 1, split_last, x2.data_ptr(), M, numbers.data_ptr(), ptrs(H), ptrs(D), None, None, stream)
            assert rc == 0, _lib.last_error()

        fwd()  # GELU' for the backward sweep
        out.append((f"pass {p} forward", fwd, lambda: None, [x2]))
        zbar2 = split2(torch.randn(M, d[nl], device=dev))
        zb = [torch.zeros(M * 2 * max(kp), dtype=torch.int16, device=dev) for _ in range(2)]
        which = C.c_int(-1)
        conv_only = 1 if p == 0 else 0  # the default path forms only the conv columns of pass 0's input adjoint

        def refill(zb=zb, zbar2=zbar2, n=M * 2 * kp[nl]):
            zb[0][:n] = zbar2.view(-1)

        def bwd(p=p, zb=zb, D=D, which=which, conv_only=conv_only):
            rc = lib.aimnet_engine_debug_mlp_sweep(eng._h, p, 1, 1, conv_only, zb[0].data_ptr(), M, numbers.data_ptr(), None, ptrs(D), ptrs(zb), C.byref(which), stream)
            assert rc == 0, _lib.last_error()

        gelu_grads = [D[l] for l in range(nl - 1)]  # GELU' of the hidden layers: what the backward sweep reads
        out.append((f"pass {p} backward" + (" (conv columns)" if conv_only else ""), bwd, refill, [zb[0][: M * 2 * kp[nl]]] + gelu_grads))
    return out


def main():
    table = {}
    sw = sweeps()
    for pf in PREFETCH:
        if pf >= 0:
            eng.set_option("chain_prefetch", pf)
        for name, launch, refill, operands in sw:
            refill()
            launch()
            torch.cuda.synchronize()

            def cold():
                refill()
                evict()

            def weights_cold():
                refill()
                evict()
                touch(operands)

            table[(pf, name)] = (time_one(launch, refill), time_one(launch, cold), time_one(launch, weights_cold))
    print(f"M = {M}, median of {REPS} single launches, eviction buffer {EVICT_MIB} MiB, library {_lib.LIB_PATH}")
    for pf in PREFETCH:
        print(f"\nchain_prefetch = {pf if pf >= 0 else '(option not set)'}\n")
        print("| sweep | hot us | all cold us | weights cold us | gap | of it weights |")
        print("|---|---|---|---|---|---|")
        tot = [0.0, 0.0, 0.0]
        for name, *_ in sw:
            h, c, w = table[(pf, name)]
            tot = [tot[0] + h, tot[1] + c, tot[2] + w]
            print(f"| {name} | {h:.1f} | {c:.1f} | {w:.1f} | {c - h:.1f} | {w - h:.1f} |")
        print(f"| sum | {tot[0]:.1f} | {tot[1]:.1f} | {tot[2]:.1f} | {tot[1] - tot[0]:.1f} | {tot[2] - tot[0]:.1f} |")


if __name__ == "__main__":
    main()
