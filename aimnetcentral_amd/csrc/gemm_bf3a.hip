// gemm_bf3a.hip - the bf16x3-split MLP GEMM with PRE-SPLIT activations: both operands reach LDS by DMA, no vector work in the loop.
//
//   C[M,N] = A[M,K] . Bt[N,K]^T, fused epilogues: the contract of gemm_bf3.hip (which replaces the torch addmm + GELU calls of
//   aimnet/modules/core.py:11-46), except that A is handed over in the "bf3" layout (per row, K/32 blocks of
//   [plane 0: 32 bf16][plane 1][plane 2] = 192 B; fp32 == p0 + p1 + p2 exactly) and that the epilogue can write C in the same
//   layout for the next layer (OUT3).  The products are those of gemm_bf3.hip; the accumulation runs in two interleaved sets
//   (even / odd k-steps, weights of the odd k-blocks negated) whose difference cancels the truncation bias of the matrix pipe.
//
// Why (profiles/r3_gemm_bf3.md, r4_gemm.md): with fp32 activations every block splits its row panel itself - 75 vector
// instructions and 9 LDS stores per wave and 32-k step, four times per panel (once per column tile) - and that work does not
// hide behind the partner wave's matrix instructions: a step took 3 300 - 3 600 cycles against 2 200 of matrix work.  Here the
// PRODUCER of an activation (the previous layer's epilogue, the convolution's row assembly) splits it once, and the main loop
// is fragment reads, DMA issue and matrix instructions only.
//
// Kernel body, schedule, launcher and tile choice are those of gemm_split.h, shared with gemm_h2.hip, and so is what the bf16x3
// form decides on the device (Bf3Operand, shared with gemm_head.hip); this file holds the launcher's choices (Bf3Fmt) and the
// entry points.
#include "gemm_split.h"

namespace aimnet {

// the entry points: the body of gemm_split.h over Bf3Fmt (below)
template <int EPI, int SM, int SN, int WN, bool OUT3>
__global__ __launch_bounds__(512, 2) void gemm_bf3a_kernel(const unsigned short* __restrict__ A3, int lda3,
                                                           const unsigned short* __restrict__ Bt, int ldb, int M, int N, int K,
                                                           const float* __restrict__ bias, float* __restrict__ C,
                                                           unsigned short* __restrict__ C3, int ldc3, float* __restrict__ D, int ldc,
                                                           const int* __restrict__ brow, int ldbias, int alt) {
  gemm_split_body<Bf3Fmt, EPI, SM, SN, WN, OUT3, 2>(A3, lda3, Bt, ldb, M, N, K, bias, C, C3, ldc3, D, ldc, brow, ldbias, alt);
}

struct Bf3Fmt : Bf3Operand {
  static constexpr const char* NAME = "gemm_bf3a";
  static constexpr int MAX_NSA = 2;            // activation ring depths 2 .. MAX_NSA: the 452 tile has no LDS for more
  static constexpr int nsb(int) { return 3; }  // weight ring depth
  static int ring_depth(int) { return 2; }
  template <int EPI, int SM, int SN, int WN, bool OUT3, int NSA>
  static constexpr auto kernel() { return &gemm_bf3a_kernel<EPI, SM, SN, WN, OUT3>; }
};

template int launch_split_cfg<Bf3Fmt>(hipStream_t stream, int cfg, int epi, bool out, const SplitArgs& a);

}  // namespace aimnet
