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
// Kernel body, schedule, launcher and tile choice are those of gemm_split.h, shared with gemm_h2.hip; this file holds what the
// bf16x3 form decides (Bf3Fmt) and its entry points.
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

struct Bf3Fmt {
  using frag = bf16x8;
  static constexpr const char* NAME = "gemm_bf3a";
  static constexpr int FMT = SPLIT_BF3, PLANES = split_planes(FMT);
  static constexpr int NACC = 2;         // accumulator sets
  static constexpr int ROW_BYTES = ROWB;  // per row and 32-k step, in memory and in LDS
  static constexpr int MAX_NSA = 2;      // activation ring depths 2 .. MAX_NSA: the 452 tile has no LDS for more
  static constexpr int passes(int rows) { return (rows * 12 + 255) / 256; }  // DMA wave-instructions per wave of the issuing group
  static constexpr int nsb(int) { return 3; }                                // weight ring depth
  static int ring_depth(int) { return 2; }
  template <int EPI, int SM, int SN, int WN, bool OUT3, int NSA>
  static constexpr auto kernel() { return &gemm_bf3a_kernel<EPI, SM, SN, WN, OUT3>; }

  // DMA granules of the issuing group: G = p * 256 + t256 -> row G / 12, plane (G % 12) / 4, slot G % 4 holding k-chunk
  // slot ^ swz(row); granules beyond the tile (padding of the last pass) re-read the last one into the stage's padding.
  static __device__ __forceinline__ unsigned goff(int p, int w4, int lane, int tile_rows, int r0, int rlim, unsigned ldbytes) {
    const int G = min(p * 256 + w4 * 64 + lane, tile_rows * 12 - 1);
    const int row = G / 12, g12 = G % 12;
    const int pl = g12 >> 2, kcx = (g12 & 3) ^ swz192(row);
    return (unsigned)(min(r0 + row, rlim) - r0) * ldbytes + pl * 64 + kcx * 16;
  }
  // fragment addresses: row r, plane P, k-chunk c = lane >> 4 -> r * 192 + P * 64 + (c ^ swz(r)) * 16
  static __device__ __forceinline__ unsigned frag_addr(int row0, int l16, int lc) {
    const int r = row0 + l16;
    return r * ROWB + ((lc ^ swz192(r)) << 4);
  }
  template <int SM, int SN>
  static __device__ __forceinline__ void load_frags(frag (&fa)[SM][3], frag (&fb)[SN][3], unsigned oa, unsigned ob) {
    read_strips<0, SN, 0>(fb, ob);
    read_strips<0, SM, 0>(fa, oa);
    read_strips<0, SN, 1>(fb, ob);
    read_strips<0, SM, 1>(fa, oa);
    read_strips<0, SN, 2>(fb, ob);
    read_strips<0, SM, 2>(fa, oa);
  }

  // Accumulation.  v_mfma_f32_16x16x32_bf16 aligns its 32 products and the accumulator in a fixed-point adder and TRUNCATES what
  // falls below - towards minus infinity, ~2^-7.5 ulp per instruction, one-signed: -4.7e-8 |z| on every output of a K = 736 layer
  // (tests/tools/bf3_bias.py), which does not average out over atoms (config 5's energies moved by twice the fp32 noise).  Round 3
  // cancelled it with a sign-flipped second phase whose start (0.56 K) had to be fitted to the growth of |acc| over k - a property of
  // the data.  Here the weights of every ODD k-block are stored negated (BF3_ALT) and even / odd k-steps accumulate into two
  // accumulator sets; the epilogue takes their difference.  Both sets see interleaved halves of the same sum - the same magnitude
  // profile whatever the data - and both are truncated downwards, so the biases cancel in the difference: no tunable.
  static __device__ __forceinline__ f32x4 mfma(frag b, frag a, f32x4 c) { return __builtin_amdgcn_mfma_f32_16x16x32_bf16(b, a, c, 0, 0, 0); }
  template <int PAR, int SM, int SN>  // PAR: parity of the k-step
  static __device__ __forceinline__ void products(f32x4 (&acc)[2][SM][SN], const frag (&fa)[SM][3], const frag (&fb)[SN][3]) {
    split_product<Bf3Fmt, PAR, 1, 1>(acc, fa, fb);
    split_product<Bf3Fmt, PAR, 0, 1>(acc, fa, fb);
    split_product<Bf3Fmt, PAR, 1, 0>(acc, fa, fb);
    split_product<Bf3Fmt, PAR, 0, 2>(acc, fa, fb);
    split_product<Bf3Fmt, PAR, 2, 0>(acc, fa, fb);
    split_product<Bf3Fmt, PAR, 0, 0>(acc, fa, fb);
  }
  template <int SM, int SN>
  static __device__ __forceinline__ f32x4 total(const f32x4 (&acc)[2][SM][SN], int i, int j, float s0, float s1) {
    return acc[0][i][j] * s0 + acc[1][i][j] * s1;
  }
};

template int launch_split_cfg<Bf3Fmt>(hipStream_t stream, int cfg, int epi, bool out, const SplitArgs& a);

}  // namespace aimnet
