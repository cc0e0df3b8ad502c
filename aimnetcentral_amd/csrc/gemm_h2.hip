// gemm_h2.hip - the MLP GEMM on fp16x2-split operands ("h2", gemm_h2_common.h): three matrix instructions per tile and k-step
// instead of the six of the bf16x3 split, 4 instead of 6 bytes per operand element.
//
//   C[M,N] = A[M,K] . Bt[N,K]^T, fused epilogues: the contract of gemm_bf3a.hip (which replaces the torch addmm + GELU calls of
//   aimnet/modules/core.py:11-46); A and Bt are handed over in the h2 layout (per row, K/32 blocks of [hi: 32 fp16][lo: 32 fp16]
//   = 128 B, fp32 == hi + lo / 4096 to 2^-24) and the epilogue can write C in the same layout for the next layer (OUT2).
//   Products per tile and k-step: ah bh into one of two interleaved accumulator sets (even / odd k-steps, the weights' hi planes
//   of the odd k-blocks negated: the one-signed truncation of the matrix pipe cancels in the difference, as in gemm_bf3a.hip),
//   ah bl and al bh into a third set that the epilogue scales by 1 / 4096.
//
// Kernel body, schedule (the ping-pong of two wave groups), launcher and tile choice are those of gemm_split.h, shared with
// gemm_bf3a.hip, and so is what the fp16x2 form decides on the device (H2Operand, shared with gemm_head.hip); this file holds the
// launcher's choices (H2Fmt), the entry points and the format dispatch of both.
// LDS tiles: 16-row strips of [hi 1 KiB][lo 1 KiB] (gemm_h2_common.h), one DMA wave-instruction per plane of a strip.
#include <math.h>
#include <stdlib.h>
#include <string.h>

#include <algorithm>

#include "gemm_split.h"

namespace aimnet {

static int g_h2_deep = 4;  // AIMNET_H2_DEEP: ring depth (2, 3 or 4) of launches that fill at most half of the CUs

// the entry points: the body of gemm_split.h over H2Fmt (below)
template <int EPI, int SM, int SN, int WN, bool OUT3, int NSA>
__global__ __launch_bounds__(512, 2) void gemm_h2_kernel(const unsigned short* __restrict__ A3, int lda3,
                                                           const unsigned short* __restrict__ Bt, int ldb, int M, int N, int K,
                                                           const float* __restrict__ bias, float* __restrict__ C,
                                                           unsigned short* __restrict__ C3, int ldc3, float* __restrict__ D, int ldc,
                                                           const int* __restrict__ brow, int ldbias, int alt) {
  gemm_split_body<H2Fmt, EPI, SM, SN, WN, OUT3, NSA>(A3, lda3, Bt, ldb, M, N, K, bias, C, C3, ldc3, D, ldc, brow, ldbias, alt);
}

struct H2Fmt : H2Operand {
  static constexpr const char* NAME = "gemm_h2";
  // Ring depth.  NSA = activation ring depth (weights: nsb).  2: the activation tile is requested ONE step ahead (weights: two).
  // 3: two steps ahead as well; 4: both three steps ahead -
  // for launches that leave CUs idle (a few hundred to ~2 000 rows): there a step is as long as the request's latency whatever the
  // tile (~0.6 us; the GEMM family costs the same 0.25 ms from 384 to 2 304 atoms), and the second step of lead takes 8 % off it;
  // on full grids the extra 20 KB of LDS cost 0.6 % (profiles/r5_size_sweep.jsonl).
  static constexpr int MAX_NSA = 4;                                  // activation ring depths 2 .. MAX_NSA
  static constexpr int nsb(int NSA) { return NSA == 4 ? 4 : 3; }  // weight ring depth that goes with an activation ring depth
  static int ring_depth(int tiles) { return 2 * tiles <= device_cus() ? g_h2_deep : 2; }  // at most half of the CUs busy: longer request lead
  template <int EPI, int SM, int SN, int WN, bool OUT3, int NSA>
  static constexpr auto kernel() { return &gemm_h2_kernel<EPI, SM, SN, WN, OUT3, NSA>; }
};

// (A one-instruction-stream-per-wave schedule - fragments of step j+1 fetched into the registers step j's products release, one
// barrier per step - was built and measured EQUAL, step 1.3452 vs 1.3456 ms: 60 matrix instructions per SIMD and step at the
// 16x16x32 shape's own rate are 1 164 of the ~1 500 cycles either schedule takes; profiles/r5_gemm_h2.md.  Removed; commit d9e6536.)

template int launch_split_cfg<H2Fmt>(hipStream_t stream, int cfg, int epi, bool out, const SplitArgs& a);
extern template int launch_split_cfg<Bf3Fmt>(hipStream_t stream, int cfg, int epi, bool out, const SplitArgs& a);  // gemm_bf3a.hip

// ---- both formats: the one entry point of the callers
int launch_gemm_split_cfg(hipStream_t stream, int fmt, int cfg, int epi, bool out, const SplitArgs& a) {
  if (fmt == SPLIT_H2) return launch_split_cfg<H2Fmt>(stream, cfg, epi, out, a);
  if (fmt == SPLIT_BF3) return launch_split_cfg<Bf3Fmt>(stream, cfg, epi, out, a);
  set_last_error("gemm_split: no split operand format %d", fmt);
  return -1;
}

int gemm_split_set_attributes() {
  const char* env = getenv("AIMNET_BF3A_TILE");
  g_split_force_tile[SPLIT_BF3] = env ? atoi(env) : 0;
  env = getenv("AIMNET_H2_TILE");
  g_split_force_tile[SPLIT_H2] = env ? atoi(env) : 0;
  env = getenv("AIMNET_H2_DEEP");
  if (env) g_h2_deep = atoi(env) == 3 ? 3 : atoi(env) == 2 ? 2 : 4;
  return 0;
}


// ---- fp32 [M][ld] (K columns) -> h2 [M][Kp/32][2][32]; columns >= K of the last block are zero; mode: H2_PLAIN / H2_ACT / H2_WEIGHT
__global__ __launch_bounds__(256) void split_h2_kernel(const float* __restrict__ src, int ld, int M, int K, int Kp,
                                                       unsigned short* __restrict__ dst, int ldd, int mode, int* __restrict__ ovf) {
  const int q = Kp >> 2;  // column quads per row
  const size_t n = (size_t)M * q;
  for (size_t e = (size_t)blockIdx.x * blockDim.x + threadIdx.x; e < n; e += (size_t)gridDim.x * blockDim.x) {
    const int m = (int)(e / q), col = (int)(e % q) * 4;
    f32x4 v;
    const float* s = src + (size_t)m * ld + col;
    if (col + 3 < K && (((size_t)s) & 15) == 0) {
      v = *reinterpret_cast<const f32x4*>(s);
    } else {
#pragma unroll
      for (int r = 0; r < 4; ++r) v[r] = col + r < K ? s[r] : 0.0f;
    }
    h2_flag_overflow(ovf, h2_amax4(v));
    const bool odd = (col & 32) != 0;
    unsigned h0, l0, h1, l1;
    const float sc = (mode == H2_ACT && odd) ? -H2_SCALE : H2_SCALE;
    split2_pair(v[0], v[1], sc, h0, l0);
    split2_pair(v[2], v[3], sc, h1, l1);
    if (mode == H2_WEIGHT && odd) {
      h0 ^= 0x80008000u;
      h1 ^= 0x80008000u;
    }
    unsigned short* p = dst + (size_t)m * ldd + (col >> 5) * 64 + (col & 31);
    *reinterpret_cast<u32x2*>(p) = u32x2{h0, h1};
    *reinterpret_cast<u32x2*>(p + 32) = u32x2{l0, l1};
  }
}

int launch_split_h2(hipStream_t s, const float* src, int ld, int M, int K, unsigned short* dst, int ldd, int mode, int* ovf) {
  if (M <= 0 || K <= 0) return 0;
  const int Kp = (K + 31) / 32 * 32;
  const size_t n = (size_t)M * (Kp >> 2);
  const int blocks = (int)std::min<size_t>((n + 255) / 256, 8192);
  hipLaunchKernelGGL(split_h2_kernel, dim3(blocks), dim3(256), 0, s, src, ld, M, K, Kp, dst, ldd, mode, ovf);
  AIMNET_LAUNCH_CHECK();
  return 0;
}

// host-side split of a weight matrix [rows][K] (K % 32 == 0) into the h2 layout (round to nearest even, like the device)
bool split_h2_host(const float* w, int rows, int K, unsigned short* out, int mode) {
  bool fits = true;
  for (int r = 0; r < rows; ++r)
    for (int k = 0; k < K; ++k) {
      const float x = w[(size_t)r * K + k];
      if (!(fabsf(x) < H2_MAX)) fits = false;
      const bool odd = ((k >> 5) & 1) != 0;
      const _Float16 h = (_Float16)x;
      const float res = (x - (float)h) * ((mode == H2_ACT && odd) ? -H2_SCALE : H2_SCALE);
      const _Float16 l = (_Float16)res;
      unsigned short hb, lb;
      memcpy(&hb, &h, 2);
      memcpy(&lb, &l, 2);
      if (mode == H2_WEIGHT && odd) hb ^= 0x8000u;
      unsigned short* o = out + (size_t)r * 2 * K + (k >> 5) * 64 + (k & 31);
      o[0] = hb;
      o[32] = lb;
    }
  return fits;
}


}  // namespace aimnet
