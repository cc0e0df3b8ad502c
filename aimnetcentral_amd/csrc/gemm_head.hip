// gemm_head.hip - the energy head, forward AND backward, as ONE launch.
//
//   e_i = w3 . GELU(W2 GELU(W1 aim_i + b1) + b2) + b3        (Output MLP 256 -> 128 -> 128 -> 1, aimnet/modules/core.py:114-132)
//   zbar_i = (dE/d aim_i) * GELU'(z_last,i)                   (E = sum_i e_i, so the adjoint seed of e_i is 1: the backward needs
//                                                              nothing that is not in this block - autograd's replay of the head)
// The four GEMMs of the head (two forward, two backward) have N = 128: one column tile, a quarter of the chip per launch, 9 - 13 us
// each for 2 % of the step's arithmetic.  Here a block owns 64 atoms and chains them on the split matrix path of gemm_split.h
// (same operand split, same products per tile in the same order, same accumulator sets and combine):
//   1  Z1 = aim W1^T   (K = 256; aim arrives pre-split from the last MLP layer's epilogue, streamed through an LDS ring)
//      H1 = GELU(Z1 + b1) -> LDS in split form, D1 = GELU' stays in registers
//   2  Z2 = H1 W2^T    (K = 128, A operand resident in LDS); H2, D2; e_i = H2 . w3 + b3 (lane, wave, block reduction)
//   3  T = (w3 * D2) W2          -> LDS;   4  aim_bar = (T * D1) W1 in two column halves; zbar = aim_bar * D_last -> memory (split form)
// The weights are ONE stream of 24 tiles of 128 rows x 32 k through a 3-stage LDS ring (DMA two steps ahead, across the seams, so
// that the next GEMM's weights arrive under the epilogue in between).
// ONE body, head_fused_body<F>, serves both operand forms: F is the format's device-side trait of gemm_split.h (Bf3Operand: six
// products per tile and k-step, 192-byte rows; H2Operand: three products, 128-byte rows in 16-row strips), which decides DMA
// mapping, fragment addresses, the order of fragment reads and products, the accumulator combine and the split-form write of the
// resident operand; the LDS layout (HeadLds<F>) and the wait counts follow from its row bytes and pass counts.
#include <type_traits>

#include "common.h"
#include "gemm_split.h"
#include "kernels.h"

namespace aimnet {

namespace {
constexpr int HT = 64;  // atoms per block
constexpr int HW = 8;   // waves per block; all of them issue every tile's DMA

// LDS of one block: [3 activation ring stages][3 weight ring stages][resident operand, 4 k-blocks][e_i partial sums]
template <class F>
struct HeadLds {
  static constexpr int NPA = F::template passes<HW>(HT);   // DMA wave-instructions per wave for an activation tile (64 rows) ...
  static constexpr int NPB = F::template passes<HW>(128);  // ... and for a weight tile (128 rows)
  static constexpr int PASS = HW * 1024;                   // bytes per pass of the block
  static constexpr int A_ST = NPA * PASS, B_ST = NPB * PASS, RING = 3 * A_ST + 3 * B_ST;  // ring stages (rounded up to whole passes)
  static constexpr int KB = HT * F::ROW_BYTES;             // one k-block of the resident operand
  static constexpr int RED = 4 * HT * 4;                   // [4 wn][64 rows] floats
  // Where a buffer of its own would exceed the 160 KiB a block may ask for (bf16x3: 173 KB), the resident operand ALIASES the
  // activation ring, which GEMM 1 is done with when the first epilogue writes it - after one more barrier (head_fused_body).
  static constexpr bool ALIAS = RING + 4 * KB + RED > 160 * 1024;
  static constexpr int RES = ALIAS ? 0 : RING;  // byte offset of the resident operand ...
  static constexpr int RED_AT = RING + (ALIAS ? 0 : 4 * KB);  // ... and of the partial sums
  static constexpr int BYTES = RED_AT + RED;
  static_assert(!ALIAS || 4 * KB <= 3 * A_ST, "the resident operand aliases the activation ring");
  static_assert(BYTES <= 160 * 1024, "LDS");
};

template <class F>
__device__ __forceinline__ void head_fused_body(const HeadFusedArgs& a) {
  using L = HeadLds<F>;
  extern __shared__ __attribute__((aligned(16))) unsigned char smem_h[];
  const int tid = threadIdx.x, lane = tid & 63;
  const int wid = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int wm = wid >> 2, wn = wid & 3;  // wave tile: rows 32 wm .. + 31, columns 32 wn .. + 31 of a 64 x 128 product
  const int l16 = lane & 15, lc = lane >> 4;
  const int m0 = blockIdx.x * HT;
  const int n_tiles = a.grad ? 24 : 12;

  const unsigned lds0 = (unsigned)(size_t)(__attribute__((address_space(3))) unsigned char*)smem_h;
  const unsigned ldsB = lds0 + 3 * L::A_ST, ldsR = lds0 + L::RES;
  float* red = reinterpret_cast<float*>(smem_h + L::RED_AT);  // [4 wn][64 rows]

  // DMA (F::goff with all HW waves issuing): byte offsets of this lane's granule per pass; W1 rows are 8 k-blocks apart, those of
  // the other three matrices 4
  unsigned goff_w1[L::NPB], goff_w[L::NPB], goff_a[L::NPA];
#pragma unroll
  for (int p = 0; p < L::NPB; ++p) {
    goff_w1[p] = F::template goff<HW>(p, wid, lane, 128, 0, 127, 8u * F::ROW_BYTES);
    goff_w[p] = F::template goff<HW>(p, wid, lane, 128, 0, 127, 4u * F::ROW_BYTES);
  }
#pragma unroll
  for (int p = 0; p < L::NPA; ++p) goff_a[p] = F::template goff<HW>(p, wid, lane, HT, m0, a.M - 1, 2u * (unsigned)a.lda3);
  const unsigned char* abase = reinterpret_cast<const unsigned char*>(a.aim3 + (size_t)m0 * a.lda3);
  auto issue = [&](int t) __attribute__((always_inline)) {  // tile t of the stream (uniform): weights, and aim for t < 8
    const int st = t % 3;
    unsigned char* bdst = smem_h + 3 * L::A_ST + st * L::B_ST + wid * 1024;
    if (t < 8) {
      unsigned char* adst = smem_h + st * L::A_ST + wid * 1024;
      const unsigned char* ga = abase + (size_t)t * F::ROW_BYTES;
#pragma unroll
      for (int p = 0; p < L::NPA; ++p) glds16b(ga + goff_a[p], adst + p * L::PASS);
      const unsigned char* gb = reinterpret_cast<const unsigned char*>(a.w1) + (size_t)t * F::ROW_BYTES;
#pragma unroll
      for (int p = 0; p < L::NPB; ++p) glds16b(gb + goff_w1[p], bdst + p * L::PASS);
    } else {
      const unsigned short* w = t < 12 ? a.w2 : t < 16 ? a.w2t : a.w1t;
      const unsigned char* gb =
          reinterpret_cast<const unsigned char*>(w) + (t >= 20 ? 128 * 4 * F::ROW_BYTES : 0) + (size_t)(t & 3) * F::ROW_BYTES;
#pragma unroll
      for (int p = 0; p < L::NPB; ++p) glds16b(gb + goff_w[p], bdst + p * L::PASS);
    }
  };

  // biases / last-layer weights of this lane's columns (loaded before the DMA stream starts)
  f32x4 b1v[2], b2v[2], w3v[2];
#pragma unroll
  for (int j = 0; j < 2; ++j) {
    const int col = wn * 32 + 16 * j + 4 * lc;
    b1v[j] = *reinterpret_cast<const f32x4*>(a.b1 + col);
    b2v[j] = *reinterpret_cast<const f32x4*>(a.b2 + col);
    w3v[j] = *reinterpret_cast<const f32x4*>(a.w3 + col);
  }
  const float b3 = a.b3[0];

  const unsigned adA = lds0 + F::frag_addr(32 * wm, l16, lc);  // activation ring stage 0, the wave's two row strips
  const unsigned adR = ldsR + F::frag_addr(32 * wm, l16, lc);  // resident operand, k-block 0
  const unsigned adB = ldsB + F::frag_addr(32 * wn, l16, lc);

  f32x4 acc[F::NACC][2][2];  // accumulator sets: F::products / F::total ("Accumulation", gemm_split.h)
  auto zero_acc = [&]() __attribute__((always_inline)) {
#pragma unroll
    for (int h = 0; h < F::NACC; ++h)
#pragma unroll
      for (int i = 0; i < 2; ++i)
#pragma unroll
        for (int j = 0; j < 2; ++j) acc[h][i][j] = f32x4{0.f, 0.f, 0.f, 0.f};
  };
  // even-step set minus odd-step set (all four weight operands carry their odd k-blocks negated)
  auto total = [&](int i, int j) __attribute__((always_inline)) -> f32x4 { return F::total(acc, i, j, 1.0f, -1.0f); };
  zero_acc();
  typename F::frag fa[2][F::PLANES], fb[2][F::PLANES];
  // one 32-k step: tile t of the stream against the activation tile at LDS address a_lds; NW = stream operations that may stay
  // outstanding at its wait (the younger tile t + 1; the memory counter retires loads in order)
  auto step = [&](int t, unsigned a_lds, auto par_c, auto nw_c) __attribute__((always_inline)) {
    constexpr int PAR = decltype(par_c)::value;  // parity of the k-step inside its GEMM: the accumulator set
    wait_vm<decltype(nw_c)::value>();
    __builtin_amdgcn_sched_barrier(0);
    __builtin_amdgcn_s_barrier();
    __builtin_amdgcn_sched_barrier(0);
    F::load_frags(fa, fb, a_lds, adB + (t % 3) * L::B_ST);
    wait_lgkm<0>();
    __builtin_amdgcn_sched_barrier(0);
    // the DMA of tile t + 2 is issued among the matrix instructions (in front of the fragment reads it cost 100 - 185 cycles per
    // piece on the critical path); its ring stage was last read in step t - 1, which every wave left before this step's barrier
    F::template products<PAR>(acc, fa, fb, [&]() __attribute__((always_inline)) {
      __builtin_amdgcn_sched_barrier(0);
      if (t + 2 < n_tiles) issue(t + 2);
      __builtin_amdgcn_sched_barrier(0);
    });
    __builtin_amdgcn_sched_barrier(0);
  };
  using P0 = std::integral_constant<int, 0>;
  using P1 = std::integral_constant<int, 1>;
#define AIMNET_HEAD_STEP(T, A_LDS, NW) \
  if ((T) & 1) step(T, A_LDS, P1{}, NW{}); else step(T, A_LDS, P0{}, NW{})  // (all four GEMMs start on an even tile of the stream)
  using W0 = std::integral_constant<int, 0>;                  // nothing younger
  using WB = std::integral_constant<int, L::NPB>;             // the younger tile is weights only
  using WAB = std::integral_constant<int, L::NPA + L::NPB>;   // ... activations and weights
  // the wave's 32 x 32 block of a 64 x 128 matrix -> the resident LDS operand (k-block wn), split form
  auto to_lds = [&](const f32x4 (&v)[2][2]) __attribute__((always_inline)) {
#pragma unroll
    for (int i = 0; i < 2; ++i)
#pragma unroll
      for (int j = 0; j < 2; ++j) F::lds_put4(ldsR + wn * L::KB, wm * 32 + 16 * i + l16, 16 * j + 4 * lc, wn, v[i][j]);
    wait_lgkm<0>();
  };
  auto seam = [&]() __attribute__((always_inline)) {  // every wave has read the operand the next epilogue overwrites
    __builtin_amdgcn_sched_barrier(0);
    __builtin_amdgcn_s_barrier();
    __builtin_amdgcn_sched_barrier(0);
  };

  issue(0);
  issue(1);
  // ---- 1: Z1 = aim W1^T ------------------------------------------------------------------------------------------------
#pragma unroll
  for (int t = 0; t < 8; ++t) {
    if (t < 7) { AIMNET_HEAD_STEP(t, adA + (t % 3) * L::A_ST, WAB); }
    else { AIMNET_HEAD_STEP(t, adA + (t % 3) * L::A_ST, WB); }
  }
  f32x4 D1[2][2], v[2][2];
  {
#pragma unroll
    for (int i = 0; i < 2; ++i)
#pragma unroll
      for (int j = 0; j < 2; ++j) {
        const f32x4 z = total(i, j);
#pragma unroll
        for (int r = 0; r < 4; ++r) {
          float h, d;
          gelu_and_grad(z[r] + b1v[j][r], h, d);
          v[i][j][r] = h;
          D1[i][j][r] = d;
        }
      }
  }
  if constexpr (L::ALIAS) seam();  // every wave has read GEMM 1's last activation tile (a buffer of its own has no reader before the next step's barrier)
  to_lds(v);
  zero_acc();
  // ---- 2: Z2 = H1 W2^T, e = H2 . w3 + b3 -------------------------------------------------------------------------------
#pragma unroll
  for (int t = 8; t < 12; ++t) {
    if (t < 11) { AIMNET_HEAD_STEP(t, adR + (t - 8) * L::KB, WB); }
    else if (a.grad) { AIMNET_HEAD_STEP(t, adR + (t - 8) * L::KB, WB); }
    else { AIMNET_HEAD_STEP(t, adR + (t - 8) * L::KB, W0); }
  }
  {
    float pe[2] = {0.f, 0.f};
#pragma unroll
    for (int i = 0; i < 2; ++i)
#pragma unroll
      for (int j = 0; j < 2; ++j) {
        const f32x4 z = total(i, j);
#pragma unroll
        for (int r = 0; r < 4; ++r) {
          float h, d;
          gelu_and_grad(z[r] + b2v[j][r], h, d);
          pe[i] += h * w3v[j][r];
          v[i][j][r] = w3v[j][r] * d;  // adjoint seed of z2: dE/de = 1
        }
      }
#pragma unroll
    for (int i = 0; i < 2; ++i) {
      pe[i] += __shfl_xor(pe[i], 16);
      pe[i] += __shfl_xor(pe[i], 32);
      if (lc == 0) red[wn * HT + wm * 32 + 16 * i + l16] = pe[i];
    }
  }
  seam();  // every wave has read the resident operand the next epilogue overwrites; `red` is complete
  if (tid < HT && m0 + tid < a.M) a.e_atom[m0 + tid] = ((red[tid] + red[HT + tid]) + (red[2 * HT + tid] + red[3 * HT + tid])) + b3;
  if (!a.grad) return;
  to_lds(v);
  zero_acc();
  // ---- 3: T = (w3 * D2) W2 ------------------------------------------------------------------------------------------
#pragma unroll
  for (int t = 12; t < 16; ++t) { AIMNET_HEAD_STEP(t, adR + (t - 12) * L::KB, WB); }
  {
#pragma unroll
    for (int i = 0; i < 2; ++i)
#pragma unroll
      for (int j = 0; j < 2; ++j) v[i][j] = total(i, j) * D1[i][j];
  }
  seam();
  to_lds(v);
  zero_acc();
  // ---- 4: aim_bar = (T * D1) W1, two halves of 128 columns; zbar = aim_bar * D_last -----------------------------------------
#pragma unroll
  for (int half = 0; half < 2; ++half) {
#pragma unroll
    for (int t = 16 + 4 * half; t < 20 + 4 * half; ++t) {
      const int kb = t - 16 - 4 * half;
      if (t < 23) { AIMNET_HEAD_STEP(t, adR + kb * L::KB, WB); }
      else { AIMNET_HEAD_STEP(t, adR + kb * L::KB, W0); }
    }
#pragma unroll
    for (int i = 0; i < 2; ++i) {
      const int row = m0 + wm * 32 + 16 * i + l16;
      if (row >= a.M) continue;  // (the lanes of a row agree: the exchange inside store_split_tile_pair stays consistent)
      const int col0 = half * 128 + wn * 32;
      const f32x4 d0 = *reinterpret_cast<const f32x4*>(a.dlast + (size_t)row * a.ldd + col0 + 4 * lc);
      const f32x4 d1 = *reinterpret_cast<const f32x4*>(a.dlast + (size_t)row * a.ldd + col0 + 16 + 4 * lc);
      store_split_tile_pair<F::FMT>(a.zbar3 + (size_t)row * a.ldz3, col0, lc, total(i, 0) * d0, total(i, 1) * d1);
    }
    zero_acc();
  }
#undef AIMNET_HEAD_STEP
}
}  // namespace

// the entry points: the body over the fp16x2 form (the default) and over the bf16x3 form.  (Their order is measured: with the same
// instructions, the fp16x2 kernel behind the bf16x3 one in the code object ran 0.2 us slower; profiles/head_one_body_ab.txt)
__global__ __launch_bounds__(512) void head_fused_h2_kernel(HeadFusedArgs a) { head_fused_body<H2Operand>(a); }
__global__ __launch_bounds__(512) void head_fused_kernel(HeadFusedArgs a) { head_fused_body<Bf3Operand>(a); }

int launch_head_fused(hipStream_t s, const HeadFusedArgs& a) {
  if (a.M <= 0) return 0;
  const int blk = 32 * split_planes(a.fmt);  // 16-bit elements per 32-k block of a row
  if ((a.lda3 % blk) || (a.ldz3 % blk) || (a.ldd & 3) ||
      (((size_t)a.aim3 | (size_t)a.w1 | (size_t)a.w2 | (size_t)a.w2t | (size_t)a.w1t | (size_t)a.b1 | (size_t)a.b2 | (size_t)a.w3 |
        (size_t)a.dlast | (size_t)a.zbar3) & 15)) {
    set_last_error("head_fused: operands must be 16-byte aligned, row strides whole 32-k blocks");
    return -1;
  }
  static PerDeviceOnce once;
  if (once.first()) {
    AIMNET_HIP_CHECK(hipFuncSetAttribute((const void*)head_fused_kernel, hipFuncAttributeMaxDynamicSharedMemorySize, 160 * 1024));
    AIMNET_HIP_CHECK(hipFuncSetAttribute((const void*)head_fused_h2_kernel, hipFuncAttributeMaxDynamicSharedMemorySize, 160 * 1024));
  }
  if (a.fmt == SPLIT_H2) hipLaunchKernelGGL(head_fused_h2_kernel, dim3(ceil_div(a.M, HT)), dim3(64 * HW), HeadLds<H2Operand>::BYTES, s, a);
  else hipLaunchKernelGGL(head_fused_kernel, dim3(ceil_div(a.M, HT)), dim3(64 * HW), HeadLds<Bf3Operand>::BYTES, s, a);
  AIMNET_LAUNCH_CHECK();
  return 0;
}

}  // namespace aimnet
