// gemm_split.h - the MLP GEMM on PRE-SPLIT operands, written once over the operand format: the two formats' device-side traits
// (Bf3Operand: bf16x3 planes, H2Operand: fp16x2 planes), and kernel body, launcher and tile choice of gemm_bf3a.hip and gemm_h2.hip.
// A trait holds what the format decides - plane count, row bytes, DMA offsets, fragment addresses, the order of fragment reads and
// products, the accumulator combine, the split-form write of an LDS-resident operand; everything the formats agree on is written
// once over it: gemm_split_body here, head_fused_body in gemm_head.hip.  The traits live here and not in gemm_bf3_common.h /
// gemm_h2_common.h because their interface IS what the bodies consume: the two stand next to each other and next to split_product,
// and the helpers of the common headers stay usable by the kernels that are not written over a trait (gemm_bf3.hip, gemm_chain.hip,
// the producers).  gemm_bf3a.hip / gemm_h2.hip derive Bf3Fmt / H2Fmt from them, adding the GEMM launcher's choices (entry points,
// ring depths), and define the __global__ entry points, which are one call of gemm_split_body.
//
//   C[M,N] = A[M,K] . Bt[N,K]^T with the fused epilogues of gemm.hip; A and Bt per row as K/32 blocks of F::PLANES planes of 32
//   16-bit elements; OUT: the GELU / chain-rule epilogues write C in the same form for the next layer.
//
// Schedule: the ping-pong of gemm_bf3.hip - waves 0-3 (group 0, upper half of the tile) and waves 4-7 (group 1, lower half, same
// SIMDs) alternate LOAD and COMPUTE segments half a step apart, one s_barrier per segment - with the DMA split by group (NSA
// activation stages, NSB = F::nsb(NSA) weight stages; NSA = 2, NSB = 3 below):
//   group 0, L(j): fragments of step j -> registers; DMA of the WHOLE activation tile of step j+1 into SA[(j+1) & 1] (last read by
//                  group 1 one segment ago); waits for it at the end of its C(j): two segments of lead
//   group 1, L(j): fragments of step j; DMA of the whole weight tile of step j+2 into ring stage (j+2) % 3; waits for the tile of
//                  step j+1 (issued one L earlier: in-order retirement, "at most one tile outstanding") before its barrier
// so every tile is complete, and waited for by the waves that requested it, one barrier before its first reader.  Deeper rings
// (gemm_h2.hip, "Ring depth") request NSA - 1 / NSB - 1 steps ahead and leave the later requests outstanding at the same waits.
#pragma once

#include <type_traits>

#include "common.h"
#include "gemm_h2_common.h"
#include "kernels.h"

namespace aimnet {

struct Bf3Fmt;  // gemm_bf3a.hip
struct H2Fmt;   // gemm_h2.hip

constexpr int SPLIT_GEMM_DMA_WAVES = 4;  // waves of a block that issue one tile's DMA: a group of the GEMM (all 8 in gemm_head.hip)

// LDS of one block: a stage is F::passes(rows) DMA wave-instructions per wave of the issuing group, 4 KiB each
template <class F>
constexpr int split_lds_bytes(int TM, int TN, int NSA) {
  return NSA * F::template passes<SPLIT_GEMM_DMA_WAVES>(TM) * 4096 + F::nsb(NSA) * F::template passes<SPLIT_GEMM_DMA_WAVES>(TN) * 4096;
}

// one product of the split: plane PA of the activation fragments x plane PB of the weight fragments, into accumulator set SET
template <class F, int SET, int PA, int PB, int SM, int SN>
__device__ __forceinline__ void split_product(f32x4 (&acc)[F::NACC][SM][SN], const typename F::frag (&fa)[SM][F::PLANES],
                                              const typename F::frag (&fb)[SN][F::PLANES]) {
#pragma unroll
  for (int i = 0; i < SM; ++i)
#pragma unroll
    for (int jj = 0; jj < SN; ++jj) acc[SET][i][jj] = F::mfma(fb[jj][PB], fa[i][PA], acc[SET][i][jj]);
}
struct SplitNoOp {  // F::products' default for what runs between the first product and the rest
  __device__ __forceinline__ void operator()() const {}
};

// ---- the bf16x3 form (layout, LDS tile and swizzle: gemm_bf3_common.h)
struct Bf3Operand {
  using frag = bf16x8;
  static constexpr int FMT = SPLIT_BF3, PLANES = split_planes(FMT);
  static constexpr int NACC = 2;          // accumulator sets
  static constexpr int ROW_BYTES = ROWB;  // per row and 32-k step, in memory and in LDS
  // DMA wave-instructions per wave of the NW issuing waves for a tile of `rows` rows (a pass = NW KiB)
  template <int NW>
  static constexpr int passes(int rows) { return (rows * 12 + 64 * NW - 1) / (64 * NW); }

  // DMA granules of the NW issuing waves: G = p * 64 NW + 64 w + lane -> row G / 12, plane (G % 12) / 4, slot G % 4 holding k-chunk
  // slot ^ swz(row); granules beyond the tile (padding of the last pass) re-read the last one into the stage's padding.
  template <int NW>
  static __device__ __forceinline__ unsigned goff(int p, int w, int lane, int tile_rows, int r0, int rlim, unsigned ldbytes) {
    const int G = min(p * 64 * NW + w * 64 + lane, tile_rows * 12 - 1);
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
  // four values of one lane - columns col .. col + 3 (col % 4 == 0) of row `row` of a 32-k tile - split into the LDS tile at `tile`
  // (an activation operand: nothing depends on kblock, the tile's k-block in its matrix)
  static __device__ __forceinline__ void lds_put4(unsigned tile, int row, int col, int /*kblock*/, f32x4 v) {
    const unsigned ad = tile + row * ROWB + (((col >> 3) ^ swz192(row)) << 4) + (col & 4) * 2;
    unsigned lo0, lo1, lo2, hi0, hi1, hi2;
    split3_pair(v[0], v[1], lo0, lo1, lo2);
    split3_pair(v[2], v[3], hi0, hi1, hi2);
    lds_write8<0>(ad, lo0, hi0);
    lds_write8<64>(ad, lo1, hi1);
    lds_write8<128>(ad, lo2, hi2);
  }

  // Accumulation.  v_mfma_f32_16x16x32_bf16 aligns its 32 products and the accumulator in a fixed-point adder and TRUNCATES what
  // falls below - towards minus infinity, ~2^-7.5 ulp per instruction, one-signed: -4.7e-8 |z| on every output of a K = 736 layer
  // (tests/tools/bf3_bias.py), which does not average out over atoms (config 5's energies moved by twice the fp32 noise).  Round 3
  // cancelled it with a sign-flipped second phase whose start (0.56 K) had to be fitted to the growth of |acc| over k - a property of
  // the data.  Here the weights of every ODD k-block are stored negated (BF3_ALT) and even / odd k-steps accumulate into two
  // accumulator sets; the epilogue takes their difference.  Both sets see interleaved halves of the same sum - the same magnitude
  // profile whatever the data - and both are truncated downwards, so the biases cancel in the difference: no tunable.
  static __device__ __forceinline__ f32x4 mfma(frag b, frag a, f32x4 c) { return __builtin_amdgcn_mfma_f32_16x16x32_bf16(b, a, c, 0, 0, 0); }
  // PAR: parity of the k-step; after_first runs between the first product and the rest (gemm_head.hip: its DMA issue)
  template <int PAR, int SM, int SN, class Mid = SplitNoOp>
  static __device__ __forceinline__ void products(f32x4 (&acc)[2][SM][SN], const frag (&fa)[SM][3], const frag (&fb)[SN][3],
                                                  Mid after_first = {}) {
    split_product<Bf3Operand, PAR, 1, 1>(acc, fa, fb);
    after_first();
    split_product<Bf3Operand, PAR, 0, 1>(acc, fa, fb);
    split_product<Bf3Operand, PAR, 1, 0>(acc, fa, fb);
    split_product<Bf3Operand, PAR, 0, 2>(acc, fa, fb);
    split_product<Bf3Operand, PAR, 2, 0>(acc, fa, fb);
    split_product<Bf3Operand, PAR, 0, 0>(acc, fa, fb);
  }
  template <int SM, int SN>
  static __device__ __forceinline__ f32x4 total(const f32x4 (&acc)[2][SM][SN], int i, int j, float s0, float s1) {
    return acc[0][i][j] * s0 + acc[1][i][j] * s1;
  }
};

// ---- the fp16x2 form (layout, signs, LDS strips and swizzle: gemm_h2_common.h)
struct H2Operand {
  using frag = f16x8;
  static constexpr int FMT = SPLIT_H2, PLANES = split_planes(FMT);
  static constexpr int NACC = 3;             // accumulator sets
  static constexpr int ROW_BYTES = H2_ROWB;  // per row and 32-k step in memory
  // DMA wave-instructions per wave of the NW issuing waves for a tile of `rows` rows (a pass = NW KiB = NW / 2 strips)
  template <int NW>
  static constexpr int passes(int rows) { return (rows + 8 * NW - 1) / (8 * NW); }

  // DMA of the NW issuing waves: pass p, wave w -> KiB q = NW p + w of the stage = plane q & 1 of the 16-row strip q >> 1; lane ->
  // row (lane >> 2) of the strip, slot lane & 3 holding k-chunk slot ^ swz(row).  Strips beyond the tile (padding of the last
  // pass) re-read the last row into the stage's padding; rows beyond the matrix re-read its last row.
  template <int NW>
  static __device__ __forceinline__ unsigned goff(int p, int w, int lane, int tile_rows, int r0, int rlim, unsigned ldbytes) {
    const int q = p * NW + w;
    const int row = min((q >> 1) * 16 + (lane >> 2), tile_rows - 1), pl = q & 1;
    const int kcx = (lane & 3) ^ swz_h2(row);
    return (unsigned)(min(r0 + row, rlim) - r0) * ldbytes + pl * 64 + kcx * 16;
  }
  // fragment addresses: row r, plane P, k-chunk c = lane >> 4 -> (r >> 4) * 2048 + P * 1024 + (r & 15) * 64 + (c ^ swz(r)) * 16
  static __device__ __forceinline__ unsigned frag_addr(int row0, int l16, int lc) {
    return (row0 >> 4) * H2_STRIP + l16 * 64 + ((lc ^ swz_h2(l16)) << 4);
  }
  template <int SM, int SN>
  static __device__ __forceinline__ void load_frags(frag (&fa)[SM][2], frag (&fb)[SN][2], unsigned oa, unsigned ob) {
    read_strips_h<0, SN, 1>(fb, ob);
    read_strips_h<0, SM, 0>(fa, oa);
    read_strips_h<0, SN, 0>(fb, ob);
    read_strips_h<0, SM, 1>(fa, oa);
  }
  // four values of one lane - columns col .. col + 3 (col % 4 == 0) of row `row` of a 32-k tile - split into the LDS tile at `tile`,
  // activation form: lo negated where kblock, the tile's k-block in its matrix, is odd
  static __device__ __forceinline__ void lds_put4(unsigned tile, int row, int col, int kblock, f32x4 v) {
    const float sc = (kblock & 1) ? -H2_SCALE : H2_SCALE;
    const unsigned ad = tile + (row >> 4) * H2_STRIP + (row & 15) * 64 + (((col >> 3) ^ swz_h2(row)) << 4) + (col & 4) * 2;
    unsigned h0, l0, h1, l1;
    split2_pair(v[0], v[1], sc, h0, l0);
    split2_pair(v[2], v[3], sc, h1, l1);
    lds_write8<0>(ad, h0, h1);
    lds_write8<1024>(ad, l0, l1);
  }

  // Accumulation.  The matrix pipe TRUNCATES the aligned sum of its 32 products and the accumulator towards minus infinity
  // (Bf3Operand, "Accumulation"; profiles/r4_bf3_bias.txt): one-signed, it does not average out over atoms.  As there, the hi
  // planes of the weights' ODD k-blocks are stored negated and the hi x hi products of even / odd k-steps go to two accumulator
  // sets whose difference the epilogue takes.  The cross terms are 2^-12 of that sum: their own truncation is irrelevant and
  // they share one set (activations carry the lo planes of the odd k-blocks negated, so both cross products keep their sign).
  // acc[0], [1]: ah bh of the even / odd k-steps; [2]: the cross terms ah bl + al bh (x 4096)
  static __device__ __forceinline__ f32x4 mfma(frag b, frag a, f32x4 c) { return __builtin_amdgcn_mfma_f32_16x16x32_f16(b, a, c, 0, 0, 0); }
  // PAR: parity of the k-step; after_first runs between the first product and the rest (gemm_head.hip: its DMA issue)
  template <int PAR, int SM, int SN, class Mid = SplitNoOp>
  static __device__ __forceinline__ void products(f32x4 (&acc)[3][SM][SN], const frag (&fa)[SM][2], const frag (&fb)[SN][2],
                                                  Mid after_first = {}) {
    split_product<H2Operand, 2, 0, 1>(acc, fa, fb);
    after_first();
    split_product<H2Operand, PAR, 0, 0>(acc, fa, fb);
    split_product<H2Operand, 2, 1, 0>(acc, fa, fb);
  }
  template <int SM, int SN>
  static __device__ __forceinline__ f32x4 total(const f32x4 (&acc)[3][SM][SN], int i, int j, float s0, float s1) {
    return acc[0][i][j] * s0 + acc[1][i][j] * s1 + acc[2][i][j] * H2_INV_SCALE;
  }
};

template <class F, int EPI, int SM, int SN, int WN, bool OUT, int NSA>
__device__ __forceinline__ void gemm_split_body(const unsigned short* __restrict__ A3, int lda3, const unsigned short* __restrict__ Bt,
                                                int ldb, int M, int N, int K, const float* __restrict__ bias, float* __restrict__ C,
                                                unsigned short* __restrict__ C3, int ldc3, float* __restrict__ D, int ldc,
                                                const int* __restrict__ brow, int ldbias, int alt) {
  static_assert(WN == 8 || WN == 4 || WN == 2, "waves across N");
  using frag = typename F::frag;
  constexpr int WM = 8 / WN;
  constexpr int TM = 16 * SM * WM, TN = 16 * SN * WN;
  constexpr int NPA = F::template passes<SPLIT_GEMM_DMA_WAVES>(TM), NPB = F::template passes<SPLIT_GEMM_DMA_WAVES>(TN);
  constexpr int SA_BYTES = NPA * 4096, SB_BYTES = NPB * 4096;
  constexpr int NSB = F::nsb(NSA);  // lead of the requests: NSA - 1 steps for activation tiles, NSB - 1 for weight tiles
  extern __shared__ __attribute__((aligned(16))) unsigned char smem_a[];

  const int tid = threadIdx.x;
  const int lane = tid & 63;
  const int wid = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int wm = wid / WN, wn = wid % WN;
  const bool late = wid >= 4;  // group 1 runs one segment behind group 0
  const int w4 = wid & 3;

  const int tiles_n = (N + TN - 1) / TN;
  const int nwg = gridDim.x;
  const int xq = nwg >> 3, xr = nwg & 7, xcd = blockIdx.x & 7;
  const int wg = (xcd < xr ? xcd * (xq + 1) : xr * (xq + 1) + (xcd - xr) * xq) + (blockIdx.x >> 3);
  const int m0 = (wg / tiles_n) * TM, n0 = (wg % tiles_n) * TN;

  f32x4 acc[F::NACC][SM][SN];  // accumulator sets: F::products / F::total ("Accumulation", Bf3Operand)
#pragma unroll
  for (int h = 0; h < F::NACC; ++h)
#pragma unroll
    for (int i = 0; i < SM; ++i)
#pragma unroll
      for (int j = 0; j < SN; ++j) acc[h][i][j] = f32x4{0.f, 0.f, 0.f, 0.f};

  const unsigned lds0 = (unsigned)(size_t)(__attribute__((address_space(3))) unsigned char*)smem_a;
  const unsigned ldsB = lds0 + NSA * SA_BYTES;

  // DMA of the issuing group: one wave-instruction per pass p moves 1 KiB into the stage at (4 p + w4) KiB; F::goff maps pass,
  // wave and lane to the 16-byte granule that belongs there (padding of the last pass re-reads the tile's last granule / row into
  // the stage's padding; rows beyond the matrix re-read its last row).
  // Offsets are bytes relative to the tile's first row (32 bits: a tile spans < 200 rows).
  constexpr int NPMAX = NPA > NPB ? NPA : NPB;
  unsigned goff[NPMAX];
  {
    const int r0 = late ? n0 : m0, rlim = (late ? N : M) - 1;
    const unsigned ldbytes = 2u * (unsigned)(late ? ldb : lda3);
#pragma unroll
    for (int p = 0; p < NPMAX; ++p) goff[p] = F::template goff<SPLIT_GEMM_DMA_WAVES>(p, w4, lane, late ? TN : TM, r0, rlim, ldbytes);
  }
  const unsigned char* abase = reinterpret_cast<const unsigned char*>(A3 + (size_t)m0 * lda3);
  const unsigned char* bbase = reinterpret_cast<const unsigned char*>(Bt + (size_t)n0 * ldb);
  auto dma_a = [&](int stage, int kt) __attribute__((always_inline)) {
    unsigned char* base = smem_a + stage * SA_BYTES + w4 * 1024;
    const unsigned char* g = abase + (size_t)kt * F::ROW_BYTES;
#pragma unroll
    for (int p = 0; p < NPA; ++p) glds16b(g + goff[p], base + p * 4096);
  };
  auto dma_b = [&](int stage, int kt) __attribute__((always_inline)) {
    unsigned char* base = smem_a + NSA * SA_BYTES + stage * SB_BYTES + w4 * 1024;
    const unsigned char* g = bbase + (size_t)kt * F::ROW_BYTES;
#pragma unroll
    for (int p = 0; p < NPB; ++p) glds16b(g + goff[p], base + p * 4096);
  };

  // fragment addresses of this wave's first strip, plane 0, k-chunk c = lane >> 4 (F::frag_addr: layout and swizzle of a stage)
  const int l16 = lane & 15, lc = lane >> 4;
  const unsigned adA = lds0 + F::frag_addr(wm * 16 * SM, l16, lc);
  const unsigned adB = ldsB + F::frag_addr(wn * 16 * SN, l16, lc);

  using I0 = std::integral_constant<int, 0>;
  using I1 = std::integral_constant<int, 1>;
  const int nk = K >> 5;
  // every step issues the same operations: k-steps past the end of K are clamped to the last one (redundant tiles nothing reads)
  auto kc = [&](int k) __attribute__((always_inline)) { return min(k, nk - 1); };

  frag fa[SM][F::PLANES], fb[SN][F::PLANES];
  // ---- prologue: A(0) .. A(NSA - 2) by group 0; B(0) .. B(NSB - 2) by group 1
  if (!late) {
#pragma unroll
    for (int t = 0; t < NSA - 1; ++t) dma_a(t, kc(t));
    wait_vm<(NSA - 2) * NPA>();  // A(0) has landed
  } else {
#pragma unroll
    for (int t = 0; t < NSB - 1; ++t) dma_b(t, kc(t));
    wait_vm<(NSB - 2) * NPB>();  // B(0) has landed
  }
  __builtin_amdgcn_sched_barrier(0);
  __builtin_amdgcn_s_barrier();
  __builtin_amdgcn_sched_barrier(0);

  // sa / sb: ring stages of this step's activation / weight tile
  auto seg_load = [&](int j, int sa, int sb, auto g_c) __attribute__((always_inline)) {
    constexpr int G = decltype(g_c)::value;
    F::load_frags(fa, fb, adA + sa * SA_BYTES, adB + sb * SB_BYTES);
    if constexpr (G == 0) {
      dma_a(sa == 0 ? NSA - 1 : sa - 1, kc(j + NSA - 1));  // stage (sa + NSA - 1) % NSA held A(j - 1)
      wait_lgkm<0>();
    } else {
      dma_b(sb == 0 ? NSB - 1 : sb - 1, kc(j + NSB - 1));  // stage (sb + NSB - 1) % NSB
      wait_vm<(NSB - 2) * NPB>();  // the weight tile of step j+1 has landed (the later requests may be outstanding)
      wait_lgkm<0>();
    }
    __builtin_amdgcn_sched_barrier(0);
  };
  auto seg_compute = [&](auto par_c, auto g_c) __attribute__((always_inline)) {
    constexpr int G = decltype(g_c)::value, PAR = decltype(par_c)::value;  // PAR: parity of the k-step = accumulator set
    __builtin_amdgcn_sched_barrier(0);
    F::template products<PAR>(acc, fa, fb);
    __builtin_amdgcn_sched_barrier(0);
    if constexpr (G == 0) wait_vm<(NSA - 2) * NPA>();  // the activation tile of step j+1 has landed
    __builtin_amdgcn_sched_barrier(0);
  };
  auto bar = [&]() __attribute__((always_inline)) {
    __builtin_amdgcn_s_barrier();
    __builtin_amdgcn_sched_barrier(0);
  };
  auto run = [&](auto g_c) __attribute__((always_inline)) {
    int sa = 0, sb = 0, j = 0;
    auto next = [&]() __attribute__((always_inline)) {
      sa = sa == NSA - 1 ? 0 : sa + 1;
      sb = sb == NSB - 1 ? 0 : sb + 1;
    };
    // (two activation stages: the stage is the parity of the k-step, a compile-time constant of the segment)
    for (; j + 1 < nk; j += 2) {
      seg_load(j, NSA == 2 ? 0 : sa, sb, g_c);
      bar();
      seg_compute(I0{}, g_c);
      next();
      bar();
      seg_load(j + 1, NSA == 2 ? 1 : sa, sb, g_c);
      bar();
      seg_compute(I1{}, g_c);
      next();
      if (j + 2 < nk) bar();
    }
    if (j < nk) {  // odd number of steps
      seg_load(j, NSA == 2 ? 0 : sa, sb, g_c);
      bar();
      seg_compute(I0{}, g_c);
    }
  };
  if (late) {
    bar();
    run(I1{});
  } else {
    run(I0{});
    bar();  // group 0 has 2 nk segments, group 1 an empty one in front: both pass 2 nk barriers
  }
  wait_vm<0>();  // the clamped look-ahead of the last steps: the wave must not end (LDS released) under its DMA
  __builtin_amdgcn_sched_barrier(0);

  // epilogue: sfin * acc[i][j][r] = C[m0 + wm*16*SM + 16 i + (lane&15)][n0 + wn*16*SN + 16 j + 4 (lane>>4) + r]
  // even-step set +/- odd-step set: alt 0 = plain weights (sum), 1 = BF3_ALT weights from an even k-block (difference), 2 = from an odd one
  const float s0 = alt == 2 ? -1.0f : 1.0f, s1 = alt == 1 ? -1.0f : 1.0f;
  // value of tile (i, j) after the fused epilogue (GELU' / chain-rule factor through D); false: outside the matrix
  auto finish = [&](int i, int j, f32x4& v) __attribute__((always_inline)) -> bool {
    const int col = n0 + wn * 16 * SN + 16 * j + 4 * lc;
    const int row = m0 + wm * 16 * SM + 16 * i + l16;
    if (col >= N || row >= M) return false;
    const size_t o = (size_t)row * ldc + col;
    v = F::total(acc, i, j, s0, s1);
    if (EPI == EPI_BIAS || EPI == EPI_BIAS_GELU) {
      const f32x4 bv = brow ? *reinterpret_cast<const f32x4*>(bias + (size_t)min(63, max(0, brow[row])) * ldbias + col)
                            : *reinterpret_cast<const f32x4*>(bias + col);
      v = v + bv;
    }
    if (EPI == EPI_BIAS_GELU) {
      f32x4 d;
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        float hh, dd;
        gelu_and_grad(v[r], hh, dd);
        v[r] = hh;
        d[r] = dd;
      }
      if (D) *reinterpret_cast<f32x4*>(D + o) = d;
    } else if (EPI == EPI_MUL) {
      v = v * *reinterpret_cast<const f32x4*>(D + o);
    }
    return true;
  };
  if constexpr (OUT) {
    // split output: 16-byte stores per plane through store_split_tile_pair (8-byte stores, 30 per lane with three planes, cost 9 us
    // on the large layers)
#pragma unroll
    for (int j = 0; j < SN; j += 2) {
#pragma unroll
      for (int i = 0; i < SM; ++i) {
        const int row = m0 + wm * 16 * SM + 16 * i + l16;
        unsigned short* crow = C3 + (size_t)row * ldc3;
        if (j + 1 < SN) {
          // N % 32 == 0: the first tile of a pair is inside whenever its first column is.  The second one can be outside: with
          // SN odd (tile 223) a wave's pairs start 16 columns past a 32-aligned column, and N % TN == TN - 32 puts that column
          // pair across N - then only the first tile is stored (the branch is uniform: the column does not depend on the lane)
          const int col0 = n0 + wn * 16 * SN + 16 * j;
          f32x4 v0, v1;
          if (!finish(i, j, v0)) continue;
          if (col0 + 16 < N) {
            finish(i, j + 1, v1);
            store_split_tile_pair<F::FMT>(crow, col0, lc, v0, v1);
          } else {
            store_split_x4<F::FMT>(crow, col0 + 4 * lc, v0);
          }
        } else {
          f32x4 v;
          if (!finish(i, j, v)) continue;
          store_split_x4<F::FMT>(crow, n0 + wn * 16 * SN + 16 * j + 4 * lc, v);
        }
      }
    }
  } else {
#pragma unroll
    for (int j = 0; j < SN; ++j) {
#pragma unroll
      for (int i = 0; i < SM; ++i) {
        f32x4 v;
        if (!finish(i, j, v)) continue;
        const int col = n0 + wn * 16 * SN + 16 * j + 4 * lc;
        const int row = m0 + wm * 16 * SM + 16 * i + l16;
        *reinterpret_cast<f32x4*>(C + (size_t)row * ldc + col) = v;
      }
    }
  }
}

// ---- host side ------------------------------------------------------------------------------------------------------------
inline int g_split_force_tile[3] = {};  // [SPLIT_BF3] AIMNET_BF3A_TILE, [SPLIT_H2] AIMNET_H2_TILE: force one configuration (A/B runs)

// id = 100 * WN (waves across N; 8 / WN across M) + 10 * SM + SN; block tile (16 SM 8 / WN) x (16 SN WN)
inline constexpr SplitTileCand kSplitCands[] = {{452, 160, 128}, {224, 128, 128}, {432, 96, 128}, {422, 64, 128},
                                                {223, 128, 96},  {851, 80, 128},  {234, 192, 128}};

// the > 64 KiB dynamic-LDS opt-in of every ring depth the format has (opt_in: first launch on this device) and the launch at `deep`
template <class F, int E, int SM, int SN, int WN, bool O, int NSA = 2>
static int launch_split_depth(hipStream_t stream, int deep, bool opt_in, const SplitArgs& a) {
  constexpr int TM = 16 * SM * (8 / WN), TN = 16 * SN * WN;
  constexpr int LDS = split_lds_bytes<F>(TM, TN, NSA);
  static_assert(LDS <= 160 * 1024, "LDS");
  const auto kernel = F::template kernel<E, SM, SN, WN, O, NSA>();
  if (opt_in) AIMNET_HIP_CHECK(hipFuncSetAttribute((const void*)kernel, hipFuncAttributeMaxDynamicSharedMemorySize, 160 * 1024));
  if (deep == NSA)
    hipLaunchKernelGGL(kernel, dim3(ceil_div(a.M, TM) * ceil_div(a.N, TN)), dim3(512), LDS, stream, a.A3, a.lda3, a.Bt, a.ldb, a.M,
                       a.N, a.K, a.bias, a.C, a.C3, a.ldc3, a.D, a.ldc, a.brow, a.ldbias, a.alt);
  if constexpr (NSA < F::MAX_NSA) return launch_split_depth<F, E, SM, SN, WN, O, NSA + 1>(stream, deep, opt_in, a);
  return 0;
}

template <class F, int SM, int SN, int WN>
static int launch_split(hipStream_t stream, int epi, bool out, const SplitArgs& a) {
  constexpr int TM = 16 * SM * (8 / WN), TN = 16 * SN * WN;
  const int deep = F::ring_depth(ceil_div(a.M, TM) * ceil_div(a.N, TN));
#define AIMNET_SPLIT_LAUNCH(E, O)                                                           \
  {                                                                                         \
    static PerDeviceOnce once;                                                              \
    rc = launch_split_depth<F, E, SM, SN, WN, O>(stream, deep, once.first(), a);            \
  }
  int rc = 0;
  if (out) {
    switch (epi) {
      case EPI_BIAS_GELU: AIMNET_SPLIT_LAUNCH(EPI_BIAS_GELU, true) break;
      case EPI_MUL: AIMNET_SPLIT_LAUNCH(EPI_MUL, true) break;
      default:
        set_last_error("%s: split output exists for the GELU and chain-rule epilogues only (got %d)", F::NAME, epi);
        return -1;
    }
  } else {
    switch (epi) {
      case EPI_NONE: AIMNET_SPLIT_LAUNCH(EPI_NONE, false) break;
      case EPI_BIAS: AIMNET_SPLIT_LAUNCH(EPI_BIAS, false) break;
      case EPI_BIAS_GELU: AIMNET_SPLIT_LAUNCH(EPI_BIAS_GELU, false) break;
      case EPI_MUL: AIMNET_SPLIT_LAUNCH(EPI_MUL, false) break;
      default:
        set_last_error("%s: bad epilogue %d", F::NAME, epi);
        return -1;
    }
  }
#undef AIMNET_SPLIT_LAUNCH
  if (rc) return rc;
  AIMNET_LAUNCH_CHECK();
  return 0;
}

// one format's entry point: instantiated explicitly in the format's file, called by launch_gemm_split_cfg (gemm_h2.hip)
template <class F>
int launch_split_cfg(hipStream_t stream, int cfg, int epi, bool out, const SplitArgs& a) {
  constexpr int BLK = 32 * F::PLANES;  // 16-bit elements per 32-k block of a row
  if (a.M <= 0) return 0;
  if (a.K % 32 != 0 || (a.lda3 % BLK) || (a.ldb % BLK) || (a.N & 3) || (a.ldc & 3) ||
      (out && (a.ldc3 % BLK || (a.N & 31) || a.ldc3 < F::PLANES * a.N)) ||
      (((size_t)a.A3 | (size_t)a.Bt | (size_t)a.bias | (size_t)a.C | (size_t)a.C3 | (size_t)a.D) & 15)) {
    set_last_error("%s: K=%d must be a multiple of 32, ldc/N multiples of 4, pointers 16-byte aligned, lda3/ldb/ldc3 whole %d-byte blocks, N %% 32 == 0 for split output",
                   F::NAME, a.K, F::ROW_BYTES);
    return -1;
  }
  if (cfg == 0) cfg = g_split_force_tile[F::FMT];
  if (cfg == 0) cfg = choose_tile_by_cost(kSplitCands, (int)(sizeof(kSplitCands) / sizeof(kSplitCands[0])), a.M, a.N);
  switch (cfg) {
#define AIMNET_SPLIT_CASE(ID, SM_, SN_, WN_) \
    case ID: return launch_split<F, SM_, SN_, WN_>(stream, epi, out, a);
    AIMNET_SPLIT_CASE(452, 5, 2, 4)  // 160 x 128 (2 x 4 waves of 80 x 32; 136 KiB of LDS)
    AIMNET_SPLIT_CASE(432, 3, 2, 4)  //  96 x 128
    AIMNET_SPLIT_CASE(422, 2, 2, 4)  //  64 x 128
    AIMNET_SPLIT_CASE(223, 2, 3, 2)  // 128 x  96 (4 x 2 waves of 32 x 48)
    AIMNET_SPLIT_CASE(224, 2, 4, 2)  // 128 x 128 (4 x 2 waves of 32 x 64)
    AIMNET_SPLIT_CASE(234, 3, 4, 2)  // 192 x 128 (4 x 2 waves of 48 x 64)
    AIMNET_SPLIT_CASE(851, 5, 1, 8)  //  80 x 128 (1 x 8 waves of 80 x 16)
#undef AIMNET_SPLIT_CASE
    default:
      set_last_error("%s: unknown tile id %d", F::NAME, cfg);
      return -1;
  }
}

}  // namespace aimnet
