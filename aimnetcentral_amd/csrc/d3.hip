// d3.hip - DFT-D3(BJ) two-body dispersion: energy, forces, virial.
//
// Reference semantics (paths relative to /root/reference/aimnet): modules/lr.py DFTD3 (:1335-1820), whose GPU
// path is the third-party nvalchemiops `dftd3` kernel and whose in-tree torch twin - the arithmetic restated
// here and in oracle/aimnet2_oracle.py::dftd3_energy - is
//   _calc_torch_coord_num :1595   cn_i = sum_j sigmoid(16 ((rcov_i + rcov_j) / d_ij - 1))        (d in Bohr)
//   _calc_torch_c6ij      :1605   C6_ij = sum_ab c6ref_ab W_ab / sum_ab W_ab over the 5x5 reference systems,
//                                 W_ab = exp(-4 ((cn_i - cnref_i[a])^2 + (cn_j - cnref_j[b])^2) - max), dropped below e^-12
//   _compute_energy_torch :1626   e_ij = -C6_ij (s6 / (d^6 + R0^6) + s8 3 r4r2_i r4r2_j / (d^8 + R0^8)) S5(d),
//                                 R0 = a1 sqrt(3 r4r2_i r4r2_j) + a2,  E = Hartree/2 * sum over ORDERED pairs
//   _s5_switch_torch      :1580   quintic switch between cutoff (1 - smoothing_fraction) and cutoff.
//
// What is different from the reference arithmetic, and why it is the same number:
//   * the reference tables store cnref_i[a] redundantly per partner species and reference b; they factorise
//     (checked at upload, engine.hip), so exp(-4 dcn_i^2 - 4 dcn_j^2) = w_i[a] w_j[b] with FIVE exponentials per
//     atom (d3_cn_kernel) instead of 25 per pair; the e^-12 drop rule is applied per (a, b) on the sum of the two
//     shifted exponents exactly as the reference does;
//   * forces are analytic (the reference kernel returns them too): the C6(cn) dependence goes through
//     dE/dcn_i accumulated in the pair pass and is pushed to positions by a third, cheap pass over the same list.
//
// Three passes over the D3 neighbour list (wave per atom, lanes over list slots), HBM-bound on the 8 B list entries
// with L2-resident gathers of 48 B per neighbour:
//   d3_cn_kernel       cn_i, then the 5 shifted exponents / weights of atom i
//   d3_pair_kernel     C6_ij, pair energy (fp64 sums), direct pair force + virial, dE/dcn_i
//   d3_cnforce_kernel  (dE/dcn_i + dE/dcn_j) dsigma/dd along u_ij  -> force + virial
#include "common.h"
#include "kernels.h"

namespace aimnet {

constexpr float HALF_HARTREE_F = 13.605693012183622f;
constexpr int D3W = 12;  // floats per atom in the weight table: s[5], w[5], cn, pad
constexpr int D3_SLOTS = 4;  // list slots per loop trip in the two light passes (cn, cnforce)

// The D3 passes are VALU-bound (112 / 397 / 147 instructions per list slot measured with IEEE division, sqrtf and expf):
// single-instruction reciprocal, square root and exp2 (1 ulp each) are ample for a term whose parity gate is 6e-6 eV on 7 eV.
__device__ __forceinline__ float frcp(float x) { return __builtin_amdgcn_rcpf(x); }
__device__ __forceinline__ float fexp(float x) { return __builtin_amdgcn_exp2f(x * 1.4426950408889634f); }

// PairAcc / pair_add / pair_store live in model.hip; the same accumulation contract is restated here
struct D3Acc {
  double e = 0.0;   // dispersion pair energies (Hartree)
  double ec = 0.0;  // DSF Coulomb pair terms w q_i q_j when the two share one pass
  float f0 = 0.f, f1 = 0.f, f2 = 0.f;
  float W[9] = {0, 0, 0, 0, 0, 0, 0, 0, 0};
};

template <bool STRESS>
__device__ __forceinline__ void d3_add(D3Acc& A, float t, float ux, float uy, float uz, float d) {
  A.f0 += t * ux;
  A.f1 += t * uy;
  A.f2 += t * uz;
  if (STRESS) {
    const float rx = ux * d, ry = uy * d, rz = uz * d;
    A.W[0] += rx * t * ux; A.W[1] += rx * t * uy; A.W[2] += rx * t * uz;
    A.W[3] += ry * t * ux; A.W[4] += ry * t * uy; A.W[5] += ry * t * uz;
    A.W[6] += rz * t * ux; A.W[7] += rz * t * uy; A.W[8] += rz * t * uz;
  }
}

// E = k sum_ordered e  ->  dE/dx_i = -2k sum_j e' u_ij ,  dE/deps_ab = k sum_ordered e' r_a u_b   (as coulomb pair_store)
template <bool GRAD, bool STRESS>
__device__ __forceinline__ void d3_store(D3Acc& A, int i, int lane, float k, double* ecoul, float* fgrad, float* virial_atom,
                                         double kc = 0.0) {
  // (fma written out: the energy must not depend on how the compiler contracts each <GRAD, STRESS> instantiation)
  const double e = kc != 0.0 ? fma(kc / (double)k, wave_sum(A.ec), wave_sum(A.e)) : wave_sum(A.e);
  float f0 = 0.f, f1 = 0.f, f2 = 0.f;
  if (GRAD) {
    f0 = wave_sum(A.f0);
    f1 = wave_sum(A.f1);
    f2 = wave_sum(A.f2);
    if (STRESS) {
#pragma unroll
      for (int q = 0; q < 9; ++q) A.W[q] = wave_sum(A.W[q]);
    }
  }
  if (lane == 0) {
    ecoul[i] = fma((double)k, e, ecoul[i]);
    if (GRAD) {
      fgrad[3 * i + 0] += -2.0f * k * f0;
      fgrad[3 * i + 1] += -2.0f * k * f1;
      fgrad[3 * i + 2] += -2.0f * k * f2;
    }
  }
  if (GRAD && STRESS && lane < 9) {
    float v = A.W[0];
#pragma unroll
    for (int q = 1; q < 9; ++q) v = (lane == q) ? A.W[q] : v;
    virial_atom[(size_t)i * 9 + lane] += k * v;
  }
}

struct D3Pair {
  float ux, uy, uz, d;  // unit vector i -> j and distance in Angstrom
  int j, sj;            // neighbour atom and its species slot
  bool ok;
};

// xs4[j] = (x, y, z, slot as int bits), packed by d3_pack_kernel: one 16-byte gather per neighbour.
// Cell row vectors of the centre atom's system in registers (zeros when non-periodic: the shift codes are 0 then).
struct D3Cell {
  float m[9];
  __device__ __forceinline__ D3Cell(const float* c) {
#pragma unroll
    for (int k = 0; k < 9; ++k) m[k] = c ? c[k] : 0.0f;
  }
};

// Pair geometry from the gathered neighbour record and the packed lattice shift.  The list loops below issue the loads of
// TWO list slots (entry -> xs4[j] -> per-neighbour data) before any arithmetic and are branch-free inside, so two
// dependent-load chains overlap per wave; out-of-range slots are clamped to a valid one and masked out.
__device__ __forceinline__ D3Pair d3_geom(const float4& xj, int j, int sh, const D3Cell& C, float xi, float yi, float zi,
                                          float cutoff, bool valid) {
  D3Pair r;
  r.j = j;
  r.sj = __float_as_int(xj.w);
  int sx, sy, sz;
  unpack_shift(sh, sx, sy, sz);
  const float rx = (xj.x - xi) + (sx * C.m[0] + sy * C.m[3] + sz * C.m[6]);
  const float ry = (xj.y - yi) + (sx * C.m[1] + sy * C.m[4] + sz * C.m[7]);
  const float rz = (xj.z - zi) + (sx * C.m[2] + sy * C.m[5] + sz * C.m[8]);
  const float d2 = fmaxf(rx * rx + ry * ry + rz * rz, 1e-24f);
  const float inv = __builtin_amdgcn_rsqf(d2);
  r.d = d2 * inv;
  r.ux = rx * inv;
  r.uy = ry * inv;
  r.uz = rz * inv;
  r.ok = valid && r.d < cutoff;
  return r;
}

__global__ void d3_pack_kernel(const float* __restrict__ xw, const int* __restrict__ aslot, int n_atoms, float4* __restrict__ xs4) {
  const int i = blockIdx.x * 256 + threadIdx.x;
  if (i < n_atoms) xs4[i] = make_float4(xw[3 * i], xw[3 * i + 1], xw[3 * i + 2], __int_as_float(aslot[i]));
}

// ------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void d3_cn_kernel(const float4* __restrict__ xs4, const int* __restrict__ mol_idx,
                                                   const float* __restrict__ cell, int n_cell,
                                                   const int* __restrict__ nb_idx,
                                                   const int* __restrict__ nb_shift, const int* __restrict__ nb_cnt, int cap,
                                                   D3Tables T, float cutoff, int n_atoms, float* __restrict__ d3w) {
  const int i = blockIdx.x * 4 + (threadIdx.x >> 6);
  if (i >= n_atoms) return;
  const int lane = threadIdx.x & 63;
  const float* c = cell ? cell + (n_cell == 1 ? 0 : (size_t)mol_idx[i] * 9) : nullptr;
  const float4 x4 = xs4[i];
  const float xi = x4.x, yi = x4.y, zi = x4.z;
  const int si = __float_as_int(x4.w);
  const float rci = T.rcov[si];
  const int cnt = nb_cnt[i];
  float cn = 0.0f;
  const D3Cell C(c);
  const size_t row = (size_t)i * cap;
  for (int m = lane; m < cnt; m += 64 * D3_SLOTS) {  // D3_SLOTS list slots per trip, their load chains issued together
    int j[D3_SLOTS], h[D3_SLOTS];
    bool v[D3_SLOTS];
    float4 x[D3_SLOTS];
    float rc[D3_SLOTS];
#pragma unroll
    for (int k = 0; k < D3_SLOTS; ++k) {
      v[k] = m + 64 * k < cnt;
      const size_t p = row + (v[k] ? m + 64 * k : m);
      j[k] = nb_idx[p];
      h[k] = c ? nb_shift[p] : 0;
    }
#pragma unroll
    for (int k = 0; k < D3_SLOTS; ++k) x[k] = xs4[j[k]];
#pragma unroll
    for (int k = 0; k < D3_SLOTS; ++k) rc[k] = T.rcov[__float_as_int(x[k].w)];
#pragma unroll
    for (int k = 0; k < D3_SLOTS; ++k) {
      const D3Pair P = d3_geom(x[k], j[k], h[k], C, xi, yi, zi, cutoff, v[k]);
      const float t = frcp(1.0f + fexp(-16.0f * ((rci + rc[k]) * frcp(fmaxf(P.d * BOHR_INV_F, 1e-12f)) - 1.0f)));
      cn += P.ok ? t : 0.0f;
    }
  }
  cn = wave_sum(cn);
  // the five reference-system exponents of atom i, shifted by their maximum (every lane computes all five)
  const int nref = T.nref[si];
  float e[5], mx = -1e30f;
#pragma unroll
  for (int a = 0; a < 5; ++a) {
    const float dc = cn - T.cnref[si * 5 + a];
    e[a] = a < nref ? -4.0f * dc * dc : -1e30f;
    mx = fmaxf(mx, e[a]);
  }
#pragma unroll
  for (int a = 0; a < 5; ++a) {
    if (lane == a) {
      const float sa = a < nref ? e[a] - mx : -1e30f;
      d3w[(size_t)i * D3W + a] = sa;
      d3w[(size_t)i * D3W + 5 + a] = a < nref ? expf(sa) : 0.0f;
    }
  }
  if (lane == 5) d3w[(size_t)i * D3W + 10] = cn;
  if (lane == 6) d3w[(size_t)i * D3W + 11] = 0.0f;
}

// ------------------------------------------------------------------------------------------------
template <bool GRAD, bool STRESS, bool DSF>
__global__ __launch_bounds__(256) void d3_pair_kernel(const float4* __restrict__ xs4, const int* __restrict__ mol_idx,
                                                     const float* __restrict__ cell, int n_cell,
                                                     const int* __restrict__ nb_idx,
                                                     const int* __restrict__ nb_shift, const int* __restrict__ nb_cnt, int cap,
                                                     D3Tables T, D3Params P3, float cutoff, int n_atoms,
                                                     const float* __restrict__ d3w, double* __restrict__ ecoul,
                                                     float* __restrict__ fgrad, float* __restrict__ virial_atom,
                                                     float* __restrict__ dEdcn, CoulombParams cp,
                                                     const float* __restrict__ q, float* __restrict__ qbar) {
  // DSF = true: the damped-shifted-force Coulomb pair terms (model.hip coulomb_dsf_kernel, same arithmetic) ride on this
  // pass - one list traversal and one geometry evaluation for both long-range terms when their cutoffs agree.
  extern __shared__ float c6lds[];  // [4 waves][ns][25]: the C6 reference block of the centre's species against every slot
  const int wid = threadIdx.x >> 6, lane = threadIdx.x & 63;
  const int i = blockIdx.x * 4 + wid;
  if (i >= n_atoms) return;
  const int ns = T.ns;
  float* c6s = c6lds + (size_t)wid * ns * 25;
  const float4 x4 = xs4[i];
  const int si = __float_as_int(x4.w);
  for (int k = lane; k < ns * 25; k += 64) c6s[k] = T.c6slot[(size_t)si * ns * 25 + k];
  __builtin_amdgcn_wave_barrier();
  const float* c = cell ? cell + (n_cell == 1 ? 0 : (size_t)mol_idx[i] * 9) : nullptr;
  const float xi = x4.x, yi = x4.y, zi = x4.z;
  const int nref_i = T.nref[si];
  float s_i[5], w_i[5], g_i[5];
  const float cn_i = d3w[(size_t)i * D3W + 10];
#pragma unroll
  for (int a = 0; a < 5; ++a) {
    s_i[a] = d3w[(size_t)i * D3W + a];
    w_i[a] = d3w[(size_t)i * D3W + 5 + a];
    g_i[a] = -8.0f * (cn_i - T.cnref[si * 5 + a]);  // d log w_i[a] / d cn_i (the max shift cancels in the ratio)
  }
  const float q_i = T.r4r2[si];
  const int cnt = nb_cnt[i];
  D3Acc A;
  float dcn = 0.0f, qb = 0.0f;
  const float al = cp.dsf_alpha, Rc = cp.dsf_rc;
  const float two_a_sqrtpi = 2.0f * al * 0.56418958354775629f;
  float sv = 0.f, slope = 0.f, qc_i = 0.f;
  const float kratio = cp.factor / HALF_HARTREE_F;  // Coulomb terms are accumulated in units of the D3 prefactor
  if (DSF) {
    const float erfc_rc = erfcf(al * Rc);
    sv = erfc_rc / Rc;
    slope = erfc_rc / (Rc * Rc) + two_a_sqrtpi * expf(-al * al * Rc * Rc) / Rc;
    qc_i = q[i];
  }
  const D3Cell C(c);
  const size_t row = (size_t)i * cap;
  // ONE arithmetic form for every instantiation: the pair energy is the same number whether or not the gradient terms are formed
  // beside it (an energy-only evaluation returns the bits of a force evaluation, tests/test_gpu_request_kinds.py).  With the
  // multiply-adds left to the compiler's contraction the <GRAD = false> and <GRAD = true> energies differed by 3e-8 - 7e-8 eV per
  // system (one rounding of the dispersion energy).  The likely cause - not pinned to one instruction - is that contraction and
  // scheduling are decided per instantiation and the GRAD terms add uses to the shared subexpressions; what is established is
  // that this form removes the difference: no contraction in this body, every fused multiply-add written out.
  auto body = [&](const D3Pair& P, const float4& sj0, const float4& sj1, const float2& sj2, float qj) {
#pragma clang fp contract(off)
    const int sj = P.sj;
    const float s_j[5] = {sj0.x, sj0.y, sj0.z, sj0.w, sj1.x};
    const float w_j[5] = {sj1.y, sj1.z, sj1.w, sj2.x, sj2.y};
    const float* cr = c6s + sj * 25;
    // sum_ab c6ref_ab w_i[a] w_j[b] [kept]: inner sums over b first, so the centre's weights enter once per a
    float N = 0.f, D = 0.f, G = 0.f, H = 0.f;
#pragma unroll
    for (int a = 0; a < 5; ++a) {
      // (a reference of the CENTRE whose log-weight is below the -12 cut on its own fails the pair cut s_i[a] + s_j[b] >= -12 for
      // every b, s_j <= 0: skipped for the whole wave - typically three or four of the five)
      if (a < nref_i && s_i[a] >= -12.0f) {
        float sb = 0.f, tb = 0.f;
#pragma unroll
        for (int b = 0; b < 5; ++b) {
          const float c6r = cr[a * 5 + b];
          const float w = (s_i[a] + s_j[b] >= -12.0f && c6r != 0.0f) ? w_j[b] : 0.0f;
          sb = fmaf(c6r, w, sb);
          tb += w;
        }
        N = fmaf(w_i[a], sb, N);
        D = fmaf(w_i[a], tb, D);
        if (GRAD) {
          const float wg = w_i[a] * g_i[a];
          G = fmaf(wg, sb, G);
          H = fmaf(wg, tb, H);
        }
      }
    }
    const bool has = D > 1.0e-12f;
    const float invD = frcp(fmaxf(D, 1.0e-12f));
    const float c6 = has ? N * invD : 0.0f;
    const float db = fmaxf(P.d * BOHR_INV_F, 1e-12f);
    const float qq = 3.0f * q_i * T.r4r2[sj];
    const float r0 = fmaf(P3.a1, __builtin_amdgcn_sqrtf(qq), P3.a2);
    const float d2 = db * db, d4 = d2 * d2, d6 = d4 * d2, d8 = d4 * d4;
    const float r2 = r0 * r0, r4 = r2 * r2, r6 = r4 * r2, r8 = r4 * r4;
    const float i6 = frcp(d6 + r6), i8 = frcp(d8 + r8);
    const float damp = fmaf(P3.s6, i6, P3.s8 * qq * i8);
    float sw = 1.0f, dsw = 0.0f;
    if (P3.r_off > P3.r_on && db > P3.r_on) {
      const float iw = frcp(P3.r_off - P3.r_on);
      const float t = fminf(fmaxf((db - P3.r_on) * iw, 0.0f), 1.0f);
      const float t2 = t * t;
      sw = fmaf(-(t2 * t), fmaf(6.0f, t2, fmaf(-15.0f, t, 10.0f)), 1.0f);
      dsw = -30.0f * t2 * (fmaf(-2.0f, t, 1.0f) + t2) * iw;
    }
    A.e += (double)(-c6 * damp * sw);
    float tc = 0.0f;
    if (DSF) {
      const float inv = frcp(P.d);
      // erfc(x) = exp(-x^2) t P(t), t = 1 / (1 + x / 2): the degree-9 fit of the list-free walk (model.hip, coulomb_dsf_walk_kernel:
      // 6.5e-9 relative + 2.5e-7 of the fp32 Horner evaluation, the class of erfcf itself) - one exponential serves the value and
      // the derivative, where erfcf() and a second exponential cost ~40 instructions more per list slot
      const float ex = fexp(-al * al * P.d * P.d);
      const float tt = frcp(fmaf(0.5f * al, P.d, 1.0f));
      float pe = 2.672036890e-02f;
      pe = fmaf(pe, tt, -2.020067459e-01f);
      pe = fmaf(pe, tt, 6.150174393e-01f);
      pe = fmaf(pe, tt, -9.195323909e-01f);
      pe = fmaf(pe, tt, 6.300562657e-01f);
      pe = fmaf(pe, tt, -2.111610618e-01f);
      pe = fmaf(pe, tt, 2.648643249e-01f);
      pe = fmaf(pe, tt, 2.301390953e-01f);
      pe = fmaf(pe, tt, 2.838921720e-01f);
      pe = fmaf(pe, tt, 2.820105286e-01f);
      const float ec = pe * tt * ex;
      const float w = fmaf(P.d - Rc, slope, fmaf(ec, inv, -sv));
      A.ec += (double)(w * qc_i * qj);
      if (GRAD) {
        qb = fmaf(w, qj, qb);
        tc = kratio * fmaf(-ec * inv, inv, fmaf(-two_a_sqrtpi * ex, inv, slope)) * qc_i * qj;
      }
    }
    if (GRAD) {
      const float ddamp = fmaf(-8.0f * P3.s8 * qq * d6 * db * i8, i8, -6.0f * P3.s6 * d4 * db * i6 * i6);
      const float de = -c6 * fmaf(ddamp, sw, damp * dsw) * BOHR_INV_F;  // d e_ij / d d_ij per Angstrom, C6 held fixed
      d3_add<STRESS>(A, de + tc, P.ux, P.uy, P.uz, P.d);
      if (has) dcn = fmaf(-damp * sw * fmaf(-c6, H, G), invD, dcn);
    }
  };
  for (int m = lane; m < cnt; m += 128) {  // two list slots per trip, all of their loads issued before the arithmetic
    const bool v1 = m + 64 < cnt;
    const int m1 = v1 ? m + 64 : m;
    const int j0 = nb_idx[row + m], j1 = nb_idx[row + m1];
    const int h0 = c ? nb_shift[row + m] : 0, h1 = c ? nb_shift[row + m1] : 0;
    const float4 x0 = xs4[j0], x1 = xs4[j1];
    const float* w0 = d3w + (size_t)j0 * D3W;
    const float* w1 = d3w + (size_t)j1 * D3W;
    const float4 a0 = *reinterpret_cast<const float4*>(w0), b0 = *reinterpret_cast<const float4*>(w0 + 4);
    const float2 c0 = *reinterpret_cast<const float2*>(w0 + 8);
    const float4 a1 = *reinterpret_cast<const float4*>(w1), b1 = *reinterpret_cast<const float4*>(w1 + 4);
    const float2 c1 = *reinterpret_cast<const float2*>(w1 + 8);
    float q0 = 0.f, q1 = 0.f;
    if (DSF) {
      q0 = q[j0];
      q1 = q[j1];
    }
    const D3Pair P0 = d3_geom(x0, j0, h0, C, xi, yi, zi, cutoff, true);
    const D3Pair P1 = d3_geom(x1, j1, h1, C, xi, yi, zi, cutoff, v1);
    if (P0.ok) body(P0, a0, b0, c0, q0);
    if (P1.ok) body(P1, a1, b1, c1, q1);
  }
  d3_store<GRAD, STRESS>(A, i, lane, HALF_HARTREE_F, ecoul, fgrad, virial_atom, DSF ? (double)cp.factor : 0.0);
  if (DSF) {  // self term and dE/dq_i of the DSF sum (lr.py:606-613)
    const float cs = -(sv * 0.5f + al * 0.56418958354775629f);
    if (GRAD) qb = wave_sum(qb);
    if (lane == 0) {
      ecoul[i] = fma(2.0 * (double)cp.factor, (double)(cs * qc_i * qc_i), ecoul[i]);
      if (GRAD) qbar[i] += 2.0f * cp.factor * qb + 4.0f * cp.factor * cs * qc_i;
    }
  }
  if (GRAD) {
    dcn = wave_sum(dcn);
    if (lane == 0) dEdcn[i] = 2.0f * HALF_HARTREE_F * dcn;  // e_ij and e_ji both depend on cn_i, symmetrically
  }
}

// ------------------------------------------------------------------------------------------------
template <bool STRESS>
__global__ __launch_bounds__(256) void d3_cnforce_kernel(const float4* __restrict__ xs4, const int* __restrict__ mol_idx,
                                                        const float* __restrict__ cell, int n_cell,
                                                        const int* __restrict__ nb_idx,
                                                        const int* __restrict__ nb_shift, const int* __restrict__ nb_cnt,
                                                        int cap, D3Tables T, float cutoff, int n_atoms,
                                                        const float* __restrict__ dEdcn, double* __restrict__ ecoul,
                                                        float* __restrict__ fgrad, float* __restrict__ virial_atom) {
  const int i = blockIdx.x * 4 + (threadIdx.x >> 6);
  if (i >= n_atoms) return;
  const int lane = threadIdx.x & 63;
  const float* c = cell ? cell + (n_cell == 1 ? 0 : (size_t)mol_idx[i] * 9) : nullptr;
  const float4 x4 = xs4[i];
  const float xi = x4.x, yi = x4.y, zi = x4.z;
  const float rci = T.rcov[__float_as_int(x4.w)];
  const float gi = dEdcn[i];
  const int cnt = nb_cnt[i];
  D3Acc A;
  const D3Cell C(c);
  const size_t row = (size_t)i * cap;
  auto term = [&](const D3Pair& P, float rcj, float gj) {
    const float R = rci + rcj;
    const float idb = frcp(fmaxf(P.d * BOHR_INV_F, 1e-12f));
    const float sg = frcp(1.0f + fexp(-16.0f * (R * idb - 1.0f)));
    const float dsg = sg * (1.0f - sg) * (-16.0f * R * idb * idb) * BOHR_INV_F;  // d sigma / d d_ij per Angstrom
    // sum_l dE/dcn_l cn_l as a pair "energy" with k = 1: per ordered pair 1/2 (g_i + g_j) sigma(d_ij)
    d3_add<STRESS>(A, P.ok ? 0.5f * (gi + gj) * dsg : 0.0f, P.ux, P.uy, P.uz, P.d);
  };
  for (int m = lane; m < cnt; m += 64 * D3_SLOTS) {
    int j[D3_SLOTS], h[D3_SLOTS];
    bool v[D3_SLOTS];
    float4 x[D3_SLOTS];
    float rc[D3_SLOTS], g[D3_SLOTS];
#pragma unroll
    for (int k = 0; k < D3_SLOTS; ++k) {
      v[k] = m + 64 * k < cnt;
      const size_t p = row + (v[k] ? m + 64 * k : m);
      j[k] = nb_idx[p];
      h[k] = c ? nb_shift[p] : 0;
    }
#pragma unroll
    for (int k = 0; k < D3_SLOTS; ++k) {
      x[k] = xs4[j[k]];
      g[k] = dEdcn[j[k]];
    }
#pragma unroll
    for (int k = 0; k < D3_SLOTS; ++k) rc[k] = T.rcov[__float_as_int(x[k].w)];
#pragma unroll
    for (int k = 0; k < D3_SLOTS; ++k) term(d3_geom(x[k], j[k], h[k], C, xi, yi, zi, cutoff, v[k]), rc[k], g[k]);
  }
  d3_store<true, STRESS>(A, i, lane, 1.0f, ecoul, fgrad, virial_atom);
}

// ------------------------------------------------------------------------------------------------
int launch_dftd3(hipStream_t s, bool grad, bool stress, const float* xw, const int* mol_idx, const float* cell, int n_cell,
                 const int* aslot, const int* nb_idx, const int* nb_shift, const int* nb_cnt, int cap, D3Tables T, D3Params P,
                 float cutoff, int n_atoms, float4* xs4, float* d3w, float* dEdcn, double* ecoul, float* fgrad,
                 float* virial_atom, bool with_dsf, CoulombParams cp, const float* q, float* qbar, bool cn_done, const DdLink* dd) {
  hipLaunchKernelGGL(d3_pack_kernel, dim3(ceil_div(n_atoms, 256)), dim3(256), 0, s, xw, aslot, n_atoms, xs4);
  AIMNET_LAUNCH_CHECK();
  dim3 grid(ceil_div(n_atoms, 4)), block(256);
  if (!cn_done) {  // (otherwise the list build left cn_i and the weights in d3w: kernels.h, D3CnRider)
    hipLaunchKernelGGL(d3_cn_kernel, grid, block, 0, s, xs4, mol_idx, cell, n_cell, nb_idx, nb_shift, nb_cnt, cap, T, cutoff, n_atoms,
                       d3w);
    AIMNET_LAUNCH_CHECK();
  }
  // domain decomposition: the coordination number (and with it the reference weights) of a halo copy is exact only if its own
  // 15 A neighbourhood is inside the cluster - the owners' rows come in through the exchange function, and so does dE/dcn below
  // (for an owned centre both are complete: the pair pass forms both directions of a pair at the centre)
  if (dd && dd->fn(dd->ctx, 2 /* AIMNET_DD_ROWS */, d3w, (int64_t)D3W * n_atoms, (void*)s) != 0) {
    set_last_error("eval: the domain-decomposition exchange function failed (DFT-D3 weights)");
    return -1;
  }
  const size_t lds = (size_t)4 * T.ns * 25 * sizeof(float);
#define AIMNET_D3_PAIR(G_, S_, C_)                                                                                             \
  hipLaunchKernelGGL((d3_pair_kernel<G_, S_, C_>), grid, block, lds, s, xs4, mol_idx, cell, n_cell, nb_idx, nb_shift, nb_cnt, cap, \
                     T, P, cutoff, n_atoms, d3w, ecoul, fgrad, virial_atom, dEdcn, cp, q, qbar)
  if (with_dsf) {
    if (grad && stress) AIMNET_D3_PAIR(true, true, true);
    else if (grad) AIMNET_D3_PAIR(true, false, true);
    else AIMNET_D3_PAIR(false, false, true);
  } else {
    if (grad && stress) AIMNET_D3_PAIR(true, true, false);
    else if (grad) AIMNET_D3_PAIR(true, false, false);
    else AIMNET_D3_PAIR(false, false, false);
  }
#undef AIMNET_D3_PAIR
  AIMNET_LAUNCH_CHECK();
  if (grad && dd && dd->fn(dd->ctx, 2 /* AIMNET_DD_ROWS */, dEdcn, (int64_t)n_atoms, (void*)s) != 0) {
    set_last_error("eval: the domain-decomposition exchange function failed (DFT-D3 dE/dcn)");
    return -1;
  }
  if (grad) {
    if (stress)
      hipLaunchKernelGGL(d3_cnforce_kernel<true>, grid, block, 0, s, xs4, mol_idx, cell, n_cell, nb_idx, nb_shift, nb_cnt, cap, T,
                         cutoff, n_atoms, dEdcn, ecoul, fgrad, virial_atom);
    else
      hipLaunchKernelGGL(d3_cnforce_kernel<false>, grid, block, 0, s, xs4, mol_idx, cell, n_cell, nb_idx, nb_shift, nb_cnt, cap, T,
                         cutoff, n_atoms, dEdcn, ecoul, fgrad, virial_atom);
    AIMNET_LAUNCH_CHECK();
  }
  return 0;
}

// ================================================================================================
// The tangent of the term's gradient along K directions v^k [K][N][3] (the cell is fixed): H_d3 v^k, ADDED onto txbar [K][N][3].
// The analytic dispersion block of the Hessian sweep (hvp.hip, armed by aimnet_engine_set_dftd3_tangent); the formulas are restated in
// include/aimnet_hip.h and, in numpy float64, in tests/d3_tangent_yardstick.py::closed_form.  launch_dftd3(grad = true) has run at x
// on the same list: xs4, d3w (shifted exponents, weights, cn) and dEdcn (G) are its outputs.
//
// Three passes mirror the primal ones - a wave per atom, lanes over list slots, the loads of two list slots issued before the
// arithmetic, the cell in registers, wave_sum, no atomics - with the two all-atom dependencies between them:
//   d3_tcn_kernel       t_cn_i = sum_j sigma' t_d                                   -> tcn4 [K][N] = (v_i, t_cn_i)
//   d3_tpair_kernel     C6 and its derivatives A_i A_j B_ii B_ij (centred moments), P P' P'' once per pair; per direction the direct pair term onto txbar and
//                       t_G_i                                                       -> tg4 [K][N] = (v_i, t_G_i)
//   d3_tcnforce_kernel  (t_G_i + t_G_j) sigma' u + (G_i + G_j)(sigma'' t_d u + sigma' t_u) onto txbar
// (the direction rides in the float4 of the quantity the NEXT pass gathers per neighbour: one 16-byte gather per neighbour and direction).
// A wave holds D3_KG directions (grid.y = groups of D3_KG): geometry, sigma and P with their derivatives and the C6 sums are formed
// once per pair and group.  Every direction owns its accumulators and runs the same instruction sequence whatever slot of a group it
// sits in - ONE instantiation, no contraction in the bodies, every fused multiply-add written out - so H v^k is bitwise repeatable and
// does not depend on how the directions are grouped or split into sweeps.  All sums are fp32 (a lane adds ~10 terms, wave_sum is a tree).
//
// STRAIN (armed, aimnet_engine_set_strain_terms with the strain tangent of hvp.hip): instantiations of their own, the unarmed ones are the
// code they were.  Direction k carries eps_k [9] (row-major, wave-uniform: scalar registers) and the pair tangent becomes t_r = v_j - v_i
// + r eps_k, whatever image the pair was found in; t_d, t_u and everything downstream keep their form.  The pair pass and the cn-force
// pass add, beside the tangent increment t_inc of a pair to txbar, the centre's share of the virial tangent in the VirAcc convention of
// hvp.hip (9 floats, row = component of r, column = component of the gradient), -1/2 sum_pairs (t_r (x) inc + r (x) t_inc), onto tvir
// [K][N][9] - wave_sum, lane q of the group writes, no atomics.  The primal share -1/2 sum_pairs r (x) inc is launch_dftd3's
// virial_atom (stress = true): the same layout and sign, added onto vir [N][9] by the block's primal launch.
constexpr int D3_KG = 4;

struct D3Dirs {  // the directions of this wave's group, clamped to the first one beyond K (computed, never stored)
  int k[D3_KG];
  bool ok[D3_KG];
  __device__ __forceinline__ D3Dirs(int group, int K) {
#pragma unroll
    for (int q = 0; q < D3_KG; ++q) {
      ok[q] = group * D3_KG + q < K;
      k[q] = ok[q] ? group * D3_KG + q : group * D3_KG;
    }
  }
};

// armed: eps of the group's directions; the addresses are uniform over the wave, so the 9 x D3_KG values live in scalar registers
template <bool STRAIN>
struct D3Eps {
  float e[STRAIN ? D3_KG : 1][9];
  __device__ __forceinline__ D3Eps(const D3Dirs& G, const float* __restrict__ strain) {
    if constexpr (STRAIN) {
#pragma unroll
      for (int q = 0; q < D3_KG; ++q)
#pragma unroll
        for (int c = 0; c < 9; ++c) e[q][c] = strain[(size_t)G.k[q] * 9 + c];
    }
  }
};
// r eps (row vector times matrix), every fused multiply-add written out
__device__ __forceinline__ void d3_r_eps(const float (&e)[9], float rx, float ry, float rz, float& ox, float& oy, float& oz) {
#pragma clang fp contract(off)
  ox = fmaf(rx, e[0], fmaf(ry, e[3], rz * e[6]));
  oy = fmaf(rx, e[1], fmaf(ry, e[4], rz * e[7]));
  oz = fmaf(rx, e[2], fmaf(ry, e[5], rz * e[8]));
}
// armed: a pair's share of the virial tangent, tw += t_r (x) (c2 u) + r (x) tf with tf = c1 u + c2 t_u the pair's tangent increment
__device__ __forceinline__ void d3_tvir_add(float (&tw)[9], const float (&r)[3], const float (&tr)[3], const float (&inc)[3],
                                            const float (&tf)[3]) {
#pragma clang fp contract(off)
#pragma unroll
  for (int a = 0; a < 3; ++a)
#pragma unroll
    for (int b = 0; b < 3; ++b) tw[a * 3 + b] = fmaf(tr[a], inc[b], fmaf(r[a], tf[b], tw[a * 3 + b]));
}

template <bool STRAIN>
__global__ __launch_bounds__(256) void d3_tcn_kernel(const float4* __restrict__ xs4, const int* __restrict__ mol_idx,
                                                    const float* __restrict__ cell, int n_cell, const int* __restrict__ nb_idx,
                                                    const int* __restrict__ nb_shift, const int* __restrict__ nb_cnt, int cap,
                                                    D3Tables T, float cutoff, int n_atoms, const float* __restrict__ tv, int K,
                                                    float4* __restrict__ tcn4, const float* __restrict__ strain) {
  const int i = blockIdx.x * 4 + (threadIdx.x >> 6);
  if (i >= n_atoms) return;
  const int lane = threadIdx.x & 63;
  const D3Dirs G(blockIdx.y, K);
  const D3Eps<STRAIN> E(G, strain);
  const float* c = cell ? cell + (n_cell == 1 ? 0 : (size_t)mol_idx[i] * 9) : nullptr;
  const float4 x4 = xs4[i];
  const float xi = x4.x, yi = x4.y, zi = x4.z;
  const float rci = T.rcov[__float_as_int(x4.w)];
  const int cnt = nb_cnt[i];
  float vi[D3_KG][3], acc[D3_KG];
#pragma unroll
  for (int q = 0; q < D3_KG; ++q) {
    const float* v = tv + ((size_t)G.k[q] * n_atoms + i) * 3;
    vi[q][0] = v[0], vi[q][1] = v[1], vi[q][2] = v[2];
    acc[q] = 0.0f;
  }
  const D3Cell C(c);
  const size_t row = (size_t)i * cap;
  auto term = [&](const D3Pair& P, float rcj, const float (&vj)[D3_KG][3]) {
#pragma clang fp contract(off)
    const float R = rci + rcj;
    const float idb = frcp(fmaxf(P.d * BOHR_INV_F, 1e-12f));
    const float sg = frcp(1.0f + fexp(-16.0f * (R * idb - 1.0f)));
    const float dsg = P.ok ? sg * (1.0f - sg) * (-16.0f * R * idb * idb) * BOHR_INV_F : 0.0f;  // d sigma / d d_ij per Angstrom
#pragma unroll
    for (int q = 0; q < D3_KG; ++q) {
      if constexpr (STRAIN) {
        float ex, ey, ez;
        d3_r_eps(E.e[q], P.ux * P.d, P.uy * P.d, P.uz * P.d, ex, ey, ez);
        const float dx = (vj[q][0] - vi[q][0]) + ex, dy = (vj[q][1] - vi[q][1]) + ey, dz = (vj[q][2] - vi[q][2]) + ez;
        const float td = fmaf(P.ux, dx, fmaf(P.uy, dy, P.uz * dz));
        acc[q] = fmaf(dsg, td, acc[q]);
      } else {
        const float td = fmaf(P.ux, vj[q][0] - vi[q][0], fmaf(P.uy, vj[q][1] - vi[q][1], P.uz * (vj[q][2] - vi[q][2])));
        acc[q] = fmaf(dsg, td, acc[q]);
      }
    }
  };
  for (int m = lane; m < cnt; m += 128) {  // two list slots per trip, all of their loads issued before the arithmetic
    const bool v1 = m + 64 < cnt;
    const int m1 = v1 ? m + 64 : m;
    const int j0 = nb_idx[row + m], j1 = nb_idx[row + m1];
    const int h0 = c ? nb_shift[row + m] : 0, h1 = c ? nb_shift[row + m1] : 0;
    const float4 x0 = xs4[j0], x1 = xs4[j1];
    float w0[D3_KG][3], w1[D3_KG][3];
#pragma unroll
    for (int q = 0; q < D3_KG; ++q) {
      const float* p0 = tv + ((size_t)G.k[q] * n_atoms + j0) * 3;
      const float* p1 = tv + ((size_t)G.k[q] * n_atoms + j1) * 3;
      w0[q][0] = p0[0], w0[q][1] = p0[1], w0[q][2] = p0[2];
      w1[q][0] = p1[0], w1[q][1] = p1[1], w1[q][2] = p1[2];
    }
    const float rc0 = T.rcov[__float_as_int(x0.w)], rc1 = T.rcov[__float_as_int(x1.w)];
    term(d3_geom(x0, j0, h0, C, xi, yi, zi, cutoff, true), rc0, w0);
    term(d3_geom(x1, j1, h1, C, xi, yi, zi, cutoff, v1), rc1, w1);
  }
#pragma unroll
  for (int q = 0; q < D3_KG; ++q) {
    const float t = wave_sum(acc[q]);
    if (lane == q && G.ok[q]) tcn4[(size_t)G.k[q] * n_atoms + i] = make_float4(vi[q][0], vi[q][1], vi[q][2], t);
  }
}

template <bool STRAIN>
__global__ __launch_bounds__(256) void d3_tpair_kernel(const float4* __restrict__ xs4, const int* __restrict__ mol_idx,
                                                      const float* __restrict__ cell, int n_cell, const int* __restrict__ nb_idx,
                                                      const int* __restrict__ nb_shift, const int* __restrict__ nb_cnt, int cap,
                                                      D3Tables T, D3Params P3, float cutoff, int n_atoms,
                                                      const float* __restrict__ d3w, const float4* __restrict__ tcn4, int K,
                                                      float4* __restrict__ tg4, float* __restrict__ txbar,
                                                      const float* __restrict__ strain, float* __restrict__ tvir) {
  extern __shared__ float c6lds[];  // [4 waves][ns][25], as d3_pair_kernel
  const int wid = threadIdx.x >> 6, lane = threadIdx.x & 63;
  const int i = blockIdx.x * 4 + wid;
  if (i >= n_atoms) return;
  const D3Dirs G(blockIdx.y, K);
  const D3Eps<STRAIN> E(G, strain);
  const int ns = T.ns;
  float* c6s = c6lds + (size_t)wid * ns * 25;
  const float4 x4 = xs4[i];
  const int si = __float_as_int(x4.w);
  for (int k = lane; k < ns * 25; k += 64) c6s[k] = T.c6slot[(size_t)si * ns * 25 + k];
  __builtin_amdgcn_wave_barrier();
  const float* c = cell ? cell + (n_cell == 1 ? 0 : (size_t)mol_idx[i] * 9) : nullptr;
  const float xi = x4.x, yi = x4.y, zi = x4.z;
  const int nref_i = T.nref[si];
  float s_i[5], w_i[5], g_i[5];
  const float cn_i = d3w[(size_t)i * D3W + 10];
#pragma unroll
  for (int a = 0; a < 5; ++a) {
    s_i[a] = d3w[(size_t)i * D3W + a];
    w_i[a] = d3w[(size_t)i * D3W + 5 + a];
    g_i[a] = -8.0f * (cn_i - T.cnref[si * 5 + a]);
  }
  const float q_i = T.r4r2[si];
  const int cnt = nb_cnt[i];
  float4 ti[D3_KG];  // (v_i, t_cn_i) of every direction
  float f[D3_KG][3], tg[D3_KG];
  float tw[STRAIN ? D3_KG : 1][9];  // armed: the virial tangent share of every direction
#pragma unroll
  for (int q = 0; q < D3_KG; ++q) {
    ti[q] = tcn4[(size_t)G.k[q] * n_atoms + i];
    f[q][0] = f[q][1] = f[q][2] = tg[q] = 0.0f;
    if constexpr (STRAIN) {
#pragma unroll
      for (int c = 0; c < 9; ++c) tw[q][c] = 0.0f;
    }
  }
  const D3Cell C(c);
  const size_t row = (size_t)i * cap;
  auto body = [&](const D3Pair& P, const float4& sj0, const float4& sj1, const float4& sj2, const float (&cr_j)[5], float q_j,
                  const float4 (&tj)[D3_KG]) {
#pragma clang fp contract(off)
    const float s_j[5] = {sj0.x, sj0.y, sj0.z, sj0.w, sj1.x};
    const float w_j[5] = {sj1.y, sj1.z, sj1.w, sj2.x, sj2.y};
    const float cn_j = sj2.z;
    float g_j[5];
#pragma unroll
    for (int b = 0; b < 5; ++b) g_j[b] = -8.0f * (cn_j - cr_j[b]);
    const float* cr = c6s + P.sj * 25;
    // The kept (a, b) are the primal's mask, a constant of the evaluation.  With p = W / D, c' = c6ref - C6 and g~ = g - sum p g the
    // combinations of the sums N_., D_. collapse to centred moments (sum p c' = 0 removes the -8 of d_ii W and every mean):
    //   A_i = sum p c' g~_i,  A_j = sum p c' g~_j,  B_ii = sum p c' g~_i^2,  B_ij = sum p c' g~_i g~_j
    // In fp32 the uncentred form (N_ii - C6 D_ii - 2 A_i D_i) / D loses 3 - 6e-5 of max|H v| to cancellation, this one 2 - 6e-6
    // (tests/d3_tangent_yardstick.py).  Two walks over the 5 x 5 block: N, D and the means, then the moments.
    float N = 0.f, D = 0.f, Di = 0.f, Dj = 0.f;
#pragma unroll
    for (int a = 0; a < 5; ++a) {
      if (a < nref_i && s_i[a] >= -12.0f) {
        float sb = 0.f, tb = 0.f, tgs = 0.f;
#pragma unroll
        for (int b = 0; b < 5; ++b) {
          const float c6r = cr[a * 5 + b];
          const float w = (s_i[a] + s_j[b] >= -12.0f && c6r != 0.0f) ? w_j[b] : 0.0f;
          sb = fmaf(c6r, w, sb);
          tb += w;
          tgs = fmaf(w, g_j[b], tgs);
        }
        N = fmaf(w_i[a], sb, N);
        D = fmaf(w_i[a], tb, D);
        Di = fmaf(w_i[a] * g_i[a], tb, Di);
        Dj = fmaf(w_i[a], tgs, Dj);
      }
    }
    const bool has = D > 1.0e-12f;
    const float invD = has ? frcp(fmaxf(D, 1.0e-12f)) : 0.0f;  // (no weight survives: C6 and all of its derivatives are zero)
    const float c6 = N * invD, gim = Di * invD, gjm = Dj * invD;
    float Ai = 0.f, Aj = 0.f, Bii = 0.f, Bij = 0.f;
#pragma unroll
    for (int a = 0; a < 5; ++a) {
      if (a < nref_i && s_i[a] >= -12.0f) {
        float m0 = 0.f, m1 = 0.f;
#pragma unroll
        for (int b = 0; b < 5; ++b) {
          const float c6r = cr[a * 5 + b];
          const float w = (s_i[a] + s_j[b] >= -12.0f && c6r != 0.0f) ? w_j[b] : 0.0f;
          const float wc = w * (c6r - c6);
          m0 += wc;
          m1 = fmaf(wc, g_j[b] - gjm, m1);
        }
        const float gc = g_i[a] - gim, wa = w_i[a] * gc;
        Ai = fmaf(wa, m0, Ai);
        Aj = fmaf(w_i[a], m1, Aj);
        Bii = fmaf(wa * gc, m0, Bii);
        Bij = fmaf(wa, m1, Bij);
      }
    }
    Ai *= invD, Aj *= invD, Bii *= invD, Bij *= invD;
    // P = damp S5 and its first two derivatives (d in Bohr inside, per Angstrom outside)
    const float db = fmaxf(P.d * BOHR_INV_F, 1e-12f);
    const float qq = 3.0f * q_i * q_j;
    const float r0 = fmaf(P3.a1, __builtin_amdgcn_sqrtf(qq), P3.a2);
    const float d2 = db * db, d4 = d2 * d2, d6 = d4 * d2, d8 = d4 * d4;
    const float r2 = r0 * r0, r4 = r2 * r2, r6 = r4 * r2, r8 = r4 * r4;
    const float i6 = frcp(d6 + r6), i8 = frcp(d8 + r8);
    const float k6 = P3.s6 * i6 * i6, k8 = P3.s8 * qq * i8 * i8;
    const float damp = fmaf(P3.s6, i6, P3.s8 * qq * i8);
    const float ddamp = fmaf(-8.0f * k8, d6 * db, -6.0f * k6 * (d4 * db));
    const float d2damp = fmaf(k8 * d6, fmaf(128.0f, d8 * i8, -56.0f), k6 * d4 * fmaf(72.0f, d6 * i6, -30.0f));
    float sw = 1.0f, dsw = 0.0f, d2sw = 0.0f;
    if (P3.r_off > P3.r_on && db > P3.r_on) {
      const float iw = frcp(P3.r_off - P3.r_on);
      const float t = fminf(fmaxf((db - P3.r_on) * iw, 0.0f), 1.0f);
      const float t2 = t * t, omt = 1.0f - t;
      sw = fmaf(-(t2 * t), fmaf(6.0f, t2, fmaf(-15.0f, t, 10.0f)), 1.0f);
      dsw = -30.0f * t2 * (omt * omt) * iw;
      d2sw = -60.0f * t * omt * fmaf(-2.0f, t, 1.0f) * (iw * iw);
    }
    const float P0 = damp * sw;
    const float P1 = fmaf(ddamp, sw, damp * dsw) * BOHR_INV_F;
    const float P2 = fmaf(d2damp, sw, fmaf(2.0f * ddamp, dsw, damp * d2sw)) * (BOHR_INV_F * BOHR_INV_F);
    const float invd = frcp(P.d);
    const float c2 = -(c6 * P1);  // d e_ij / d d_ij, C6 held fixed: multiplies t_u
    const float c6p2 = c6 * P2, p1a = P1 * Ai;
#pragma unroll
    for (int q = 0; q < D3_KG; ++q) {
      if constexpr (STRAIN) {  // t_r = v_j - v_i + r eps; the pair's increments inc = c2 u, t_inc = c1 u + c2 t_u (times -2k at the end)
        const float r[3] = {P.ux * P.d, P.uy * P.d, P.uz * P.d};
        float ex, ey, ez;
        d3_r_eps(E.e[q], r[0], r[1], r[2], ex, ey, ez);
        const float tr[3] = {(tj[q].x - ti[q].x) + ex, (tj[q].y - ti[q].y) + ey, (tj[q].z - ti[q].z) + ez};
        const float td = fmaf(P.ux, tr[0], fmaf(P.uy, tr[1], P.uz * tr[2]));
        const float tci = ti[q].w, tcj = tj[q].w;
        const float tc6 = fmaf(Ai, tci, Aj * tcj);
        const float c1 = fmaf(-tc6, P1, -(c6p2 * td));
        const float inc[3] = {c2 * P.ux, c2 * P.uy, c2 * P.uz};
        const float tf[3] = {fmaf(c1, P.ux, c2 * (fmaf(-P.ux, td, tr[0]) * invd)), fmaf(c1, P.uy, c2 * (fmaf(-P.uy, td, tr[1]) * invd)),
                             fmaf(c1, P.uz, c2 * (fmaf(-P.uz, td, tr[2]) * invd))};
        f[q][0] += tf[0], f[q][1] += tf[1], f[q][2] += tf[2];
        d3_tvir_add(tw[q], r, tr, inc, tf);
        tg[q] = fmaf(-p1a, td, fmaf(-P0, fmaf(Bii, tci, Bij * tcj), tg[q]));
      } else {
        const float dx = tj[q].x - ti[q].x, dy = tj[q].y - ti[q].y, dz = tj[q].z - ti[q].z;
        const float td = fmaf(P.ux, dx, fmaf(P.uy, dy, P.uz * dz));
        const float tci = ti[q].w, tcj = tj[q].w;
        const float tc6 = fmaf(Ai, tci, Aj * tcj);
        const float c1 = fmaf(-tc6, P1, -(c6p2 * td));
        f[q][0] = fmaf(c1, P.ux, fmaf(c2, fmaf(-P.ux, td, dx) * invd, f[q][0]));
        f[q][1] = fmaf(c1, P.uy, fmaf(c2, fmaf(-P.uy, td, dy) * invd, f[q][1]));
        f[q][2] = fmaf(c1, P.uz, fmaf(c2, fmaf(-P.uz, td, dz) * invd, f[q][2]));
        tg[q] = fmaf(-p1a, td, fmaf(-P0, fmaf(Bii, tci, Bij * tcj), tg[q]));
      }
    }
  };
  for (int m = lane; m < cnt; m += 128) {  // two list slots per trip, all of their loads issued before the arithmetic
    const bool v1 = m + 64 < cnt;
    const int m1 = v1 ? m + 64 : m;
    const int j0 = nb_idx[row + m], j1 = nb_idx[row + m1];
    const int h0 = c ? nb_shift[row + m] : 0, h1 = c ? nb_shift[row + m1] : 0;
    const float4 x0 = xs4[j0], x1 = xs4[j1];
    const float4* w0 = reinterpret_cast<const float4*>(d3w + (size_t)j0 * D3W);
    const float4* w1 = reinterpret_cast<const float4*>(d3w + (size_t)j1 * D3W);
    const float4 a0 = w0[0], b0 = w0[1], e0 = w0[2], a1 = w1[0], b1 = w1[1], e1 = w1[2];
    float4 t0[D3_KG], t1[D3_KG];
#pragma unroll
    for (int q = 0; q < D3_KG; ++q) {
      t0[q] = tcn4[(size_t)G.k[q] * n_atoms + j0];
      t1[q] = tcn4[(size_t)G.k[q] * n_atoms + j1];
    }
    const int s0 = __float_as_int(x0.w), s1 = __float_as_int(x1.w);
    float cr0[5], cr1[5];
#pragma unroll
    for (int b = 0; b < 5; ++b) {
      cr0[b] = T.cnref[s0 * 5 + b];
      cr1[b] = T.cnref[s1 * 5 + b];
    }
    const float q0 = T.r4r2[s0], q1 = T.r4r2[s1];
    const D3Pair P0 = d3_geom(x0, j0, h0, C, xi, yi, zi, cutoff, true);
    const D3Pair P1 = d3_geom(x1, j1, h1, C, xi, yi, zi, cutoff, v1);
    if (P0.ok) body(P0, a0, b0, e0, cr0, q0, t0);
    if (P1.ok) body(P1, a1, b1, e1, cr1, q1, t1);
  }
#pragma unroll
  for (int q = 0; q < D3_KG; ++q) {
    const float f0 = wave_sum(f[q][0]), f1 = wave_sum(f[q][1]), f2 = wave_sum(f[q][2]), g = wave_sum(tg[q]);
    if (lane == q && G.ok[q]) {  // E = k sum_ordered e: -2k on the gradient; e_ij and e_ji both depend on cn_i: 2k on t_G
      const size_t o = (size_t)G.k[q] * n_atoms + i;
      txbar[o * 3 + 0] += -2.0f * HALF_HARTREE_F * f0;
      txbar[o * 3 + 1] += -2.0f * HALF_HARTREE_F * f1;
      txbar[o * 3 + 2] += -2.0f * HALF_HARTREE_F * f2;
      tg4[o] = make_float4(ti[q].x, ti[q].y, ti[q].z, 2.0f * HALF_HARTREE_F * g);
    }
    if constexpr (STRAIN) {  // -1/2 (t_r (x) inc + r (x) t_inc) with the -2k of the increments: k times the sums
#pragma unroll
      for (int c = 0; c < 9; ++c) {
        const float w = wave_sum(tw[q][c]);
        if (lane == q && G.ok[q]) tvir[((size_t)G.k[q] * n_atoms + i) * 9 + c] += HALF_HARTREE_F * w;
      }
    }
  }
}

template <bool STRAIN>
__global__ __launch_bounds__(256) void d3_tcnforce_kernel(const float4* __restrict__ xs4, const int* __restrict__ mol_idx,
                                                         const float* __restrict__ cell, int n_cell,
                                                         const int* __restrict__ nb_idx, const int* __restrict__ nb_shift,
                                                         const int* __restrict__ nb_cnt, int cap, D3Tables T, float cutoff,
                                                         int n_atoms, const float* __restrict__ dEdcn,
                                                         const float4* __restrict__ tg4, int K, float* __restrict__ txbar,
                                                         const float* __restrict__ strain, float* __restrict__ tvir) {
  const int i = blockIdx.x * 4 + (threadIdx.x >> 6);
  if (i >= n_atoms) return;
  const int lane = threadIdx.x & 63;
  const D3Dirs G(blockIdx.y, K);
  const D3Eps<STRAIN> E(G, strain);
  const float* c = cell ? cell + (n_cell == 1 ? 0 : (size_t)mol_idx[i] * 9) : nullptr;
  const float4 x4 = xs4[i];
  const float xi = x4.x, yi = x4.y, zi = x4.z;
  const float rci = T.rcov[__float_as_int(x4.w)];
  const float gi = dEdcn[i];
  const int cnt = nb_cnt[i];
  float4 ti[D3_KG];  // (v_i, t_G_i)
  float f[D3_KG][3];
  float tw[STRAIN ? D3_KG : 1][9];  // armed: the virial tangent share of every direction
#pragma unroll
  for (int q = 0; q < D3_KG; ++q) {
    ti[q] = tg4[(size_t)G.k[q] * n_atoms + i];
    f[q][0] = f[q][1] = f[q][2] = 0.0f;
    if constexpr (STRAIN) {
#pragma unroll
      for (int c = 0; c < 9; ++c) tw[q][c] = 0.0f;
    }
  }
  const D3Cell C(c);
  const size_t row = (size_t)i * cap;
  auto term = [&](const D3Pair& P, float rcj, float gj, const float4 (&tj)[D3_KG]) {
#pragma clang fp contract(off)
    const float R = rci + rcj;
    const float idb = frcp(fmaxf(P.d * BOHR_INV_F, 1e-12f));
    const float sg = frcp(1.0f + fexp(-16.0f * (R * idb - 1.0f)));
    const float a1 = -16.0f * R * idb * idb, sp = sg * (1.0f - sg);
    const float s1 = P.ok ? sp * a1 * BOHR_INV_F : 0.0f;  // sigma' and sigma'' per Angstrom (and per Angstrom^2)
    const float s2 = P.ok ? sp * fmaf(fmaf(-2.0f, sg, 1.0f) * a1, a1, 32.0f * R * idb * idb * idb) * (BOHR_INV_F * BOHR_INV_F) : 0.0f;
    const float gs = gi + gj;
    const float c2 = gs * s1, gs2 = gs * s2;
    const float invd = frcp(P.d);
#pragma unroll
    for (int q = 0; q < D3_KG; ++q) {
      if constexpr (STRAIN) {  // as in the pair pass; the increments carry -1 here
        const float r[3] = {P.ux * P.d, P.uy * P.d, P.uz * P.d};
        float ex, ey, ez;
        d3_r_eps(E.e[q], r[0], r[1], r[2], ex, ey, ez);
        const float tr[3] = {(tj[q].x - ti[q].x) + ex, (tj[q].y - ti[q].y) + ey, (tj[q].z - ti[q].z) + ez};
        const float td = fmaf(P.ux, tr[0], fmaf(P.uy, tr[1], P.uz * tr[2]));
        const float c1 = fmaf(ti[q].w + tj[q].w, s1, gs2 * td);
        const float inc[3] = {c2 * P.ux, c2 * P.uy, c2 * P.uz};
        const float tf[3] = {fmaf(c1, P.ux, c2 * (fmaf(-P.ux, td, tr[0]) * invd)), fmaf(c1, P.uy, c2 * (fmaf(-P.uy, td, tr[1]) * invd)),
                             fmaf(c1, P.uz, c2 * (fmaf(-P.uz, td, tr[2]) * invd))};
        f[q][0] += tf[0], f[q][1] += tf[1], f[q][2] += tf[2];
        d3_tvir_add(tw[q], r, tr, inc, tf);
      } else {
        const float dx = tj[q].x - ti[q].x, dy = tj[q].y - ti[q].y, dz = tj[q].z - ti[q].z;
        const float td = fmaf(P.ux, dx, fmaf(P.uy, dy, P.uz * dz));
        const float c1 = fmaf(ti[q].w + tj[q].w, s1, gs2 * td);
        f[q][0] = fmaf(c1, P.ux, fmaf(c2, fmaf(-P.ux, td, dx) * invd, f[q][0]));
        f[q][1] = fmaf(c1, P.uy, fmaf(c2, fmaf(-P.uy, td, dy) * invd, f[q][1]));
        f[q][2] = fmaf(c1, P.uz, fmaf(c2, fmaf(-P.uz, td, dz) * invd, f[q][2]));
      }
    }
  };
  for (int m = lane; m < cnt; m += 128) {
    const bool v1 = m + 64 < cnt;
    const int m1 = v1 ? m + 64 : m;
    const int j0 = nb_idx[row + m], j1 = nb_idx[row + m1];
    const int h0 = c ? nb_shift[row + m] : 0, h1 = c ? nb_shift[row + m1] : 0;
    const float4 x0 = xs4[j0], x1 = xs4[j1];
    const float g0 = dEdcn[j0], g1 = dEdcn[j1];
    float4 t0[D3_KG], t1[D3_KG];
#pragma unroll
    for (int q = 0; q < D3_KG; ++q) {
      t0[q] = tg4[(size_t)G.k[q] * n_atoms + j0];
      t1[q] = tg4[(size_t)G.k[q] * n_atoms + j1];
    }
    const float rc0 = T.rcov[__float_as_int(x0.w)], rc1 = T.rcov[__float_as_int(x1.w)];
    term(d3_geom(x0, j0, h0, C, xi, yi, zi, cutoff, true), rc0, g0, t0);
    term(d3_geom(x1, j1, h1, C, xi, yi, zi, cutoff, v1), rc1, g1, t1);
  }
#pragma unroll
  for (int q = 0; q < D3_KG; ++q) {
    const float f0 = wave_sum(f[q][0]), f1 = wave_sum(f[q][1]), f2 = wave_sum(f[q][2]);
    if (lane == q && G.ok[q]) {
      const size_t o = ((size_t)G.k[q] * n_atoms + i) * 3;
      txbar[o + 0] -= f0;
      txbar[o + 1] -= f1;
      txbar[o + 2] -= f2;
    }
    if constexpr (STRAIN) {  // -1/2 (t_r (x) inc + r (x) t_inc) with the -1 of the increments
#pragma unroll
      for (int c = 0; c < 9; ++c) {
        const float w = wave_sum(tw[q][c]);
        if (lane == q && G.ok[q]) tvir[((size_t)G.k[q] * n_atoms + i) * 9 + c] += 0.5f * w;
      }
    }
  }
}

int launch_dftd3_tangent(hipStream_t s, const int* mol_idx, const float* cell, int n_cell, const int* nb_idx, const int* nb_shift,
                         const int* nb_cnt, int cap, D3Tables T, D3Params P, float cutoff, int n_atoms, const float4* xs4,
                         const float* d3w, const float* dEdcn, const float* tv, int n_dir, float4* tcn4, float4* tg4, float* txbar,
                         const float* strain, float* tvir) {
  const dim3 grid(ceil_div(n_atoms, 4), ceil_div(n_dir, D3_KG)), block(256);
  const size_t lds = (size_t)4 * T.ns * 25 * sizeof(float);
  if (strain) {  // armed (plan: d3_strain): the instantiations that take r eps and write the virial tangent
    if (!tvir || !cell) {
      set_last_error("hvp: the DFT-D3 block under strain needs a cell and the virial rows");
      return -1;
    }
    hipLaunchKernelGGL(d3_tcn_kernel<true>, grid, block, 0, s, xs4, mol_idx, cell, n_cell, nb_idx, nb_shift, nb_cnt, cap, T, cutoff,
                       n_atoms, tv, n_dir, tcn4, strain);
    AIMNET_LAUNCH_CHECK();
    hipLaunchKernelGGL(d3_tpair_kernel<true>, grid, block, lds, s, xs4, mol_idx, cell, n_cell, nb_idx, nb_shift, nb_cnt, cap, T, P, cutoff,
                       n_atoms, d3w, tcn4, n_dir, tg4, txbar, strain, tvir);
    AIMNET_LAUNCH_CHECK();
    hipLaunchKernelGGL(d3_tcnforce_kernel<true>, grid, block, 0, s, xs4, mol_idx, cell, n_cell, nb_idx, nb_shift, nb_cnt, cap, T, cutoff,
                       n_atoms, dEdcn, tg4, n_dir, txbar, strain, tvir);
    AIMNET_LAUNCH_CHECK();
    return 0;
  }
  hipLaunchKernelGGL(d3_tcn_kernel<false>, grid, block, 0, s, xs4, mol_idx, cell, n_cell, nb_idx, nb_shift, nb_cnt, cap, T, cutoff,
                     n_atoms, tv, n_dir, tcn4, nullptr);
  AIMNET_LAUNCH_CHECK();
  hipLaunchKernelGGL(d3_tpair_kernel<false>, grid, block, lds, s, xs4, mol_idx, cell, n_cell, nb_idx, nb_shift, nb_cnt, cap, T, P, cutoff,
                     n_atoms, d3w, tcn4, n_dir, tg4, txbar, nullptr, nullptr);
  AIMNET_LAUNCH_CHECK();
  hipLaunchKernelGGL(d3_tcnforce_kernel<false>, grid, block, 0, s, xs4, mol_idx, cell, n_cell, nb_idx, nb_shift, nb_cnt, cap, T, cutoff,
                     n_atoms, dEdcn, tg4, n_dir, txbar, nullptr, nullptr);
  AIMNET_LAUNCH_CHECK();
  return 0;
}

}  // namespace aimnet
