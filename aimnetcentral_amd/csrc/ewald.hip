// Ewald summation for periodic point charges (LRCoulomb "ewald", reference aimnet/modules/lr.py:617-720, parameters and the
// per-call real-space list calculator.py:1560-1603).  The reference delegates the arithmetic to nvalchemiops.ewald_summation
// (un-vendored, 0.4.0; unpinned against that kernel).  Restated from the published method and from the reference's in-tree
// pure-PyTorch Ewald (ops.py:196-276), to whose golden matrices the oracle is pinned: oracle/aimnet2_oracle.py (ewald_*).
//
//   E / k_e = 1/2 sum'_{i,j,n} q_i q_j erfc(alpha r) / r                         real space, r < rc      (model.hip: the cell-grid walk)
//           + (2 pi / V) sum_{k != 0} exp(-k^2 / 4 alpha^2) / k^2 |S(k)|^2       reciprocal space, |k| <= kc   (here)
//           - alpha / sqrt(pi) sum_i q_i^2                                        self term               (the walk's self term)
//           - pi Q^2 / (2 V alpha^2)                                              neutralising background (here)
//
// UNPINNED against the reference's production kernel: three conventions follow the textbook form and the in-tree torch
// Ewald, not nvalchemiops (absent from the reference tree) - the background term for CHARGED cells (a constant energy / stress
// offset if the production kernel omits or scales it), the inclusive cut k^2 <= kc^2 (ops.py uses <), and "pme" requests being
// served by this exact sum (calculator.set_lrcoulomb_method warns).  Neutral cells are pinned (golden matrices, Madelung constants).
//
// Per system: eta = (V^2 / N)^(1/6) / sqrt(2 pi), alpha = 1 / (sqrt(2) eta), rc = f eta, kc = f / eta, f = sqrt(-2 ln accuracy) -
// both sums cost O(N^1.5).  Everything is decided on the device from the cell (no host round trip, NPT-safe); the host only
// provides the capacity of the k arrays.
//
// Reciprocal space in potential form: phi_i = sum_{k in half space} A(k) Re[conj(S(k)) e^{i k.r_i}], A = (8 pi / V) exp(..) / k^2,
// so that E_rec = k_e/2 sum_i q_i phi_i, dE/dq_i = k_e phi_i, dE/dr_i = k_e q_i grad phi_i and the strain derivative
// dE/d eps_ab = k_e/2 sum_i q_i sum_k A Re[..] (2 k_a k_b (1/k^2 + 1/(4 alpha^2)) - delta_ab) all come from ONE pass per atom.
// Phases are formed in double from fractional coordinates (n . f reduced to [-1/2, 1/2] before the fp32 sin / cos), sums in double.
#include <hip/hip_runtime.h>

#include "common.h"
#include "ewald_common.h"
#include "kernels.h"

namespace aimnet {

namespace {

__global__ void ewald_setup_kernel(const float* __restrict__ cell, int n_cell, const int* __restrict__ mol_start,
                                   const float* __restrict__ charge, int nq, int n_mol, float accuracy, int max_k,
                                   EwaldSystem* __restrict__ es, int* __restrict__ status_k) {
  for (int s = threadIdx.x; s < n_mol; s += blockDim.x) {
    double Q = 0.0;
    for (int ch = 0; ch < nq; ++ch) Q += (double)charge[(size_t)ch * n_mol + s];
    double m[9];
    EwaldSystem E;
    ewald_system_setup(cell + (n_cell == 1 ? 0 : (size_t)s * 9), mol_start[s + 1] - mol_start[s], accuracy, Q, m, E);
    es[s] = E;
  }
  __syncthreads();
  ewald_k_slices(es, n_mol, max_k, status_k);
}

__global__ void ewald_frac_kernel(const float* __restrict__ xw, const int* __restrict__ mol_idx, int n_atoms,
                                  const EwaldSystem* __restrict__ es, double* __restrict__ frac) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n_atoms) return;
  const EwaldSystem& E = es[mol_idx[i]];
  const double x = xw[3 * i], y = xw[3 * i + 1], z = xw[3 * i + 2];
  for (int a = 0; a < 3; ++a) frac[(size_t)i * 3 + a] = x * E.inv[a] + y * E.inv[3 + a] + z * E.inv[6 + a];
}

__device__ __forceinline__ void phase_sincos(double f0, double f1, double f2, int n1, int n2, int n3, float& sn, float& cs) {
  double ph = (double)n1 * f0 + (double)n2 * f1 + (double)n3 * f2;
  ph -= rint(ph);  // turns, [-1/2, 1/2]
  sincosf((float)(EW_TWO_PI * ph), &sn, &cs);
}

// S(k) = sum_i q_i e^{i k.r_i} for EWALD_KB consecutive entries of one system's k box: the block's threads stride the system's atoms
__global__ __launch_bounds__(256) void ewald_sfac_kernel(const double* __restrict__ frac, const float* __restrict__ q,
                                                        const int* __restrict__ mol_start, int n_mol,
                                                        const EwaldSystem* __restrict__ es, EwaldK* __restrict__ kk) {
  const int e0 = blockIdx.x * EWALD_KB;
  if (e0 >= es[n_mol - 1].k_offset + es[n_mol - 1].n_box) return;
  int s = 0;
  while (s + 1 < n_mol && e0 >= es[s].k_offset + es[s].n_box) ++s;  // (block-uniform; systems with an empty slice are skipped)
  const EwaldSystem& E = es[s];
  int n1[EWALD_KB], n2[EWALD_KB], n3[EWALD_KB];
  bool ok[EWALD_KB];
  double kv[EWALD_KB][3], k2[EWALD_KB];
  const long box = (long)(E.nmax[0] + 1) * E.n2w * E.n3w;
#pragma unroll
  for (int j = 0; j < EWALD_KB; ++j) {
    const int r = e0 + j - E.k_offset;
    n1[j] = r / (E.n2w * E.n3w);
    const int rem = r - n1[j] * (E.n2w * E.n3w);
    n2[j] = rem / E.n3w - E.nmax[1];
    n3[j] = rem % E.n3w - E.nmax[2];
    const bool half = n1[j] > 0 || (n1[j] == 0 && (n2[j] > 0 || (n2[j] == 0 && n3[j] > 0)));
    k2[j] = 0.0;
    for (int c = 0; c < 3; ++c) {
      kv[j][c] = (double)n1[j] * E.b[c] + (double)n2[j] * E.b[3 + c] + (double)n3[j] * E.b[6 + c];
      k2[j] += kv[j][c] * kv[j][c];
    }
    ok[j] = r < box && r < E.n_box && half && k2[j] <= (double)E.kc2;
  }
  double re[EWALD_KB], im[EWALD_KB];
#pragma unroll
  for (int j = 0; j < EWALD_KB; ++j) re[j] = im[j] = 0.0;
  for (int i = mol_start[s] + (int)threadIdx.x; i < mol_start[s + 1]; i += 256) {
    const double f0 = frac[(size_t)i * 3], f1 = frac[(size_t)i * 3 + 1], f2 = frac[(size_t)i * 3 + 2];
    const double qi = q[i];
#pragma unroll
    for (int j = 0; j < EWALD_KB; ++j) {
      if (!ok[j]) continue;  // (block-uniform)
      float sn, cs;
      phase_sincos(f0, f1, f2, n1[j], n2[j], n3[j], sn, cs);
      re[j] += qi * (double)cs;
      im[j] += qi * (double)sn;
    }
  }
  __shared__ double sh[4][2 * EWALD_KB];
  const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
#pragma unroll
  for (int j = 0; j < EWALD_KB; ++j) {
    const double a = wave_sum(re[j]), b = wave_sum(im[j]);
    if (lane == 0) {
      sh[w][2 * j] = a;
      sh[w][2 * j + 1] = b;
    }
  }
  __syncthreads();
  if (threadIdx.x < EWALD_KB) {
    const int j = threadIdx.x;
    // (the unrolled per-j registers are indexed dynamically here: recompute this entry's constants)
    const int r = e0 + j - E.k_offset;
    if (r >= E.n_box) return;
    const int m1 = r / (E.n2w * E.n3w);
    const int rem = r - m1 * (E.n2w * E.n3w);
    const int m2 = rem / E.n3w - E.nmax[1], m3 = rem % E.n3w - E.nmax[2];
    const bool half = m1 > 0 || (m1 == 0 && (m2 > 0 || (m2 == 0 && m3 > 0)));
    double kx[3], kq = 0.0;
    for (int c = 0; c < 3; ++c) {
      kx[c] = (double)m1 * E.b[c] + (double)m2 * E.b[3 + c] + (double)m3 * E.b[6 + c];
      kq += kx[c] * kx[c];
    }
    const bool valid = r < box && half && kq <= (double)E.kc2;
    EwaldK K;
    K.P = K.Q = 0.0;
    K.kx = K.ky = K.kz = K.vfac = 0.0f;
    K.n1 = m1; K.n2 = m2; K.n3 = m3; K.pad = 0;
    if (valid) {
      const double sre = sh[0][2 * j] + sh[1][2 * j] + sh[2][2 * j] + sh[3][2 * j];
      const double sim = sh[0][2 * j + 1] + sh[1][2 * j + 1] + sh[2][2 * j + 1] + sh[3][2 * j + 1];
      const double A = E.pref * exp(-kq * (double)E.inv4a2) / kq;
      K.P = A * sre;
      K.Q = A * sim;
      K.kx = (float)kx[0]; K.ky = (float)kx[1]; K.kz = (float)kx[2];
      K.vfac = (float)(2.0 * (1.0 / kq + (double)E.inv4a2));
    }
    kk[e0 + j] = K;
  }
}

// one wave per atom, lanes over the system's k entries
template <bool GRAD, bool STRESS>
__global__ __launch_bounds__(256) void ewald_atom_kernel(const double* __restrict__ frac, const float* __restrict__ q,
                                                        const int* __restrict__ mol_idx, int n_atoms,
                                                        const EwaldSystem* __restrict__ es, const EwaldK* __restrict__ kk, float factor,
                                                        double* __restrict__ ecoul, float* __restrict__ qbar,
                                                        float* __restrict__ fgrad, float* __restrict__ virial_atom) {
  const int i = blockIdx.x * 4 + (threadIdx.x >> 6);
  if (i >= n_atoms) return;
  const int lane = threadIdx.x & 63;
  const EwaldSystem& E = es[mol_idx[i]];
  const double f0 = frac[(size_t)i * 3], f1 = frac[(size_t)i * 3 + 1], f2 = frac[(size_t)i * 3 + 2];
  double phi = 0.0, g[3] = {0.0, 0.0, 0.0}, W[6] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0};
  const int e1 = E.k_offset + E.n_box;
  for (int e = E.k_offset + lane; e < e1; e += 64) {
    const EwaldK K = kk[e];
    if (K.P == 0.0 && K.Q == 0.0) continue;
    float sn, cs;
    phase_sincos(f0, f1, f2, K.n1, K.n2, K.n3, sn, cs);
    const double t = (double)cs * K.P + (double)sn * K.Q;
    phi += t;
    if (GRAD) {
      const double d = (double)cs * K.Q - (double)sn * K.P;
      g[0] += d * (double)K.kx; g[1] += d * (double)K.ky; g[2] += d * (double)K.kz;
      if (STRESS) {
        const double tv = t * (double)K.vfac;
        W[0] += tv * (double)(K.kx * K.kx); W[1] += tv * (double)(K.kx * K.ky); W[2] += tv * (double)(K.kx * K.kz);
        W[3] += tv * (double)(K.ky * K.ky); W[4] += tv * (double)(K.ky * K.kz); W[5] += tv * (double)(K.kz * K.kz);
      }
    }
  }
  phi = wave_sum(phi);
  if (GRAD) {
    for (int c = 0; c < 3; ++c) g[c] = wave_sum(g[c]);
    if (STRESS)
      for (int c = 0; c < 6; ++c) W[c] = wave_sum(W[c]);
  }
  if (lane != 0) return;
  const double qi = q[i];
  const double phi_all = phi + (double)E.phi_bg;
  ecoul[i] += (double)factor * qi * phi_all;
  if (GRAD) {
    qbar[i] += (float)(2.0 * (double)factor * phi_all);
    for (int c = 0; c < 3; ++c) fgrad[3 * i + c] += (float)(2.0 * (double)factor * qi * g[c]);
    if (STRESS) {
      const double sc = (double)factor * qi;
      float* v = virial_atom + (size_t)i * 9;
      v[0] += (float)(sc * (W[0] - phi_all)); v[1] += (float)(sc * W[1]); v[2] += (float)(sc * W[2]);
      v[3] += (float)(sc * W[1]); v[4] += (float)(sc * (W[3] - phi_all)); v[5] += (float)(sc * W[4]);
      v[6] += (float)(sc * W[2]); v[7] += (float)(sc * W[4]); v[8] += (float)(sc * (W[5] - phi_all));
    }
  }
}

// ---- tangents for the Hessian-vector sweep (hvp.hip) ---------------------------------------------------------------------------
// A direction carries t_r (the caller's vector) and t_q (the tangent of the final charges; two channels: their sum).  With
// t_theta_i = k . t_r_i:   t_S(k) = sum_j (t_q_j + i q_j t_theta_j) e^{i theta_j},   t_P = A Re t_S,   t_Q = A Im t_S   (the cell is
// fixed: A and k carry no tangent; neither does the background, sum_j t_q_j = 0 under the NSE normalisation).
constexpr int EWALD_TD = 4;  // directions whose sums one block holds in registers: the sin / cos of an (atom, k) pair is formed once

__device__ __forceinline__ void total_charge_tangent(const float* __restrict__ tq, int nq, int n_atoms, int k, int i, double& tqi) {
  tqi = (double)tq[((size_t)k * nq) * n_atoms + i];
  if (nq == 2) tqi += (double)tq[((size_t)k * nq + 1) * n_atoms + i];
}

// entry r of a system's k box: its integer triplet, k, k^2 and whether it lies inside the slice and the half-space sphere.  One
// definition for the accumulation and the write phase of ewald_tsfac_kernel (k^2 by explicit fma: both decide alike).  The primal
// kernel keeps its own copy untouched; the per-atom pass trusts the primal's vfac, so an entry the two should ever judge differently at
// exactly |k| = kc either carries a zero tangent or is skipped - never read unwritten.
__device__ __forceinline__ bool ewald_k_entry(const EwaldSystem& E, int r, int& n1, int& n2, int& n3, double kv[3], double& k2) {
  const long box = (long)(E.nmax[0] + 1) * E.n2w * E.n3w;
  n1 = r / (E.n2w * E.n3w);
  const int rem = r - n1 * (E.n2w * E.n3w);
  n2 = rem / E.n3w - E.nmax[1];
  n3 = rem % E.n3w - E.nmax[2];
  const bool half = n1 > 0 || (n1 == 0 && (n2 > 0 || (n2 == 0 && n3 > 0)));
  k2 = 0.0;
  for (int c = 0; c < 3; ++c) {
    kv[c] = fma((double)n3, E.b[6 + c], fma((double)n2, E.b[3 + c], (double)n1 * E.b[c]));
    k2 = fma(kv[c], kv[c], k2);
  }
  return r < box && r < E.n_box && half && k2 <= (double)E.kc2;
}

// block = (EWALD_KB entries of one system's k box - the mapping of ewald_sfac_kernel -, EWALD_TD directions); the sums of a
// direction are the same expressions in the same order whichever slot of whichever block holds it (explicit fma: no contraction
// left to the compiler), so a direction's numbers do not depend on how the directions were grouped.
__global__ __launch_bounds__(256) void ewald_tsfac_kernel(const double* __restrict__ frac, const float* __restrict__ q,
                                                         const float* __restrict__ tq, int nq, const float* __restrict__ tv,
                                                         int n_atoms, int n_dir, const int* __restrict__ mol_start, int n_mol,
                                                         const EwaldSystem* __restrict__ es, int max_k, double2* __restrict__ tk) {
  const int e0 = blockIdx.x * EWALD_KB, d0 = blockIdx.y * EWALD_TD;
  if (e0 >= es[n_mol - 1].k_offset + es[n_mol - 1].n_box) return;
  int s = 0;
  while (s + 1 < n_mol && e0 >= es[s].k_offset + es[s].n_box) ++s;  // (block-uniform, as in ewald_sfac_kernel)
  const EwaldSystem& E = es[s];
  const int nd = min(EWALD_TD, n_dir - d0);
  int n1[EWALD_KB], n2[EWALD_KB], n3[EWALD_KB];
  bool ok[EWALD_KB];
  double kv[EWALD_KB][3];
#pragma unroll
  for (int j = 0; j < EWALD_KB; ++j) {
    double k2;
    ok[j] = ewald_k_entry(E, e0 + j - E.k_offset, n1[j], n2[j], n3[j], kv[j], k2);
  }
  double re[EWALD_KB][EWALD_TD], im[EWALD_KB][EWALD_TD];
#pragma unroll
  for (int j = 0; j < EWALD_KB; ++j)
#pragma unroll
    for (int d = 0; d < EWALD_TD; ++d) re[j][d] = im[j][d] = 0.0;
  for (int i = mol_start[s] + (int)threadIdx.x; i < mol_start[s + 1]; i += 256) {
    const double f0 = frac[(size_t)i * 3], f1 = frac[(size_t)i * 3 + 1], f2 = frac[(size_t)i * 3 + 2];
    const double qi = q[i];
    double tr[EWALD_TD][3], tqi[EWALD_TD];
#pragma unroll
    for (int d = 0; d < EWALD_TD; ++d) {
      tr[d][0] = tr[d][1] = tr[d][2] = tqi[d] = 0.0;
      if (d < nd) {  // (block-uniform)
        const float* t = tv + ((size_t)(d0 + d) * n_atoms + i) * 3;
        tr[d][0] = t[0]; tr[d][1] = t[1]; tr[d][2] = t[2];
        total_charge_tangent(tq, nq, n_atoms, d0 + d, i, tqi[d]);
      }
    }
#pragma unroll
    for (int j = 0; j < EWALD_KB; ++j) {
      if (!ok[j]) continue;  // (block-uniform)
      float snf, csf;
      phase_sincos(f0, f1, f2, n1[j], n2[j], n3[j], snf, csf);
      const double sn = snf, cs = csf;
#pragma unroll
      for (int d = 0; d < EWALD_TD; ++d) {
        if (d >= nd) continue;
        const double tth = fma(kv[j][2], tr[d][2], fma(kv[j][1], tr[d][1], kv[j][0] * tr[d][0]));
        const double qt = qi * tth;
        re[j][d] = fma(-qt, sn, fma(tqi[d], cs, re[j][d]));
        im[j][d] = fma(qt, cs, fma(tqi[d], sn, im[j][d]));
      }
    }
  }
  __shared__ double sh[4][2 * EWALD_KB * EWALD_TD];
  const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
#pragma unroll
  for (int j = 0; j < EWALD_KB; ++j)
#pragma unroll
    for (int d = 0; d < EWALD_TD; ++d) {
      const double a = wave_sum(re[j][d]), b = wave_sum(im[j][d]);
      if (lane == 0) {
        sh[w][2 * (j * EWALD_TD + d)] = a;
        sh[w][2 * (j * EWALD_TD + d) + 1] = b;
      }
    }
  __syncthreads();
  if (threadIdx.x < EWALD_KB * EWALD_TD) {
    const int j = threadIdx.x / EWALD_TD, d = threadIdx.x % EWALD_TD;
    const int r = e0 + j - E.k_offset;
    if (r >= E.n_box || d >= nd) return;
    // (the unrolled per-j registers are indexed dynamically here: recompute this entry's constants)
    int m1, m2, m3;
    double kx[3], kq;
    double2 T = make_double2(0.0, 0.0);
    if (ewald_k_entry(E, r, m1, m2, m3, kx, kq)) {
      const int o = 2 * (j * EWALD_TD + d);
      const double sre = sh[0][o] + sh[1][o] + sh[2][o] + sh[3][o];
      const double sim = sh[0][o + 1] + sh[1][o + 1] + sh[2][o + 1] + sh[3][o + 1];
      const double A = E.pref * exp(-kq * (double)E.inv4a2) / kq;
      T = make_double2(A * sre, A * sim);
    }
    tk[(size_t)(d0 + d) * max_k + e0 + j] = T;
  }
}

// one wave per (atom, direction), lanes over the system's k entries.  With t = cs P + sn Q and d = cs Q - sn P (phi_i = sum t,
// g_i = sum d k):   t_phi_i = sum_k (cs t_P + sn t_Q + t_theta_i d),   t_g_i = sum_k k (cs t_Q - sn t_P - t_theta_i t).
// ADDS onto the seeds of the sweep in the convention of hvp.hip's coul_store (E_rec = factor sum_i q_i phi_i):
//   qbar_i += 2 factor (phi_i + phi_bg)   t_qbar_i += 2 factor t_phi_i     (every charge channel: the term sees their sum)
//   xbar_i += 2 factor q_i g_i            t_xbar_i += 2 factor (t_q_i g_i + q_i t_g_i)
// An entry is valid by its own vfac (0 outside the half-space sphere): S = 0 with t_S != 0 is a valid entry.
__global__ __launch_bounds__(256) void ewald_tatom_kernel(const double* __restrict__ frac, const float* __restrict__ q,
                                                         const float* __restrict__ tq, int nq, const float* __restrict__ tv,
                                                         const int* __restrict__ mol_idx, int n_atoms,
                                                         const EwaldSystem* __restrict__ es, const EwaldK* __restrict__ kk, int max_k,
                                                         const double2* __restrict__ tk, float factor, float* __restrict__ qbar,
                                                         float* __restrict__ tqbar, float* __restrict__ xbar,
                                                         float* __restrict__ txbar) {
  const int i = blockIdx.x * 4 + (threadIdx.x >> 6), k = blockIdx.y;
  if (i >= n_atoms) return;
  const int lane = threadIdx.x & 63;
  const EwaldSystem& E = es[mol_idx[i]];
  const double f0 = frac[(size_t)i * 3], f1 = frac[(size_t)i * 3 + 1], f2 = frac[(size_t)i * 3 + 2];
  const float* t = tv + ((size_t)k * n_atoms + i) * 3;
  const double tr0 = t[0], tr1 = t[1], tr2 = t[2];
  const double2* __restrict__ tkk = tk + (size_t)k * max_k;
  double phi = 0.0, tphi = 0.0, g[3] = {0.0, 0.0, 0.0}, tg[3] = {0.0, 0.0, 0.0};
  const int e1 = E.k_offset + E.n_box;
  for (int e = E.k_offset + lane; e < e1; e += 64) {
    const EwaldK K = kk[e];
    if (K.vfac == 0.0f) continue;
    const double2 T = tkk[e];
    double kx[3];
    for (int c = 0; c < 3; ++c)  // (the expression of ewald_k_entry: the same k bit for bit)
      kx[c] = fma((double)K.n3, E.b[6 + c], fma((double)K.n2, E.b[3 + c], (double)K.n1 * E.b[c]));
    float snf, csf;
    phase_sincos(f0, f1, f2, K.n1, K.n2, K.n3, snf, csf);
    const double sn = snf, cs = csf;
    const double tth = fma(kx[2], tr2, fma(kx[1], tr1, kx[0] * tr0));
    const double tt = fma(sn, K.Q, cs * K.P), d = fma(-sn, K.P, cs * K.Q);
    const double tp = fma(tth, d, fma(sn, T.y, cs * T.x));
    const double td = fma(-tth, tt, fma(-sn, T.x, cs * T.y));
    phi += tt;
    tphi += tp;
    for (int c = 0; c < 3; ++c) {
      g[c] = fma(d, kx[c], g[c]);
      tg[c] = fma(td, kx[c], tg[c]);
    }
  }
  phi = wave_sum(phi);
  tphi = wave_sum(tphi);
  for (int c = 0; c < 3; ++c) {
    g[c] = wave_sum(g[c]);
    tg[c] = wave_sum(tg[c]);
  }
  if (lane != 0) return;
  const double qi = q[i], f2x = 2.0 * (double)factor;
  double tqi;
  total_charge_tangent(tq, nq, n_atoms, k, i, tqi);
  const float qv = (float)(f2x * (phi + (double)E.phi_bg)), tqv = (float)(f2x * tphi);
  for (int ch = 0; ch < nq; ++ch) {
    const size_t pe = (size_t)ch * n_atoms + i, te = ((size_t)k * nq + ch) * n_atoms + i;
    if (k == 0) qbar[pe] += qv;
    tqbar[te] += tqv;
  }
  for (int c = 0; c < 3; ++c) {
    const size_t pe = (size_t)i * 3 + c, te = ((size_t)k * n_atoms + i) * 3 + c;
    if (k == 0) xbar[pe] += (float)(f2x * qi * g[c]);
    txbar[te] += (float)(f2x * fma(tqi, g[c], qi * tg[c]));
  }
}

}  // namespace

int launch_ewald_setup(hipStream_t s, const float* cell, int n_cell, const int* mol_start, const int* mol_idx, const float* xw,
                       const float* charge, int nq, int n_atoms, int n_mol, float accuracy, EwaldBuffers& b, int* status_k) {
  hipLaunchKernelGGL(ewald_setup_kernel, dim3(1), dim3(256), 0, s, cell, n_cell, mol_start, charge, nq, n_mol, accuracy, b.max_k, b.sys,
                     status_k);
  AIMNET_LAUNCH_CHECK();
  return launch_ewald_frac(s, xw, mol_idx, n_atoms, b);
}

int launch_ewald_frac(hipStream_t s, const float* xw, const int* mol_idx, int n_atoms, const EwaldBuffers& b) {
  hipLaunchKernelGGL(ewald_frac_kernel, dim3(ceil_div(n_atoms, 256)), dim3(256), 0, s, xw, mol_idx, n_atoms, b.sys, b.frac);
  AIMNET_LAUNCH_CHECK();
  return 0;
}

int launch_ewald_sfac(hipStream_t s, const float* q, const int* mol_start, int n_mol, const EwaldBuffers& b) {
  hipLaunchKernelGGL(ewald_sfac_kernel, dim3(ceil_div(b.max_k, EWALD_KB)), dim3(256), 0, s, b.frac, q, mol_start, n_mol, b.sys, b.k);
  AIMNET_LAUNCH_CHECK();
  return 0;
}

int launch_ewald_tangent(hipStream_t s, const float* q, const float* tq, int nq, const float* tv, const int* mol_idx,
                         const int* mol_start, int n_atoms, int n_mol, int n_dir, const EwaldBuffers& b, double* tk, float factor,
                         float* qbar, float* tqbar, float* xbar, float* txbar) {
  hipLaunchKernelGGL(ewald_tsfac_kernel, dim3(ceil_div(b.max_k, EWALD_KB), ceil_div(n_dir, EWALD_TD)), dim3(256), 0, s, b.frac, q, tq,
                     nq, tv, n_atoms, n_dir, mol_start, n_mol, b.sys, b.max_k, (double2*)tk);
  AIMNET_LAUNCH_CHECK();
  hipLaunchKernelGGL(ewald_tatom_kernel, dim3(ceil_div(n_atoms, 4), n_dir), dim3(256), 0, s, b.frac, q, tq, nq, tv, mol_idx, n_atoms,
                     b.sys, b.k, b.max_k, (const double2*)tk, factor, qbar, tqbar, xbar, txbar);
  AIMNET_LAUNCH_CHECK();
  return 0;
}

int launch_ewald_recip(hipStream_t s, bool grad, bool stress, const float* q, const int* mol_idx, const int* mol_start, int n_atoms,
                       int n_mol, const EwaldBuffers& b, float factor, double* ecoul, float* qbar, float* fgrad, float* virial_atom) {
  if (const int rc = launch_ewald_sfac(s, q, mol_start, n_mol, b)) return rc;
  const dim3 grid(ceil_div(n_atoms, 4)), block(256);
  if (grad && stress)
    hipLaunchKernelGGL((ewald_atom_kernel<true, true>), grid, block, 0, s, b.frac, q, mol_idx, n_atoms, b.sys, b.k, factor, ecoul, qbar,
                       fgrad, virial_atom);
  else if (grad)
    hipLaunchKernelGGL((ewald_atom_kernel<true, false>), grid, block, 0, s, b.frac, q, mol_idx, n_atoms, b.sys, b.k, factor, ecoul, qbar,
                       fgrad, virial_atom);
  else
    hipLaunchKernelGGL((ewald_atom_kernel<false, false>), grid, block, 0, s, b.frac, q, mol_idx, n_atoms, b.sys, b.k, factor, ecoul, qbar,
                       fgrad, virial_atom);
  AIMNET_LAUNCH_CHECK();
  return 0;
}

}  // namespace aimnet
