// embed.hip - electrostatic embedding of the model's charges in an external potential (aimnet_engine_set_embedding):
//   E_emb = sum_i q_i phi_i,  phi_i = k_e sum_A Q_A / |x_i - X_A| + potential_i,  k_e = Hartree * Bohr (eV A / e^2)
// over the point charges (X_A, Q_A) of atom i's own molecule and / or a per-atom potential the caller computed.  The charges do not
// respond to the field (they are the model's): this is the first-order coupling with its exact gradient
//   dE_emb/dx_i = q_i grad phi_i + sum_j phi_j dq_j/dx_i ,
// whose second term is the backward sweep's own job - the seed pass adds phi_i to the adjoint dE/dq_i (qbar) that the Coulomb block
// has seeded, exactly as the Ewald block does with its potential.
// The tangent sweep (aimnet_engine_set_embedding_tangent, hvp.hip) carries the term through the Hessian-vector product with the
// atoms moving along v and the sites clamped: with g = grad phi, T = grad grad phi = k_e sum_A Q_A (3 r r^T / d^5 - 1 / d^3)
//   t_qbar_i^k += g_i . v_i^k        t_xbar_i^k += t_q_i^k g_i + q_i T_i v_i^k        (embed_tseed_kernel)
// and the backward sweep does the rest (sum_j phi_j d2q_j v, J t_phi).  The mixed atom-site block comes from embed_tsite_kernel.
// Pair terms in fp32 (the tensor's in double), every sum in double; no atomics on results, fixed summation orders: bitwise repeatable.
#include "common.h"
#include "ewald_common.h"
#include "kernels.h"

namespace aimnet {

namespace {

constexpr double KE = 27.211386024367243 * 0.5291772105638411;  // Hartree * Bohr = 2 * COULOMB_FACTOR (constants.py)

// 256 threads: wave_sum, then the four waves in index order
__device__ __forceinline__ double embed_block_sum(double v, double* sh) {
  v = wave_sum(v);
  __syncthreads();
  if ((threadIdx.x & 63) == 0) sh[threadIdx.x >> 6] = v;
  __syncthreads();
  return ((sh[0] + sh[1]) + sh[2]) + sh[3];
}

// thread = site: its clamped molecule index and the molecule offsets of the (sorted) site list - mol_start_kernel's scheme: site a
// stores the offsets of the molecules in (mol[a-1], mol[a]], the last one those above its own; every entry of ext_start is written
// with a value in [0, n_ext] whatever the input holds
__global__ __launch_bounds__(256) void embed_sites_kernel(const int* __restrict__ ext_mol_idx, int n_ext, int n_mol,
                                                          int* __restrict__ ext_start, int* __restrict__ ext_mol_c,
                                                          int* __restrict__ status6) {
  const int a = blockIdx.x * blockDim.x + threadIdx.x;
  if (a >= n_ext) return;
  const int raw = ext_mol_idx ? ext_mol_idx[a] : 0;
  const int before = (a == 0 || !ext_mol_idx) ? (a == 0 ? -1 : 0) : ext_mol_idx[a - 1];
  const int prev = min(max(before, -1), n_mol - 1);
  const int cur = min(max(raw, 0), n_mol - 1);
  ext_mol_c[a] = cur;
  if (raw < 0 || raw >= n_mol || (a > 0 && raw < before)) atomicOr(status6, STATUS_EXT_MOL_IDX);  // (a flag, not a result)
  for (int m = prev + 1; m <= cur; ++m) ext_start[m] = a;
  if (a == n_ext - 1)
    for (int m = cur + 1; m <= n_mol; ++m) ext_start[m] = n_ext;
}

// block = (atom i, slot s): lanes stride over the sites of the chunks s, s + n_slots, ... of the atom's molecule (consecutive lanes
// read consecutive sites; the site stream is shared by every atom of the molecule and stays in L2).  One partial
// (sum Q / d, -sum Q (x_i - X) / d^3) per block; it depends on the geometry alone.  TENSOR (the tangent sweep): six more sums, the
// components xx, yy, zz, xy, xz, yz of sum Q (3 r r^T / d^5 - 1 / d^3), 10 partials per block, the tensor's pair terms in double (see
// there).  With ten double accumulators and the double pair term the four-fold unrolled loop takes 101 VGPRs, four waves per SIMD
// (the plain instantiation: 44, eight) - one pass per aimnet_engine_hvp call, bound by the site stream.  The flag being a template
// parameter, the instantiation aimnet_engine_eval launches compiles to the instructions it had before the flag existed.
template <bool TENSOR>
__global__ __launch_bounds__(256) void embed_field_kernel(const float* __restrict__ x, const int* __restrict__ mol_c, int n_slots,
                                                          const float* __restrict__ ext_coord,
                                                          const float* __restrict__ ext_charge,
                                                          const int* __restrict__ ext_start, double* __restrict__ part) {
  constexpr int NP = TENSOR ? EMBED_NP_TENSOR : 4;
  __shared__ double sh[4];
  const int i = blockIdx.x / n_slots, s = blockIdx.x % n_slots;
  const int m = mol_c[i];
  const int s0 = ext_start[m], cnt = max(0, ext_start[m + 1] - s0);
  const int n_chunk = (int)(((long long)cnt + EMBED_CHUNK - 1) / EMBED_CHUNK);
  if (s >= n_chunk) {  // (block-uniform) this slot has no chunk of the molecule: its partial is zero
    if (threadIdx.x < NP) part[(size_t)blockIdx.x * NP + threadIdx.x] = 0.0;
    return;
  }
  const float xi = x[3 * (size_t)i], yi = x[3 * (size_t)i + 1], zi = x[3 * (size_t)i + 2];
  double acc[NP] = {};
  for (int k = s; k < n_chunk; k += n_slots) {
    const int lo = k * EMBED_CHUNK;  // (relative to s0: lo < cnt)
    const int hi = (int)min((long long)cnt, (long long)lo + EMBED_CHUNK);
#pragma unroll 4
    for (int r = lo + (int)threadIdx.x; r < hi; r += 256) {
      const size_t a = (size_t)s0 + (size_t)r;
      const float dx = xi - ext_coord[3 * a], dy = yi - ext_coord[3 * a + 1], dz = zi - ext_coord[3 * a + 2];
      const float d2 = fmaf(dz, dz, fmaf(dy, dy, dx * dx));
      const float rinv = rsqrtf(d2);
      const float p = ext_charge[a] * rinv;
      const float t = p * rinv * rinv;
      acc[0] += (double)p;
      acc[1] -= (double)(t * dx);
      acc[2] -= (double)(t * dy);
      acc[3] -= (double)(t * dz);
      if constexpr (TENSOR) {
        // The tensor's pair term in double.  In fp32 a component reaches 2 |Q| / d^3 through some nineteen roundings (d^-5 takes
        // the error of the reciprocal root five times), which the eight-rounding allowance of a field sum does not cover for a
        // single site (measured: 12.9 * 2^-24 |Q| / d^3 at one site).  The fp32 reciprocal root is the seed of two Newton steps.
        const double ex = (double)xi - (double)ext_coord[3 * a], ey = (double)yi - (double)ext_coord[3 * a + 1],
                     ez = (double)zi - (double)ext_coord[3 * a + 2];
        const double e2 = ex * ex + ey * ey + ez * ez;
        double y = (double)rinv;
        y = y * (1.5 - 0.5 * e2 * y * y);
        y = y * (1.5 - 0.5 * e2 * y * y);
        const double td = (double)ext_charge[a] * y * y * y, t5 = 3.0 * td * y * y;
        acc[4] += t5 * ex * ex - td;
        acc[5] += t5 * ey * ey - td;
        acc[6] += t5 * ez * ez - td;
        acc[7] += t5 * ex * ey;
        acc[8] += t5 * ex * ez;
        acc[9] += t5 * ey * ez;
      }
    }
  }
#pragma unroll
  for (int c = 0; c < NP; ++c) {
    const double v = embed_block_sum(acc[c], sh);
    if (threadIdx.x == 0) part[(size_t)blockIdx.x * NP + c] = v;
  }
}

// thread = atom: the slot partials in slot order, times k_e, plus the caller's potential; then the energy term and the seeds
template <bool GRAD>
__global__ __launch_bounds__(256) void embed_seed_kernel(const float* __restrict__ q, int n_atoms, int n_slots,
                                                         const double* __restrict__ part, const float* __restrict__ potential,
                                                         const float* __restrict__ potential_grad, double* __restrict__ e_atom,
                                                         double* __restrict__ ecoul, float* __restrict__ qbar,
                                                         float* __restrict__ fgrad) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n_atoms) return;
  double v[4] = {0.0, 0.0, 0.0, 0.0};
  for (int s = 0; s < n_slots; ++s)
#pragma unroll
    for (int c = 0; c < 4; ++c) v[c] += part[((size_t)i * n_slots + s) * 4 + c];
#pragma unroll
  for (int c = 0; c < 4; ++c) v[c] *= KE;
  if (potential) v[0] += (double)potential[i];
  if (GRAD && potential_grad)
#pragma unroll
    for (int c = 0; c < 3; ++c) v[1 + c] += (double)potential_grad[3 * (size_t)i + c];
  const double qi = (double)q[i];
  const double e = qi * v[0];  // the full product: the sites are not atoms, nothing is counted twice
  e_atom[i] = e;
  ecoul[i] += e;
  if (GRAD) {
    qbar[i] += (float)v[0];
#pragma unroll
    for (int c = 0; c < 3; ++c) fgrad[3 * (size_t)i + c] += (float)(qi * v[1 + c]);
  }
}

// block = molecule: strided loop, wave_sum, the waves in index order (the pattern of crs_dipole_kernel)
__global__ __launch_bounds__(256) void embed_energy_kernel(const double* __restrict__ e_atom, const int* __restrict__ mol_start,
                                                           double* __restrict__ energy) {
  __shared__ double sh[4];
  const int m = blockIdx.x;
  const int i0 = mol_start[m], i1 = mol_start[m + 1];
  double acc = 0.0;
  for (int i = i0 + (int)threadIdx.x; i < i1; i += 256) acc += e_atom[i];
  const double v = embed_block_sum(acc, sh);
  if (threadIdx.x == 0) energy[m] = v;
}

// thread = site, block = 256 consecutive sites: for every molecule the block's sites belong to, its atoms (x, q) pass through LDS in
// tiles of 256 and the threads of that molecule's sites sum over them in atom order
__global__ __launch_bounds__(256) void embed_site_kernel(const float* __restrict__ x, const float* __restrict__ q,
                                                         const int* __restrict__ mol_start, int n_mol,
                                                         const float* __restrict__ ext_coord, const float* __restrict__ ext_charge,
                                                         const int* __restrict__ ext_mol_c, int n_ext,
                                                         float* __restrict__ ext_forces, float* __restrict__ ext_potential) {
  __shared__ float4 tile[256];
  const int a0 = blockIdx.x * 256, a = a0 + (int)threadIdx.x;
  const bool live = a < n_ext;
  const int a_last = min(n_ext, a0 + 256) - 1;
  const int mf = ext_mol_c[a0], ml = ext_mol_c[a_last];  // (block-uniform; a sorted list: the block's molecules lie between them)
  const int m_lo = min(mf, ml), m_hi = max(mf, ml);
  const int mine = live ? ext_mol_c[a] : -1;
  float X = 0.f, Y = 0.f, Z = 0.f;
  if (live) { X = ext_coord[3 * (size_t)a]; Y = ext_coord[3 * (size_t)a + 1]; Z = ext_coord[3 * (size_t)a + 2]; }
  double acc[4] = {0.0, 0.0, 0.0, 0.0};
  for (int m = m_lo; m <= m_hi; ++m) {
    const int i0 = mol_start[m], i1 = mol_start[m + 1];
    for (int t0 = i0; t0 < i1; t0 += 256) {
      const int nt = min(256, i1 - t0);
      __syncthreads();
      if ((int)threadIdx.x < nt) {
        const size_t i = (size_t)t0 + threadIdx.x;
        tile[threadIdx.x] = make_float4(x[3 * i], x[3 * i + 1], x[3 * i + 2], q[i]);
      }
      __syncthreads();
      if (mine == m) {
        for (int k = 0; k < nt; ++k) {
          const float4 at = tile[k];
          const float dx = X - at.x, dy = Y - at.y, dz = Z - at.z;
          const float d2 = fmaf(dz, dz, fmaf(dy, dy, dx * dx));
          const float rinv = rsqrtf(d2);
          const float p = at.w * rinv;
          const float t = p * rinv * rinv;
          acc[0] += (double)p;
          acc[1] += (double)(t * dx);
          acc[2] += (double)(t * dy);
          acc[3] += (double)(t * dz);
        }
      }
    }
  }
  if (!live) return;
  if (ext_potential) ext_potential[a] = (float)(KE * acc[0]);
  if (ext_forces) {
    const double kq = KE * (double)ext_charge[a];  // -dE_emb/dX_A = k_e Q_A sum_i q_i (X_A - x_i) / d^3
#pragma unroll
    for (int c = 0; c < 3; ++c) ext_forces[3 * (size_t)a + c] = (float)(kq * acc[1 + c]);
  }
}

// ---- the tangent sweep (hvp.hip, Tangent::embedding_seeds) ------------------------------------------------------------------------
// thread = (atom i, direction k): the slot partials in slot order, times k_e, plus the caller's potential / grad / hess; then the
// addends of the seeds in the layouts of hvp.hip's coul_store (qbar [nq][N], tqbar [K][nq][N], xbar [N][3], txbar [K][N][3]; the
// Coulomb terms see alpha + beta: every channel takes the same seed).  The k = 0 threads add the primal seeds and write `field`.
// Every thread forms the same ten sums in the same order: what an atom adds does not depend on how many directions ride along.
__global__ __launch_bounds__(256) void embed_tseed_kernel(const float* __restrict__ q, const float* __restrict__ tq, int nq,
                                                          const float* __restrict__ tv, int n_atoms, int n_slots,
                                                          const double* __restrict__ part, const float* __restrict__ potential,
                                                          const float* __restrict__ potential_grad,
                                                          const float* __restrict__ potential_hess, float* __restrict__ qbar,
                                                          float* __restrict__ tqbar, float* __restrict__ xbar,
                                                          float* __restrict__ txbar, double* __restrict__ field) {
  constexpr int NP = EMBED_NP_TENSOR;
  const int i = blockIdx.x * blockDim.x + threadIdx.x, k = blockIdx.y;
  if (i >= n_atoms) return;
  const size_t N = (size_t)n_atoms;
  double f[NP] = {};
  for (int s = 0; s < n_slots; ++s)
#pragma unroll
    for (int c = 0; c < NP; ++c) f[c] += part[((size_t)i * n_slots + s) * NP + c];
#pragma unroll
  for (int c = 0; c < NP; ++c) f[c] *= KE;
  if (potential) f[0] += (double)potential[i];
  if (potential_grad)
#pragma unroll
    for (int c = 0; c < 3; ++c) f[1 + c] += (double)potential_grad[3 * (size_t)i + c];
  if (potential_hess)
#pragma unroll
    for (int c = 0; c < 6; ++c) f[4 + c] += (double)potential_hess[6 * (size_t)i + c];
  float qf = q[i], tqf = tq[((size_t)k * nq) * N + i];  // total charge and its tangent (hvp.hip, q_total)
  if (nq == 2) {
    qf += q[N + i];
    tqf += tq[((size_t)k * nq + 1) * N + i];
  }
  const double qi = (double)qf, tqi = (double)tqf;
  const size_t te = ((size_t)k * N + i) * 3;
  const double vx = (double)tv[te], vy = (double)tv[te + 1], vz = (double)tv[te + 2];
  const double gv = f[1] * vx + f[2] * vy + f[3] * vz;
  const double Tv[3] = {f[4] * vx + f[7] * vy + f[8] * vz, f[7] * vx + f[5] * vy + f[9] * vz, f[8] * vx + f[9] * vy + f[6] * vz};
  for (int ch = 0; ch < nq; ++ch) {
    if (k == 0) qbar[(size_t)ch * N + i] += (float)f[0];
    tqbar[((size_t)k * nq + ch) * N + i] += (float)gv;
  }
#pragma unroll
  for (int c = 0; c < 3; ++c) {
    if (k == 0) xbar[3 * (size_t)i + c] += (float)(qi * f[1 + c]);
    txbar[te + c] += (float)(tqi * f[1 + c] + qi * Tv[c]);
  }
  if (k == 0 && field)
#pragma unroll
    for (int c = 0; c < NP; ++c) field[(size_t)i * NP + c] = f[c];
}

// mixed atom-site block: ext_hv[k][A] = d/d eps of dE_emb/dX_A along v^k, the charge response included,
//   -k_e Q_A sum_i [ t_q_i s / |s|^3 + q_i (-v_i / |s|^3 + 3 (s . v_i) s / |s|^5) ] ,  s = X_A - x_i .
// block = (256 consecutive sites, direction k), thread = site - embed_site_kernel's mapping: the atoms (x, q, v^k, t_q^k) of every
// molecule the block's sites belong to pass through LDS in tiles of 256, and a thread sums over its molecule's atoms in atom order.
__global__ __launch_bounds__(256) void embed_tsite_kernel(const float* __restrict__ x, const float* __restrict__ q,
                                                          const float* __restrict__ tq, int nq, const float* __restrict__ tv,
                                                          int n_atoms, const int* __restrict__ mol_start,
                                                          const float* __restrict__ ext_coord, const float* __restrict__ ext_charge,
                                                          const int* __restrict__ ext_mol_c, int n_ext, float* __restrict__ ext_hv) {
  __shared__ float4 tile_x[256], tile_v[256];  // (x, q) and (v, t_q)
  const int a0 = blockIdx.x * 256, a = a0 + (int)threadIdx.x, k = blockIdx.y;
  const size_t N = (size_t)n_atoms;
  const bool live = a < n_ext;
  const int a_last = min(n_ext, a0 + 256) - 1;
  const int mf = ext_mol_c[a0], ml = ext_mol_c[a_last];  // (block-uniform; a sorted list: the block's molecules lie between them)
  const int m_lo = min(mf, ml), m_hi = max(mf, ml);
  const int mine = live ? ext_mol_c[a] : -1;
  float X = 0.f, Y = 0.f, Z = 0.f;
  if (live) { X = ext_coord[3 * (size_t)a]; Y = ext_coord[3 * (size_t)a + 1]; Z = ext_coord[3 * (size_t)a + 2]; }
  double acc[3] = {0.0, 0.0, 0.0};
  for (int m = m_lo; m <= m_hi; ++m) {
    const int i0 = mol_start[m], i1 = mol_start[m + 1];
    for (int t0 = i0; t0 < i1; t0 += 256) {
      const int nt = min(256, i1 - t0);
      __syncthreads();
      if ((int)threadIdx.x < nt) {
        const size_t i = (size_t)t0 + threadIdx.x, te = ((size_t)k * N + i) * 3;
        float qf = q[i], tqf = tq[((size_t)k * nq) * N + i];
        if (nq == 2) {
          qf += q[N + i];
          tqf += tq[((size_t)k * nq + 1) * N + i];
        }
        tile_x[threadIdx.x] = make_float4(x[3 * i], x[3 * i + 1], x[3 * i + 2], qf);
        tile_v[threadIdx.x] = make_float4(tv[te], tv[te + 1], tv[te + 2], tqf);
      }
      __syncthreads();
      if (mine == m) {
        for (int j = 0; j < nt; ++j) {
          const float4 at = tile_x[j], av = tile_v[j];
          const float sx = X - at.x, sy = Y - at.y, sz = Z - at.z;
          const float d2 = fmaf(sz, sz, fmaf(sy, sy, sx * sx));
          const float rinv = rsqrtf(d2);
          const float r3 = rinv * rinv * rinv;
          const float sv = fmaf(sz, av.z, fmaf(sy, av.y, sx * av.x));
          const float cs = r3 * (av.w + 3.0f * at.w * sv * rinv * rinv);  // coefficient of s
          const float cv = at.w * r3;                                     // coefficient of -v
          acc[0] += (double)(cs * sx - cv * av.x);
          acc[1] += (double)(cs * sy - cv * av.y);
          acc[2] += (double)(cs * sz - cv * av.z);
        }
      }
    }
  }
  if (!live) return;
  const double kq = -KE * (double)ext_charge[a];
#pragma unroll
  for (int c = 0; c < 3; ++c) ext_hv[((size_t)k * n_ext + a) * 3 + c] = (float)(kq * acc[c]);
}

// ---- sites that are periodic with the cell (aimnet_engine_set_embedding_periodic) ------------------------------------------------
// phi_i / k_e = sum_A sum_n Q_A erfc(alpha d) / d  (d = |x_i - X_A + n C| < rc)  +  sum_k A(k) Re[conj(S_ext(k)) e^{i k x_i}]
//               - pi Q_ext / (V alpha^2),  and psi_A the same with atoms and sites exchanged.  No self term, no site-site term.
// Real space: the fractional difference of a pair is reduced to [-1/2, 1/2]^3 in double, then every translation |n_a| <= img[a] is
// tried (one when rc is below half the perpendicular widths); the pair term inside rc is fp32 with the walk's erfc (common.h).
// Reciprocal space: ewald_sfac_kernel forms A(k) S(k) of either particle set, one wave per atom / site sums over the k entries.

// block = system: Q_ext in double, eight strided loads in flight per thread (a single wave per system is bound by the latency of
// its loads, profiles/embedding_periodic.md), the eight chains added pairwise, wave_sum, the four waves in index order - a fixed order
__global__ __launch_bounds__(256) void embed_pbc_charge_kernel(const int* __restrict__ ext_start, const float* __restrict__ ext_charge,
                                                               EmbedPbcSystem* __restrict__ ps) {
  __shared__ double sh[4];
  const int s = blockIdx.x, a1 = ext_start[s + 1];
  double Q8[8] = {};
  for (int a = ext_start[s] + (int)threadIdx.x; a < a1; a += 8 * 256)
#pragma unroll
    for (int u = 0; u < 8; ++u)
      if (a + 256 * u < a1) Q8[u] += (double)ext_charge[a + 256 * u];
  const double Q = embed_block_sum(((Q8[0] + Q8[1]) + (Q8[2] + Q8[3])) + ((Q8[4] + Q8[5]) + (Q8[6] + Q8[7])), sh);
  if (threadIdx.x == 0) ps[s].bg_ext = Q;  // (the sum; embed_pbc_setup_kernel turns it into the background)
}

// one block, thread = system: ewald_setup_kernel's rule with n_eff = atoms + sites, the two backgrounds (ps[s].bg_ext holds Q_ext on
// entry), the image counts; then the slices of the k arrays.  status2[0] = k entries the batch needs, status2[1] = 0.
__global__ __launch_bounds__(256) void embed_pbc_setup_kernel(const float* __restrict__ cell, int n_cell,
                                                              const int* __restrict__ mol_start, const float* __restrict__ charge,
                                                              int nq, int n_mol, const int* __restrict__ ext_start,
                                                              float accuracy, int max_k,
                                                              EwaldSystem* __restrict__ es, EmbedPbcSystem* __restrict__ ps,
                                                              int* __restrict__ status2) {
  for (int s = threadIdx.x; s < n_mol; s += blockDim.x) {
    const double Qe = ps[s].bg_ext;
    double Qa = 0.0;
    for (int ch = 0; ch < nq; ++ch) Qa += (double)charge[(size_t)ch * n_mol + s];
    const int n_eff = max(0, mol_start[s + 1] - mol_start[s]) + max(0, ext_start[s + 1] - ext_start[s]);
    EwaldSystem E;
    EmbedPbcSystem S;
    const double vol = ewald_system_setup(cell + (n_cell == 1 ? 0 : (size_t)s * 9), n_eff, accuracy, Qe, S.cell, E);
    const double al = (double)E.alpha, bg = -3.141592653589793 / (vol * al * al);  // (the alpha the pair terms see)
    S.bg_ext = bg * Qe;
    S.bg_atoms = bg * Qa;
    for (int a = 0; a < 3; ++a) {
      const double h = 1.0 / sqrt(E.inv[a] * E.inv[a] + E.inv[3 + a] * E.inv[3 + a] + E.inv[6 + a] * E.inv[6 + a]);
      S.img[a] = (int)floor((double)E.rc / h + 0.5);
    }
    S.pad = 0;
    es[s] = E;
    ps[s] = S;
  }
  __syncthreads();
  ewald_k_slices(es, n_mol, max_k, status2);
  if (threadIdx.x == 0) status2[1] = 0;
}

// the pair term of one image: p = erfc(alpha d) / d and t = (erfc(alpha d) / d + 2 alpha / sqrt(pi) e^{-alpha^2 d^2}) / d^2, so that
// grad_r [erfc(alpha d) / d] = -t r; false at and beyond rc.  A particle on top of another one (d2 = 0: d = 0 * inf is NaN) is NOT
// outside: its term is not finite and surfaces as status[6] bit 5, as in the non-periodic sums.
__device__ __forceinline__ bool embed_pbc_pair(float rx, float ry, float rz, float al, float c2, float rc, float& p, float& t) {
  const float d2 = fmaf(rz, rz, fmaf(ry, ry, rx * rx));
  const float inv = __builtin_amdgcn_rsqf(d2);
  const float d = d2 * inv;
  if (d >= rc) return false;
  float ex;
  const float ec = erfc_walk(al, d, d2, ex);
  p = ec * inv;
  t = fmaf(c2, ex, p) * inv * inv;
  return true;
}

// The real-space sum over the images of one pair, shared by the atoms' and the sites' kernels.  One system's constants in
// registers: the cell in double (the base vector) and in float (the translations), the image counts, alpha, rc.
struct EmbedPbcImages {
  double Cd[9];
  float C[9];
  int m0, m1, m2;
  float al, rc, c2;
  __device__ __forceinline__ EmbedPbcImages(const EwaldSystem& E, const EmbedPbcSystem& S)
      : m0(S.img[0]), m1(S.img[1]), m2(S.img[2]), al(E.alpha), rc(E.rc), c2(1.1283791670955126f * E.alpha) {
#pragma unroll
    for (int c = 0; c < 9; ++c) {
      Cd[c] = S.cell[c];
      C[c] = (float)S.cell[c];
    }
  }
  // (d0, d1, d2): the fractional difference of the pair, here minus there; w: the charge there.  Reduced to [-1/2, 1/2]^3 in double,
  // then every translation |n_a| <= m_a: acc += w (erfc(alpha d) / d, grad of it with respect to here) over the images inside rc
  __device__ __forceinline__ void add(double d0, double d1, double d2, float w, double acc[4]) const {
    d0 -= rint(d0); d1 -= rint(d1); d2 -= rint(d2);
    const float bx = (float)(d0 * Cd[0] + d1 * Cd[3] + d2 * Cd[6]);
    const float by = (float)(d0 * Cd[1] + d1 * Cd[4] + d2 * Cd[7]);
    const float bz = (float)(d0 * Cd[2] + d1 * Cd[5] + d2 * Cd[8]);
    for (int n0 = -m0; n0 <= m0; ++n0)
      for (int n1 = -m1; n1 <= m1; ++n1)
        for (int n2 = -m2; n2 <= m2; ++n2) {
          const float u0 = (float)n0, u1 = (float)n1, u2 = (float)n2;
          const float rx = fmaf(u2, C[6], fmaf(u1, C[3], fmaf(u0, C[0], bx)));
          const float ry = fmaf(u2, C[7], fmaf(u1, C[4], fmaf(u0, C[1], by)));
          const float rz = fmaf(u2, C[8], fmaf(u1, C[5], fmaf(u0, C[2], bz)));
          float p, t;
          if (embed_pbc_pair(rx, ry, rz, al, c2, rc, p, t)) {
            t *= w;
            acc[0] += (double)(w * p);
            acc[1] -= (double)(t * rx);
            acc[2] -= (double)(t * ry);
            acc[3] -= (double)(t * rz);
          }
        }
  }
};

// block = (atom i, slot s), embed_field_kernel's mapping; the partial goes to slot s of the atom's n_slots + 1
__global__ __launch_bounds__(256) void embed_pbc_field_kernel(const double* __restrict__ frac, const int* __restrict__ mol_c,
                                                              int n_slots, const double* __restrict__ frac_ext,
                                                              const float* __restrict__ ext_charge,
                                                              const int* __restrict__ ext_start, const EwaldSystem* __restrict__ es,
                                                              const EmbedPbcSystem* __restrict__ ps, double* __restrict__ part) {
  __shared__ double sh[4];
  const int i = blockIdx.x / n_slots, s = blockIdx.x % n_slots;
  const size_t po = ((size_t)i * (n_slots + 1) + s) * 4;
  const int m = mol_c[i];
  const int s0 = ext_start[m], cnt = max(0, ext_start[m + 1] - s0);
  const int n_chunk = (int)(((long long)cnt + EMBED_CHUNK - 1) / EMBED_CHUNK);
  if (s >= n_chunk) {  // (block-uniform) this slot has no chunk of the system: its partial is zero
    if (threadIdx.x < 4) part[po + threadIdx.x] = 0.0;
    return;
  }
  const EmbedPbcImages im(es[m], ps[m]);  // (block-uniform)
  const double f0 = frac[3 * (size_t)i], f1 = frac[3 * (size_t)i + 1], f2 = frac[3 * (size_t)i + 2];
  double acc[4] = {0.0, 0.0, 0.0, 0.0};
  for (int k = s; k < n_chunk; k += n_slots) {
    const int lo = k * EMBED_CHUNK;  // (relative to s0: lo < cnt)
    const int hi = (int)min((long long)cnt, (long long)lo + EMBED_CHUNK);
    for (int r = lo + (int)threadIdx.x; r < hi; r += 256) {
      const size_t a = (size_t)s0 + (size_t)r;
      im.add(f0 - frac_ext[3 * a], f1 - frac_ext[3 * a + 1], f2 - frac_ext[3 * a + 2], ext_charge[a], acc);
    }
  }
#pragma unroll
  for (int c = 0; c < 4; ++c) {
    const double v = embed_block_sum(acc[c], sh);
    if (threadIdx.x == 0) part[po + c] = v;
  }
}

// one wave per particle (atom or site), lanes over its system's k entries - ewald_atom_kernel's loop: (phi + background, grad phi)
// as four doubles at out[p * stride + offset].  sites_bg: the background of the sites' charges (the particles are atoms), else of
// the atoms' (the particles are sites).
__global__ __launch_bounds__(256) void embed_pbc_recip_kernel(const double* __restrict__ frac, const int* __restrict__ sys_of, int n,
                                                              const EwaldSystem* __restrict__ es,
                                                              const EmbedPbcSystem* __restrict__ ps, const EwaldK* __restrict__ kk,
                                                              bool sites_bg, double* __restrict__ out, int stride, int offset) {
  const int i = blockIdx.x * 4 + (threadIdx.x >> 6);
  if (i >= n) return;
  const int lane = threadIdx.x & 63;
  const int m = sys_of[i];
  const EwaldSystem& E = es[m];
  const double f0 = frac[(size_t)i * 3], f1 = frac[(size_t)i * 3 + 1], f2 = frac[(size_t)i * 3 + 2];
  double phi = 0.0, g[3] = {0.0, 0.0, 0.0};
  const int e1 = E.k_offset + E.n_box;
  for (int e = E.k_offset + lane; e < e1; e += 64) {
    const EwaldK K = kk[e];
    if (K.P == 0.0 && K.Q == 0.0) continue;
    double ph = (double)K.n1 * f0 + (double)K.n2 * f1 + (double)K.n3 * f2;
    ph -= rint(ph);  // turns, [-1/2, 1/2]
    float sn, cs;
    sincosf((float)(6.283185307179586 * ph), &sn, &cs);
    phi += (double)cs * K.P + (double)sn * K.Q;
    const double d = (double)cs * K.Q - (double)sn * K.P;
    g[0] += d * (double)K.kx; g[1] += d * (double)K.ky; g[2] += d * (double)K.kz;
  }
  phi = wave_sum(phi);
  for (int c = 0; c < 3; ++c) g[c] = wave_sum(g[c]);
  if (lane != 0) return;
  double* o = out + (size_t)i * stride + offset;
  o[0] = phi + (sites_bg ? ps[m].bg_ext : ps[m].bg_atoms);
  o[1] = g[0]; o[2] = g[1]; o[3] = g[2];
}

// thread = site, block = 256 consecutive sites - embed_site_kernel's mapping: the atoms (fractional coordinates, q) of every system
// the block's sites belong to pass through LDS in tiles of 256; a thread sums over its system's atoms in atom order, every
// translation of a pair inside; then the reciprocal-space sums of the site (site_part, background included) join.
__global__ __launch_bounds__(256) void embed_pbc_site_kernel(const double* __restrict__ frac, const float* __restrict__ q,
                                                             const int* __restrict__ mol_start, const double* __restrict__ frac_ext,
                                                             const float* __restrict__ ext_charge, const int* __restrict__ ext_mol_c,
                                                             int n_ext, const EwaldSystem* __restrict__ es,
                                                             const EmbedPbcSystem* __restrict__ ps, const double* __restrict__ site_part,
                                                             float* __restrict__ ext_forces, float* __restrict__ ext_potential) {
  __shared__ double tile_f[256][3];
  __shared__ float tile_q[256];
  const int a0 = blockIdx.x * 256, a = a0 + (int)threadIdx.x;
  const bool live = a < n_ext;
  const int a_last = min(n_ext, a0 + 256) - 1;
  const int mf = ext_mol_c[a0], ml = ext_mol_c[a_last];  // (block-uniform; a sorted list: the block's systems lie between them)
  const int m_lo = min(mf, ml), m_hi = max(mf, ml);
  const int mine = live ? ext_mol_c[a] : -1;
  double F0 = 0.0, F1 = 0.0, F2 = 0.0;
  if (live) { F0 = frac_ext[3 * (size_t)a]; F1 = frac_ext[3 * (size_t)a + 1]; F2 = frac_ext[3 * (size_t)a + 2]; }
  double acc[4] = {0.0, 0.0, 0.0, 0.0};
  for (int m = m_lo; m <= m_hi; ++m) {
    const EmbedPbcImages im(es[m], ps[m]);  // (block-uniform)
    const int i0 = mol_start[m], i1 = mol_start[m + 1];
    for (int t0 = i0; t0 < i1; t0 += 256) {
      const int nt = min(256, i1 - t0);
      __syncthreads();
      if ((int)threadIdx.x < nt) {
        const size_t i = (size_t)t0 + threadIdx.x;
        tile_f[threadIdx.x][0] = frac[3 * i]; tile_f[threadIdx.x][1] = frac[3 * i + 1]; tile_f[threadIdx.x][2] = frac[3 * i + 2];
        tile_q[threadIdx.x] = q[i];
      }
      __syncthreads();
      if (mine == m) {
        for (int k = 0; k < nt; ++k) im.add(F0 - tile_f[k][0], F1 - tile_f[k][1], F2 - tile_f[k][2], tile_q[k], acc);
      }
    }
  }
  if (!live) return;
#pragma unroll
  for (int c = 0; c < 4; ++c) acc[c] += site_part[4 * (size_t)a + c];
  if (ext_potential) ext_potential[a] = (float)(KE * acc[0]);
  if (ext_forces) {
    const double kq = -KE * (double)ext_charge[a];  // -dE_emb/dX_A = -Q_A grad psi_A
#pragma unroll
    for (int c = 0; c < 3; ++c) ext_forces[3 * (size_t)a + c] = (float)(kq * acc[1 + c]);
  }
}

}  // namespace

void embed_carve(EmbedBuffers& b, char* base, int n_atoms, int n_mol, int n_ext, bool tensor) {
  size_t off = 0;
  auto take = [&](size_t bytes) {
    char* r = base ? base + off : nullptr;
    off += align_up(bytes, 256);
    return r;
  };
  const size_t n = (size_t)n_atoms, ns = (size_t)embed_slots(n_ext, n_mol);
  b.ext_start = (int*)take(((size_t)n_mol + 1) * sizeof(int));
  b.ext_mol_c = (int*)take((size_t)n_ext * sizeof(int));
  b.part = (double*)take(n * ns * (tensor ? EMBED_NP_TENSOR : 4) * sizeof(double));
  b.e_atom = (double*)take(tensor ? 0 : n * sizeof(double));  // (the tangent sweep forms no energy)
  b.total = off;
}

int launch_embed_sites(hipStream_t s, const int* ext_mol_idx, int n_ext, int n_mol, const EmbedBuffers& b, int* status6) {
  if (n_ext <= 0) return 0;
  hipLaunchKernelGGL(embed_sites_kernel, dim3(ceil_div(n_ext, 256)), dim3(256), 0, s, ext_mol_idx, n_ext, n_mol, b.ext_start,
                     b.ext_mol_c, status6);
  AIMNET_LAUNCH_CHECK();
  return 0;
}

int launch_embed_field(hipStream_t s, const float* x, const int* mol_c, int n_atoms, int n_mol, const float* ext_coord,
                       const float* ext_charge, int n_ext, const EmbedBuffers& b, bool tensor) {
  const int ns = embed_slots(n_ext, n_mol);
  if (ns == 0 || n_atoms <= 0) return 0;
  if ((long long)n_atoms * ns > (long long)INT32_MAX) {
    set_last_error("embedding: n_atoms * slots exceeds the grid limit");
    return -1;
  }
  const dim3 grid((unsigned)(n_atoms * ns)), block(256);
  if (tensor)
    hipLaunchKernelGGL((embed_field_kernel<true>), grid, block, 0, s, x, mol_c, ns, ext_coord, ext_charge, b.ext_start, b.part);
  else
    hipLaunchKernelGGL((embed_field_kernel<false>), grid, block, 0, s, x, mol_c, ns, ext_coord, ext_charge, b.ext_start, b.part);
  AIMNET_LAUNCH_CHECK();
  return 0;
}

int launch_embed_seed(hipStream_t s, bool grad, const float* q, int n_atoms, int n_ext, const float* potential,
                      const float* potential_grad, const EmbedBuffers& b, double* ecoul, float* qbar, float* fgrad,
                      const int* mol_start, int n_mol, double* energy, int extra_slots) {
  const int ns = embed_slots(n_ext, n_mol) + extra_slots;
  const dim3 grid(ceil_div(n_atoms, 256)), block(256);
  if (grad)
    hipLaunchKernelGGL((embed_seed_kernel<true>), grid, block, 0, s, q, n_atoms, ns, b.part, potential, potential_grad, b.e_atom, ecoul,
                       qbar, fgrad);
  else
    hipLaunchKernelGGL((embed_seed_kernel<false>), grid, block, 0, s, q, n_atoms, ns, b.part, potential, potential_grad, b.e_atom,
                       ecoul, qbar, fgrad);
  AIMNET_LAUNCH_CHECK();
  if (energy) {
    hipLaunchKernelGGL(embed_energy_kernel, dim3(n_mol), dim3(256), 0, s, b.e_atom, mol_start, energy);
    AIMNET_LAUNCH_CHECK();
  }
  return 0;
}

int launch_embed_site_pass(hipStream_t s, const float* x, const float* q, const int* mol_start, int n_mol, const float* ext_coord,
                           const float* ext_charge, int n_ext, const EmbedBuffers& b, float* ext_forces, float* ext_potential) {
  if (n_ext <= 0 || (!ext_forces && !ext_potential)) return 0;
  hipLaunchKernelGGL(embed_site_kernel, dim3(ceil_div(n_ext, 256)), dim3(256), 0, s, x, q, mol_start, n_mol, ext_coord, ext_charge,
                     b.ext_mol_c, n_ext, ext_forces, ext_potential);
  AIMNET_LAUNCH_CHECK();
  return 0;
}

void embed_pbc_carve(EmbedPbcBuffers& b, char* base, int n_atoms, int n_mol, int n_ext, int max_k) {
  size_t off = 0;
  auto take = [&](size_t bytes) {
    char* r = base ? base + off : nullptr;
    off += align_up(bytes, 256);
    return r;
  };
  const size_t n = (size_t)n_atoms, nm = (size_t)n_mol, ne = (size_t)n_ext, nk = (size_t)std::max(0, max_k);
  b = EmbedPbcBuffers{};
  b.ew.sys = (EwaldSystem*)take(nm * sizeof(EwaldSystem));
  b.ps = (EmbedPbcSystem*)take(nm * sizeof(EmbedPbcSystem));
  b.ew.frac = (double*)take(n * 3 * sizeof(double));
  b.frac_ext = (double*)take(ne * 3 * sizeof(double));
  b.ew.k = (EwaldK*)take(nk * sizeof(EwaldK));
  b.k_atoms = (EwaldK*)take(nk * sizeof(EwaldK));
  b.ew.max_k = max_k;
  b.part = (double*)take(n * ((size_t)embed_slots(n_ext, n_mol) + 1) * 4 * sizeof(double));
  b.site_part = (double*)take(ne * 4 * sizeof(double));
  b.total = off;
}

int launch_embed_pbc_field(hipStream_t s, const float* x, const int* mol_c, const int* mol_start, int n_atoms, int n_mol,
                           const float* cell, int n_cell, const float* charge, int nq, const float* ext_coord, const float* ext_charge,
                           int n_ext, float accuracy, const EmbedBuffers& eb, EmbedPbcBuffers& b, int* status2) {
  const int ns = embed_slots(n_ext, n_mol);
  if (ns == 0 || n_atoms <= 0) return 0;
  if ((long long)n_atoms * ns > (long long)INT32_MAX) {
    set_last_error("embedding: n_atoms * slots exceeds the grid limit");
    return -1;
  }
  hipLaunchKernelGGL(embed_pbc_charge_kernel, dim3(n_mol), dim3(256), 0, s, eb.ext_start, ext_charge, b.ps);
  AIMNET_LAUNCH_CHECK();
  hipLaunchKernelGGL(embed_pbc_setup_kernel, dim3(1), dim3(256), 0, s, cell, n_cell, mol_start, charge, nq, n_mol, eb.ext_start,
                     accuracy, b.ew.max_k, b.ew.sys, b.ps, status2);
  AIMNET_LAUNCH_CHECK();
  EwaldBuffers sites = b.ew;  // the same systems and k array, the sites' fractional coordinates
  sites.frac = b.frac_ext;
  if (const int rc = launch_ewald_frac(s, x, mol_c, n_atoms, b.ew)) return rc;
  if (const int rc = launch_ewald_frac(s, ext_coord, eb.ext_mol_c, n_ext, sites)) return rc;
  if (const int rc = launch_ewald_sfac(s, ext_charge, eb.ext_start, n_mol, sites)) return rc;  // A(k) S_ext(k)
  hipLaunchKernelGGL(embed_pbc_field_kernel, dim3((unsigned)(n_atoms * ns)), dim3(256), 0, s, b.ew.frac, mol_c, ns, b.frac_ext,
                     ext_charge, eb.ext_start, b.ew.sys, b.ps, b.part);
  AIMNET_LAUNCH_CHECK();
  hipLaunchKernelGGL(embed_pbc_recip_kernel, dim3(ceil_div(n_atoms, 4)), dim3(256), 0, s, b.ew.frac, mol_c, n_atoms, b.ew.sys, b.ps,
                     b.ew.k, true, b.part, (ns + 1) * 4, ns * 4);
  AIMNET_LAUNCH_CHECK();
  return 0;
}

int launch_embed_pbc_site_pass(hipStream_t s, const float* q, const int* mol_start, int n_atoms, int n_mol, const float* ext_charge,
                               int n_ext, const EmbedBuffers& eb, const EmbedPbcBuffers& b, float* ext_forces, float* ext_potential) {
  if (n_ext <= 0 || n_atoms <= 0 || (!ext_forces && !ext_potential)) return 0;
  EwaldBuffers atoms = b.ew;  // the atoms' fractional coordinates, the second k array: A(k) S_q(k)
  atoms.k = b.k_atoms;
  if (const int rc = launch_ewald_sfac(s, q, mol_start, n_mol, atoms)) return rc;
  hipLaunchKernelGGL(embed_pbc_recip_kernel, dim3(ceil_div(n_ext, 4)), dim3(256), 0, s, b.frac_ext, eb.ext_mol_c, n_ext, b.ew.sys, b.ps,
                     b.k_atoms, false, b.site_part, 4, 0);
  AIMNET_LAUNCH_CHECK();
  hipLaunchKernelGGL(embed_pbc_site_kernel, dim3(ceil_div(n_ext, 256)), dim3(256), 0, s, b.ew.frac, q, mol_start, b.frac_ext, ext_charge,
                     eb.ext_mol_c, n_ext, b.ew.sys, b.ps, b.site_part, ext_forces, ext_potential);
  AIMNET_LAUNCH_CHECK();
  return 0;
}

int launch_embed_tseed(hipStream_t s, const float* q, const float* tq, int nq, const float* vectors, int n_atoms, int n_vec, int n_ext,
                       int n_mol, const float* potential, const float* potential_grad, const float* potential_hess,
                       const EmbedBuffers& b, float* qbar, float* tqbar, float* xbar, float* txbar, double* field) {
  if (n_atoms <= 0 || n_vec <= 0) return 0;
  hipLaunchKernelGGL(embed_tseed_kernel, dim3(ceil_div(n_atoms, 256), n_vec), dim3(256), 0, s, q, tq, nq, vectors, n_atoms,
                     embed_slots(n_ext, n_mol), b.part, potential, potential_grad, potential_hess, qbar, tqbar, xbar, txbar, field);
  AIMNET_LAUNCH_CHECK();
  return 0;
}

int launch_embed_tsite(hipStream_t s, const float* x, const float* q, const float* tq, int nq, const float* vectors, int n_atoms,
                       int n_vec, const int* mol_start, const float* ext_coord, const float* ext_charge, int n_ext,
                       const EmbedBuffers& b, float* ext_hv) {
  if (n_ext <= 0 || n_vec <= 0 || !ext_hv) return 0;
  hipLaunchKernelGGL(embed_tsite_kernel, dim3(ceil_div(n_ext, 256), n_vec), dim3(256), 0, s, x, q, tq, nq, vectors, n_atoms, mol_start,
                     ext_coord, ext_charge, b.ext_mol_c, n_ext, ext_hv);
  AIMNET_LAUNCH_CHECK();
  return 0;
}

}  // namespace aimnet
