// embed.hip - electrostatic embedding of the model's charges in an external potential (aimnet_engine_set_embedding):
//   E_emb = sum_i q_i phi_i,  phi_i = k_e sum_A Q_A / |x_i - X_A| + potential_i,  k_e = Hartree * Bohr (eV A / e^2)
// over the point charges (X_A, Q_A) of atom i's own molecule and / or a per-atom potential the caller computed.  The charges do not
// respond to the field (they are the model's): this is the first-order coupling with its exact gradient
//   dE_emb/dx_i = q_i grad phi_i + sum_j phi_j dq_j/dx_i ,
// whose second term is the backward sweep's own job - the seed pass adds phi_i to the adjoint dE/dq_i (qbar) that the Coulomb block
// has seeded, exactly as the Ewald block does with its potential.
// Pair terms in fp32, every sum in double; no atomics on results, fixed summation orders: bitwise repeatable.
#include "common.h"
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
// (sum Q / d, -sum Q (x_i - X) / d^3) per block; it depends on the geometry alone.
__global__ __launch_bounds__(256) void embed_field_kernel(const float* __restrict__ x, const int* __restrict__ mol_c, int n_slots,
                                                          const float* __restrict__ ext_coord,
                                                          const float* __restrict__ ext_charge,
                                                          const int* __restrict__ ext_start, double* __restrict__ part) {
  __shared__ double sh[4];
  const int i = blockIdx.x / n_slots, s = blockIdx.x % n_slots;
  const int m = mol_c[i];
  const int s0 = ext_start[m], cnt = max(0, ext_start[m + 1] - s0);
  const int n_chunk = (int)(((long long)cnt + EMBED_CHUNK - 1) / EMBED_CHUNK);
  if (s >= n_chunk) {  // (block-uniform) this slot has no chunk of the molecule: its partial is zero
    if (threadIdx.x < 4) part[(size_t)blockIdx.x * 4 + threadIdx.x] = 0.0;
    return;
  }
  const float xi = x[3 * (size_t)i], yi = x[3 * (size_t)i + 1], zi = x[3 * (size_t)i + 2];
  double acc[4] = {0.0, 0.0, 0.0, 0.0};
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
    }
  }
#pragma unroll
  for (int c = 0; c < 4; ++c) {
    const double v = embed_block_sum(acc[c], sh);
    if (threadIdx.x == 0) part[(size_t)blockIdx.x * 4 + c] = v;
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

}  // namespace

void embed_carve(EmbedBuffers& b, char* base, int n_atoms, int n_mol, int n_ext) {
  size_t off = 0;
  auto take = [&](size_t bytes) {
    char* r = base ? base + off : nullptr;
    off += align_up(bytes, 256);
    return r;
  };
  const size_t n = (size_t)n_atoms, ns = (size_t)embed_slots(n_ext, n_mol);
  b.ext_start = (int*)take(((size_t)n_mol + 1) * sizeof(int));
  b.ext_mol_c = (int*)take((size_t)n_ext * sizeof(int));
  b.part = (double*)take(n * ns * 4 * sizeof(double));
  b.e_atom = (double*)take(n * sizeof(double));
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
                       const float* ext_charge, int n_ext, const EmbedBuffers& b) {
  const int ns = embed_slots(n_ext, n_mol);
  if (ns == 0) return 0;
  if ((long long)n_atoms * ns > (long long)INT32_MAX) {
    set_last_error("embedding: n_atoms * slots exceeds the grid limit");
    return -1;
  }
  hipLaunchKernelGGL(embed_field_kernel, dim3((unsigned)(n_atoms * ns)), dim3(256), 0, s, x, mol_c, ns, ext_coord, ext_charge,
                     b.ext_start, b.part);
  AIMNET_LAUNCH_CHECK();
  return 0;
}

int launch_embed_seed(hipStream_t s, bool grad, const float* q, int n_atoms, int n_ext, const float* potential,
                      const float* potential_grad, const EmbedBuffers& b, double* ecoul, float* qbar, float* fgrad,
                      const int* mol_start, int n_mol, double* energy) {
  const int ns = embed_slots(n_ext, n_mol);
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

}  // namespace aimnet
