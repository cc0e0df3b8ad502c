// Shared by ewald.hip, pme.hip and embed.hip: the cell's inverse (fractional coordinates) in double, and the per-system Ewald setup
// (parameters from the cell, the k box, the slices of the k arrays) that the system's own sum and the embedding's site sums share.
#pragma once
#include <hip/hip_runtime.h>

#include "kernels.h"

namespace aimnet {

constexpr double EW_TWO_PI = 6.283185307179586;

// m = the row-vector cell in double, E.inv = its inverse (fractional coordinate a = sum_c x_c inv[c * 3 + a]); returns det(cell)
__device__ __forceinline__ double ewald_cell_geometry(const float* __restrict__ c, double m[9], EwaldSystem& E) {
  for (int k = 0; k < 9; ++k) m[k] = c[k];
  const double det = m[0] * (m[4] * m[8] - m[5] * m[7]) - m[1] * (m[3] * m[8] - m[5] * m[6]) + m[2] * (m[3] * m[7] - m[4] * m[6]);
  const double id = 1.0 / det;
  E.inv[0] = (m[4] * m[8] - m[5] * m[7]) * id;
  E.inv[1] = (m[2] * m[7] - m[1] * m[8]) * id;
  E.inv[2] = (m[1] * m[5] - m[2] * m[4]) * id;
  E.inv[3] = (m[5] * m[6] - m[3] * m[8]) * id;
  E.inv[4] = (m[0] * m[8] - m[2] * m[6]) * id;
  E.inv[5] = (m[2] * m[3] - m[0] * m[5]) * id;
  E.inv[6] = (m[3] * m[7] - m[4] * m[6]) * id;
  E.inv[7] = (m[1] * m[6] - m[0] * m[7]) * id;
  E.inv[8] = (m[0] * m[4] - m[1] * m[3]) * id;
  return det;
}

// One system's parameters and k box from its cell c, the particle count n_eff the balance rule sees, the accuracy and the total charge
// Q of the particles whose background phi_bg is: eta = (V^2 / n_eff)^(1/6) / sqrt(2 pi), alpha = 1 / (sqrt(2) eta), rc = f eta,
// kc = f / eta, f = sqrt(-2 ln accuracy).  k_offset = 0 and the untruncated n_box: ewald_k_slices assigns the slices.  m: the cell
// in double.  Returns the volume.
__device__ __forceinline__ double ewald_system_setup(const float* __restrict__ c, int n_eff, float accuracy, double Q, double m[9],
                                                     EwaldSystem& E) {
  const double det = ewald_cell_geometry(c, m, E);
  const double vol = fabs(det);
  const int ns = max(1, n_eff);
  const double eta = cbrt(sqrt(vol * vol / (double)ns)) / sqrt(EW_TWO_PI);
  const double f = sqrt(-2.0 * log((double)accuracy));
  const double alpha = 1.0 / (sqrt(2.0) * eta), rc = f * eta, kc = f / eta;
  E.alpha = (float)alpha;
  E.rc = (float)rc;
  E.kc2 = (float)(kc * kc);
  E.inv4a2 = (float)(1.0 / (4.0 * alpha * alpha));
  E.phi_bg = (float)(-3.141592653589793 * Q / (vol * alpha * alpha));
  E.pref = 8.0 * 3.141592653589793 / vol;
  for (int a = 0; a < 3; ++a) {
    for (int cc = 0; cc < 3; ++cc) E.b[a * 3 + cc] = EW_TWO_PI * E.inv[cc * 3 + a];
    const double len = sqrt(m[3 * a] * m[3 * a] + m[3 * a + 1] * m[3 * a + 1] + m[3 * a + 2] * m[3 * a + 2]);
    E.nmax[a] = (int)floor(kc * len / EW_TWO_PI);
  }
  E.n2w = 2 * E.nmax[1] + 1;
  E.n3w = 2 * E.nmax[2] + 1;
  const long box = (long)(E.nmax[0] + 1) * E.n2w * E.n3w;
  E.n_box = (int)min(box, (long)(1 << 28));
  E.k_offset = 0;
  return vol;
}

// Called by every thread of ONE block after es[0 .. n_mol) is written and a __syncthreads(): the slices of the k arrays, offsets =
// running sum of the box sizes padded to whole blocks of the structure-factor kernel; *status_k = the entries the batch needs.  The
// serial pass runs over LDS (a batch of 10^3 small cells would otherwise pay a dependent global round trip per system); batches
// beyond the LDS table take the slow form.
__device__ __forceinline__ void ewald_k_slices(EwaldSystem* __restrict__ es, int n_mol, int max_k, int* __restrict__ status_k) {
  constexpr int TAB = 4096;
  __shared__ int s_need[TAB];
  __shared__ long s_total;
  const bool in_lds = n_mol <= TAB;
  if (in_lds)
    for (int s = threadIdx.x; s < n_mol; s += blockDim.x) s_need[s] = (es[s].n_box + EWALD_KB - 1) / EWALD_KB * EWALD_KB;
  __syncthreads();
  if (threadIdx.x == 0) {
    long off = 0;
    for (int s = 0; s < n_mol; ++s) {
      const long need = in_lds ? (long)s_need[s] : ((long)es[s].n_box + EWALD_KB - 1) / EWALD_KB * EWALD_KB;
      const long at = min(off, (long)max_k);
      const int take = (int)max(0L, min(need, (long)max_k - at));  // truncated when the capacity is too small (flagged)
      if (in_lds) {
        s_need[s] = (int)at;  // (the offset; the size follows from the next offset below)
      } else {
        es[s].k_offset = (int)at;
        es[s].n_box = take;
      }
      off += need;
    }
    s_total = off;
    *status_k = (int)min(off, (long)INT32_MAX);
  }
  __syncthreads();
  if (in_lds)
    for (int s = threadIdx.x; s < n_mol; s += blockDim.x) {
      const long end = s + 1 < n_mol ? (long)s_need[s + 1] : min(s_total, (long)max_k);
      es[s].k_offset = s_need[s];
      es[s].n_box = (int)max(0L, min(end, (long)max_k) - (long)s_need[s]);
    }
}

}  // namespace aimnet
