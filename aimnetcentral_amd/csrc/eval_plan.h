// eval_plan.h - every decision of one aimnet_engine_eval call, taken once from plain values and named once.  Host code only (no
// HIP): engine.hip fills an EvalRequest, checks it (eval_validate / eval_validate_lists), plans it (eval_plan) and then runs its
// stages off the plan; tests/eval_plan_main.cpp walks the same three functions on the CPU.  The part of the plan that depends on
// (engine, n_atoms, n_mol, options) alone is LayoutPlan: aimnet_engine_workspace_bytes has no inputs and fills just that.
#pragma once

#include <stdarg.h>
#include <stdint.h>
#include <stdio.h>

#include <algorithm>

#include "../../include/aimnet_hip.h"

namespace aimnet {

// ---- what the workspace layout depends on ---------------------------------------------------------------------------------
struct LayoutRequest {
  int N, n_mol, n_pass;
  unsigned flags;          // AIMNET_FORCES | AIMNET_STRESS
  int coulomb, dftd3;      // options.coulomb, options.dftd3
  bool d3_same_cutoff;     // options.d3_cutoff == options.dsf_rc (on the float32 fields)
  int max_nb, max_nb_lr, max_nb_d3, ewald_max_k, pme_max_mesh;  // options, as the caller passed them
  int ewald_kb, pme_part;  // EWALD_KB, PME_PART (kernels.h)
  int conv_xe, split_max;  // engine switches
  bool pair_rev_ok;        // pair_rev_supported(N, cap)
  int split_format;        // split_format(engine, N): SPLIT_NONE / SPLIT_BF3 / SPLIT_H2
  int split_planes;        // 16-bit elements per fp32 value of a split row (split_planes(split_format))
};
struct LayoutPlan {
  bool grad;
  int cap, cap_lr;      // row capacities of the short-range and of the long-range buffers
  int cap_d3;           // of the D3 buffers; 0: none of their own (no D3, or the D3 matrix lives in the long-range buffers)
  bool d3_in_lr;        // D3 at the DSF cutoff, long-range buffers present: ONE matrix is stored
  int ewald_max_k, pme_max_mesh, pme_max_parts;  // Ewald k entries / PME mesh points and blocks of one system (0: method not chosen)
  bool xe;              // reverse-pair conv backward: pair buffer, reverse map and hash tables exist
  int split_format, split_planes;
  int S;                // slices per molecule of the molecule reductions
};
inline LayoutPlan layout_plan(const LayoutRequest& r) {
  LayoutPlan L{};
  L.grad = (r.flags & (AIMNET_FORCES | AIMNET_STRESS)) != 0;
  L.cap = std::max(1, r.max_nb);
  L.cap_lr = std::max(0, r.max_nb_lr);
  // The D3 list and the list-based DSF list are the same neighbour matrix when their cutoffs agree (both default to 15 A): it is
  // stored once.  The layout does not know about periodicity: max_nb_lr > 0 means "a DSF list may be built".
  L.d3_in_lr = r.dftd3 != 0 && r.coulomb == AIMNET_COULOMB_DSF && L.cap_lr > 0 && r.d3_same_cutoff;
  L.cap_d3 = r.dftd3 != 0 && !L.d3_in_lr ? std::max(1, r.max_nb_d3) : 0;
  L.ewald_max_k = r.coulomb == AIMNET_COULOMB_EWALD ? std::max(r.ewald_kb, r.ewald_max_k / r.ewald_kb * r.ewald_kb) : 0;
  L.pme_max_mesh = r.coulomb == AIMNET_COULOMB_PME ? std::max(512, r.pme_max_mesh) : 0;
  L.pme_max_parts = (L.pme_max_mesh + r.pme_part - 1) / r.pme_part;
  L.xe = r.conv_xe != 0 && L.grad && r.n_pass > 1 && r.N > r.split_max && r.pair_rev_ok &&
         (size_t)r.N * (size_t)L.cap < (size_t)INT32_MAX;
  L.split_format = r.split_format;
  L.split_planes = r.split_planes;
  L.S = std::min(128, std::max(1, (r.N / std::max(1, r.n_mol) + 511) / 512));
  return L;
}

// ---- one evaluation ---------------------------------------------------------------------------------------------------------
struct EvalRequest {
  LayoutRequest L;
  int n_cell, nq;
  bool pbc;                                     // inputs.cell given
  bool has_stress_out, has_forces_out, has_spin_out;
  int ewald_args;                               // Ewald / PME only: ewald_args_check (engine.h) of the inputs, else 0
  // caller-supplied matrices
  bool nbmat, shifts, nbmat_lr, shifts_lr, nbmat_d3, shifts_d3;
  int nbmat_width, nbmat_lr_width, nbmat_d3_width;
  bool dd;                                      // domain decomposition on (aimnet_engine_set_dd)
  bool d3_tables;                               // aimnet_engine_set_dftd3 was called
  // engine switches the plan reads
  int prep_fused, energy_rides, status_rides, setup_rides, status_owned, nse_merged, d3_cn_rides, dsf_np_walk, p0_moments,
      spatial_order;
  // size predicates (kernels.h, engine.h)
  bool prep_small_ok;   // prep_small_applies(N, n_mol, pbc)
  bool cell_setup_ok;   // cell_setup_rides(N, n_mol)
  bool bbox_ok;         // bbox_applies(N, n_mol)
  bool head_fusable;    // head_fusable(engine)
  // electrostatic embedding (aimnet_engine_set_embedding); emb == 0: off, nothing below is read
  int emb;
  int emb_n_ext;                                            // point charges
  bool emb_sites_ok;                                        // n_ext == 0, or ext_coord and ext_charge given
  bool emb_ext_mol_idx, emb_potential, emb_potential_grad;  // which optional arrays are given
  bool emb_scratch_ok;                                      // scratch given and at least aimnet_embedding_scratch_bytes
  // sites periodic with the cell (aimnet_engine_set_embedding_periodic); emb_periodic == 0: unarmed, nothing below is read
  int emb_periodic;
  bool emb_pbc_full;                                        // pbc all true and no per-system flags
  float emb_periodic_accuracy;
  int emb_periodic_max_k;
  bool emb_periodic_status;                                 // status given
  bool emb_periodic_scratch_ok;                             // scratch given and at least aimnet_embedding_periodic_scratch_bytes
};

enum class Prep { FusedSmall, Separate, SeparateSetupRider };  // launch_prep_small / launch_mol_start + launch_wrap (+ the setup rider)
enum class StatusZero { Memset, FusedPrep, RiderOwned };       // who leaves the eight status words defined
enum class ListFrom { None, Built, Imported, LongRange };      // LongRange (D3 only): the long-range list as it stands
enum class LongRange { None, SimpleInSr, SimpleMatrix, DsfMatrix, DsfInD3, DsfWalk, EwaldWalk, PmeWalk };
enum class RevLookup { None, OnWalk, OnEnergyLaunch };         // the lookup of the reverse-pair map (its hash build rides on SR-Coulomb)
enum class EnergySum { OwnLaunch, StressRider, ForceRider };
enum class ChargesBy { Walk, EnergyLaunch, ForceRider };
enum class NseAdjoint { Decomposed, Merged, Sliced };

struct EvalPlan {
  LayoutPlan layout;
  bool want_f, want_s, grad, ext;
  Prep prep;
  StatusZero status;
  bool sr_status_rides;  // the short-range list's status words are reduced by rider blocks of the SR-Coulomb launch
  bool want_species;     // species slots + present masks are formed (pass-0 moments, DFT-D3)
  bool bbox;             // non-periodic: bounding-box cell grid
  bool binned;           // the list builder (and the bin order) see a cell grid
  ListFrom sr, lr, d3;
  int cap_d3;            // row capacity of the D3 list where it sits
  bool d3_cn_rides;      // the coordination numbers ride on the build of the D3 list
  LongRange lr_term;
  bool stream_rides;     // the (x, y, z, q) stream of the list-free walk rides on the SR-Coulomb launch
  bool rev_hash;         // hash build of the reverse-pair map (rider of the SR-Coulomb launch)
  RevLookup rev_lookup;
  EnergySum energy;
  ChargesBy charges;
  bool pair_force_rides;  // the pair-force gather rides on the stress launch
  NseAdjoint nse;
  bool head_fused, p0_moments, bin_order;
};

inline bool lr_is_walk(LongRange t) { return t == LongRange::DsfWalk || t == LongRange::EwaldWalk || t == LongRange::PmeWalk; }

// large non-periodic systems evaluate DSF by the list-free walk over the bounding-box grid, unless the pair terms ride on D3
inline bool plan_np_walk(const EvalRequest& r) {
  return r.dsf_np_walk && !r.pbc && !r.nbmat && r.L.coulomb == AIMNET_COULOMB_DSF && r.bbox_ok && !(r.L.dftd3 != 0 && r.L.d3_same_cutoff);
}

// ---- argument checks: 0, or AIMNET_E_INVALID with the message in msg -----------------------------------------------------------
inline int plan_reject(char* msg, size_t n, const char* fmt, ...) {
  va_list ap;
  va_start(ap, fmt);
  vsnprintf(msg, n, fmt, ap);
  va_end(ap);
  return AIMNET_E_INVALID;
}
inline int eval_validate(const EvalRequest& r, char* msg, size_t n) {
  const bool want_f = (r.L.flags & AIMNET_FORCES) != 0, want_s = (r.L.flags & AIMNET_STRESS) != 0;
  const int coulomb = r.L.coulomb;
  if (want_s && ((!r.pbc && !r.dd) || !r.has_stress_out))  // (domain decomposition: the rank's virial, see aimnet_engine_set_dd)
    return plan_reject(msg, n, "eval: stress requires a cell and a stress buffer");
  if (want_f && !r.has_forces_out) return plan_reject(msg, n, "eval: forces requested without a forces buffer");
  if (r.nq == 1 && r.has_spin_out) return plan_reject(msg, n, "eval: spin_charges requested from a 1-channel (closed-shell) model");
  if (r.pbc && !(r.n_cell == 1 || r.n_cell == r.L.n_mol)) return plan_reject(msg, n, "eval: n_cell must be 1 or n_mol");
  if (coulomb == AIMNET_COULOMB_DSF && !r.pbc && r.L.max_nb_lr <= 0 && !plan_np_walk(r))
    return plan_reject(msg, n, "eval: non-periodic DSF Coulomb needs max_nb_lr > 0 (periodic DSF walks the cell grid, no list)");
  if (coulomb == AIMNET_COULOMB_SIMPLE && r.pbc)
    return plan_reject(msg, n, "eval: 'simple' Coulomb is undefined for periodic input (host must switch to DSF, calculator.py:1044)");
  if (coulomb == AIMNET_COULOMB_EWALD || coulomb == AIMNET_COULOMB_PME) {
    if (r.ewald_args == 1)
      return plan_reject(msg, n, "eval: Ewald summation needs a cell that is periodic along all three axes (lr.py:655-657)");
    if (r.nbmat)
      return plan_reject(msg, n,
                         "eval: Ewald summation walks the engine's own cell grid: caller-supplied neighbour matrices are not taken with it "
                         "(the reference builds its own per-call list for this method too, calculator.py:1560-1603)");
    if (r.ewald_args)
      return plan_reject(msg, n, "eval: Ewald summation needs 0 < ewald_accuracy < 1 and ewald_max_k >= %d (PME: pme_max_mesh >= 512)",
                         r.L.ewald_kb);
  }
  // caller-supplied neighbour matrices (aimnet_inputs.nbmat ...): no list is built, the coordinates are taken as given
  if (r.nbmat) {
    if (r.nbmat_width <= 0 || r.L.max_nb < r.nbmat_width)
      return plan_reject(msg, n, "eval: caller-supplied nbmat needs 0 < nbmat_width <= options.max_nb (got %d, %d)", r.nbmat_width,
                         r.L.max_nb);
    if (r.pbc && !r.shifts) return plan_reject(msg, n, "eval: a caller-supplied nbmat of a periodic system needs its shifts");
    if (r.nbmat_lr && (r.nbmat_lr_width <= 0 || r.L.max_nb_lr < r.nbmat_lr_width || (r.pbc && !r.shifts_lr)))
      return plan_reject(msg, n,
                         "eval: caller-supplied nbmat_lr needs 0 < nbmat_lr_width <= options.max_nb_lr, and shifts_lr when periodic");
    if (coulomb == AIMNET_COULOMB_DSF && !r.nbmat_lr)
      return plan_reject(msg, n, "eval: DSF Coulomb with a caller-supplied nbmat needs nbmat_lr as well (no list is built in this mode)");
    if (r.L.dftd3 != 0) {
      if (!r.nbmat_d3 && !r.nbmat_lr) return plan_reject(msg, n, "eval: DFT-D3 with a caller-supplied nbmat needs nbmat_d3 or nbmat_lr");
      if (r.nbmat_d3 && (r.nbmat_d3_width <= 0 || (r.pbc && !r.shifts_d3)))
        return plan_reject(msg, n, "eval: caller-supplied nbmat_d3 needs a width, and shifts_d3 when periodic");
    }
  } else if (r.nbmat_lr || r.nbmat_d3) {
    return plan_reject(msg, n, "eval: nbmat_lr / nbmat_d3 are only read together with nbmat");
  }
  // spatial domain decomposition (aimnet_engine_set_dd): the local cluster of owned + halo atoms is a non-periodic system
  if (r.dd && (r.pbc || r.nbmat || !(coulomb == AIMNET_COULOMB_NONE || coulomb == AIMNET_COULOMB_DSF)))
    return plan_reject(msg, n,
                       "eval: a domain-decomposed evaluation takes a non-periodic cluster (no cell, no caller-supplied lists), Coulomb "
                       "'none' or 'dsf'");
  // electrostatic embedding (aimnet_engine_set_embedding)
  if (r.emb) {
    if (want_s) return plan_reject(msg, n, "eval: the embedding term has no stress (AIMNET_STRESS with an embedding set)");
    if (r.dd) return plan_reject(msg, n, "eval: the embedding term is not carried by a domain-decomposed evaluation");
    if (r.emb_n_ext < 0 || !r.emb_sites_ok) return plan_reject(msg, n, "eval: embedding: n_ext > 0 needs ext_coord and ext_charge");
    if (r.emb_periodic) {  // armed (aimnet_engine_set_embedding_periodic): the sites are periodic with the cell
      if (!r.pbc) return plan_reject(msg, n, "eval: periodic embedding sites need a cell");
      if (!r.emb_pbc_full)
        return plan_reject(msg, n, "eval: periodic embedding sites need a cell that is periodic along all three axes (no pbc_sys)");
      if (!(r.emb_periodic_accuracy > 0.0f && r.emb_periodic_accuracy < 1.0f))
        return plan_reject(msg, n, "eval: periodic embedding sites need 0 < accuracy < 1");
      if (r.emb_periodic_max_k <= 0 || r.emb_periodic_max_k % r.L.ewald_kb != 0)
        return plan_reject(msg, n, "eval: periodic embedding sites need max_k > 0, a multiple of %d (got %d)", r.L.ewald_kb,
                           r.emb_periodic_max_k);
      if (!r.emb_periodic_scratch_ok)
        return plan_reject(msg, n, "eval: periodic embedding sites: scratch missing or smaller than "
                                   "aimnet_embedding_periodic_scratch_bytes");
      if (!r.emb_periodic_status) return plan_reject(msg, n, "eval: periodic embedding sites: status is required");
    } else if (r.emb_n_ext > 0 && r.pbc)
      return plan_reject(msg, n, "eval: embedding point charges take non-periodic input (no images of the sites): pass a per-atom "
                                 "potential with a cell");
    if (r.emb_potential_grad && !r.emb_potential) return plan_reject(msg, n, "eval: embedding: potential_grad without potential");
    if (r.emb_potential && !r.emb_potential_grad && want_f)
      return plan_reject(msg, n, "eval: embedding: forces need potential_grad beside potential");
    if (r.emb_n_ext > 0 && !r.emb_ext_mol_idx && r.L.n_mol > 1)
      return plan_reject(msg, n, "eval: embedding: ext_mol_idx == NULL is allowed with one molecule only (n_mol = %d)", r.L.n_mol);
    if (!r.emb_scratch_ok) return plan_reject(msg, n, "eval: embedding: scratch missing or smaller than aimnet_embedding_scratch_bytes");
  }
  return 0;
}
// the checks that follow the workspace-size check: DFT-D3 tables, and the caller's D3 matrix against the layout
inline int eval_validate_lists(const EvalRequest& r, const LayoutPlan& L, char* msg, size_t n) {
  if (r.L.dftd3 == 0) return 0;
  if (!r.d3_tables) return plan_reject(msg, n, "eval: DFT-D3 requested but aimnet_engine_set_dftd3 was never called");
  if (!r.nbmat) return 0;
  if (L.d3_in_lr) {
    if (r.nbmat_d3)
      return plan_reject(msg, n, "eval: with d3_cutoff == dsf_rc one caller-supplied matrix serves both terms: pass it as nbmat_lr only");
  } else {
    const int src_w = r.nbmat_d3 ? r.nbmat_d3_width : r.nbmat_lr_width;
    if (L.cap_d3 < src_w)
      return plan_reject(msg, n, "eval: options.max_nb_d3 (%d) is smaller than the caller-supplied D3 matrix (%d)", L.cap_d3, src_w);
  }
  return 0;
}

// ---- the plan of a request that passed the checks ---------------------------------------------------------------------------------
inline EvalPlan eval_plan(const EvalRequest& r) {
  EvalPlan P{};
  const LayoutPlan& L = P.layout = layout_plan(r.L);
  const int N = r.L.N, coulomb = r.L.coulomb;
  const bool pbc = r.pbc, d3 = r.L.dftd3 != 0, same = r.L.d3_same_cutoff;
  P.want_f = (r.L.flags & AIMNET_FORCES) != 0;
  P.want_s = (r.L.flags & AIMNET_STRESS) != 0;
  P.grad = L.grad;
  P.ext = r.nbmat;
  // -- preparation and status words
  // small batches: status zeroing, molecule offsets / sanity / species, cell + bin setup, wrapping and binning in one launch;
  // else the periodic fast path lets the cell + bin-grid setup block ride on the molecule-offset launch
  P.prep = (r.prep_fused && !P.ext && r.prep_small_ok)          ? Prep::FusedSmall
           : (r.setup_rides && !P.ext && pbc && r.cell_setup_ok) ? Prep::SeparateSetupRider
                                                                 : Prep::Separate;
  // no second list build follows the short-range one (periodic DSF walks the grid, "simple" sums all pairs, no D3 list): its
  // status words are reduced by rider blocks of the SR-Coulomb launch.  That rider can just as well STORE all eight status words
  // (with the sanity flags of the molecule-offset launch collected per wave): then nothing is zeroed in front of the evaluation.
  const bool one_list = !P.ext && !(coulomb == AIMNET_COULOMB_DSF && !pbc) && !d3;
  P.sr_status_rides = r.status_rides && one_list;
  P.status = P.prep == Prep::FusedSmall                                 ? StatusZero::FusedPrep
             : (P.sr_status_rides && r.status_owned && N <= 32768) ? StatusZero::RiderOwned
                                                                    : StatusZero::Memset;
  P.p0_moments = r.p0_moments && P.grad;
  P.want_species = P.p0_moments || d3;
  // large non-periodic molecules get a bounding-box cell list instead of the O(n^2) scan
  P.bbox = !P.ext && !pbc && r.bbox_ok;
  P.binned = !P.ext && (pbc || P.bbox);
  P.bin_order = P.binned && r.spatial_order;
  // -- the long-range term
  const bool np_walk = plan_np_walk(r);
  switch (coulomb) {
    case AIMNET_COULOMB_SIMPLE:  // all pairs of the molecule in the waves of the SR launch, or coul_simple over the caller's matrix
      P.lr_term = (P.ext && r.nbmat_lr) ? LongRange::SimpleMatrix : LongRange::SimpleInSr;
      break;
    case AIMNET_COULOMB_DSF:  // one cutoff with DFT-D3: the pair terms ride on the D3 pair pass; cell grids are walked, no matrix
      P.lr_term = (!P.ext && d3 && same)          ? LongRange::DsfInD3
                  : (np_walk || (pbc && !P.ext)) ? LongRange::DsfWalk
                                                 : LongRange::DsfMatrix;
      break;
    case AIMNET_COULOMB_EWALD: P.lr_term = LongRange::EwaldWalk; break;
    case AIMNET_COULOMB_PME: P.lr_term = LongRange::PmeWalk; break;
    default: P.lr_term = LongRange::None;
  }
  P.stream_rides = lr_is_walk(P.lr_term);
  // -- lists
  P.sr = P.ext ? ListFrom::Imported : ListFrom::Built;
  P.lr = P.ext ? (r.nbmat_lr && coulomb != AIMNET_COULOMB_NONE ? ListFrom::Imported : ListFrom::None)
               : (coulomb == AIMNET_COULOMB_DSF && !pbc && !np_walk ? ListFrom::Built : ListFrom::None);
  P.cap_d3 = !d3 ? 0 : L.d3_in_lr ? L.cap_lr : L.cap_d3;
  // one cutoff: a long-range list that exists IS the D3 list; periodic DSF walks the grid, so the shared buffers are free for it
  P.d3 = !d3 ? ListFrom::None : (L.d3_in_lr && P.lr != ListFrom::None) ? ListFrom::LongRange : P.ext ? ListFrom::Imported : ListFrom::Built;
  P.d3_cn_rides = P.d3 == ListFrom::Built && r.d3_cn_rides && P.binned;
  // -- reverse-pair map: its only reader is the pair-force gather, the last kernel of the backward
  P.rev_hash = L.xe && P.want_f;
  P.rev_lookup = !P.rev_hash ? RevLookup::None : P.stream_rides ? RevLookup::OnWalk : RevLookup::OnEnergyLaunch;
  P.pair_force_rides = P.rev_hash && P.want_s && pbc;
  // -- the molecule energies are outputs only.  With a stress request (the walk has written the charges and looked the map up) their
  // sums ride on the two stress launches; forces only, one slice per molecule, the force-negation launch at the end (not the
  // reverse-pair gather): the sums and the copy of the charges ride there.
  if (r.energy_rides && P.want_s && pbc && P.stream_rides)
    P.energy = EnergySum::StressRider;
  else if (r.energy_rides && P.want_f && !(P.want_s && pbc) && !L.xe && L.S == 1)
    P.energy = EnergySum::ForceRider;
  else
    P.energy = EnergySum::OwnLaunch;
  P.charges = P.stream_rides ? ChargesBy::Walk : P.energy == EnergySum::ForceRider ? ChargesBy::ForceRider : ChargesBy::EnergyLaunch;
  // -- backward
  P.nse = r.dd ? NseAdjoint::Decomposed : (r.nse_merged && N <= 1024) ? NseAdjoint::Merged : NseAdjoint::Sliced;
  P.head_fused = L.split_format != 0 && r.head_fusable;
  return P;
}

}  // namespace aimnet
