// tangent_plan.h - every decision of one aimnet_engine_hvp / aimnet_engine_charge_response call, taken once from plain values, as
// eval_plan.h does for aimnet_engine_eval.  Host code only (no HIP): hvp.hip fills a TangentRequest, checks it (tangent_validate),
// plans it (tangent_plan), lays the workspace out and runs its stages off the plan; tests/tangent_plan_main.cpp walks the same
// functions on the CPU.  What the layout reads depends on (engine, sizes, options) alone: the size queries fill no inputs or outputs.
#pragma once

#include "eval_plan.h"  // plan_reject

namespace aimnet {

enum class TangentEntry { Hvp, ChargeResponse };

struct TangentRequest {
  TangentEntry entry;
  int N, n_mol, n_vec, n_cell;  // n_cell as the caller passed it (read with pbc only)
  bool pbc;                     // inputs.cell given
  int nq, n_pass, max_width;    // engine: charge channels, passes, max_width(engine)
  int coulomb, dftd3, max_nb, max_nb_lr, max_nb_d3, ewald_max_k;  // the options the sweeps read ...
  bool dsf_rc_set;                                                // ... and options.dsf_rc > 0
  int ewald_kb, ewald_args;  // EWALD_KB (kernels.h); Ewald only: ewald_args_check (engine.h) of the inputs, else 0
  bool d3_tables, emb_on;    // aimnet_engine_set_dftd3 was called; an embedding is set (aimnet_engine_set_embedding)
  bool bbox_ok, arrays;      // bbox_applies(N, n_mol); coord, numbers, mol_idx and charge are all given
  bool nbmat, nbmat_lr, nbmat_d3;            // caller-supplied matrices
  bool hv, forces, dq, dspin, dmu, charges;  // outputs given: of Hvp (hv, forces), of ChargeResponse (the other four)
  // aimnet_engine_set_embedding_tangent armed the sweep for the embedding (read with emb_on and Hvp only); then, of the two structs:
  bool emb_tangent;
  int emb_n_ext;                                                // point charges
  bool emb_potential, emb_potential_grad, emb_potential_hess;  // which per-atom arrays are given
  bool emb_mol_idx, emb_scratch_ok;  // ext_mol_idx given; scratch given and at least aimnet_embedding_tangent_scratch_bytes
  // aimnet_engine_set_pme_tangent armed the sweep for particle-mesh Ewald (read with coulomb == PME and Hvp only); then ewald_args
  // holds ewald_args_check of the inputs as for Ewald, and of the options:
  bool pme_tangent;
  int pme_max_mesh, pme_part;  // options.pme_max_mesh; PME_PART (kernels.h)
  // aimnet_engine_set_dftd3_tangent armed the sweep for the dispersion term (read with dftd3 != 0 and Hvp only): its block is the
  // analytic tangent of csrc/d3.hip on the one D3 list, not the central difference over 4 n_vec displaced copies
  bool d3_tangent;
  // aimnet_engine_set_strain_tangent armed the sweep for strain directions (read by both entries: charge_response refuses it); then
  // strain_arrays: the struct's strain and dvirial are both given
  bool strain_tangent, strain_arrays;
  // aimnet_engine_set_strain_terms named AIMNET_STRAIN_TERM_DFTD3: the armed strain sweep may carry the dispersion block (read with
  // strain_tangent and dftd3 != 0 only), by its analytic tangent (d3_tangent).  Last, so that `TangentRequest rq{}` leaves it false
  bool strain_d3;
};

// ---- argument checks: 0, or AIMNET_E_INVALID with the message in msg.  Nothing has been launched when they run --------------------
inline int tangent_validate(const TangentRequest& r, char* msg, size_t n) {
  const bool hvp = r.entry == TangentEntry::Hvp;
  const char* who = hvp ? "hvp" : "charge_response";
  const bool d3 = hvp && r.dftd3 != 0;
  if (!hvp && !r.dq) return plan_reject(msg, n, "charge_response: dq is required");
  if (r.N <= 0 || r.n_mol <= 0 || !r.arrays) return plan_reject(msg, n, "%s: null or empty input", who);
  if (hvp && r.emb_on && !r.emb_tangent)
    return plan_reject(msg, n, "hvp: the embedding term is not carried by the tangent sweep (aimnet_engine_set_embedding(e, NULL) first)");
  if (hvp && r.emb_on) {  // armed (aimnet_engine_set_embedding_tangent)
    if (r.emb_n_ext > 0 && r.pbc)
      return plan_reject(msg, n, "hvp: embedding point charges take non-periodic input (no images of the sites): pass a per-atom "
                                 "potential with its gradient and Hessian");
    if (r.emb_potential && !r.emb_potential_grad)
      return plan_reject(msg, n, "hvp: embedding: the tangent sweep needs potential_grad beside potential");
    if (r.emb_potential && !r.emb_potential_hess)
      return plan_reject(msg, n, "hvp: embedding: the tangent sweep needs potential_hess beside potential (zeros for a uniform field)");
    if (!r.emb_potential && (r.emb_potential_grad || r.emb_potential_hess))
      return plan_reject(msg, n, "hvp: embedding: potential_grad / potential_hess without potential");
    if (r.emb_n_ext > 0 && !r.emb_mol_idx && r.n_mol > 1)
      return plan_reject(msg, n, "hvp: embedding: ext_mol_idx == NULL is allowed with one molecule only (n_mol = %d)", r.n_mol);
    if (r.coulomb == AIMNET_COULOMB_PME)
      return plan_reject(msg, n, "hvp: embedding: the analytic tangent sweep does not cover particle-mesh Ewald");
    if (!r.emb_scratch_ok)
      return plan_reject(msg, n, "hvp: embedding: scratch missing or smaller than aimnet_embedding_tangent_scratch_bytes");
  }
  if (r.nbmat || r.nbmat_lr || r.nbmat_d3)
    return plan_reject(msg, n, "%s: caller-supplied neighbour matrices are not read by the tangent sweep (it builds its own %s)", who,
                       hvp ? "lists" : "list");
  if (d3 && !r.d3_tables) return plan_reject(msg, n, "hvp: DFT-D3 requested but aimnet_engine_set_dftd3 was never called");
  // the tangent kernels index the directions with grid.y (HIP limit 65535); the D3 block replicates every direction four times
  // (armed, aimnet_engine_set_dftd3_tangent: nothing is replicated, and the two limits of the replicas do not apply)
  const bool d3_fd = d3 && !r.d3_tangent;
  const int k_max = d3_fd ? 16383 : 65535;
  if (r.n_vec > k_max)
    return plan_reject(msg, n, "%s: at most %d directions per sweep (%d given): split them over several calls", who, k_max, r.n_vec);
  if (hvp) {
    if (d3_fd && 4 * (size_t)r.n_vec * (size_t)r.N * (size_t)std::max(1, r.max_nb_d3) >= (size_t)INT32_MAX)
      return plan_reject(msg, n, "hvp: n_vec * n_atoms * max_nb_d3 too large for one sweep (split the directions)");
    if (r.coulomb == AIMNET_COULOMB_DSF && r.max_nb_lr <= 0)
      return plan_reject(msg, n,
                         "hvp: DSF Coulomb needs max_nb_lr > 0 (the tangent sweep runs on the neighbour list, also for periodic input)");
    if (r.coulomb == AIMNET_COULOMB_PME && !r.pme_tangent)
      return plan_reject(msg, n,
                         "hvp: the analytic tangent sweep does not cover particle-mesh Ewald (use the exact Ewald sum or DSF, or "
                         "differences of forces as the reference does for its PME block, lr.py:903-926)");
    if (r.coulomb == AIMNET_COULOMB_PME) {  // armed (aimnet_engine_set_pme_tangent)
      if (r.ewald_args == 1)
        return plan_reject(msg, n, "hvp: particle-mesh Ewald needs a cell that is periodic along all three axes (lr.py:655-657)");
      if (r.ewald_args || r.pme_max_mesh < 512)
        return plan_reject(msg, n, "hvp: particle-mesh Ewald needs 0 < ewald_accuracy < 1 and pme_max_mesh >= 512");
      if (r.max_nb_lr <= 0 || !r.dsf_rc_set)
        return plan_reject(msg, n,
                           "hvp: particle-mesh Ewald runs its real-space term on the neighbour list: dsf_rc (the list cutoff, at least "
                           "every system's real-space cutoff) and max_nb_lr must be > 0");
      // the tangent charge meshes hold at most n_atoms 2^40 per point (pme.hip); a (direction, system) slice is a grid.y index
      if (r.N >= (1 << 21)) return plan_reject(msg, n, "hvp: the particle-mesh Ewald tangent takes fewer than %d atoms", 1 << 21);
      if ((size_t)r.n_vec * (size_t)r.n_mol > 65535)
        return plan_reject(msg, n, "hvp: particle-mesh Ewald: at most 65535 directions x systems per sweep (%d x %d given): split the "
                                   "directions over several calls", r.n_vec, r.n_mol);
    }
    if (r.coulomb == AIMNET_COULOMB_EWALD) {
      if (r.ewald_args == 1)
        return plan_reject(msg, n, "hvp: Ewald summation needs a cell that is periodic along all three axes (lr.py:655-657)");
      if (r.ewald_args)
        return plan_reject(msg, n, "hvp: Ewald summation needs 0 < ewald_accuracy < 1 and ewald_max_k >= %d", r.ewald_kb);
      if (r.max_nb_lr <= 0 || !r.dsf_rc_set)
        return plan_reject(msg, n,
                           "hvp: Ewald summation runs its real-space term on the neighbour list: dsf_rc (the list cutoff, at least every "
                           "system's real-space cutoff) and max_nb_lr must be > 0");
    }
    if (r.coulomb == AIMNET_COULOMB_SIMPLE && r.pbc) return plan_reject(msg, n, "hvp: 'simple' Coulomb is undefined for periodic input");
  } else {
    if (r.n_pass < 2) return plan_reject(msg, n, "charge_response: a model with one pass has no charges");
    if (r.dspin && r.nq != 2)
      return plan_reject(msg, n, "charge_response: dspin is defined for two charge channels; this model has one");
    if (r.dmu && r.pbc)
      return plan_reject(msg, n, "charge_response: the dipole moment of a periodic cell is not defined (pass dmu = NULL)");
  }
  if (r.pbc && !(r.n_cell == 1 || r.n_cell == r.n_mol)) return plan_reject(msg, n, "%s: n_cell must be 1 or n_mol", who);
  if ((size_t)r.n_vec * (size_t)r.N * (size_t)r.max_width >= (size_t)INT32_MAX)
    return plan_reject(msg, n, "%s: n_vec * n_atoms too large for one sweep (split the directions)", who);
  if (r.strain_tangent) {  // armed (aimnet_engine_set_strain_tangent): after every other check, so that each keeps its precedence
    if (!hvp)
      return plan_reject(msg, n, "charge_response: a strain tangent is armed, and the charge response carries displacements only "
                                 "(aimnet_engine_set_strain_tangent(e, NULL) first)");
    if (!r.pbc) return plan_reject(msg, n, "hvp: strain tangent: a strain direction needs a cell");
    if (r.coulomb == AIMNET_COULOMB_EWALD)
      return plan_reject(msg, n, "hvp: strain tangent: Ewald summation is not carried under strain (its k vectors move with the cell); "
                                 "use DSF");
    if (r.coulomb == AIMNET_COULOMB_PME)
      return plan_reject(msg, n, "hvp: strain tangent: particle-mesh Ewald is not carried under strain (its mesh moves with the cell); "
                                 "use DSF");
    if (r.dftd3 != 0 && !r.strain_d3)
      return plan_reject(msg, n, "hvp: strain tangent: the DFT-D3 block is not carried under strain (options.dftd3 = 0)");
    if (r.dftd3 != 0 && !r.d3_tangent)
      return plan_reject(msg, n, "hvp: strain tangent: the DFT-D3 block is carried under strain by its analytic tangent only "
                                 "(aimnet_engine_set_dftd3_tangent(e, 1))");
    if (r.emb_on)
      return plan_reject(msg, n, "hvp: strain tangent: the embedding term is not carried under strain (aimnet_engine_set_embedding(e, "
                                 "NULL) first)");
    if (!r.strain_arrays) return plan_reject(msg, n, "hvp: strain tangent: strain and dvirial are required");
  }
  return 0;
}

// ---- the plan of a request that passed the checks ---------------------------------------------------------------------------------
struct TangentPlan {
  // forward + tangent: Hvp runs every pass and the energy head after them; ChargeResponse stops after the NSE charges of pass
  // n_pass - 2 (the charges see nothing after it).  Pass p ends with the NSE charge update / with a^{p+1} = a^p + delta_a:
  int n_fwd_pass;
  bool nse[AIMNET_MAX_PASS], update_a[AIMNET_MAX_PASS];
  bool head;      // energy head, forward and backward
  bool backward;  // Coulomb seeds of qbar / xbar and the backward + tangent sweep (with the buffers of both)
  // the backward reads the MLP rows x / z / y, the moments V / Vq and the NSE sums Fm / Dm of every pass again: each pass owns
  // its set.  Without it ONE set, sized by the widest pass, is written again by every pass.
  bool keep_passes;
  int cap, cap_lr, cap_d3;  // row capacities: short-range list, long-range buffers, D3 list (0: no D3 block)
  bool lr_list;             // a long-range list is built (DSF, or the real-space term of Ewald summation)
  bool ewald, ewald_qtot;   // Ewald stages; a two-channel model: the structure factors see alpha + beta, formed in a buffer of its own
  int ewald_max_k;          // Ewald k entries (0: method not chosen)
  bool d3_block;            // the external DFT-D3 block (central difference of its gradient over all directions)
  bool d3_analytic;         // ... armed: the block is the analytic tangent (d3.hip); tcn4 / tg4 [K][N] take the place of the 4 K replicas
  bool want_species;        // species slots + present masks are formed (DFT-D3)
  bool bbox;                // non-periodic: bounding-box cell grid
  bool embedding;           // the embedding's seeds join the Coulomb seeds (armed), and after the backward its site pass
  // particle-mesh Ewald (armed): pme_setup in front of the list, the real-space term over the list with the systems' own (alpha, rc),
  // the primal potential mesh + field pass and the mesh tangents of every direction (pme.hip)
  bool pme, pme_qtot;       // pme_qtot: a two-channel model - the mesh sees alpha + beta, formed in a buffer of its own
  int pme_max_mesh, pme_max_parts;  // mesh points of one system's slice, blocks of its influence kernel (0: branch not taken)
  // strain directions (armed): the pair tangents take r eps_k, the three centre-major pair kernels write the per-atom virial and its
  // tangent (36 bytes per atom, 36 per direction and atom), summed per system in double after the backward sweep
  bool strain;
  // ... with the dispersion block (armed: strain, d3_analytic and aimnet_engine_set_strain_terms): the three tangent passes of d3.hip
  // take r eps_k and add their share onto the same virial rows; no bytes of its own
  bool d3_strain;
};

inline TangentPlan tangent_plan(const TangentRequest& r) {
  TangentPlan P{};
  const bool hvp = r.entry == TangentEntry::Hvp;
  P.n_fwd_pass = hvp ? r.n_pass : r.n_pass - 1;
  for (int p = 0; p < P.n_fwd_pass; ++p) {  // (Hvp: the last pass feeds the energy head only)
    P.nse[p] = p < r.n_pass - 1;
    P.update_a[p] = p + 1 < P.n_fwd_pass;
  }
  P.head = P.backward = P.keep_passes = hvp;
  P.cap = std::max(1, r.max_nb);
  P.cap_lr = hvp ? std::max(0, r.max_nb_lr) : 0;
  P.d3_block = hvp && r.dftd3 != 0;
  P.d3_analytic = P.d3_block && r.d3_tangent;
  P.cap_d3 = P.d3_block ? std::max(1, r.max_nb_d3) : 0;
  P.ewald = hvp && r.coulomb == AIMNET_COULOMB_EWALD;
  P.pme = hvp && r.coulomb == AIMNET_COULOMB_PME && r.pme_tangent;
  P.lr_list = hvp && (r.coulomb == AIMNET_COULOMB_DSF || P.ewald || P.pme);
  P.pme_qtot = P.pme && r.nq == 2;
  P.pme_max_mesh = P.pme ? std::max(512, r.pme_max_mesh) : 0;
  P.pme_max_parts = P.pme && r.pme_part > 0 ? (P.pme_max_mesh + r.pme_part - 1) / r.pme_part : 0;
  P.ewald_max_k = P.ewald ? std::max(r.ewald_kb, r.ewald_max_k / r.ewald_kb * r.ewald_kb) : 0;
  P.ewald_qtot = P.ewald && r.nq == 2;
  P.want_species = P.d3_block;
  P.bbox = !r.pbc && r.bbox_ok;
  P.embedding = hvp && r.emb_on && r.emb_tangent;
  P.strain = hvp && r.strain_tangent;
  P.d3_strain = P.strain && P.d3_analytic && r.strain_d3;
  return P;
}

}  // namespace aimnet
