// Host check of the evaluation plan of csrc/engine.hip (built and run by tests/test_eval_plan.py with -fsanitize=address,undefined).
// It includes the header aimnet_engine_eval includes and calls the functions it calls - eval_validate, eval_validate_lists,
// eval_plan, layout_plan - over the product of
//   periodic or not  x  caller-supplied lists (none, nbmat, + nbmat_lr, + nbmat_d3, all three)  x  the five Coulomb methods
//   x  D3 (off, same cutoff, another cutoff)  x  (energy, forces, stress alone, forces + stress)  x  nq 1 / 2
//   x  domain decomposition on / off
//   x  max_nb_lr 0 / 600  x  N in {8, 300, 1025, 3000, 40000}  x  n_mol 1 / 2  x  the split format (none, bf16x3, fp16x2)
// and, of the 11 engine switches and 5 size predicates the plan reads (16 binary knobs), every setting that differs from all-on in
// at most two knobs and from all-off in at most one - a SAMPLE: the full 2^16 product over that shape list takes minutes under the
// sanitizers, this one about a quarter of a minute.  Requests that eval rejects are skipped by eval's own checks.
// What is asserted are the invariants that the stages of eval rely on - each job has exactly one owner, and whatever a stage reads
// was produced before it - not a second copy of the plan's expressions.
#include <cstdio>
#include <cstdlib>

#include "eval_plan.h"

using namespace aimnet;

#define CHECK(cond, what)                                                                                                    \
  do {                                                                                                                       \
    if (!(cond)) {                                                                                                           \
      std::fprintf(stderr, "FAILED: %s  [%s]\n", what, #cond);                                                               \
      dump(rq);                                                                                                              \
      std::exit(1);                                                                                                          \
    }                                                                                                                        \
  } while (0)

static void dump(const EvalRequest& r) {
  std::fprintf(stderr,
               "  N %d n_mol %d pbc %d flags %u coulomb %d dftd3 %d same %d nq %d dd %d max_nb_lr %d sfmt %d | nbmat %d lr %d d3 %d |"
               " switches xe %d prep %d erides %d srides %d setup %d owned %d nse %d cn %d npw %d p0m %d order %d |"
               " predicates prep %d setup %d bbox %d head %d rev %d\n",
               r.L.N, r.L.n_mol, r.pbc, r.L.flags, r.L.coulomb, r.L.dftd3, r.L.d3_same_cutoff, r.nq, r.dd, r.L.max_nb_lr, r.L.split_format,
               r.nbmat, r.nbmat_lr, r.nbmat_d3, r.L.conv_xe, r.prep_fused, r.energy_rides, r.status_rides, r.setup_rides, r.status_owned,
               r.nse_merged, r.d3_cn_rides, r.dsf_np_walk, r.p0_moments, r.spatial_order, r.prep_small_ok, r.cell_setup_ok, r.bbox_ok,
               r.head_fusable, r.L.pair_rev_ok);
}

constexpr int N_KNOBS = 16;
static void set_knobs(EvalRequest& r, unsigned m) {
  int k = 0;
  auto bit = [&]() { return (int)((m >> k++) & 1u); };
  r.L.conv_xe = bit(); r.prep_fused = bit(); r.energy_rides = bit(); r.status_rides = bit(); r.setup_rides = bit();
  r.status_owned = bit(); r.nse_merged = bit(); r.d3_cn_rides = bit(); r.dsf_np_walk = bit(); r.p0_moments = bit();
  r.spatial_order = bit();
  r.prep_small_ok = bit(); r.cell_setup_ok = bit(); r.bbox_ok = bit(); r.head_fusable = bit(); r.L.pair_rev_ok = bit();
  if (k != N_KNOBS) std::abort();
}

static long g_checked = 0, g_rejected = 0;
static unsigned g_seen_lr = 0, g_seen_prep = 0, g_seen_status = 0, g_seen_energy = 0, g_seen_charges = 0, g_seen_nse = 0,
                g_seen_rev = 0, g_seen_d3 = 0;

static void check(const EvalRequest& rq) {
  char msg[512];
  if (eval_validate(rq, msg, sizeof msg) || eval_validate_lists(rq, layout_plan(rq.L), msg, sizeof msg)) {
    ++g_rejected;
    return;
  }
  ++g_checked;
  const EvalPlan P = eval_plan(rq);
  const LayoutPlan& L = P.layout;
  const bool d3 = rq.L.dftd3 != 0, walk = lr_is_walk(P.lr_term);
  g_seen_lr |= 1u << (int)P.lr_term; g_seen_prep |= 1u << (int)P.prep; g_seen_status |= 1u << (int)P.status;
  g_seen_energy |= 1u << (int)P.energy; g_seen_charges |= 1u << (int)P.charges; g_seen_nse |= 1u << (int)P.nse;
  g_seen_rev |= 1u << (int)P.rev_lookup; g_seen_d3 |= 1u << (int)P.d3;

  {
    const LayoutPlan A = layout_plan(rq.L);  // what aimnet_engine_workspace_bytes computes
    CHECK(L.grad == A.grad && L.cap == A.cap && L.cap_lr == A.cap_lr && L.cap_d3 == A.cap_d3 && L.d3_in_lr == A.d3_in_lr &&
              L.ewald_max_k == A.ewald_max_k && L.pme_max_mesh == A.pme_max_mesh && L.pme_max_parts == A.pme_max_parts && L.xe == A.xe &&
              L.split_format == A.split_format && L.split_planes == A.split_planes && L.S == A.S,
          "the layout sub-plan is the one computed from (engine, N, n_mol, options) alone");
  }
  CHECK(P.grad == (P.want_f || P.want_s) && P.grad == L.grad, "gradient request");
  // one long-range term
  CHECK((P.lr_term == LongRange::None) == (rq.L.coulomb == AIMNET_COULOMB_NONE), "the long-range term is none exactly without Coulomb");
  CHECK(P.stream_rides == walk, "the charge stream rides exactly when the term is a walk");
  // status words
  CHECK((P.status == StatusZero::FusedPrep) == (P.prep == Prep::FusedSmall), "the fused preparation zeroes the status words itself");
  if (P.status == StatusZero::RiderOwned) {
    CHECK(P.sr_status_rides, "the owned form needs the status rider");
    CHECK(P.sr == ListFrom::Built && P.lr == ListFrom::None && P.d3 == ListFrom::None, "the owned form needs ONE list");
    CHECK(rq.L.N <= 32768, "the owned form is one block: up to 32 768 atoms");
  }
  if (P.sr_status_rides)  // (the row counts live in scratch that the next list build overwrites)
    CHECK(P.sr == ListFrom::Built && P.lr != ListFrom::Built && P.d3 != ListFrom::Built, "no list build between the SR list and its status rider");
  if (P.prep == Prep::SeparateSetupRider) CHECK(rq.pbc && !P.ext, "the setup rider prepares a periodic cell grid");
  if (P.prep == Prep::FusedSmall) CHECK(!P.ext && rq.prep_small_ok, "the fused preparation has its size limits");
  // lists: what a stage reads was built or imported, into a buffer that holds it, and no two live lists share a buffer
  CHECK(P.sr == (P.ext ? ListFrom::Imported : ListFrom::Built), "the short-range list always exists");
  CHECK(L.cap >= 1 && (!P.ext || rq.nbmat_width <= L.cap), "short-range capacity");
  if (P.lr_term == LongRange::SimpleMatrix || P.lr_term == LongRange::DsfMatrix) {
    CHECK(P.lr != ListFrom::None && L.cap_lr > 0, "a matrix term reads the long-range list");
    CHECK(P.lr_term != LongRange::SimpleMatrix || P.lr == ListFrom::Imported, "'simple' over a matrix: only a caller's");
  }
  if (P.lr == ListFrom::Imported) CHECK(P.ext && rq.nbmat_lr && rq.nbmat_lr_width <= L.cap_lr, "imported long-range list fits");
  if (P.lr == ListFrom::Built) CHECK(!P.ext && L.cap_lr > 0, "built long-range list has a buffer");
  if (walk) CHECK(P.binned && !P.ext && (rq.pbc || P.bbox), "a walk needs the cell grid (periodic cell or bounding box)");
  if (P.bbox) CHECK(!rq.pbc && !P.ext, "bounding boxes are for the engine's own non-periodic lists");
  if (P.bin_order) CHECK(P.binned, "bin order needs bins");
  if (P.ext) CHECK(!P.binned, "caller-supplied lists: no bins");
  CHECK((P.d3 != ListFrom::None) == d3, "the D3 list exists exactly with D3");
  if (d3) {
    if (L.d3_in_lr) {  // where the D3 list sits is the layout's decision
      CHECK(L.cap_d3 == 0 && P.cap_d3 == L.cap_lr && L.cap_lr > 0, "D3 in the long-range buffers: their capacity, none of its own");
      // a long-range list in those buffers IS the D3 list; anything else written there needs them free
      CHECK((P.d3 == ListFrom::LongRange) == (P.lr != ListFrom::None), "no two live lists share a buffer");
    } else {
      CHECK(P.d3 != ListFrom::LongRange && P.cap_d3 == L.cap_d3 && L.cap_d3 >= 1, "D3 in its own buffers");
    }
    if (P.d3 == ListFrom::Imported)
      CHECK(P.ext && (rq.nbmat_d3 ? rq.nbmat_d3_width : rq.nbmat_lr_width) <= P.cap_d3, "imported D3 list fits");
    if (P.d3 == ListFrom::Built) CHECK(!P.ext, "built D3 list");
  }
  if (P.lr_term == LongRange::DsfInD3) CHECK(d3 && !P.ext && rq.L.d3_same_cutoff, "DSF inside the D3 pass: one cutoff, the engine's list");
  if (P.d3_cn_rides) CHECK(P.d3 == ListFrom::Built && P.binned, "the CN rider sits in the cell-grid build of the D3 list");
  CHECK(P.want_species || !(d3 || P.p0_moments), "species slots for D3 and the pass-0 moments");
  if (P.p0_moments) CHECK(P.grad, "pass-0 moments are a backward form");
  // reverse-pair map
  CHECK(P.rev_hash == (L.xe && P.want_f), "the map is built exactly for the reverse-pair force gather");
  CHECK((P.rev_lookup != RevLookup::None) == P.rev_hash, "hash build and lookup run together, once each");
  if (P.rev_lookup == RevLookup::OnWalk) CHECK(walk, "lookup on the walk: the walk runs");
  if (P.rev_lookup == RevLookup::OnEnergyLaunch) CHECK(P.energy == EnergySum::OwnLaunch, "lookup on the energy launch: it is launched (before the gather)");
  if (P.pair_force_rides) CHECK(P.rev_hash && P.want_s, "the gather rides on a stress launch");
  if (!P.want_f)  // energy only, stress alone (layout.xe may hold without the map): no force launch, so nothing is deferred to one
    CHECK(!P.rev_hash && !P.pair_force_rides && P.energy != EnergySum::ForceRider && P.charges != ChargesBy::ForceRider,
          "without a force request no job waits for the force gather or the force-negation launch");
  if (P.energy == EnergySum::StressRider) CHECK(rq.pbc && walk, "the stress riders sum the energies after a walk has written the charges");
  // energies and charges: one owner each, and a deferred job has a launch to ride on
  if (!P.grad) CHECK(P.energy == EnergySum::OwnLaunch, "energy only: nothing to ride on");
  if (P.energy == EnergySum::StressRider) CHECK(P.want_s, "stress rider needs the stress launches");
  if (P.energy == EnergySum::ForceRider) CHECK(P.want_f && !L.xe && L.S == 1, "force rider needs the force-negation launch, one slice");
  CHECK((P.charges == ChargesBy::Walk) == walk, "the walk writes the charges when it runs");
  CHECK((P.charges == ChargesBy::ForceRider) == (!walk && P.energy == EnergySum::ForceRider), "charges ride with the energy sums");
  if (P.charges == ChargesBy::EnergyLaunch) CHECK(P.energy == EnergySum::OwnLaunch, "charges on the energy launch: it is launched");
  // domain decomposition
  CHECK((P.nse == NseAdjoint::Decomposed) == rq.dd, "decomposed NSE adjoint exactly under domain decomposition");
  if (P.nse == NseAdjoint::Merged) CHECK(rq.L.N <= 1024, "merged NSE adjoint: small systems");
  if (rq.dd) {
    CHECK(!rq.pbc && !P.ext, "domain decomposition: a non-periodic cluster, the engine's lists");
    CHECK(!walk || P.bbox, "domain decomposition never gets a periodic walk");
    CHECK(P.lr_term != LongRange::EwaldWalk && P.lr_term != LongRange::PmeWalk && P.lr_term != LongRange::SimpleInSr &&
              P.lr_term != LongRange::SimpleMatrix,
          "domain decomposition: Coulomb none or DSF");
  }
  if (P.head_fused) CHECK(L.split_format != 0 && rq.head_fusable, "the fused head reads split activations");
}

int main() {
  const int Ns[] = {8, 300, 1025, 3000, 40000};
  // stress alone: the request that has layout.xe (a gradient above split_max) without the reverse-pair map (no force gather)
  const unsigned flags[] = {0u, AIMNET_FORCES, AIMNET_STRESS, AIMNET_FORCES | AIMNET_STRESS};
  const int coulombs[] = {AIMNET_COULOMB_NONE, AIMNET_COULOMB_SIMPLE, AIMNET_COULOMB_DSF, AIMNET_COULOMB_EWALD, AIMNET_COULOMB_PME};
  // knob settings: all-on with at most two knobs flipped, all-off with at most one
  static unsigned masks[2 + 2 * N_KNOBS + N_KNOBS * (N_KNOBS - 1) / 2];
  int n_masks = 0;
  masks[n_masks++] = 0xffffu;
  masks[n_masks++] = 0u;
  for (int a = 0; a < N_KNOBS; ++a) {
    masks[n_masks++] = 0xffffu ^ (1u << a);
    masks[n_masks++] = 1u << a;
    for (int b = a + 1; b < N_KNOBS; ++b) masks[n_masks++] = 0xffffu ^ (1u << a) ^ (1u << b);
  }
  for (int pbc = 0; pbc < 2; ++pbc)
    for (int lists = 0; lists < 5; ++lists)
      for (int coulomb : coulombs)
        for (int d3 = 0; d3 < 3; ++d3)
          for (unsigned fl : flags)
            for (int nq = 1; nq <= 2; ++nq)
              for (int dd = 0; dd < 2; ++dd)
                for (int cap_lr : {0, 600})
                  for (int N : Ns)
                    for (int n_mol = 1; n_mol <= 2; ++n_mol)
                      for (int sfmt = 0; sfmt < 3; ++sfmt) {
                        EvalRequest rq{};
                        rq.L.N = N; rq.L.n_mol = n_mol; rq.L.n_pass = 3;
                        rq.L.flags = fl; rq.L.coulomb = coulomb; rq.L.dftd3 = d3 != 0; rq.L.d3_same_cutoff = d3 == 1;
                        rq.L.max_nb = 64; rq.L.max_nb_lr = cap_lr; rq.L.max_nb_d3 = 600;
                        rq.L.ewald_max_k = 4096; rq.L.pme_max_mesh = 4096; rq.L.ewald_kb = 8; rq.L.pme_part = 1024;
                        rq.L.split_max = 1024;
                        rq.L.split_format = sfmt; rq.L.split_planes = sfmt == 1 ? 3 : sfmt == 2 ? 2 : 1;
                        rq.pbc = pbc != 0; rq.n_cell = pbc ? 1 : 0; rq.nq = nq;
                        rq.has_forces_out = (fl & AIMNET_FORCES) != 0; rq.has_stress_out = (fl & AIMNET_STRESS) != 0;
                        rq.has_spin_out = nq == 2;
                        const bool ew = coulomb == AIMNET_COULOMB_EWALD || coulomb == AIMNET_COULOMB_PME;
                        rq.ewald_args = ew && !pbc ? 1 : 0;
                        rq.nbmat = lists >= 1; rq.nbmat_lr = lists == 2 || lists == 4; rq.nbmat_d3 = lists == 3 || lists == 4;
                        rq.shifts = rq.nbmat && pbc; rq.shifts_lr = rq.nbmat_lr && pbc; rq.shifts_d3 = rq.nbmat_d3 && pbc;
                        rq.nbmat_width = rq.nbmat ? 40 : 0; rq.nbmat_lr_width = rq.nbmat_lr ? 500 : 0; rq.nbmat_d3_width = rq.nbmat_d3 ? 500 : 0;
                        rq.dd = dd != 0;
                        rq.d3_tables = true;
                        for (int m = 0; m < n_masks; ++m) {
                          set_knobs(rq, masks[m]);
                          check(rq);
                        }
                      }
  // the walk reached every branch of the plan (a product that skipped one would prove nothing about it)
  const bool all = g_seen_lr == 0xffu && g_seen_prep == 7u && g_seen_status == 7u && g_seen_energy == 7u && g_seen_charges == 7u &&
                   g_seen_nse == 7u && g_seen_rev == 7u && g_seen_d3 == 0xfu;
  if (!all || g_checked == 0) {
    std::fprintf(stderr, "FAILED: a plan branch was never reached (lr %x prep %x status %x energy %x charges %x nse %x rev %x d3 %x)\n",
                 g_seen_lr, g_seen_prep, g_seen_status, g_seen_energy, g_seen_charges, g_seen_nse, g_seen_rev, g_seen_d3);
    return 1;
  }
  std::printf("eval plan ok: %ld plans checked, %ld requests rejected by eval's own checks\n", g_checked, g_rejected);
  return 0;
}
