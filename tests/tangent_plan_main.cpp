// Host check of the plan of the two tangent entry points of csrc/hvp.hip (built and run by tests/test_tangent_plan.py with
// -fsanitize=address,undefined).  It includes the header aimnet_engine_hvp / aimnet_engine_charge_response include and calls the
// functions they call - tangent_validate, tangent_plan - over the product of
//   entry (hvp, charge_response)  x  periodic or not  x  the five Coulomb methods  x  dftd3 on / off  x  D3 tables set or not
//   x  nq 1 / 2  x  n_pass 1 / 2 / 3  x  embedding on / off  x  caller matrices (none, nbmat, nbmat_lr, nbmat_d3)
//   x  n_vec in {1, 16383, 16384, 65535, 65536}  x  max_nb_lr 0 / 600  x  bbox_ok  x  the output sets of the entry
//   x  one "spoiler" at a time: bad Ewald arguments, no list cutoff, a wrong n_cell, too many atoms, missing input arrays.
// What is asserted: (1) the checks reject exactly what the chain of inline checks they replace rejected, in the same order of
// precedence - `expected` below is that chain as a table of (entry prefix, keyword); (2) the invariants the layout and the stages
// rely on, for every plan; (3) the walk reached every reject and every plan branch.
#include <cstdio>
#include <cstdlib>
#include <cstring>

#include "tangent_plan.h"

using namespace aimnet;

#define CHECK(cond, what)                                                                                                    \
  do {                                                                                                                       \
    if (!(cond)) {                                                                                                           \
      std::fprintf(stderr, "FAILED: %s  [%s]\n", what, #cond);                                                               \
      dump(rq);                                                                                                              \
      std::exit(1);                                                                                                          \
    }                                                                                                                        \
  } while (0)

static void dump(const TangentRequest& r) {
  std::fprintf(stderr,
               "  entry %d N %d n_mol %d n_vec %d n_cell %d pbc %d nq %d n_pass %d width %d | coulomb %d dftd3 %d dsf_rc %d max_nb_lr %d"
               " max_nb_d3 %d ewald_args %d | tables %d emb %d bbox %d arrays %d | nbmat %d %d %d | out hv %d f %d dq %d dspin %d dmu %d q %d\n",
               (int)r.entry, r.N, r.n_mol, r.n_vec, r.n_cell, r.pbc, r.nq, r.n_pass, r.max_width, r.coulomb, r.dftd3, r.dsf_rc_set,
               r.max_nb_lr, r.max_nb_d3, r.ewald_args, r.d3_tables, r.emb_on, r.bbox_ok, r.arrays, r.nbmat, r.nbmat_lr, r.nbmat_d3, r.hv,
               r.forces, r.dq, r.dspin, r.dmu, r.charges);
}

// the rejects, in the order of precedence of each entry: the keyword is a piece of the message that the tests of the C
// interface match on
enum Reject {
  OK = -1,
  H_EMPTY, H_EMB, H_NBMAT, H_TABLES, H_NVEC, H_D3_SIZE, H_DSF_LIST, H_PME, H_EWALD_CELL, H_EWALD_ARGS, H_EWALD_LIST, H_SIMPLE, H_NCELL, H_SIZE,
  C_DQ, C_EMPTY, C_NBMAT, C_NVEC, C_ONE_PASS, C_DSPIN, C_DMU, C_NCELL, C_SIZE,
  N_REJECTS
};
static const char* const KEYWORD[N_REJECTS] = {
    "null or empty input", "embedding term is not carried", "caller-supplied neighbour matrices", "aimnet_engine_set_dftd3 was never called",
    "at most 16383 directions|at most 65535 directions", "n_vec * n_atoms * max_nb_d3 too large", "DSF Coulomb needs max_nb_lr > 0",
    "does not cover particle-mesh Ewald", "periodic along all three axes", "0 < ewald_accuracy < 1 and ewald_max_k >= 8",
    "runs its real-space term on the neighbour list", "'simple' Coulomb is undefined for periodic input", "n_cell must be 1 or n_mol",
    "n_vec * n_atoms too large",
    "dq is required", "null or empty input", "caller-supplied neighbour matrices", "at most 65535 directions",
    "a model with one pass has no charges", "dspin is defined for two charge channels", "dipole moment of a periodic cell is not defined",
    "n_cell must be 1 or n_mol", "n_vec * n_atoms too large"};

static Reject expected(const TangentRequest& r) {
  const bool bad_cell = r.pbc && !(r.n_cell == 1 || r.n_cell == r.n_mol);
  const bool too_large = (size_t)r.n_vec * (size_t)r.N * (size_t)r.max_width >= (size_t)INT32_MAX;
  if (r.entry == TangentEntry::Hvp) {
    const bool d3 = r.dftd3 != 0;
    if (r.N <= 0 || r.n_mol <= 0 || !r.arrays) return H_EMPTY;
    if (r.emb_on) return H_EMB;
    if (r.nbmat || r.nbmat_lr || r.nbmat_d3) return H_NBMAT;
    if (d3 && !r.d3_tables) return H_TABLES;
    if (r.n_vec > (d3 ? 16383 : 65535)) return H_NVEC;
    if (d3 && 4 * (size_t)r.n_vec * (size_t)r.N * (size_t)(r.max_nb_d3 > 1 ? r.max_nb_d3 : 1) >= (size_t)INT32_MAX) return H_D3_SIZE;
    if (r.coulomb == AIMNET_COULOMB_DSF && r.max_nb_lr <= 0) return H_DSF_LIST;
    if (r.coulomb == AIMNET_COULOMB_PME) return H_PME;
    if (r.coulomb == AIMNET_COULOMB_EWALD) {
      if (r.ewald_args == 1) return H_EWALD_CELL;
      if (r.ewald_args) return H_EWALD_ARGS;
      if (r.max_nb_lr <= 0 || !r.dsf_rc_set) return H_EWALD_LIST;
    }
    if (r.coulomb == AIMNET_COULOMB_SIMPLE && r.pbc) return H_SIMPLE;
    if (bad_cell) return H_NCELL;
    return too_large ? H_SIZE : OK;
  }
  if (!r.dq) return C_DQ;
  if (r.N <= 0 || r.n_mol <= 0 || !r.arrays) return C_EMPTY;
  if (r.nbmat || r.nbmat_lr || r.nbmat_d3) return C_NBMAT;
  if (r.n_vec > 65535) return C_NVEC;
  if (r.n_pass < 2) return C_ONE_PASS;
  if (r.dspin && r.nq != 2) return C_DSPIN;
  if (r.dmu && r.pbc) return C_DMU;
  if (bad_cell) return C_NCELL;
  return too_large ? C_SIZE : OK;
}

static bool has_keyword(const char* msg, const char* alternatives) {  // "a|b": either piece
  char buf[256];
  std::snprintf(buf, sizeof buf, "%s", alternatives);
  for (char* k = std::strtok(buf, "|"); k; k = std::strtok(nullptr, "|"))
    if (std::strstr(msg, k)) return true;
  return false;
}

static long g_checked = 0, g_rejected = 0;
static unsigned long g_seen_reject = 0;
static unsigned g_seen_plan = 0;  // bit 2 b + v: branch b took value v
enum Branch { B_ENTRY, B_LR_LIST, B_EWALD, B_QTOT, B_D3, B_BBOX, B_FWD_ALL, N_BRANCHES };

static void check(const TangentRequest& rq) {
  char msg[512] = "";
  const bool hvp = rq.entry == TangentEntry::Hvp;
  const int rc = tangent_validate(rq, msg, sizeof msg);
  const Reject want = expected(rq);
  if (want != OK) {
    const char* prefix = hvp ? "hvp: " : "charge_response: ";
    CHECK(rc == AIMNET_E_INVALID, "a request the inline checks rejected is rejected, with the same code");
    CHECK(std::strncmp(msg, prefix, std::strlen(prefix)) == 0, "the message names its entry");
    CHECK(has_keyword(msg, KEYWORD[want]), "the first check that fails is the one that failed first before");
    g_seen_reject |= 1ul << want;
    ++g_rejected;
    return;
  }
  CHECK(rc == 0 && msg[0] == 0, "a request the inline checks accepted is accepted, and no message is written");
  ++g_checked;
  const TangentPlan P = tangent_plan(rq);
  const bool dsf = rq.coulomb == AIMNET_COULOMB_DSF, ewald = rq.coulomb == AIMNET_COULOMB_EWALD, d3 = rq.dftd3 != 0;
  const bool seen[N_BRANCHES] = {hvp, P.lr_list, P.ewald, P.ewald_qtot, P.d3_block, P.bbox, P.n_fwd_pass == rq.n_pass};
  for (int b = 0; b < N_BRANCHES; ++b) g_seen_plan |= 1u << (2 * b + (seen[b] ? 1 : 0));

  CHECK(P.lr_list == (hvp && (dsf || ewald)), "a long-range list is built exactly for DSF and Ewald in hvp");
  CHECK(P.ewald == (hvp && ewald), "Ewald stages exactly with the method");
  CHECK(P.want_species == P.d3_block && P.d3_block == (hvp && d3), "species slots exactly for the D3 block");
  CHECK(!P.ewald_qtot || (P.ewald && rq.nq == 2), "alpha + beta is formed for two channels only");
  CHECK(P.ewald_qtot || !(P.ewald && rq.nq == 2), "... and always for them");
  CHECK(P.keep_passes == P.backward, "the passes keep their buffers exactly when a backward reads them again");
  CHECK(P.head == P.backward, "the energy head belongs to the sweep that runs backward");
  if (!hvp) CHECK(!P.head && !P.backward && !P.lr_list && !P.d3_block && !P.ewald, "charge_response stops at the charges");
  // forward: the final charges q[n_pass - 2] are written, and every buffer a pass writes exists
  CHECK(P.n_fwd_pass == (hvp ? rq.n_pass : rq.n_pass - 1) && P.n_fwd_pass >= 1 && P.n_fwd_pass <= AIMNET_MAX_PASS, "forward passes");
  if (rq.n_pass >= 2) CHECK(P.nse[rq.n_pass - 2], "the pass that forms the final charges ends with the NSE update");
  for (int p = 0; p < P.n_fwd_pass; ++p) {
    if (P.update_a[p]) CHECK(p + 1 < P.n_fwd_pass, "a^{p+1} is written only where a pass reads it");
    if (p + 1 < P.n_fwd_pass) CHECK(P.update_a[p] && P.nse[p], "a pass that is followed by another hands it a^{p+1} and the charges");
    if (hvp && p == rq.n_pass - 1) CHECK(!P.nse[p] && !P.update_a[p], "the last pass feeds the energy head only");
  }
  // capacities
  CHECK(P.cap >= 1 && P.cap >= rq.max_nb, "short-range capacity");
  if (P.lr_list) CHECK(P.cap_lr > 0 && P.cap_lr == rq.max_nb_lr, "a list that is built has rows");
  CHECK((P.cap_d3 >= 1) == P.d3_block && (P.d3_block || P.cap_d3 == 0), "D3 capacity exactly with the D3 block");
  if (P.ewald)
    CHECK(P.ewald_max_k >= rq.ewald_kb && P.ewald_max_k % rq.ewald_kb == 0 && P.ewald_max_k <= rq.ewald_max_k, "Ewald k entries: whole blocks");
  else
    CHECK(P.ewald_max_k == 0, "no k entries without Ewald");
  CHECK(P.bbox == (!rq.pbc && rq.bbox_ok), "bounding boxes are for non-periodic input");
  // the layout of the size queries (no inputs, no outputs) is the layout of the call
  TangentRequest sz{};
  sz.entry = rq.entry; sz.N = rq.N; sz.n_mol = rq.n_mol; sz.n_vec = rq.n_vec; sz.nq = rq.nq; sz.n_pass = rq.n_pass; sz.max_width = rq.max_width;
  sz.coulomb = rq.coulomb; sz.dftd3 = rq.dftd3; sz.dsf_rc_set = rq.dsf_rc_set; sz.max_nb = rq.max_nb; sz.max_nb_lr = rq.max_nb_lr;
  sz.max_nb_d3 = rq.max_nb_d3; sz.ewald_max_k = rq.ewald_max_k; sz.ewald_kb = rq.ewald_kb; sz.d3_tables = rq.d3_tables; sz.bbox_ok = rq.bbox_ok;
  const TangentPlan A = tangent_plan(sz);
  CHECK(A.n_fwd_pass == P.n_fwd_pass && A.head == P.head && A.backward == P.backward && A.keep_passes == P.keep_passes && A.cap == P.cap &&
            A.cap_lr == P.cap_lr && A.cap_d3 == P.cap_d3 && A.ewald == P.ewald && A.ewald_max_k == P.ewald_max_k &&
            A.ewald_qtot == P.ewald_qtot && A.d3_block == P.d3_block,
        "what the layout reads depends on (engine, sizes, options) alone");
}

int main() {
  const int coulombs[] = {AIMNET_COULOMB_NONE, AIMNET_COULOMB_SIMPLE, AIMNET_COULOMB_DSF, AIMNET_COULOMB_EWALD, AIMNET_COULOMB_PME};
  const int n_vecs[] = {1, 16383, 16384, 65535, 65536};
  enum Spoiler { NONE, EWALD_ARGS, NO_LIST_CUTOFF, N_CELL, TOO_MANY_ATOMS, NO_ARRAYS, N_SPOILERS };
  for (int entry = 0; entry < 2; ++entry)
    for (int pbc = 0; pbc < 2; ++pbc)
      for (int coulomb : coulombs)
        for (int d3 = 0; d3 < 2; ++d3)
          for (int tables = 0; tables < 2; ++tables)
            for (int nq = 1; nq <= 2; ++nq)
              for (int n_pass = 1; n_pass <= 3; ++n_pass)
                for (int emb = 0; emb < 2; ++emb)
                  for (int mats = 0; mats < 4; ++mats)
                    for (int n_vec : n_vecs)
                      for (int cap_lr : {0, 600})
                        for (int bbox = 0; bbox < 2; ++bbox)
                          for (int outs = 0; outs < (entry == 0 ? 2 : 5); ++outs)
                            for (int spoil = 0; spoil < N_SPOILERS; ++spoil) {
                              TangentRequest rq{};
                              rq.entry = entry == 0 ? TangentEntry::Hvp : TangentEntry::ChargeResponse;
                              rq.N = spoil == TOO_MANY_ATOMS ? 40000 : 40; rq.n_mol = 2; rq.n_vec = n_vec;
                              rq.pbc = pbc != 0; rq.n_cell = !pbc ? 0 : spoil == N_CELL ? 3 : 1;
                              rq.nq = nq; rq.n_pass = n_pass; rq.max_width = 704;  // 65535 x 40 x 704 < 2^31
                              rq.coulomb = coulomb; rq.dftd3 = d3; rq.dsf_rc_set = spoil != NO_LIST_CUTOFF;
                              rq.max_nb = 112; rq.max_nb_lr = cap_lr; rq.max_nb_d3 = 2832; rq.ewald_max_k = 8197; rq.ewald_kb = 8;
                              rq.ewald_args = coulomb != AIMNET_COULOMB_EWALD || entry != 0 ? 0 : !pbc ? 1 : spoil == EWALD_ARGS ? 2 : 0;
                              rq.d3_tables = tables != 0; rq.emb_on = emb != 0; rq.bbox_ok = bbox != 0; rq.arrays = spoil != NO_ARRAYS;
                              rq.nbmat = mats == 1; rq.nbmat_lr = mats == 2; rq.nbmat_d3 = mats == 3;
                              if (entry == 0) {
                                rq.hv = true; rq.forces = outs == 1;
                              } else {  // none; dq; + dspin; + dmu; all four
                                rq.dq = outs >= 1; rq.dspin = outs == 2 || outs == 4; rq.dmu = outs >= 3; rq.charges = outs == 4;
                              }
                              check(rq);
                            }
  // the walk reached every reject and both values of every plan branch (a product that skipped one would prove nothing about it)
  if (g_seen_reject != (1ul << N_REJECTS) - 1 || g_seen_plan != (1u << (2 * N_BRANCHES)) - 1 || g_checked == 0) {
    std::fprintf(stderr, "FAILED: a reject or a plan branch was never reached (rejects %lx, plan %x)\n", g_seen_reject, g_seen_plan);
    return 1;
  }
  std::printf("tangent plan ok: %ld plans checked, %ld requests rejected as before\n", g_checked, g_rejected);
  return 0;
}
