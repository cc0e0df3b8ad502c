// Host check of eval_validate (csrc/eval_plan.h) for sites periodic with the cell (aimnet_engine_set_embedding_periodic), built and
// run by tests/test_embedding_periodic_host.py the way tests/test_eval_plan.py builds its program.  It walks
//   {armed, unarmed} x {cell, none} x {pbc all / partial} x {scratch ok / short} x {max_k ok / 12 / 0} x {stress} x {dd}
//   x {accuracy ok / 0 / 1} x {status given / missing} x {sites / none}
// and asserts the exact rejection of each: the order of the checks is written down once more here, by the messages alone.  The
// unarmed column must be what it was before the arming existed: the same code and message whatever the periodic fields hold.
#include <cstdio>
#include <cstdlib>
#include <cstring>

#include "eval_plan.h"

using namespace aimnet;

static const char* NONPERIODIC =
    "eval: embedding point charges take non-periodic input (no images of the sites): pass a per-atom potential with a cell";
static const char* STRESS_CELL = "eval: stress requires a cell and a stress buffer";
static const char* DD_CLUSTER =
    "eval: a domain-decomposed evaluation takes a non-periodic cluster (no cell, no caller-supplied lists), Coulomb 'none' or 'dsf'";
static const char* EMB_STRESS = "eval: the embedding term has no stress (AIMNET_STRESS with an embedding set)";
static const char* EMB_DD = "eval: the embedding term is not carried by a domain-decomposed evaluation";
static const char* P_CELL = "eval: periodic embedding sites need a cell";
static const char* P_PBC = "eval: periodic embedding sites need a cell that is periodic along all three axes (no pbc_sys)";
static const char* P_ACC = "eval: periodic embedding sites need 0 < accuracy < 1";
static const char* P_SCRATCH = "eval: periodic embedding sites: scratch missing or smaller than aimnet_embedding_periodic_scratch_bytes";
static const char* P_STATUS = "eval: periodic embedding sites: status is required";

static EvalRequest base() {
  EvalRequest r{};
  r.L.N = 96; r.L.n_mol = 1; r.L.n_pass = 3;
  r.L.flags = AIMNET_FORCES;
  r.L.coulomb = AIMNET_COULOMB_NONE;
  r.L.max_nb = 64;
  r.L.ewald_kb = 8; r.L.pme_part = 1024;
  r.n_cell = 1; r.nq = 1;
  r.has_forces_out = r.has_stress_out = true;
  r.emb = 1;
  r.emb_sites_ok = true;
  r.emb_scratch_ok = true;
  return r;
}

static long g_cases = 0;

static void expect(const EvalRequest& r, const char* want, const char* what) {
  char msg[512] = "";
  const int rc = eval_validate(r, msg, sizeof msg);
  ++g_cases;
  const bool ok = want ? (rc == AIMNET_E_INVALID && std::strcmp(msg, want) == 0) : rc == 0;
  if (!ok) {
    std::fprintf(stderr, "FAILED: %s\n  got  %d '%s'\n  want '%s'\n  armed %d cell %d full %d acc %g max_k %d status %d scratch %d flags %u dd %d n_ext %d\n",
                 what, rc, msg, want ? want : "(accepted)", r.emb_periodic, r.pbc, r.emb_pbc_full, (double)r.emb_periodic_accuracy,
                 r.emb_periodic_max_k, r.emb_periodic_status, r.emb_periodic_scratch_ok, r.L.flags, r.dd, r.emb_n_ext);
    std::exit(1);
  }
}

int main() {
  char bad_k12[128], bad_k0[128];
  std::snprintf(bad_k12, sizeof bad_k12, "eval: periodic embedding sites need max_k > 0, a multiple of %d (got %d)", 8, 12);
  std::snprintf(bad_k0, sizeof bad_k0, "eval: periodic embedding sites need max_k > 0, a multiple of %d (got %d)", 8, 0);
  const float accs[3] = {1e-6f, 0.0f, 1.0f};
  const int ks[3] = {8192, 12, 0};
  for (int armed = 0; armed < 2; ++armed)
    for (int cell = 0; cell < 2; ++cell)
      for (int full = 0; full < 2; ++full)
        for (int scratch = 0; scratch < 2; ++scratch)
          for (int ki = 0; ki < 3; ++ki)
            for (int stress = 0; stress < 2; ++stress)
              for (int dd = 0; dd < 2; ++dd)
                for (int ai = 0; ai < 3; ++ai)
                  for (int status = 0; status < 2; ++status)
                    for (int n_ext = 0; n_ext <= 64; n_ext += 64) {
                      EvalRequest r = base();
                      r.pbc = cell != 0;
                      r.dd = dd != 0;
                      if (stress) r.L.flags |= AIMNET_STRESS;
                      r.emb_n_ext = n_ext;
                      r.emb_ext_mol_idx = false;
                      r.emb_periodic = armed;
                      r.emb_pbc_full = full != 0;
                      r.emb_periodic_accuracy = accs[ai];
                      r.emb_periodic_max_k = ks[ki];
                      r.emb_periodic_status = status != 0;
                      r.emb_periodic_scratch_ok = scratch != 0;
                      // the checks in front of the embedding's, then the embedding's own: unchanged
                      const char* want = nullptr;
                      if (stress && !cell && !dd) want = STRESS_CELL;
                      else if (dd && cell) want = DD_CLUSTER;
                      else if (stress) want = EMB_STRESS;
                      else if (dd) want = EMB_DD;
                      else if (!armed) want = (n_ext > 0 && cell) ? NONPERIODIC : nullptr;
                      else if (!cell) want = P_CELL;
                      else if (!full) want = P_PBC;
                      else if (ai != 0) want = P_ACC;
                      else if (ki == 1) want = bad_k12;
                      else if (ki == 2) want = bad_k0;
                      else if (!scratch) want = P_SCRATCH;
                      else if (!status) want = P_STATUS;
                      expect(r, want, "the walk");
                      if (!armed) {  // the unarmed column does not read the periodic fields: all of them cleared gives the same
                        EvalRequest z = r;
                        z.emb_pbc_full = false; z.emb_periodic_accuracy = 0.0f; z.emb_periodic_max_k = 0;
                        z.emb_periodic_status = z.emb_periodic_scratch_ok = false;
                        expect(z, want, "unarmed, periodic fields cleared");
                      }
                    }
  // the rest of the embedding's checks follow the armed ones as they follow the unarmed refusal
  EvalRequest r = base();
  r.pbc = true; r.emb_n_ext = 64; r.emb_periodic = 1; r.emb_pbc_full = true; r.emb_periodic_accuracy = 1e-6f; r.emb_periodic_max_k = 64;
  r.emb_periodic_status = r.emb_periodic_scratch_ok = true;
  expect(r, nullptr, "armed and complete");
  r.emb_scratch_ok = false;
  expect(r, "eval: embedding: scratch missing or smaller than aimnet_embedding_scratch_bytes", "the embedding's own scratch");
  r.emb_scratch_ok = true;
  r.L.n_mol = 2; r.n_cell = 2;
  expect(r, "eval: embedding: ext_mol_idx == NULL is allowed with one molecule only (n_mol = 2)", "ext_mol_idx with two systems");
  r.emb_ext_mol_idx = true;
  expect(r, nullptr, "two systems with their own cells");
  r.L.coulomb = AIMNET_COULOMB_EWALD; r.L.ewald_max_k = 8192;  // the system's own Ewald sum beside the embedding's
  expect(r, nullptr, "with Ewald Coulomb");
  r.emb = 0;  // no embedding: nothing of it is read
  r.emb_periodic_max_k = 12;
  expect(r, nullptr, "embedding off");
  std::printf("embedding periodic plan ok: %ld cases\n", g_cases);
  return 0;
}
