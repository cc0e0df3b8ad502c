// Host check of the strain part of the tangent plan (csrc/tangent_plan.h; built and run by tests/test_tangent_plan_strain.py with
// -fsanitize=address,undefined, in the style of tests/d3_tangent_plan_main.cpp; tests/tangent_plan_main.cpp models the unarmed contract
// and stays as it is).  Unarmed (TangentRequest.strain_tangent false, the default) every request is checked and planned as it always
// was, word for word.  Armed (aimnet_engine_set_strain_tangent) every refusal the unarmed request meets keeps its words and its
// precedence; a request that would pass is refused, each case with its own message, for charge_response, no cell, Ewald, PME, DFT-D3,
// an embedding and missing arrays, and is planned with `strain` - and nothing else moved - for Coulomb none / DSF, one and two
// channels, n_cell 1 or n_mol.
// Walked: armed or not  x  both entries  x  Coulomb methods  x  cell / n_cell  x  dftd3  x  embedding  x  arrays  x  channels  x  armed mesh.
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>

#include "tangent_plan.h"

using namespace aimnet;

#define CHECK(cond, what)                                                        \
  do {                                                                           \
    if (!(cond)) {                                                               \
      std::fprintf(stderr, "FAILED: %s  [%s]\n  message: %s\n", what, #cond, msg); \
      std::exit(1);                                                              \
    }                                                                            \
  } while (0)

static TangentRequest base(bool hvp) {
  TangentRequest r{};
  r.entry = hvp ? TangentEntry::Hvp : TangentEntry::ChargeResponse;
  r.N = 18; r.n_mol = 3; r.n_vec = 9; r.nq = 1; r.n_pass = 3; r.max_width = 704;
  r.coulomb = AIMNET_COULOMB_DSF; r.max_nb = 112; r.max_nb_lr = 600; r.max_nb_d3 = 1904; r.ewald_max_k = 8192; r.ewald_kb = 8;
  r.pme_max_mesh = 8192; r.pme_part = 256;
  r.d3_tables = true;
  r.dsf_rc_set = true; r.arrays = true; r.bbox_ok = false; r.pbc = true; r.n_cell = 3;
  r.hv = hvp; r.dq = !hvp;
  return r;
}

static bool same_plan_but_strain(const TangentPlan& P, const TangentPlan& Q) {
  TangentPlan a = P, b = Q;
  a.strain = b.strain = false;
  return std::memcmp(&a, &b, sizeof a) == 0;  // (both value-initialised by tangent_plan: the padding is zero in both)
}

int main() {
  char msg[512];
  long accepted = 0, rejected = 0, refused_by_strain = 0;
  const char* own[] = {"charge_response: a strain tangent is armed", "hvp: strain tangent: a strain direction needs a cell",
                       "hvp: strain tangent: Ewald summation is not carried", "hvp: strain tangent: particle-mesh Ewald is not carried",
                       "hvp: strain tangent: the DFT-D3 block is not carried", "hvp: strain tangent: the embedding term is not carried",
                       "hvp: strain tangent: strain and dvirial are required"};
  long seen[7] = {0, 0, 0, 0, 0, 0, 0};
  {  // the default of the new fields is "unarmed"
    TangentRequest r = base(true);
    msg[0] = 0;
    CHECK(!r.strain_tangent && !r.strain_arrays, "strain_tangent defaults to false");
    CHECK(tangent_validate(r, msg, sizeof msg) == 0, "a plain periodic DSF request passes");
    CHECK(!tangent_plan(r).strain, "and plans no strain");
  }
  for (int hvp = 0; hvp < 2; ++hvp)
    for (int armed = 0; armed < 2; ++armed)
      for (int arrays = 0; arrays < 2; ++arrays)
        for (int coulomb : {AIMNET_COULOMB_NONE, AIMNET_COULOMB_SIMPLE, AIMNET_COULOMB_DSF, AIMNET_COULOMB_EWALD, AIMNET_COULOMB_PME})
          for (int mesh_armed = 0; mesh_armed < 2; ++mesh_armed)
            for (int cellmode = 0; cellmode < 4; ++cellmode)  // none, n_cell 1, n_cell n_mol, n_cell 2 (invalid)
              for (int d3 = 0; d3 < 2; ++d3)
                for (int emb = 0; emb < 3; ++emb)  // none, set, set and armed for the sweep
                  for (int nq = 1; nq <= 2; ++nq)
                    for (int lr_rows : {0, 600}) {
                      TangentRequest r = base(hvp != 0);
                      r.strain_tangent = armed != 0; r.strain_arrays = arrays != 0;
                      r.coulomb = coulomb; r.pme_tangent = mesh_armed != 0 && hvp;
                      r.pbc = cellmode != 0; r.n_cell = cellmode == 1 ? 1 : cellmode == 2 ? r.n_mol : cellmode == 3 ? 2 : 0;
                      r.dftd3 = d3; r.nq = nq; r.max_nb_lr = lr_rows;
                      r.emb_on = emb != 0;
                      if (emb == 2 && hvp) {
                        r.emb_tangent = true; r.emb_potential = r.emb_potential_grad = r.emb_potential_hess = true; r.emb_scratch_ok = true;
                      }
                      msg[0] = 0;
                      const int rc = tangent_validate(r, msg, sizeof msg);
                      TangentRequest off = r;
                      off.strain_tangent = false;
                      char off_msg[512] = "";
                      const int off_rc = tangent_validate(off, off_msg, sizeof off_msg);
                      if (!armed) {  // unarmed: strain_arrays is not read, nothing of the feature is planned
                        TangentRequest other = r;
                        other.strain_arrays = !r.strain_arrays;
                        char other_msg[512] = "";
                        CHECK(tangent_validate(other, other_msg, sizeof other_msg) == rc && std::strcmp(other_msg, msg) == 0,
                              "unarmed: strain_arrays is not read");
                        for (const char* o : own) CHECK(!std::strstr(msg, o), "unarmed: none of the feature's messages");
                        if (rc == 0) CHECK(!tangent_plan(r).strain, "unarmed: no strain in the plan");
                        rc == 0 ? ++accepted : ++rejected;
                        continue;
                      }
                      if (off_rc != 0) {  // every existing refusal keeps its words and its precedence
                        CHECK(rc == off_rc && std::strcmp(msg, off_msg) == 0, "armed: an existing refusal keeps its words and comes first");
                        ++rejected;
                        continue;
                      }
                      // the unarmed request passes: armed, exactly one of the feature's refusals, in this order, or the armed plan
                      int want = -1;
                      if (!hvp) want = 0;
                      else if (!r.pbc) want = 1;
                      else if (coulomb == AIMNET_COULOMB_EWALD) want = 2;
                      else if (coulomb == AIMNET_COULOMB_PME) want = 3;
                      else if (d3) want = 4;
                      else if (r.emb_on) want = 5;
                      else if (!arrays) want = 6;
                      if (want >= 0) {
                        CHECK(rc == AIMNET_E_INVALID && std::strstr(msg, own[want]) == msg, "armed: the refusal of this case, with its own message");
                        ++seen[want]; ++refused_by_strain; ++rejected;
                        continue;
                      }
                      CHECK(rc == 0, "armed: carried");
                      CHECK(coulomb == AIMNET_COULOMB_NONE || coulomb == AIMNET_COULOMB_DSF, "armed: Coulomb none and DSF are what is carried");
                      CHECK(r.n_cell == 1 || r.n_cell == r.n_mol, "armed: n_cell 1 or n_mol");
                      const TangentPlan P = tangent_plan(r), Q = tangent_plan(off);
                      CHECK(P.strain && !Q.strain, "armed: strain is planned");
                      CHECK(same_plan_but_strain(P, Q), "nothing else in the plan moves");
                      ++accepted;
                    }
  {  // charge_response never plans it
    TangentRequest r = base(false);
    r.strain_tangent = r.strain_arrays = true;
    CHECK(!tangent_plan(r).strain, "charge_response plans no strain");
  }
  for (int k = 0; k < 7; ++k)
    if (!seen[k]) {
      std::fprintf(stderr, "FAILED: refusal %d (%s) was never reached\n", k, own[k]);
      return 1;
    }
  if (accepted == 0 || rejected == 0) {
    std::fprintf(stderr, "FAILED: accepted %ld, rejected %ld\n", accepted, rejected);
    return 1;
  }
  std::printf("strain tangent plan ok: %ld accepted, %ld rejected (%ld by the armed checks)\n", accepted, rejected, refused_by_strain);
  return 0;
}
