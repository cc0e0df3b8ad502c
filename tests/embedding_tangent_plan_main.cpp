// Host check of the embedding's part of the tangent plan (csrc/tangent_plan.h; built and run by tests/test_embedding_hessian_host.py
// with -fsanitize=address,undefined, in the style of tests/tangent_plan_main.cpp, which models the unarmed contract and stays as it
// is).  aimnet_engine_hvp with an embedding set is refused with the message it always had unless
// aimnet_engine_set_embedding_tangent armed the sweep (TangentRequest.emb_tangent); armed, the request is checked against what the
// sweep carries, and a request that passes plans the embedding stages.  Walked: armed or not  x  sites or none  x  cell or not  x
// which of potential / potential_grad / potential_hess are given  x  the five Coulomb methods  x  ext_mol_idx given or not  x
// one or two molecules  x  scratch ok or not  x  both entries.
#include <cstdio>
#include <cstdlib>
#include <cstring>

#include "tangent_plan.h"

using namespace aimnet;

static const char* const UNARMED =
    "hvp: the embedding term is not carried by the tangent sweep (aimnet_engine_set_embedding(e, NULL) first)";

#define CHECK(cond, what)                                                                                       \
  do {                                                                                                          \
    if (!(cond)) {                                                                                              \
      std::fprintf(stderr, "FAILED: %s  [%s]\n  message: %s\n", what, #cond, msg);                                \
      std::exit(1);                                                                                             \
    }                                                                                                           \
  } while (0)

static TangentRequest base(bool hvp) {
  TangentRequest r{};
  r.entry = hvp ? TangentEntry::Hvp : TangentEntry::ChargeResponse;
  r.N = 40; r.n_mol = 1; r.n_vec = 3; r.nq = 1; r.n_pass = 3; r.max_width = 704;
  r.coulomb = AIMNET_COULOMB_SIMPLE; r.max_nb = 112; r.max_nb_lr = 600; r.max_nb_d3 = 2832; r.ewald_max_k = 8197; r.ewald_kb = 8;
  r.dsf_rc_set = true; r.arrays = true; r.bbox_ok = false;
  r.hv = hvp; r.dq = !hvp;
  return r;
}

int main() {
  char msg[512];
  long accepted = 0, rejected = 0;
  unsigned seen = 0;  // bit per reject reached
  const int coulombs[] = {AIMNET_COULOMB_NONE, AIMNET_COULOMB_SIMPLE, AIMNET_COULOMB_DSF, AIMNET_COULOMB_EWALD, AIMNET_COULOMB_PME};
  // the default of the new field is "unarmed": a zero-initialised request with an embedding set is refused as before
  {
    TangentRequest r = base(true);
    r.emb_on = true;
    msg[0] = 0;
    CHECK(tangent_validate(r, msg, sizeof msg) == AIMNET_E_INVALID && std::strcmp(msg, UNARMED) == 0, "unarmed: today's message, word for word");
    CHECK(!r.emb_tangent, "emb_tangent defaults to false");
  }
  for (int hvp = 0; hvp < 2; ++hvp)
    for (int armed = 0; armed < 2; ++armed)
      for (int emb_on = 0; emb_on < 2; ++emb_on)
        for (int n_ext : {0, 64})
          for (int pbc = 0; pbc < 2; ++pbc)
            for (int arrays = 0; arrays < 8; ++arrays)  // bit 0 potential, 1 potential_grad, 2 potential_hess
              for (int coulomb : coulombs)
                for (int mol_idx = 0; mol_idx < 2; ++mol_idx)
                  for (int n_mol = 1; n_mol <= 2; ++n_mol)
                    for (int scratch = 0; scratch < 2; ++scratch) {
                      TangentRequest r = base(hvp != 0);
                      r.emb_on = emb_on != 0; r.emb_tangent = armed != 0; r.emb_n_ext = n_ext; r.n_mol = n_mol;
                      r.pbc = pbc != 0; r.n_cell = pbc ? 1 : 0; r.coulomb = coulomb;
                      r.ewald_args = coulomb == AIMNET_COULOMB_EWALD && hvp && !pbc ? 1 : 0;
                      r.emb_potential = arrays & 1; r.emb_potential_grad = (arrays & 2) != 0; r.emb_potential_hess = (arrays & 4) != 0;
                      r.emb_mol_idx = mol_idx != 0; r.emb_scratch_ok = scratch != 0;
                      msg[0] = 0;
                      const int rc = tangent_validate(r, msg, sizeof msg);
                      // the same request without the embedding: what the rest of the checks say
                      TangentRequest bare = r;
                      bare.emb_on = false;
                      char bare_msg[512] = "";
                      const int bare_rc = tangent_validate(bare, bare_msg, sizeof bare_msg);
                      if (!hvp || !emb_on) {  // charge_response ignores the embedding; nothing set: nothing read
                        CHECK(rc == bare_rc && std::strcmp(msg, bare_msg) == 0, "the embedding fields are read by hvp with an embedding set only");
                        continue;
                      }
                      if (!armed) {
                        CHECK(rc == AIMNET_E_INVALID && std::strcmp(msg, UNARMED) == 0, "unarmed: refused with today's message");
                        seen |= 1u << 0;
                        ++rejected;
                        continue;
                      }
                      const bool pot = arrays & 1, grad = (arrays & 2) != 0, hess = (arrays & 4) != 0;
                      const char* want = nullptr;
                      int bit = 0;
                      if (n_ext > 0 && pbc) want = "non-periodic input", bit = 1;
                      else if (pot && !grad) want = "potential_grad beside potential", bit = 2;
                      else if (pot && !hess) want = "potential_hess beside potential", bit = 3;
                      else if (!pot && (grad || hess)) want = "without potential", bit = 4;
                      else if (n_ext > 0 && !mol_idx && n_mol > 1) want = "ext_mol_idx == NULL", bit = 5;
                      else if (coulomb == AIMNET_COULOMB_PME) want = "particle-mesh Ewald", bit = 6;
                      else if (!scratch) want = "aimnet_embedding_tangent_scratch_bytes", bit = 7;
                      if (want) {
                        CHECK(rc == AIMNET_E_INVALID && std::strncmp(msg, "hvp: ", 5) == 0 && std::strstr(msg, want), "armed: the reject and its message");
                        seen |= 1u << bit;
                        ++rejected;
                        continue;
                      }
                      CHECK(rc == bare_rc && std::strcmp(msg, bare_msg) == 0, "armed and complete: the remaining checks decide, as without an embedding");
                      if (rc != 0) continue;
                      ++accepted;
                      const TangentPlan P = tangent_plan(r), B = tangent_plan(bare);
                      CHECK(P.embedding && !B.embedding, "the embedding stages run exactly for an armed request");
                      CHECK(P.backward && P.head && P.keep_passes, "they join a sweep that runs backward");
                      CHECK(P.n_fwd_pass == B.n_fwd_pass && P.cap == B.cap && P.cap_lr == B.cap_lr && P.lr_list == B.lr_list && P.ewald == B.ewald &&
                                P.d3_block == B.d3_block && P.bbox == B.bbox,
                            "nothing else of the plan (and so nothing of the workspace layout) depends on the embedding");
                    }
  {  // an armed request of charge_response plans no embedding stage
    TangentRequest r = base(false);
    r.emb_on = r.emb_tangent = r.emb_scratch_ok = true;
    CHECK(!tangent_plan(r).embedding, "charge_response keeps ignoring the embedding");
  }
  if (seen != 0xffu || accepted == 0) {
    std::fprintf(stderr, "FAILED: a reject was never reached (%x), or nothing was accepted (%ld)\n", seen, accepted);
    return 1;
  }
  std::printf("embedding tangent plan ok: %ld accepted, %ld rejected\n", accepted, rejected);
  return 0;
}
