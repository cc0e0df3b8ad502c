// Host check of the particle-mesh Ewald part of the tangent plan (csrc/tangent_plan.h; built and run by
// tests/test_tangent_plan_pme.py with -fsanitize=address,undefined, in the style of tests/embedding_tangent_plan_main.cpp;
// tests/tangent_plan_main.cpp models the unarmed contract and stays as it is).  aimnet_engine_hvp with AIMNET_COULOMB_PME is refused
// with the message it always had unless aimnet_engine_set_pme_tangent armed the sweep (TangentRequest.pme_tangent); armed, the request
// is checked against what the mesh tangent carries, and a request that passes plans the `pme` branch.  Walked: armed or not  x  the
// five Coulomb methods  x  both entries  x  cell or not  x  ewald_args 0 / 1 / 2  x  mesh capacity  x  list capacity and cutoff  x
// caller matrices  x  embedding (unarmed / armed)  x  atom count  x  directions x systems.
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>

#include "tangent_plan.h"

using namespace aimnet;

static const char* const UNARMED =
    "hvp: the analytic tangent sweep does not cover particle-mesh Ewald (use the exact Ewald sum or DSF, or differences of forces as the "
    "reference does for its PME block, lr.py:903-926)";

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
  r.N = 40; r.n_mol = 1; r.n_vec = 3; r.nq = 1; r.n_pass = 3; r.max_width = 704;
  r.coulomb = AIMNET_COULOMB_PME; r.max_nb = 112; r.max_nb_lr = 600; r.max_nb_d3 = 2832; r.ewald_max_k = 8197; r.ewald_kb = 8;
  r.pme_max_mesh = 8192; r.pme_part = 1024;
  r.dsf_rc_set = true; r.arrays = true; r.bbox_ok = false; r.pbc = true; r.n_cell = 1;
  r.hv = hvp; r.dq = !hvp;
  return r;
}

int main() {
  char msg[512];
  long accepted = 0, rejected = 0;
  unsigned seen = 0;
  {  // the default of the new field is "unarmed": today's refusal, word for word, and today's plan
    TangentRequest r = base(true);
    msg[0] = 0;
    CHECK(!r.pme_tangent, "pme_tangent defaults to false");
    CHECK(tangent_validate(r, msg, sizeof msg) == AIMNET_E_INVALID && std::strcmp(msg, UNARMED) == 0, "unarmed: today's message");
    const TangentPlan P = tangent_plan(r);
    CHECK(!P.pme && !P.lr_list && !P.ewald && P.pme_max_mesh == 0 && P.pme_max_parts == 0, "unarmed: the plan has no mesh branch");
  }
  const int coulombs[] = {AIMNET_COULOMB_NONE, AIMNET_COULOMB_SIMPLE, AIMNET_COULOMB_DSF, AIMNET_COULOMB_EWALD, AIMNET_COULOMB_PME};
  for (int hvp = 0; hvp < 2; ++hvp)
    for (int armed = 0; armed < 2; ++armed)
      for (int coulomb : coulombs)
        for (int ewald_args = 0; ewald_args < 3; ++ewald_args)
          for (int mesh : {0, 511, 512, 8192})
            for (int nb_lr : {0, 600})
              for (int rc_set = 0; rc_set < 2; ++rc_set)
                for (int nbmat = 0; nbmat < 2; ++nbmat)
                  for (int emb = 0; emb < 3; ++emb)  // 0 none, 1 set (unarmed), 2 set and armed
                    for (int N : {40, (1 << 21) - 1, 1 << 21})
                      for (int big : {0, 1}) {
                        TangentRequest r = base(hvp != 0);
                        r.pme_tangent = armed != 0; r.coulomb = coulomb; r.pme_max_mesh = mesh; r.max_nb_lr = nb_lr;
                        r.dsf_rc_set = rc_set != 0; r.nbmat = nbmat != 0; r.N = N;
                        const bool uses_args = hvp && (coulomb == AIMNET_COULOMB_EWALD || (coulomb == AIMNET_COULOMB_PME && armed));
                        r.ewald_args = uses_args ? ewald_args : 0;  // (what tangent_request fills)
                        if (coulomb == AIMNET_COULOMB_SIMPLE) r.pbc = false, r.n_cell = 0;
                        r.emb_on = emb != 0; r.emb_tangent = emb == 2; r.emb_potential = r.emb_potential_grad = r.emb_potential_hess = emb == 2;
                        r.emb_scratch_ok = true;
                        if (big) r.n_vec = 300, r.n_mol = 219;  // 65 700 slices
                        if (N > 40) r.n_vec = 1, r.n_mol = big ? 2 : 1;  // (keep n_vec N max_width below 2^31)
                        msg[0] = 0;
                        const int rc = tangent_validate(r, msg, sizeof msg);
                        TangentRequest off = r;  // the same request with the switch off
                        off.pme_tangent = false;
                        if (uses_args && coulomb == AIMNET_COULOMB_PME) off.ewald_args = 0;
                        char off_msg[512] = "";
                        const int off_rc = tangent_validate(off, off_msg, sizeof off_msg);
                        if (!hvp || coulomb != AIMNET_COULOMB_PME) {
                          CHECK(rc == off_rc && std::strcmp(msg, off_msg) == 0, "the switch is read by hvp with AIMNET_COULOMB_PME only");
                          if (rc == 0) {
                            const TangentPlan P = tangent_plan(r), Q = tangent_plan(off);
                            CHECK(!P.pme && !P.pme_qtot && P.pme_max_mesh == 0 && P.lr_list == Q.lr_list && P.ewald == Q.ewald &&
                                      P.cap_lr == Q.cap_lr, "and plans nothing there");
                          }
                          continue;
                        }
                        if (!armed) {
                          // every earlier check keeps its precedence; where none fires, today's message
                          CHECK(rc == AIMNET_E_INVALID, "unarmed: refused");
                          if (!std::strstr(msg, "embedding") && !std::strstr(msg, "caller-supplied") && !std::strstr(msg, "at most"))
                            CHECK(std::strcmp(msg, UNARMED) == 0, "unarmed: today's message, word for word");
                          seen |= 1u << 0;
                          ++rejected;
                          continue;
                        }
                        const char* want = nullptr;
                        int bit = 0;
                        if (emb == 1) want = "embedding term is not carried", bit = 1;
                        else if (emb == 2) want = "embedding: the analytic tangent sweep does not cover particle-mesh Ewald", bit = 2;
                        else if (nbmat) want = "caller-supplied neighbour matrices", bit = 3;
                        else if (ewald_args == 1) want = "periodic along all three axes", bit = 4;
                        else if (ewald_args == 2 || mesh < 512) want = "0 < ewald_accuracy < 1 and pme_max_mesh >= 512", bit = 5;
                        else if (nb_lr <= 0 || !rc_set) want = "runs its real-space term on the neighbour list", bit = 6;
                        else if (N >= (1 << 21)) want = "fewer than 2097152 atoms", bit = 7;
                        else if ((long)r.n_vec * r.n_mol > 65535) want = "at most 65535 directions x systems", bit = 8;
                        if (want) {
                          CHECK(rc == AIMNET_E_INVALID && std::strncmp(msg, "hvp: ", 5) == 0 && std::strstr(msg, want), "armed: the reject and its message");
                          seen |= 1u << bit;
                          ++rejected;
                          continue;
                        }
                        CHECK(rc == 0, "armed and complete: accepted");
                        ++accepted;
                        for (int nq = 1; nq <= 2; ++nq) {
                          r.nq = nq;
                          const TangentPlan P = tangent_plan(r);
                          CHECK(P.pme && P.lr_list && !P.ewald && P.ewald_max_k == 0 && !P.ewald_qtot, "the mesh branch, with the list, without the k arrays");
                          CHECK(P.backward && P.head && P.keep_passes && P.cap_lr == nb_lr && !P.embedding, "it joins a sweep that runs backward");
                          CHECK(P.pme_qtot == (nq == 2), "two channels: their sum in a buffer of its own");
                          CHECK(P.pme_max_mesh == mesh && P.pme_max_mesh >= 512, "one slice holds the capacity the caller gave");
                          CHECK((long)P.pme_max_parts * r.pme_part >= P.pme_max_mesh && (long)(P.pme_max_parts - 1) * r.pme_part < P.pme_max_mesh,
                                "the influence blocks cover the slice");
                          // 40 bytes per point, direction and system: the slices index grid.y and their bytes fit size_t
                          const size_t slices = (size_t)r.n_vec * r.n_mol;
                          CHECK(slices <= 65535 && slices * (size_t)P.pme_max_mesh <= SIZE_MAX / 40, "the per-direction meshes are in bounds");
                        }
                      }
  {  // charge_response never plans the branch
    TangentRequest r = base(false);
    r.pme_tangent = true;
    CHECK(!tangent_plan(r).pme && !tangent_plan(r).lr_list, "charge_response keeps ignoring the Coulomb method");
  }
  if (seen != 0x1ffu || accepted == 0) {
    std::fprintf(stderr, "FAILED: a reject was never reached (%x), or nothing was accepted (%ld)\n", seen, accepted);
    return 1;
  }
  std::printf("pme tangent plan ok: %ld accepted, %ld rejected\n", accepted, rejected);
  return 0;
}
