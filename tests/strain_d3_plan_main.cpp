// Host check of the DFT-D3 term in the strain part of the tangent plan (csrc/tangent_plan.h; built and run by
// tests/test_tangent_plan_strain_d3.py with -fsanitize=address,undefined, in the style of tests/strain_tangent_plan_main.cpp, which
// models the contract without the term and stays as it is).  TangentRequest.strain_d3 is what aimnet_engine_set_strain_terms names.
//   bit clear (the default of `TangentRequest rq{}`): every verdict and message is what it was - an armed strain with options.dftd3 is
//     refused with "the DFT-D3 block is not carried under strain", with the finite-difference block and with the analytic one, at its
//     place between the mesh and the embedding; d3_strain is never planned;
//   bit set: read only by an armed strain sweep of aimnet_engine_hvp with options.dftd3 - everywhere else nothing moves; there every
//     refusal that came before the old message keeps its words and its precedence; then, D3 unarmed, the new message; D3 armed, the
//     request goes on to the checks that followed (embedding, arrays) and is accepted where the same request without the term is, with
//     d3_strain planned and nothing else in the plan moved: no buffer of its own.
// Walked: bit  x  strain armed  x  both entries  x  Coulomb methods  x  cell / n_cell  x  dftd3  x  D3 armed  x  tables  x  embedding  x  arrays
//         x  directions (1, 9, 20000: beyond the finite-difference block's limit).
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

static const char* OLD = "hvp: strain tangent: the DFT-D3 block is not carried under strain (options.dftd3 = 0)";
static const char* NEW =
    "hvp: strain tangent: the DFT-D3 block is carried under strain by its analytic tangent only (aimnet_engine_set_dftd3_tangent(e, 1))";

static TangentRequest base(bool hvp) {
  TangentRequest r{};
  r.entry = hvp ? TangentEntry::Hvp : TangentEntry::ChargeResponse;
  r.N = 18; r.n_mol = 3; r.n_vec = 9; r.nq = 1; r.n_pass = 3; r.max_width = 704;
  r.coulomb = AIMNET_COULOMB_DSF; r.max_nb = 112; r.max_nb_lr = 600; r.max_nb_d3 = 354; r.ewald_max_k = 8192; r.ewald_kb = 8;
  r.pme_max_mesh = 8192; r.pme_part = 256;
  r.d3_tables = true;
  r.dsf_rc_set = true; r.arrays = true; r.bbox_ok = false; r.pbc = true; r.n_cell = 3;
  r.hv = hvp; r.dq = !hvp;
  return r;
}

static bool same_plan_but(const TangentPlan& P, const TangentPlan& Q, bool strain, bool d3) {
  TangentPlan a = P, b = Q;
  a.d3_strain = b.d3_strain = false;
  if (strain) a.strain = b.strain = false;
  if (d3) {
    a.d3_block = b.d3_block = a.d3_analytic = b.d3_analytic = a.want_species = b.want_species = false;
    a.cap_d3 = b.cap_d3 = 0;
  }
  return std::memcmp(&a, &b, sizeof a) == 0;  // (both value-initialised by tangent_plan: the padding is zero in both)
}

int main() {
  char msg[512];
  long accepted = 0, rejected = 0, old_seen = 0, new_seen = 0, carried = 0, went_on = 0;
  {  // the default of the new field is "not named"
    TangentRequest r{};
    msg[0] = 0;
    CHECK(!r.strain_d3, "strain_d3 defaults to false");
    TangentRequest b = base(true);
    CHECK(!b.strain_d3 && tangent_validate(b, msg, sizeof msg) == 0 && !tangent_plan(b).d3_strain, "a plain request plans no d3_strain");
  }
  for (int hvp = 0; hvp < 2; ++hvp)
    for (int armed = 0; armed < 2; ++armed)
      for (int arrays = 0; arrays < 2; ++arrays)
        for (int coulomb : {AIMNET_COULOMB_NONE, AIMNET_COULOMB_SIMPLE, AIMNET_COULOMB_DSF, AIMNET_COULOMB_EWALD, AIMNET_COULOMB_PME})
          for (int cellmode = 0; cellmode < 4; ++cellmode)  // none, n_cell 1, n_cell n_mol, n_cell 2 (invalid)
            for (int d3 = 0; d3 < 2; ++d3)
              for (int d3_armed = 0; d3_armed < 2; ++d3_armed)
                for (int tables = 0; tables < 2; ++tables)
                  for (int emb = 0; emb < 3; ++emb)  // none, set, set and armed for the sweep
                    for (int n_vec : {1, 9, 20000}) {
                      TangentRequest r = base(hvp != 0);
                      r.strain_tangent = armed != 0; r.strain_arrays = arrays != 0;
                      r.coulomb = coulomb; r.pme_tangent = hvp != 0;
                      r.pbc = cellmode != 0; r.n_cell = cellmode == 1 ? 1 : cellmode == 2 ? r.n_mol : cellmode == 3 ? 2 : 0;
                      r.dftd3 = d3; r.d3_tangent = d3_armed != 0 && hvp; r.d3_tables = tables != 0; r.n_vec = n_vec;
                      r.emb_on = emb != 0;
                      if (emb == 2 && hvp) {
                        r.emb_tangent = true; r.emb_potential = r.emb_potential_grad = r.emb_potential_hess = true; r.emb_scratch_ok = true;
                      }
                      // ---- bit clear: the contract as it was --------------------------------------------------------------------
                      msg[0] = 0;
                      const int rc0 = tangent_validate(r, msg, sizeof msg);
                      char msg0[512];
                      std::strcpy(msg0, msg);
                      const bool old_here = rc0 != 0 && std::strcmp(msg0, OLD) == 0;
                      CHECK(!std::strstr(msg0, "carried under strain by its analytic tangent"), "bit clear: never the new message");
                      if (rc0 == 0) CHECK(!tangent_plan(r).d3_strain, "bit clear: d3_strain is never planned");
                      if (rc0 == 0 && hvp && armed) CHECK(!d3, "bit clear: an armed strain sweep that passes has no D3 term");
                      if (old_here) {
                        CHECK(hvp && armed && d3 && r.pbc && coulomb != AIMNET_COULOMB_EWALD && coulomb != AIMNET_COULOMB_PME,
                              "bit clear: the old message at its place");
                        ++old_seen;
                      } else if (hvp && armed && d3 && rc0 != 0) {  // something came first: it must also stop the request without the strain,
                        TangentRequest off = r;                      // or be one of the strain checks in front of the D3 one
                        off.strain_tangent = false;
                        char off_msg[512] = "";
                        const int off_rc = tangent_validate(off, off_msg, sizeof off_msg);
                        CHECK(off_rc != 0 ? std::strcmp(off_msg, msg0) == 0
                                          : (std::strstr(msg0, "needs a cell") || std::strstr(msg0, "Ewald") != nullptr),
                              "bit clear: what precedes the D3 refusal is an earlier check");
                      }
                      // ---- bit set ---------------------------------------------------------------------------------------------
                      TangentRequest s = r;
                      s.strain_d3 = true;
                      msg[0] = 0;
                      const int rc1 = tangent_validate(s, msg, sizeof msg);
                      if (!old_here) {  // the bit is read nowhere else: same verdict, same words, same plan
                        CHECK(rc1 == rc0 && std::strcmp(msg, msg0) == 0, "bit set: nothing moves where the old refusal did not decide");
                        if (rc1 == 0) {
                          const TangentPlan P = tangent_plan(s), Q = tangent_plan(r);
                          CHECK(!P.d3_strain && std::memcmp(&P, &Q, sizeof P) == 0, "bit set: the plan of every other request is what it was");
                        }
                        rc1 == 0 ? ++accepted : ++rejected;
                        continue;
                      }
                      if (!s.d3_tangent) {
                        CHECK(rc1 == AIMNET_E_INVALID && std::strcmp(msg, NEW) == 0, "bit set, D3 unarmed: the new message");
                        ++new_seen; ++rejected;
                        continue;
                      }
                      // D3 armed: the request goes on exactly as the same request without the term does
                      TangentRequest no_d3 = r;
                      no_d3.dftd3 = 0;
                      char nd_msg[512] = "";
                      const int nd_rc = tangent_validate(no_d3, nd_msg, sizeof nd_msg);
                      CHECK(rc1 == nd_rc && std::strcmp(msg, nd_msg) == 0, "bit set, D3 armed: the checks that followed decide, in their words");
                      if (rc1 != 0) {
                        CHECK(std::strstr(msg, "the embedding term is not carried under strain") || std::strstr(msg, "strain and dvirial are required"),
                              "bit set, D3 armed: only the embedding and the arrays can still refuse");
                        ++went_on; ++rejected;
                        continue;
                      }
                      const TangentPlan P = tangent_plan(s);
                      CHECK(P.strain && P.d3_block && P.d3_analytic && P.d3_strain, "bit set, D3 armed: d3_strain is planned");
                      TangentRequest off = s;
                      off.strain_tangent = false;
                      CHECK(same_plan_but(P, tangent_plan(off), true, false), "against the armed block without strain only the strain flags move");
                      CHECK(same_plan_but(P, tangent_plan(no_d3), false, true), "against the strain sweep without the term only the block's fields move");
                      CHECK(P.cap_d3 == tangent_plan(off).cap_d3, "no bytes of its own: the block's rows are the armed block's");
                      ++carried; ++accepted;
                    }
  {  // charge_response and an unarmed sweep never plan it, whatever the bit says
    TangentRequest r = base(false);
    r.strain_tangent = r.strain_arrays = r.strain_d3 = true; r.dftd3 = 1; r.d3_tangent = true;
    CHECK(!tangent_plan(r).d3_strain, "charge_response plans no d3_strain");
    TangentRequest h = base(true);
    h.strain_d3 = true; h.dftd3 = 1; h.d3_tangent = true;
    msg[0] = 0;
    CHECK(tangent_validate(h, msg, sizeof msg) == 0 && !tangent_plan(h).d3_strain && tangent_plan(h).d3_analytic,
          "without a strain the armed block is the block it was");
  }
  if (!old_seen || !new_seen || !carried || !went_on || !accepted || !rejected) {
    std::fprintf(stderr, "FAILED: old %ld new %ld carried %ld went on %ld accepted %ld rejected %ld\n", old_seen, new_seen, carried, went_on,
                 accepted, rejected);
    return 1;
  }
  std::printf("strain d3 plan ok: %ld accepted, %ld rejected; old message %ld, new message %ld, carried %ld, refused later %ld\n", accepted,
              rejected, old_seen, new_seen, carried, went_on);
  return 0;
}
