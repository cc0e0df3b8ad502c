// Host check of the DFT-D3 part of the tangent plan (csrc/tangent_plan.h; built and run by tests/test_tangent_plan_d3.py with
// -fsanitize=address,undefined, in the style of tests/pme_tangent_plan_main.cpp; tests/tangent_plan_main.cpp models the unarmed
// contract and stays as it is).  Unarmed (TangentRequest.d3_tangent false, the default) a request with the dispersion term is checked
// and planned as it always was: at most 16383 directions, 4 n_vec N max_nb_d3 below 2^31, the finite-difference block.  Armed
// (aimnet_engine_set_dftd3_tangent) the two limits of the replicas are lifted, every other refusal keeps its words and its precedence,
// and the plan sets d3_analytic; the bytes the layout of csrc/hvp.hip gives the block (mirrored below) shrink by at least the replicas.
// Walked: armed or not  x  both entries  x  dftd3  x  tables  x  directions  x  atoms  x  row capacity  x  caller matrices  x  Coulomb.
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
  r.N = 40; r.n_mol = 1; r.n_vec = 3; r.nq = 1; r.n_pass = 3; r.max_width = 704;
  r.coulomb = AIMNET_COULOMB_DSF; r.max_nb = 112; r.max_nb_lr = 600; r.max_nb_d3 = 1904; r.ewald_max_k = 8197; r.ewald_kb = 8;
  r.dftd3 = 1; r.d3_tables = true;
  r.dsf_rc_set = true; r.arrays = true; r.bbox_ok = false; r.pbc = true; r.n_cell = 1;
  r.hv = hvp; r.dq = !hvp;
  return r;
}

static size_t up(size_t b) { return (b + 255) / 256 * 256; }  // Carver::take aligns every buffer to 256 bytes

// bytes of the block's buffers in tangent_layout (csrc/hvp.hip), field by field
static size_t block_bytes(const TangentPlan& P, size_t n, size_t K) {
  if (!P.d3_block) return 0;
  const size_t kn = K * n, cap = (size_t)P.cap_d3;
  const size_t shared = 2 * up(4 * n * cap) + up(4 * n) + up(4 * n) + up(8 * ((n + 255) / 256));  // d3_idx, d3_shift, d3_cnt, aslot, present_part
  if (P.d3_analytic)
    return shared + up(12 * n) + up(48 * n) + up(4 * n) + up(16 * n) + up(8 * n) + 2 * up(16 * kn);  // g, w, dEdcn, xs, e; tcn4, tg4
  const size_t cn = 4 * kn;
  return shared + 2 * up(4 * cn * cap) + 3 * up(4 * cn) + 2 * up(12 * cn) + up(48 * cn) + up(4 * cn) + up(16 * cn) + up(8 * cn) + up(4 * K);
}

int main() {
  char msg[512];
  long accepted = 0, rejected = 0, lifted = 0;
  {  // the default of the new field is "unarmed": today's limits, word for word, and today's plan
    TangentRequest r = base(true);
    msg[0] = 0;
    CHECK(!r.d3_tangent, "d3_tangent defaults to false");
    CHECK(tangent_validate(r, msg, sizeof msg) == 0, "a plain request with the term passes");
    TangentPlan P = tangent_plan(r);
    CHECK(P.d3_block && !P.d3_analytic && P.cap_d3 == 1904 && P.want_species, "unarmed: the finite-difference block");
    r.n_vec = 16384;
    CHECK(tangent_validate(r, msg, sizeof msg) == AIMNET_E_INVALID &&
              std::strcmp(msg, "hvp: at most 16383 directions per sweep (16384 given): split them over several calls") == 0,
          "unarmed: today's direction limit, word for word");
    r.n_vec = 8000; r.N = 40;  // 4 * 8000 * 40 * 1904 = 2.4e9
    CHECK(tangent_validate(r, msg, sizeof msg) == AIMNET_E_INVALID &&
              std::strcmp(msg, "hvp: n_vec * n_atoms * max_nb_d3 too large for one sweep (split the directions)") == 0,
          "unarmed: today's replica limit, word for word");
  }
  for (int hvp = 0; hvp < 2; ++hvp)
    for (int armed = 0; armed < 2; ++armed)
      for (int d3 = 0; d3 < 2; ++d3)
        for (int tables = 0; tables < 2; ++tables)
          for (int K : {1, 3, 5, 8000, 16383, 16384, 65535, 65536})
            for (int N : {1, 27, 40, 2304})
              for (int cap : {0, 16, 1904})
                for (int nbmat = 0; nbmat < 4; ++nbmat)  // none, nbmat, nbmat_lr, nbmat_d3
                  for (int coulomb : {AIMNET_COULOMB_NONE, AIMNET_COULOMB_DSF, AIMNET_COULOMB_PME}) {
                    TangentRequest r = base(hvp != 0);
                    r.d3_tangent = armed != 0; r.dftd3 = d3; r.d3_tables = tables != 0; r.n_vec = K; r.N = N; r.max_nb_d3 = cap;
                    r.nbmat = nbmat == 1; r.nbmat_lr = nbmat == 2; r.nbmat_d3 = nbmat == 3; r.coulomb = coulomb;
                    msg[0] = 0;
                    const int rc = tangent_validate(r, msg, sizeof msg);
                    TangentRequest off = r;
                    off.d3_tangent = false;
                    char off_msg[512] = "";
                    const int off_rc = tangent_validate(off, off_msg, sizeof off_msg);
                    if (!hvp || !d3) {  // the switch is read by hvp with the term only
                      CHECK(rc == off_rc && std::strcmp(msg, off_msg) == 0, "the switch is read by hvp with dftd3 only");
                      if (rc == 0) {
                        const TangentPlan P = tangent_plan(r);
                        CHECK(!P.d3_block && !P.d3_analytic && P.cap_d3 == 0 && !P.want_species, "and plans nothing there");
                      }
                      continue;
                    }
                    if (!armed) {
                      if (rc == 0) {
                        const TangentPlan P = tangent_plan(r);
                        CHECK(P.d3_block && !P.d3_analytic, "unarmed: the finite-difference block");
                        CHECK(K <= 16383 && 4 * (size_t)K * N * (size_t)(cap > 1 ? cap : 1) < (size_t)INT32_MAX, "unarmed: inside both limits");
                        ++accepted;
                      } else {
                        ++rejected;
                      }
                      continue;
                    }
                    // armed: the only two rejects that may differ from the unarmed request's are the two limits of the replicas
                    const bool k_limit = std::strstr(off_msg, "at most 16383 directions") != nullptr;
                    const bool rep_limit = std::strstr(off_msg, "n_vec * n_atoms * max_nb_d3 too large") != nullptr;
                    if (off_rc != 0 && !k_limit && !rep_limit) {
                      CHECK(rc == off_rc && std::strcmp(msg, off_msg) == 0, "armed: every other refusal keeps its words");
                      ++rejected;
                      continue;
                    }
                    if (nbmat) CHECK(rc == AIMNET_E_INVALID && std::strstr(msg, "caller-supplied neighbour matrices"), "armed: matrices stay refused");
                    if (!tables) CHECK(rc == AIMNET_E_INVALID, "armed: no tables, no term");
                    if (K > 65535)
                      CHECK(rc == AIMNET_E_INVALID && std::strstr(msg, "at most 65535 directions per sweep"), "armed: the grid.y limit itself");
                    if (rc != 0) {
                      CHECK(!std::strstr(msg, "16383") && !std::strstr(msg, "max_nb_d3 too large"), "armed: the replicas' limits are gone");
                      ++rejected;
                      continue;
                    }
                    if (off_rc != 0) ++lifted;
                    ++accepted;
                    const TangentPlan P = tangent_plan(r), Q = tangent_plan(off);
                    CHECK(P.d3_block && P.d3_analytic && P.want_species && P.cap_d3 == (cap > 1 ? cap : 1), "armed: the analytic block on the one list");
                    CHECK(P.cap == Q.cap && P.cap_lr == Q.cap_lr && P.lr_list == Q.lr_list && P.backward == Q.backward && P.pme == Q.pme &&
                              P.ewald == Q.ewald && P.cap_d3 == Q.cap_d3,
                          "nothing else in the plan moves");
                    // the new buffers: 32 bytes per (direction, atom); armed is smaller by at least the 4 K replicas of the matrix
                    const size_t a = block_bytes(P, (size_t)N, (size_t)K), u = block_bytes(Q, (size_t)N, (size_t)K);
                    const size_t replicas = 2 * 4 * (size_t)K * N * (size_t)P.cap_d3 * 4;
                    CHECK(a < u && u - a >= replicas, "armed: smaller by at least the replicas");
                    CHECK(a >= 2 * 16 * (size_t)K * N, "tcn4 and tg4 are counted");
                  }
  {  // charge_response never plans the block
    TangentRequest r = base(false);
    r.d3_tangent = true;
    CHECK(!tangent_plan(r).d3_block && !tangent_plan(r).d3_analytic, "charge_response keeps ignoring the term");
  }
  if (accepted == 0 || rejected == 0 || lifted == 0) {
    std::fprintf(stderr, "FAILED: accepted %ld, rejected %ld, lifted %ld\n", accepted, rejected, lifted);
    return 1;
  }
  std::printf("d3 tangent plan ok: %ld accepted (%ld only when armed), %ld rejected\n", accepted, lifted, rejected);
  return 0;
}
