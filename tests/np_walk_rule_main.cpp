// Prints what csrc/eval_plan.h decides about the long-range list of every request without caller-supplied lists, for
// tests/test_np_walk_rule.py to hold against the host's copy of that rule (aimnetcentral_amd/capacity.py, builds_lr_list).  The host
// sends max_nb_lr > 0 exactly when it expects the engine to build the list; this program does not know the host rule, so every
// request is printed twice - with max_nb_lr = 0 and with a positive one - and the test reads the line the host would have sent.
// One line per request:  pbc coulomb bbox_ok dsf_np_walk dftd3 d3_same_cutoff max_nb_lr | accepted built | eval_validate's message
// Built and run with -fsanitize=address,undefined as a process of its own.
#include <cstdio>

#include "eval_plan.h"

using namespace aimnet;

int main() {
  long lines = 0;
  for (int pbc = 0; pbc < 2; ++pbc)
    for (int coulomb = AIMNET_COULOMB_NONE; coulomb <= AIMNET_COULOMB_PME; ++coulomb)
      for (int bbox_ok = 0; bbox_ok < 2; ++bbox_ok)
        for (int np_walk = 0; np_walk < 2; ++np_walk)
          for (int d3 = 0; d3 < 2; ++d3)
            for (int same = 0; same < 2; ++same)
              for (int max_nb_lr : {0, 2832}) {
                if ((coulomb == AIMNET_COULOMB_EWALD || coulomb == AIMNET_COULOMB_PME) && !pbc) continue;  // the host refuses these itself
                EvalRequest r{};
                r.L.N = bbox_ok ? 1500 : 1499;  // (bbox_applies(N, n_mol) of csrc/engine.h is an input here: bbox_ok)
                r.L.n_mol = 1;
                r.L.n_pass = 3;
                r.L.coulomb = coulomb;
                r.L.dftd3 = d3;
                r.L.d3_same_cutoff = same != 0;
                r.L.max_nb = 112;
                r.L.max_nb_lr = max_nb_lr;
                r.L.max_nb_d3 = d3 ? 2832 : 0;
                r.L.ewald_max_k = r.L.pme_max_mesh = 8192;
                r.L.ewald_kb = 64;
                r.L.pme_part = 512;
                r.nq = 1;
                r.pbc = pbc != 0;
                r.n_cell = pbc;  // Ewald / PME: a full periodic cell (ewald_args stays 0)
                r.d3_tables = true;
                r.dsf_np_walk = np_walk;
                r.bbox_ok = bbox_ok != 0;
                char msg[512] = "";
                const bool ok = eval_validate(r, msg, sizeof msg) == 0 && eval_validate_lists(r, layout_plan(r.L), msg, sizeof msg) == 0;
                const bool built = eval_plan(r).lr == ListFrom::Built;
                std::printf("%d %d %d %d %d %d %d | %d %d | %s\n", pbc, coulomb, bbox_ok, np_walk, d3, same, max_nb_lr, (int)ok, (int)built, msg);
                ++lines;
              }
  std::printf("np walk rule: %ld lines\n", lines);
  return 0;
}
