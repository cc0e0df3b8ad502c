// engine.hip - C ABI, device weight store, workspace layout and the launch sequence of one
// AIMNet2 energy(+force, +virial) evaluation.  See include/aimnet_hip.h for the boundary and
// DESIGN.md for the data layout; oracle/aimnet2_analytic.py is the executable specification of
// the order of operations below.
#include <stdarg.h>
#include <stdio.h>
#include <string.h>

#include <map>
#include <string>
#include <vector>

#include "engine.h"
#include "eval_plan.h"

namespace aimnet {

static thread_local char g_err[512] = "";
void set_last_error(const char* fmt, ...) {
  va_list ap;
  va_start(ap, fmt);
  vsnprintf(g_err, sizeof(g_err), fmt, ap);
  va_end(ap);
}

}  // namespace aimnet

using namespace aimnet;

namespace {

enum { FAM_NLIST = 0, FAM_GEOM, FAM_CONV_FWD, FAM_GEMM, FAM_POINTWISE, FAM_COULOMB, FAM_UNCONCAT, FAM_CONV_BWD, FAM_OTHER, FAM_COUNT };

// mark "kernels launched from here on belong to family `fam`" (fam < 0 closes the last interval)
int prof_mark(aimnet_engine* e, hipStream_t s, int fam) {
  if (e->prof_level == 0 || !e->prof_on) return 0;
  if (e->prof_level == 1 && fam >= 0) fam = (fam == FAM_GEMM) ? FAM_GEMM : FAM_OTHER;
  if (fam == e->prof_last) return 0;
  if (e->prof_used == e->prof_ev.size()) {
    hipEvent_t ev;
    AIMNET_HIP_CHECK(hipEventCreate(&ev));
    e->prof_ev.push_back(ev);
    e->prof_fam.push_back(0);
  }
  AIMNET_HIP_CHECK(hipEventRecord(e->prof_ev[e->prof_used], s));
  e->prof_fam[e->prof_used] = fam;
  e->prof_used++;
  e->prof_last = fam;
  return 0;
}

template <typename T>
int dev_upload(aimnet_engine* e, const T* host, size_t n, T** out) {
  void* p = nullptr;
  AIMNET_HIP_CHECK(hipMalloc(&p, n * sizeof(T)));
  e->allocs.push_back(p);
  AIMNET_HIP_CHECK(hipMemcpy(p, host, n * sizeof(T), hipMemcpyHostToDevice));
  *out = (T*)p;
  return 0;
}

// k0_fwd: first k-column the forward GEMM of this layer reads by default (pass 0's first layer skips the embedding block)
int upload_layer(aimnet_engine* e, const float* w, const float* b, int n_in, int n_out, Layer* L, int k0_fwd = 0) {
  L->n_in = n_in;
  L->n_out = n_out;
  L->k_in = pad32(n_in);
  L->k_out = pad32(n_out);
  std::vector<float> wp((size_t)L->k_out * L->k_in, 0.0f), wtp((size_t)L->k_in * L->k_out, 0.0f), bp(L->k_out, 0.0f);
  for (int o = 0; o < n_out; ++o) {
    bp[o] = b[o];
    for (int i = 0; i < n_in; ++i) {
      const float v = w[(size_t)o * n_in + i];
      wp[(size_t)o * L->k_in + i] = v;
      wtp[(size_t)i * L->k_out + o] = v;
    }
  }
  int rc;
  if ((rc = dev_upload(e, wp.data(), wp.size(), &L->w))) return rc;
  if ((rc = dev_upload(e, wtp.data(), wtp.size(), &L->wt))) return rc;
  if ((rc = dev_upload(e, bp.data(), bp.size(), &L->b))) return rc;
  {  // split once, on the host (round to nearest even like v_cvt_pk_bf16_f32)
    // the last 44 % of the k-steps a launch runs over accumulate with the opposite sign (gemm_bf3.hip, "Accumulation bias").
    // 0.56 from the end-to-end energy error against the fp64 oracle (tests/tools/cfg5_ratio.py, relaxed256_probe.py): on the hot
    // config-5 frames the engine's rms distance from fp64 is 1.03 / 1.05 / 1.30 / 1.37 / 1.92 x the fp32 oracle's with the flip
    // at 0.50 / 0.56 / 0.60 / 0.64 / none (exact-fp32 kernels: 0.97); on the relaxed 256-molecule set 0.56 gives the smallest
    // worst-case error (0.66 of the un-widened gate; exact-fp32 kernels 1.05).
    std::vector<unsigned short> s3(wp.size() * 3);
    const int kb0 = k0_fwd / 32, nkf = L->k_in / 32 - kb0, nkb = L->k_out / 32;
    const char* fenv = getenv("AIMNET_BF3_FLIP");  // experiment knob: per mille of the k-steps in the first phase
    const int pm = fenv ? atoi(fenv) : 560;
    L->neg_w3 = kb0 + (pm * nkf + 500) / 1000;
    L->neg_wt3 = (pm * nkb + 500) / 1000;
    split_bf3_host(wp.data(), L->k_out, L->k_in, s3.data(), L->neg_w3);
    if ((rc = dev_upload(e, s3.data(), s3.size(), &L->w3))) return rc;
    split_bf3_host(wtp.data(), L->k_in, L->k_out, s3.data(), L->neg_wt3);
    if ((rc = dev_upload(e, s3.data(), s3.size(), &L->wt3))) return rc;
    // the operand form of gemm_bf3a.hip / gemm_head.hip: odd k-blocks negated, two interleaved accumulator sets (no fitted constant)
    split_bf3_host(wp.data(), L->k_out, L->k_in, s3.data(), BF3_ALT);
    if ((rc = dev_upload(e, s3.data(), s3.size(), &L->w3a))) return rc;
    split_bf3_host(wtp.data(), L->k_in, L->k_out, s3.data(), BF3_ALT);
    if ((rc = dev_upload(e, s3.data(), s3.size(), &L->wt3a))) return rc;
    // the operand form of gemm_h2.hip: fp16 hi + scaled fp16 lo, hi planes of the odd k-blocks negated
    std::vector<unsigned short> s2(wp.size() * 2);
    bool fits = split_h2_host(wp.data(), L->k_out, L->k_in, s2.data(), H2_WEIGHT);
    if ((rc = dev_upload(e, s2.data(), s2.size(), &L->w2a))) return rc;
    L->h_w2a = s2;
    fits = split_h2_host(wtp.data(), L->k_in, L->k_out, s2.data(), H2_WEIGHT) && fits;
    if ((rc = dev_upload(e, s2.data(), s2.size(), &L->wt2a))) return rc;
    L->h_wt2a = s2;
    if (!fits) e->h2_fits = false;
  }
  return 0;
}

// ---- engine switches: one row per switch.  The environment (once, at engine create), aimnet_engine_set_option and
// aimnet_engine_get_option all walk this table; what each switch does is described next to its member in engine.h, the
// user-facing list is in include/aimnet_hip.h.
enum OptKind { OPT_BOOL, OPT_RANGE, OPT_RETIRED };  // stored as value != 0 / clamped to [lo, hi] / reads 0 and accepts only 0
struct OptionRow {
  const char* name;  // option name (NULL: environment only)
  const char* env;   // environment variable read at engine create (OPT_RETIRED: where the removal is recorded)
  int aimnet_engine::*field;
  OptKind kind;
  int lo, hi;
};
const OptionRow OPTIONS[] = {
    {"conv_xe", "AIMNET_CONV_XE", &aimnet_engine::conv_xe, OPT_BOOL, 0, 1},
    {"emb_bias", "AIMNET_EMB_BIAS", &aimnet_engine::emb_bias, OPT_BOOL, 0, 1},
    {"gemm_bf3", "AIMNET_GEMM_BF3", &aimnet_engine::gemm_bf3, OPT_RANGE, 0, 2},
    {"gemm_presplit", "AIMNET_GEMM_PRESPLIT", &aimnet_engine::gemm_presplit, OPT_BOOL, 0, 1},
    {"gemm_h2", "AIMNET_GEMM_H2", &aimnet_engine::gemm_h2, OPT_BOOL, 0, 1},
    {"head_fused", "AIMNET_HEAD_FUSED", &aimnet_engine::head_fused, OPT_BOOL, 0, 1},
    {"prep_fused", "AIMNET_PREP_FUSED", &aimnet_engine::prep_fused, OPT_BOOL, 0, 1},
    {"energy_rides", "AIMNET_ENERGY_RIDES", &aimnet_engine::energy_rides, OPT_BOOL, 0, 1},
    {"status_rides", "AIMNET_STATUS_RIDES", &aimnet_engine::status_rides, OPT_BOOL, 0, 1},
    {"setup_rides", "AIMNET_SETUP_RIDES", &aimnet_engine::setup_rides, OPT_BOOL, 0, 1},
    {"status_owned", "AIMNET_STATUS_OWNED", &aimnet_engine::status_owned, OPT_BOOL, 0, 1},
    {"sums_whole", "AIMNET_SUMS_WHOLE", &aimnet_engine::sums_whole, OPT_BOOL, 0, 1},
    {"nse_merged", "AIMNET_NSE_MERGED", &aimnet_engine::nse_merged, OPT_BOOL, 0, 1},
    {"gemm_chain", "AIMNET_GEMM_CHAIN", &aimnet_engine::gemm_chain, OPT_BOOL, 0, 1},
    {"chain_prefetch", "AIMNET_CHAIN_PREFETCH", &aimnet_engine::chain_prefetch, OPT_RANGE, 0, 2},
    {"d3_cn_rides", "AIMNET_D3_CN_RIDES", &aimnet_engine::d3_cn_rides, OPT_BOOL, 0, 1},
    {"dsf_np_walk", "AIMNET_DSF_NP_WALK", &aimnet_engine::dsf_np_walk, OPT_BOOL, 0, 1},
    {"split_max", "AIMNET_SPLIT_MAX", &aimnet_engine::split_max, OPT_RANGE, 0, INT32_MAX},
    {"p0_moments", "AIMNET_P0_MOMENTS", &aimnet_engine::p0_moments, OPT_BOOL, 0, 1},
    {"spatial_order", "AIMNET_SPATIAL_ORDER", &aimnet_engine::spatial_order, OPT_BOOL, 0, 1},
    {nullptr, "AIMNET_KEEP_INTERMEDIATES", &aimnet_engine::keep_intermediates, OPT_BOOL, 0, 1},
    {"conv_mfma", "profiles/r2_conv_mfma.md", nullptr, OPT_RETIRED, 0, 0},
    {"overlap_coulomb", "profiles/r6_overlap_coulomb_ab.txt", nullptr, OPT_RETIRED, 0, 0},
};
const OptionRow* find_option(const char* name) {
  for (const OptionRow& r : OPTIONS)
    if (r.name && !strcmp(r.name, name)) return &r;
  return nullptr;
}
// the value a switch stores for a request from either source
int option_value(const OptionRow& r, int v) {
  if (r.field == &aimnet_engine::split_max && v < 0) return conv_split_max_default();
  return r.kind == OPT_BOOL ? v != 0 : std::min(r.hi, std::max(r.lo, v));
}
void apply_env_options(aimnet_engine* e) {
  for (const OptionRow& r : OPTIONS) {
    const char* env = r.kind == OPT_RETIRED ? nullptr : getenv(r.env);
    if (env) e->*r.field = option_value(r, atoi(env));
  }
}

// ---- chain plans (gemm_chain.hip): match an MLP sweep against the instantiated shapes and pack its weight streams ----------------
constexpr int CHAIN_NW = 8;  // waves per block of the instantiated shapes
struct PassDesc { int layer, n0, ncols, nk, nt, kb0; bool fwd; };
int chain_build(aimnet_engine* e, const std::vector<Layer>& Ls, const std::vector<PassDesc>& ps, bool bwd, int n_hidden, ChainPlan* plan) {
  plan->shape = -1;
  if (ps.empty() || (int)ps.size() > CHAIN_MAX_PASS) return 0;
  int nk[CHAIN_MAX_PASS] = {}, nt[CHAIN_MAX_PASS] = {};
  for (size_t i = 0; i < ps.size(); ++i) { nk[i] = ps[i].nk; nt[i] = ps[i].nt; }
  if (ps[0].nk > CHAIN_MAX_KB) return 0;
  const int shape = chain_find_shape(CHAIN_NW, bwd, (int)ps.size(), nk, nt, n_hidden);
  if (shape < 0) return 0;
  std::vector<unsigned short> packed;
  for (size_t i = 0; i < ps.size(); ++i) {
    const PassDesc& d = ps[i];
    const Layer& L = Ls[d.layer];
    // forward: rows of W [k_out][k_in]; backward: rows of W^T [k_in][k_out]
    const std::vector<unsigned short>& w2 = d.fwd ? L.h_w2a : L.h_wt2a;
    const int n_rows = d.fwd ? L.k_out : L.k_in, ldk = d.fwd ? L.k_in : L.k_out;
    if (w2.empty()) return 0;
    const int nta = chain_group_a(d.nt);
    for (int g = 0; g < 2; ++g) {  // column group A: the first nta tile slots of every wave, B: the rest
      const int ntg = g == 0 ? nta : d.nt - nta, s0 = g == 0 ? 0 : nta;
      plan->pass[i].w[g] = nullptr;
      if (ntg == 0) continue;
      chain_pack_weights(w2.data(), std::min(n_rows, d.n0 + d.ncols), ldk, d.n0 + 16 * CHAIN_NW * s0, CHAIN_NW, ntg, d.kb0, d.nk, packed);
      unsigned short* dev = nullptr;
      int rc = dev_upload(e, packed.data(), packed.size(), &dev);
      if (rc) return rc;
      plan->pass[i].w[g] = dev;
    }
    plan->pass[i].layer = d.layer;
    plan->pass[i].n0 = d.n0;
    plan->pass[i].ncols = d.ncols;
  }
  plan->n_pass = (int)ps.size();
  plan->shape = shape;
  return 0;
}
// forward sweep of one MLP; k0: leading input columns of the first layer that are skipped (the embedding block behind the bias table)
int chain_plan_fwd(aimnet_engine* e, const std::vector<Layer>& Ls, int k0, ChainPlan* plan) {
  std::vector<PassDesc> ps;
  const int nl = (int)Ls.size();
  for (int l = 0; l < nl; ++l) {
    const int K = Ls[l].k_in - (l == 0 ? k0 : 0), N = Ls[l].k_out;
    if (l > 0 && Ls[l].k_in != Ls[l - 1].k_out) return 0;
    ps.push_back(PassDesc{l, 0, N, K / 32, ceil_div(N / 16, CHAIN_NW), l == 0 ? k0 / 32 : 0, true});
  }
  return chain_build(e, Ls, ps, false, nl - 1, plan);
}
// backward sweep: zbar (k_out of the last layer) -> ... -> xbar (k_in of the first layer from column n0 on; wide outputs in column passes)
int chain_plan_bwd(aimnet_engine* e, const std::vector<Layer>& Ls, int n0, ChainPlan* plan) {
  std::vector<PassDesc> ps;
  const int nl = (int)Ls.size();
  for (int l = nl - 1; l >= 1; --l) ps.push_back(PassDesc{l, 0, Ls[l].k_in, Ls[l].k_out / 32, ceil_div(Ls[l].k_in / 16, CHAIN_NW), 0, false});
  const int N = Ls[0].k_in - n0, tiles = N / 16;
  const int n_col = ceil_div(tiles, 4 * CHAIN_NW);  // column passes of the last product (<= 4 tile slots per wave)
  if (tiles % n_col) return 0;
  for (int c = 0; c < n_col; ++c)
    ps.push_back(PassDesc{0, n0 + c * (N / n_col), N / n_col, Ls[0].k_out / 32, ceil_div(tiles / n_col, CHAIN_NW), 0, false});
  return chain_build(e, Ls, ps, true, nl - 1, plan);
}

}  // namespace

namespace aimnet {
// One MLP GEMM C = epilogue(A . W^T) (fwd: W = L.w [k_out][k_in]) or C = epilogue(A . W) (bwd: L.wt [k_in][k_out]) over the
// operand's k-columns [k0, k0 + K) (fwd) resp. output rows [n0, n0 + N) (bwd) - the sub-blocks the embedding-bias table and the
// pass-0 backward use.  Picks the bf16x3-split kernel or the exact-fp32 one (aimnet_engine::gemm_bf3).
int mlp_gemm(const aimnet_engine* e, hipStream_t s, int epi, const float* A, int lda, const Layer& L, bool fwd, int k0, int n0, int M,
             int N, int K, const float* bias, float* C, float* D, int ldc, const int* brow, int ldbias) {
  const int ldw = fwd ? L.k_in : L.k_out;  // row stride of the weight operand
  const bool bf3 = e->gemm_bf3 == 2 || (e->gemm_bf3 == 1 && M > 256);
  if (bf3) {
    const unsigned short* w3 = (fwd ? L.w3 : L.wt3) + (size_t)n0 * 3 * ldw + (size_t)(k0 / 32) * 96;
    const int kneg = std::max(0, (fwd ? L.neg_w3 : L.neg_wt3) - k0 / 32);  // leading k-steps of this launch with the stored sign
    return launch_gemm_bf3_cfg(s, 0, epi, A, lda, w3, 3 * ldw, M, N, K, bias, C, D, ldc, brow, ldbias, kneg);
  }
  const float* w = (fwd ? L.w : L.wt) + (size_t)n0 * ldw + k0;
  return launch_gemm_nt(s, epi, A, lda, w, ldw, M, N, K, bias, C, D, ldc, brow, ldbias);
}
int mlp_gemm3(const aimnet_engine* e, hipStream_t s, int fmt, int epi, bool out3, const unsigned short* A3, int lda3, const Layer& L,
              bool fwd, int k0, int n0, int M, int N, int K, const float* bias, float* C, unsigned short* C3, int ldc3, float* D, int ldc,
              const int* brow, int ldbias) {
  const int ldw = fwd ? L.k_in : L.k_out;
  const int alt = ((k0 / 32) & 1) ? 2 : 1;
  const int pm = split_planes(fmt);
  const size_t koff = (size_t)(k0 / 32) * 32 * pm;  // first k-block of the launch, in 16-bit elements of a split row
  const unsigned short* w = fmt == SPLIT_H2 ? (fwd ? L.w2a : L.wt2a) : (fwd ? L.w3a : L.wt3a);
  return launch_gemm_split_cfg(s, fmt, 0, epi, out3, SplitArgs{A3 + koff, lda3, w + (size_t)n0 * pm * ldw + koff, pm * ldw, M, N, K, bias, C,
                                                              C3, ldc3, D, ldc, brow, ldbias, alt});
}
// the one-launch energy head of gemm_head.hip covers the shipped architecture (256 -> 128 -> 128 -> 1)
bool head_fusable(const aimnet_engine* e) {
  return e->head.size() == 3 && e->head[0].n_in == 256 && e->head[0].n_out == 128 && e->head[1].n_in == 128 &&
         e->head[1].n_out == 128 && e->head[2].n_in == 128 && e->head[2].n_out == 1 && e->mlp[e->arch.n_pass - 1].back().k_out == 256 &&
         !e->arch.last_linear[e->arch.n_pass - 1] && e->head_fused != 0;
}
// GEMM activations in split form for this batch?  SPLIT_NONE, or SPLIT_H2 (fp16x2, gemm_h2.hip) / SPLIT_BF3 (bf16x3, gemm_bf3a.hip)
int split_format(const aimnet_engine* e, int n_rows) {
  const bool bf3 = e->gemm_bf3 == 2 || (e->gemm_bf3 == 1 && n_rows > 256);  // the batches that take the split GEMMs at all (mlp_gemm)
  if (!(e->gemm_presplit != 0 && bf3 && !e->keep_intermediates)) return SPLIT_NONE;
  return (e->gemm_h2 && e->h2_fits) ? SPLIT_H2 : SPLIT_BF3;
}

// ---- one MLP sweep.  Split activations (sfmt SPLIT_BF3 = bf16x3, SPLIT_H2 = fp16x2): ONE launch of gemm_chain.hip where the pass has a plan
// (fp16x2 form only), else one launch per layer.  x: the input rows in split form; H[l]: layer outputs (hidden ones in split form -
// the chain does not write them -, the last in fp32, or in split form for the fused energy head: `split_last`); D[l]: GELU' (fp32).
// SPLIT_NONE: fp32 rows throughout, one mlp_gemm per layer.
int mlp_sweep_fwd(const aimnet_engine* e, hipStream_t s, int sfmt, int p, int N, const int* numbers, const float* x, float* const* H,
                  float* const* D, bool split_last, bool chain) {
  const aimnet_arch& ar = e->arch;
  const std::vector<Layer>& Ls = e->mlp[p];
  const int nl = (int)Ls.size(), pm = split_planes(sfmt);
  const bool emb0 = p == 0 && e->emb_bias && e->emb_bias0;
  const ChainPlan& cf = e->chain_fwd[p][emb0 ? 1 : 0];
  if (sfmt == SPLIT_H2 && chain && cf.shape >= 0) {
    ChainArgs ca{};
    ca.x = reinterpret_cast<const unsigned short*>(x) + (emb0 ? (256 / 32) * 64 : 0);
    ca.ldx = 2 * Ls[0].k_in;
    ca.M = N;
    ca.prefetch = e->chain_prefetch;
    for (int i = 0; i < cf.n_pass; ++i) {
      const int l = cf.pass[i].layer, ko = Ls[l].k_out;
      const bool last = l == nl - 1, linear = last && ar.last_linear[p];
      ChainPass& cp = ca.p[i];
      cp.w[0] = cf.pass[i].w[0];
      cp.w[1] = cf.pass[i].w[1];
      cp.kb0 = 0;
      cp.ncols = cf.pass[i].ncols;
      cp.epi = linear ? CH_BIAS_F32 : (last && split_last) ? CH_GELU_H2G : CH_GELU_F32;
      cp.bias = (l == 0 && emb0) ? e->emb_bias0 : Ls[l].b;
      cp.brow = (l == 0 && emb0) ? numbers : nullptr;
      cp.ldbias = ko;
      cp.D = linear ? nullptr : D[l];
      cp.ldd = ko;
      cp.C = H[l];
      cp.ldc = ko;
      cp.C2 = last ? reinterpret_cast<unsigned short*>(H[l]) : nullptr;
      cp.ldc2 = 2 * ko;
    }
    return launch_gemm_chain(s, cf.shape, ca);
  }
  const float* hin = x;  // fp32 rows, or split rows behind the same pointer
  int ld_in = Ls[0].k_in;
  for (int l = 0; l < nl; ++l) {
    const bool last = l == nl - 1, linear = last && ar.last_linear[p];
    // the last layer's output is read by pointwise kernels (fp32) - or, in split form, by the fused head
    const bool f32out = sfmt == SPLIT_NONE || (last && !split_last);
    const int epi = linear ? EPI_BIAS : EPI_BIAS_GELU, ko = Ls[l].k_out;
    const int k0 = (l == 0 && emb0) ? 256 : 0;  // embedding columns folded into the per-element bias table
    const float* bias = k0 ? e->emb_bias0 : Ls[l].b;
    const int* brow = k0 ? numbers : nullptr;
    float* Dl = linear ? nullptr : D[l];
    if (sfmt == SPLIT_NONE)
      RC(mlp_gemm(e, s, epi, hin + k0, ld_in, Ls[l], true, k0, 0, N, ko, Ls[l].k_in - k0, bias, H[l], Dl, ko, brow, k0 ? ko : 0));
    else
      RC(mlp_gemm3(e, s, sfmt, epi, !f32out, reinterpret_cast<const unsigned short*>(hin), pm * ld_in, Ls[l], true, k0, 0, N, ko,
                   Ls[l].k_in - k0, bias, f32out ? H[l] : nullptr, f32out ? nullptr : reinterpret_cast<unsigned short*>(H[l]), pm * ko, Dl,
                   ko, brow, k0 ? ko : 0));
    hin = H[l];
    ld_in = ko;
  }
  return 0;
}
// adjoint sweep: zcur = adjoint of the last layer's pre-activation (split form - SPLIT_NONE: fp32 -, GELU' applied) -> zcur = xbar
// (fp32, row stride k_in of the first layer; conv_only: only its columns 256.. are formed).  zcur / znext are the ping-pong buffers.
int mlp_sweep_bwd(const aimnet_engine* e, hipStream_t s, int sfmt, int p, int N, bool conv_only, float*& zcur, float*& znext,
                  float* const* D, bool chain) {
  const std::vector<Layer>& Ls = e->mlp[p];
  const int nl = (int)Ls.size(), pm = split_planes(sfmt);
  int ld = Ls[nl - 1].k_out;
  const ChainPlan& cb = e->chain_bwd[p][(p == 0 && conv_only) ? 1 : 0];
  if (sfmt == SPLIT_H2 && chain && cb.shape >= 0 && !(conv_only && p != 0)) {
    ChainArgs ca{};
    ca.x = reinterpret_cast<const unsigned short*>(zcur);
    ca.ldx = 2 * ld;
    ca.M = N;
    ca.prefetch = e->chain_prefetch;
    for (int i = 0; i < cb.n_pass; ++i) {
      const int l = cb.pass[i].layer;
      ChainPass& cp = ca.p[i];
      cp.w[0] = cb.pass[i].w[0];
      cp.w[1] = cb.pass[i].w[1];
      cp.kb0 = 0;
      cp.ncols = cb.pass[i].ncols;
      if (l > 0) {  // adjoint of a hidden activation: x GELU'(z_{l-1}), stays in LDS
        cp.D = D[l - 1];
        cp.ldd = Ls[l].k_in;
      } else {  // xbar (fp32), in column passes
        cp.C = znext + cb.pass[i].n0;
        cp.ldc = Ls[0].k_in;
      }
    }
    int rc = launch_gemm_chain(s, cb.shape, ca);
    std::swap(zcur, znext);
    return rc;
  }
  for (int l = nl - 1; l >= 0; --l) {
    const Layer& L = Ls[l];
    const int n0 = (l == 0 && conv_only) ? 256 : 0;  // first column of xbar that is formed
    const int epi = l > 0 ? EPI_MUL : EPI_NONE;
    float* Dl = l > 0 ? D[l - 1] : nullptr;
    if (sfmt == SPLIT_NONE)
      RC(mlp_gemm(e, s, epi, zcur, ld, L, false, 0, n0, N, L.k_in - n0, L.k_out, nullptr, znext + n0, Dl, L.k_in));
    else  // the adjoints of hidden activations stay in split form, xbar is fp32
      RC(mlp_gemm3(e, s, sfmt, epi, l > 0, reinterpret_cast<const unsigned short*>(zcur), pm * ld, L, false, 0, n0, N, L.k_in - n0, L.k_out,
                   nullptr, l > 0 ? nullptr : znext + n0, l > 0 ? reinterpret_cast<unsigned short*>(znext) : nullptr,
                   l > 0 ? pm * L.k_in : 0, Dl, L.k_in));
    std::swap(zcur, znext);
    ld = L.k_in;
  }
  return 0;
}
int max_width(const aimnet_engine* e) {
  int w = 32;
  for (int p = 0; p < e->arch.n_pass; ++p)
    for (const Layer& L : e->mlp[p]) w = std::max(w, std::max(L.k_in, L.k_out));
  for (const Layer& L : e->head) w = std::max(w, std::max(L.k_in, L.k_out));
  return w;
}
}  // namespace aimnet

namespace {

// ---- workspace layout ---------------------------------------------------------------------------
struct Workspace {
  NlistBuffers nl;
  int *nb_idx, *nb_shift, *nb_cnt;
  int *lr_idx, *lr_shift, *lr_cnt;
  float4* pg;
  float* a[AIMNET_MAX_PASS];       // features entering pass p
  float* q[AIMNET_MAX_PASS];       // charges after pass p (p < n_pass-1)
  float* x[AIMNET_MAX_PASS];       // MLP input rows
  float* V[AIMNET_MAX_PASS];
  float* Vq[AIMNET_MAX_PASS];
  float* H[AIMNET_MAX_PASS][AIMNET_MAX_LAYERS];
  float* D[AIMNET_MAX_PASS][AIMNET_MAX_LAYERS];
  float* Fm[AIMNET_MAX_PASS];
  float* Dm[AIMNET_MAX_PASS];
  float* hH[AIMNET_MAX_LAYERS];
  float* hD[AIMNET_MAX_LAYERS];
  float* e_atom;
  double* ecoul;
  float *qbar, *qbar2, *fgrad, *virial_atom, *abar;
  float* qtot;   // NSE models: alpha + beta charges (the Coulomb kernels and the `charges` output see these)
  double* part;  // per-(system, slice) partial sums of the molecule reductions
  double* part_e;  // [n_mol][S] energy partial sums when the energy reduction rides on the stress launches
  int S;         // slices per molecule
  float4* pairbuf;   // reverse-pair conv backward (LayoutPlan::xe): pair buffer + reverse map
  int* rev;
  unsigned long long* rev_tab;  // per-atom hash tables of the rows (hash form of the reverse-pair map)
  float *zb0, *zb1;  // ping-pong adjoint buffers (N x max padded width)
  float *Sbar, *Sqbar;
  int *d3_idx, *d3_shift, *d3_cnt;   // DFT-D3 neighbour matrix (aliases the LR list when both use one cutoff)
  float *d3w, *dEdcn;                // per-atom D3 reference weights (12 floats) and dE/dCN
  float4* d3xs;                      // (x, y, z, species slot) per atom: one 16 B gather per D3 neighbour
  EwaldBuffers ew;                   // Ewald: per-system parameters, fractional coordinates, k entries (ewald.hip)
  int* bad_part;                     // per-wave input sanity flags of launch_mol_start (status array not zeroed, SrRiders::status_all)
  int* aslot;                        // species slot of every atom (pass-0 moments, DFT-D3)
  unsigned long long* present_part;  // per-block masks of the slots present
  int n_part;
  size_t total;
};

// P: what the layout has to know beyond the sizes (eval_plan.h) - taken as decided, nothing is re-derived here
void layout(const aimnet_engine* e, int N, int n_mol, const aimnet_eval_options* opt, const LayoutPlan& P, char* base, Workspace& W,
            std::map<std::string, View>* views) {
  Carver c{base, 0, views};
  const int np = e->arch.n_pass;
  const bool grad = P.grad;
  const size_t n = (size_t)N;
  const int cap = P.cap, cap_lr = P.cap_lr;
  char* nl_base = c.take<char>(nlist_scratch_bytes(N, n_mol));
  if (base) nlist_carve(W.nl, nl_base, N, n_mol);
  if (views)  // the wrapped coordinates sit at a fixed position inside the nlist scratch
    (*views)["xw"] = View{(size_t)(nl_base - base) + nlist_xw_offset(n_mol), n * 3, 4, 3};
  W.nb_idx = c.take<int>(n * cap, "nb_idx", cap);
  W.nb_shift = c.take<int>(n * cap, "nb_shift", cap);
  W.nb_cnt = c.take<int>(n, "nb_cnt", 1);
  W.lr_idx = c.take<int>(n * cap_lr, "lr_idx", cap_lr);
  W.lr_shift = c.take<int>(n * cap_lr, "lr_shift", cap_lr);
  W.lr_cnt = c.take<int>(n, "lr_cnt", 1);
  {
    const bool d3 = opt->dftd3 != 0;
    const bool share = P.d3_in_lr;  // one matrix for the D3 list and the DSF list
    const int cap_d3 = P.cap_d3;
    W.d3_idx = share ? W.lr_idx : c.take<int>(n * cap_d3, "d3_idx", cap_d3);
    W.d3_shift = share ? W.lr_shift : c.take<int>(n * cap_d3, "d3_shift", cap_d3);
    W.d3_cnt = share ? W.lr_cnt : c.take<int>(d3 ? n : 0, "d3_cnt", 1);
    W.d3w = c.take<float>(d3 ? n * 12 : 0);
    W.dEdcn = c.take<float>(d3 ? n : 0);
    W.d3xs = c.take<float4>(d3 ? n : 0);
  }
  {
    const bool pme = opt->coulomb == AIMNET_COULOMB_PME;
    const bool ew = opt->coulomb == AIMNET_COULOMB_EWALD;
    W.ew.max_k = P.ewald_max_k;
    W.ew.sys = c.take<EwaldSystem>(ew || pme ? (size_t)n_mol : 0);
    W.ew.frac = c.take<double>(ew ? n * 3 : 0);
    W.ew.k = c.take<EwaldK>(ew ? (size_t)W.ew.max_k : 0);
    W.ew.max_mesh = P.pme_max_mesh;
    W.ew.max_parts = P.pme_max_parts;
    const size_t mesh_all = (size_t)W.ew.max_mesh * (pme ? (size_t)n_mol : 0);
    W.ew.meshq = c.take<long long>(mesh_all);
    W.ew.ma = c.take<double>(2 * mesh_all);
    W.ew.mb = c.take<double>(2 * mesh_all);
    W.ew.bmod = c.take<double>(pme ? (size_t)n_mol * 3 * PME_MAX_AXIS : 0);
    W.ew.vpart = c.take<double>(pme ? (size_t)n_mol * W.ew.max_parts * 8 : 0);
  }
  W.pg = c.take<float4>(n * cap, "pair_geom", cap);
  char name[32];
  float* x_shared = nullptr;
  float* h_shared[2] = {nullptr, nullptr};
  const bool share = !e->keep_intermediates;  // (not the pointers: in the size-query pass every pointer is NULL)
  // pre-split activations (gemm_bf3a.hip): the shared operand buffers hold 6 instead of 4 bytes per element
  const size_t ps_num = P.split_format != SPLIT_NONE ? 3 : 2;
  if (share) {
    int ldx_max = 32, h_max = 32;
    for (int p = 0; p < np; ++p) {
      ldx_max = std::max(ldx_max, e->mlp[p][0].k_in);
      for (size_t l = 0; l + 1 < e->mlp[p].size(); ++l) h_max = std::max(h_max, e->mlp[p][l].k_out);
    }
    for (size_t l = 0; l + 1 < e->head.size(); ++l) h_max = std::max(h_max, e->head[l].k_out);
    x_shared = c.take<float>(n * ldx_max * ps_num / 2, "x_shared", ldx_max);
    h_shared[0] = c.take<float>(n * h_max * ps_num / 2, "h_shared0", h_max);
    h_shared[1] = c.take<float>(n * h_max * ps_num / 2, "h_shared1", h_max);
  }
  for (int p = 0; p < np; ++p) {
    snprintf(name, sizeof name, "a%d", p);
    W.a[p] = p == 0 ? nullptr : c.take<float>(n * 256, name, 256);  // pass 0 reads the embedding table itself
    snprintf(name, sizeof name, "q%d", p);
    W.q[p] = c.take<float>(n * e->nq, name, 1);
    const int ldx = e->mlp[p][0].k_in;
    snprintf(name, sizeof name, "x%d", p);
    W.x[p] = share ? x_shared : c.take<float>(n * ldx, name, ldx);
    W.V[p] = c.take<float>(n * 576);
    W.Vq[p] = c.take<float>(n * 36 * e->nq);
    for (size_t l = 0; l < e->mlp[p].size(); ++l) {
      const int ld = e->mlp[p][l].k_out;
      snprintf(name, sizeof name, "h%d_%d", p, (int)l);
      const bool hidden = l + 1 < e->mlp[p].size();  // the last layer's output (q~, f~, delta_a / aim) is read again later
      // (pre-split activations: the last pass' output feeds the fused head in split form - 6 bytes per element)
      const size_t own = (!hidden && p == np - 1) ? n * ld * ps_num / 2 : n * ld;
      W.H[p][l] = (hidden && share) ? h_shared[l & 1] : c.take<float>(own, name, ld);
      snprintf(name, sizeof name, "d%d_%d", p, (int)l);
      W.D[p][l] = grad ? c.take<float>(n * ld, name, ld) : nullptr;
    }
    W.Fm[p] = c.take<float>((size_t)n_mol * e->nq);
    W.Dm[p] = c.take<float>((size_t)n_mol * e->nq);
  }
  for (size_t l = 0; l + 1 < e->head.size(); ++l) {
    const int ld = e->head[l].k_out;
    W.hH[l] = share ? h_shared[l & 1] : c.take<float>(n * ld);
    W.hD[l] = grad ? c.take<float>(n * ld) : nullptr;
  }
  W.e_atom = c.take<float>(n, "e_atom", 1);
  W.ecoul = c.take<double>(n, "ecoul", 1);
  W.qbar = c.take<float>(n * e->nq, "qbar", 1);
  W.qbar2 = c.take<float>(n * e->nq, "qbar2", 1);  // (the merged NSE adjoint writes the next pass' qbar beside the one it sums over)
  W.qtot = c.take<float>(e->nq > 1 ? n : 0, "qtot", 1);
  W.fgrad = c.take<float>(n * 3, "fgrad", 3);
  W.virial_atom = c.take<float>(n * 9);
  W.S = P.S;
  W.part = c.take<double>((size_t)n_mol * W.S * 9);
  W.part_e = c.take<double>((size_t)n_mol * W.S);
  if (grad) {
    const int mw = max_width(e);
    W.abar = c.take<float>(n * 256, "abar", 256);
    W.zb0 = c.take<float>(n * mw * ps_num / 2, "zb0", mw);
    W.zb1 = c.take<float>(n * mw * ps_num / 2, "zb1", mw);
    // Sbar doubles as the species-moment table T of pass 0 (N x nslots x 64), which outlives no Sbar
    W.Sbar = c.take<float>(n * std::max(1024, e->nslots * 64), "Sbar", 1024);
    W.Sqbar = c.take<float>(n * 64 * e->nq, "Sqbar", 64);
  } else {
    W.abar = W.zb0 = W.zb1 = W.Sbar = W.Sqbar = nullptr;
  }
  W.pairbuf = c.take<float4>(P.xe ? n * cap : 0);
  W.rev = c.take<int>(P.xe ? n * cap : 0);
  W.rev_tab = c.take<unsigned long long>(P.xe ? pair_hash_bytes(N) / sizeof(unsigned long long) : 0);
  W.n_part = (N + 255) / 256;
  W.aslot = c.take<int>(n);
  W.bad_part = c.take<int>((n + 63) / 64);
  W.present_part = c.take<unsigned long long>((size_t)W.n_part);
  W.total = align_up(c.off, 256);
}

// ---- one evaluation in stages -------------------------------------------------------------------
// eval_plan.h decides, once, who does which job; every stage below (a member of this context) reads from the plan whether a job is
// its own.
struct Eval {
  aimnet_engine* e;
  hipStream_t s;
  const aimnet_inputs* in;
  const aimnet_eval_options* opt;
  const aimnet_outputs* out;
  Workspace& W;
  const EvalPlan& P;
  int N, n_mol, n_cell, np, nq;
  bool pbc;
  const aimnet::DdLink* dd;  // spatial domain decomposition (aimnet_engine_set_dd) or NULL
  const int* mol_c;          // mol_idx clamped to [0, n_mol): memory-safe whatever the caller passed (status[6] reports it)
  const int* order;          // binned systems: centre atoms are processed in the bin-sorted order of the cell list (kernels.h, `order`)
  const float* q_fin;        // final charges (NSE: alpha + beta is the charge everything downstream sees)
  // reverse-pair map through per-atom hash tables of the rows (once per neighbour list).  Its only reader is launch_pair_force, the
  // last kernel of the backward, so the two small kernels ride on later launches: the hash build on the SR-Coulomb launch, the lookup
  // on the DSF walk (VALU-bound, the lookup is latency-bound) or else on the energy reduction - kernels.h PairMapRider
  PairMapRider pair_map() const {
    if (!P.rev_hash) return PairMapRider{};
    return PairMapRider{W.nb_idx, n_cell > 0 ? W.nb_shift : nullptr, W.nb_cnt, P.layout.cap, N, W.rev_tab, W.rev, ceil_div(N, 4)};
  }
  int prepare(), lists_built(), lists_imported(), forward(), head(SrRiders& rider), coulomb(const SrRiders& head_rider), join();
  int embedding();
  int head_bwd(float*& zcur, float*& znext), nse_bwd(int p, float* znext), backward(), finalize();
};

// status words, molecule offsets / sanity flags / species slots (and, small periodic batches, the whole cell-list preparation)
int Eval::prepare() {
  const int* slot_of_z = P.want_species ? e->slot_of_z : nullptr;
  if (P.prep == Prep::FusedSmall)
    return launch_prep_small(s, in->coord, in->mol_idx, in->numbers, N, n_mol, pbc ? in->cell : nullptr, n_cell, in->pbc,
                             in->pbc_sys, e->arch.rc, out->status, slot_of_z, W.aslot, W.present_part, W.nl);
  const bool owned = P.status == StatusZero::RiderOwned;
  if (!owned) AIMNET_HIP_CHECK(hipMemsetAsync(out->status, 0, 8 * sizeof(int), s));
  // periodic fast path: the cell + bin-grid setup block rides on this launch (it needs none of its output)
  CellSetupRider csr{};
  const bool setup_rides = P.prep == Prep::SeparateSetupRider;
  if (setup_rides) csr = cell_setup_rider(in->cell, n_cell, in->pbc, in->pbc_sys, e->arch.rc, N, n_mol, W.nl);
  return launch_mol_start(s, in->mol_idx, N, n_mol, W.nl.mol_start, W.nl.mol_c, in->numbers, out->status + 6, slot_of_z,
                          W.aslot, W.present_part,  // + aslot / present species
                          setup_rides ? &csr : nullptr, owned ? W.bad_part : nullptr);
}

// the engine's own lists (the pair geometry (u, d) of the short-range list is written by the list builder itself)
int Eval::lists_built() {
  const float rc = e->arch.rc;
  int* status = out->status;
  if (P.prep != Prep::FusedSmall)
    RC(launch_wrap(s, in->coord, mol_c, N, n_mol, in->cell, n_cell, in->pbc, W.nl, in->pbc_sys, pbc ? rc : 0.0f,
                   P.prep == Prep::SeparateSetupRider));
  if (P.bbox) RC(launch_bbox(s, n_mol, W.nl));
  RC(launch_nlist(s, N, n_mol, mol_c, in->cell, n_cell, in->pbc, rc, rc, P.layout.cap, N, 0, W.nl, W.nb_idx, W.nb_shift, W.nb_cnt,
                  status + 0, status + 2, W.pg, P.sr_status_rides));
  if (P.lr == ListFrom::Built)  // (periodic DSF and large non-periodic systems need no list: they walk the short-range cell grid)
    RC(launch_nlist(s, N, n_mol, mol_c, in->cell, n_cell, in->pbc, opt->dsf_rc, -1.0f, P.layout.cap_lr, N, 0, W.nl, W.lr_idx,
                    W.lr_shift, W.lr_cnt, status + 1, status + 3));
  if (P.d3 == ListFrom::Built) {
    D3CnRider cnr;  // the coordination numbers ride on the (cell-grid) build of the D3 matrix
    if (P.d3_cn_rides) {
      cnr.aslot = W.aslot; cnr.rcov = e->d3.rcov; cnr.nref = e->d3.nref; cnr.cnref = e->d3.cnref; cnr.d3w = W.d3w;
    }
    RC(launch_nlist(s, N, n_mol, mol_c, in->cell, n_cell, in->pbc, opt->d3_cutoff, -1.0f, P.cap_d3, N, 0, W.nl, W.d3_idx,
                    W.d3_shift, W.d3_cnt, status + 4, status + 5, nullptr, false, P.d3_cn_rides ? &cnr : nullptr));
  }
  return 0;
}

// caller-supplied matrices: the reference hands them to the model as they are (calculator.py:1069-1071) - import them into the row
// format of the kernels; coordinates as given (the shifts refer to them), no bins, centres processed in input order
int Eval::lists_imported() {
  const int cap = P.layout.cap, cap_lr = P.layout.cap_lr;
  int* status = out->status;
  RC(launch_wrap(s, in->coord, mol_c, N, n_mol, nullptr, 0, in->pbc, W.nl));
  RC(launch_import_list(s, in->nbmat, pbc ? in->shifts : nullptr, in->nbmat_width, N, mol_c, in->cell, n_cell, cap, W.nl, W.nb_idx,
                        W.nb_shift, W.nb_cnt, status + 0, status + 2, W.pg, status + 6));
  RC(launch_list_symmetry_check(s, W.nb_idx, pbc ? W.nb_shift : nullptr, W.nb_cnt, cap, N, status + 6));
  if (P.lr == ListFrom::Imported) {
    RC(launch_import_list(s, in->nbmat_lr, pbc ? in->shifts_lr : nullptr, in->nbmat_lr_width, N, mol_c, in->cell, n_cell, cap_lr,
                          W.nl, W.lr_idx, W.lr_shift, W.lr_cnt, status + 1, status + 3, nullptr, status + 6));
    // (the bin-ordered coordinate stream of the list builder is unused with caller-supplied matrices: 16 bytes per atom of scratch)
    RC(launch_list_symmetry_check(s, W.lr_idx, pbc ? W.lr_shift : nullptr, W.lr_cnt, cap_lr, N, status + 6, 64,
                                  (unsigned long long*)W.nl.xs));
  }
  if (P.d3 == ListFrom::Imported) {
    const int* src = in->nbmat_d3 ? in->nbmat_d3 : in->nbmat_lr;
    const int* src_sh = in->nbmat_d3 ? in->shifts_d3 : in->shifts_lr;
    const int src_w = in->nbmat_d3 ? in->nbmat_d3_width : in->nbmat_lr_width;
    RC(launch_import_list(s, src, pbc ? src_sh : nullptr, src_w, N, mol_c, in->cell, n_cell, P.cap_d3, W.nl, W.d3_idx, W.d3_shift,
                          W.d3_cnt, status + 4, status + 5, nullptr, status + 6));
    RC(launch_list_symmetry_check(s, W.d3_idx, pbc ? W.d3_shift : nullptr, W.d3_cnt, P.cap_d3, N, status + 6, 64,
                                  (unsigned long long*)W.nl.xs));
  }
  return 0;
}

// a^0 = afv[Z] is never materialised: pass 0 gathers the embedding rows directly (conv_fwd / conv_bwd row_of, update_a)
int Eval::forward() {
  const int sfmt = P.layout.split_format;
  for (int p = 0; p < np; ++p) {
    const std::vector<Layer>& Ls = e->mlp[p];
    const int nl = (int)Ls.size();
    RC(prof_mark(e, s, FAM_CONV_FWD));
    RC(launch_conv_fwd(s, p > 0 ? nq : 0, p == 0 ? e->afv : W.a[p], p == 0 ? in->numbers : nullptr, p > 0 ? W.q[p - 1] : nullptr,
                       W.nb_idx, W.nb_cnt, W.pg, P.layout.cap, e->agh_a, e->agh_q, e->bp, W.x[p], Ls[0].k_in, W.V[p], W.Vq[p], N,
                       order, p == 0 && e->p0_moments, e->split_max, sfmt));
    RC(prof_mark(e, s, FAM_GEMM));
    RC(mlp_sweep_fwd(e, s, sfmt, p, N, in->numbers, W.x[p], W.H[p], W.D[p], P.head_fused && p == np - 1, e->gemm_chain != 0));
    if (p == np - 1) break;
    RC(prof_mark(e, s, FAM_POINTWISE));
    // (the feature update a^{p+1} = a^p + delta_a rides on the NSE launch: independent work, one kernel boundary less)
    RC(launch_nse_fwd(s, W.H[p][nl - 1], Ls[nl - 1].k_out, nq, p > 0 ? W.q[p - 1] : nullptr, W.nl.mol_start, in->charge, n_mol, N,
                      W.S, (float*)W.part, W.q[p], W.Fm[p], W.Dm[p], p == 0 ? e->afv : W.a[p], p == 0 ? in->numbers : nullptr,
                      W.a[p + 1], dd));
    // domain decomposition: the final charges of halo copies are exact only within one cutoff of the owned region, the Coulomb
    // sums reach further - the owners' values come in through the exchange function
    if (dd && p == np - 2 && dd->fn(dd->ctx, AIMNET_DD_CHARGES, W.q[p], (int64_t)nq * N, (void*)s) != 0) {
      set_last_error("eval: the domain-decomposition exchange function failed (charges)");
      return AIMNET_E_INVALID;
    }
  }
  return 0;
}

// energy head: forward + backward in one launch (gemm_head.hip), or its GEMMs here and the last layer as `rider` of the SR-Coulomb
// launch (independent of the Coulomb block, so it shares that block's first launch - kernels.h, SrRiders)
int Eval::head(SrRiders& rider) {
  const int sfmt = P.layout.split_format, pm = P.layout.split_planes;
  const bool grad = P.grad;
  const int nlp = (int)e->mlp[np - 1].size();
  const float* hin = W.H[np - 1][nlp - 1];
  int ld_in = e->mlp[np - 1][nlp - 1].k_out;
  const int nh = (int)e->head.size();
  RC(prof_mark(e, s, FAM_GEMM));
  if (P.head_fused) {
    HeadFusedArgs ha{};
    ha.aim3 = reinterpret_cast<const unsigned short*>(hin);
    ha.lda3 = pm * ld_in;
    ha.fmt = sfmt;
    if (sfmt == SPLIT_H2) { ha.w1 = e->head[0].w2a; ha.w2 = e->head[1].w2a; ha.w2t = e->head[1].wt2a; ha.w1t = e->head[0].wt2a; }
    else { ha.w1 = e->head[0].w3a; ha.w2 = e->head[1].w3a; ha.w2t = e->head[1].wt3a; ha.w1t = e->head[0].wt3a; }
    ha.b1 = e->head[0].b; ha.b2 = e->head[1].b; ha.w3 = e->head_w_last; ha.b3 = e->head_b_last;
    ha.dlast = grad ? W.D[np - 1][nlp - 1] : nullptr;
    ha.ldd = ld_in;
    ha.e_atom = W.e_atom;
    ha.zbar3 = grad ? reinterpret_cast<unsigned short*>(W.zb0) : nullptr;
    ha.ldz3 = pm * ld_in;
    ha.M = N;
    ha.grad = grad ? 1 : 0;
    return launch_head_fused(s, ha);
  }
  for (int l = 0; l + 1 < nh; ++l) {
    const Layer& L = e->head[l];
    RC(mlp_gemm(e, s, EPI_BIAS_GELU, hin, ld_in, L, true, 0, 0, N, L.k_out, L.k_in, L.b, W.hH[l], W.hD[l], L.k_out));
    hin = W.hH[l];
    ld_in = L.k_out;
  }
  RC(prof_mark(e, s, FAM_POINTWISE));
  // with gradients: the rider also writes the backward seed d e / d z_{nh-2} = w_last * GELU'(z) into zb0
  rider.h = hin; rider.ldh = ld_in; rider.w = e->head_w_last; rider.b = e->head_b_last;
  rider.k = e->head[nh - 1].n_in; rider.e_atom = W.e_atom;
  rider.d = grad ? W.hD[nh - 2] : nullptr; rider.zbar = grad ? W.zb0 : nullptr;
  rider.n_head_blocks = ceil_div(N, 4);
  return 0;
}

// ---- Coulomb + DFT-D3: energies, and the seeds of qbar / dE/dx / virial ----
int Eval::coulomb(const SrRiders& head_rider) {
  const aimnet_arch& ar = e->arch;
  const int cap = P.layout.cap, cap_lr = P.layout.cap_lr;
  const bool grad = P.grad, want_s = P.want_s;
  if (nq == 2) RC(launch_charge_sum(s, W.q[np - 2], N, W.qtot, out->spin_charges));  // (aimnet2.py:102-106)
  CoulombParams cp = coulomb_params(ar, opt);
  const bool pme = P.lr_term == LongRange::PmeWalk;
  const bool ewald = P.lr_term == LongRange::EwaldWalk || pme;  // (the real-space walk and the self term are the same)
  if (pme) {  // per-system (alpha, rc, mesh) from the cell, fractional coordinates in double (pme.hip)
    RC(launch_pme_setup(s, in->cell, n_cell, W.nl.mol_start, in->charge, nq, n_mol, opt->ewald_accuracy, W.ew, out->status + 7));
    cp.ewald = W.ew.sys;
  } else if (ewald) {  // per-system (alpha, rc, kc) and k boxes from the cell, fractional coordinates in double (ewald.hip)
    RC(launch_ewald_setup(s, in->cell, n_cell, W.nl.mol_start, mol_c, W.nl.xw, in->charge, nq, N, n_mol, opt->ewald_accuracy, W.ew,
                          out->status + 7));
    cp.ewald = W.ew.sys;
  }
  const PairMapRider pmap = pair_map();
  SrRiders rd = head_rider;
  if (P.stream_rides) {  // the list-free walk runs below: its charge stream rides here
    rd.xs = W.nl.xs;
    rd.xq = (float4*)W.nl.sorted_tmp_xq;
    rd.charges_out = out->charges;
    rd.n_stream_blocks = ceil_div(N, 256);
  }
  if (P.lr_term == LongRange::SimpleInSr) {  // all pairs of the molecule: same waves
    rd.simple_xw = W.nl.xw;
    rd.simple_mol_idx = mol_c;
    rd.simple_mol_start = W.nl.mol_start;
  }
  rd.hash = pmap;  // hash build of the reverse-pair map (n_blocks = 0: none)
  if (P.sr_status_rides) {
    rd.cnt_true = W.nl.sorted_tmp;  // the row counts launch_nlist left (status_later)
    rd.status_cap = cap;
    rd.status_max = out->status + 0;
    rd.status_ovf = out->status + 2;
    rd.n_status_blocks = ceil_div(N, 1024);
    if (P.status == StatusZero::RiderOwned) {
      rd.n_status_blocks = 1;
      rd.status_all = out->status;
      rd.bad_part = W.bad_part;
      rd.keep7 = ewald ? 1 : 0;
    }
  }
  RC(launch_coulomb_sr(s, grad, want_s, ar.sr_coulomb != 0, q_fin, W.nb_idx, W.nb_cnt, W.pg, cap, cp, N, W.ecoul, W.qbar, W.fgrad,
                       W.virial_atom, &rd));
  switch (P.lr_term) {
    case LongRange::None:
    case LongRange::SimpleInSr:  // ran inside the SR-Coulomb launch above (SrRiders::simple_xw)
    case LongRange::DsfInD3:     // rides on the D3 pair pass below (one list, one geometry evaluation)
      break;
    case LongRange::SimpleMatrix:  // coul_simple over the caller's matrix (lr.py:311-331)
      RC(launch_coulomb_dsf(s, grad, false, q_fin, W.nl.xw, mol_c, in->cell, n_cell, W.lr_idx, W.lr_shift, W.lr_cnt, cap_lr, cp, N,
                            W.ecoul, W.qbar, W.fgrad, W.virial_atom, true));
      break;
    case LongRange::DsfMatrix:
      RC(launch_coulomb_dsf(s, grad, want_s, q_fin, W.nl.xw, mol_c, in->cell, n_cell, W.lr_idx, W.lr_shift, W.lr_cnt, cap_lr, cp, N,
                            W.ecoul, W.qbar, W.fgrad, W.virial_atom));
      break;
    case LongRange::DsfWalk:
    case LongRange::EwaldWalk:
    case LongRange::PmeWalk:  // the walk copies q to the `charges` output on its way
      RC(launch_coulomb_dsf_walk(s, grad, want_s, q_fin, mol_c, W.nl, cp, N, W.ecoul, W.qbar, W.fgrad, W.virial_atom, out->charges,
                                 true, P.rev_lookup == RevLookup::OnWalk ? &pmap : nullptr));
      if (pme)  // reciprocal space on the mesh + neutralising background (pme.hip)
        RC(launch_pme_recip(s, grad, want_s, W.nl.xw, q_fin, mol_c, W.nl.mol_start, order, N, n_mol, W.ew, cp.factor, W.ecoul,
                            W.qbar, W.fgrad, W.virial_atom));
      else if (ewald)  // reciprocal space + neutralising background, accumulated onto what the pair kernels have stored
        RC(launch_ewald_recip(s, grad, want_s, q_fin, mol_c, W.nl.mol_start, N, n_mol, W.ew, cp.factor, W.ecoul, W.qbar, W.fgrad,
                              W.virial_atom));
      break;
  }
  if (P.d3 != ListFrom::None)  // external DFT-D3: adds to the per-atom pair energies, dE/dx and the virial seeded by the Coulomb kernels
    RC(launch_dftd3(s, grad, want_s, W.nl.xw, mol_c, in->cell, n_cell, W.aslot, W.d3_idx, W.d3_shift, W.d3_cnt, P.cap_d3, e->d3,
                    d3_params(opt), opt->d3_cutoff, N, W.d3xs, W.d3w, W.dEdcn, W.ecoul, W.fgrad, W.virial_atom,
                    P.lr_term == LongRange::DsfInD3, cp, q_fin, W.qbar, P.d3_cn_rides, dd));
  if (e->emb_on) RC(embedding());  // one more addend to ecoul and to the seeds; in front of the copy of qbar: both channels take it
  if (grad && nq == 2) RC(launch_copy_f32(s, W.qbar, W.qbar + N, (size_t)N));  // dE/dq_alpha = dE/dq_beta = dE/dq at this point
  if (dd) {  // halo copies: no energy, no Coulomb adjoint / direct force, no backward seed (model.hip, dd_mask_kernel)
    const int nlp = (int)e->mlp[np - 1].size();
    const int seed_bytes = P.head_fused ? P.layout.split_planes * e->mlp[np - 1][nlp - 1].k_out * 2 : e->head[e->head.size() - 2].k_out * 4;
    RC(launch_dd_mask(s, dd->owned, in->numbers, e->sae, W.e_atom, W.ecoul, grad ? W.qbar : nullptr, nq, grad ? W.fgrad : nullptr,
                      want_s ? W.virial_atom : nullptr, grad ? W.zb0 : nullptr, seed_bytes, N));
  }
  return 0;
}

// electrostatic embedding (embed.hip): E_emb = sum_i q_i phi_i joins the pair energies, phi_i the adjoint dE/dq_i that the backward
// sweep carries to the coordinates, q_i grad phi_i the direct dE/dx_i.  The coordinates are the caller's (in->coord), the frame of
// the sites.  Energy-only requests run the same field and seed passes without the adjoint stores.
int Eval::embedding() {
  const aimnet_embedding& m = e->emb;
  EmbedBuffers b;
  embed_carve(b, (char*)m.scratch, N, n_mol, m.n_ext);
  if (e->emb_periodic_on && m.n_ext > 0) {  // armed: the sites are periodic with the cell - Ewald sums instead of the bare 1 / d
    const aimnet_embedding_periodic& mp = e->emb_periodic;
    EmbedPbcBuffers pb;
    embed_pbc_carve(pb, (char*)mp.scratch, N, n_mol, m.n_ext, mp.max_k);
    RC(launch_embed_sites(s, m.ext_mol_idx, m.n_ext, n_mol, b, out->status + 6));
    RC(launch_embed_pbc_field(s, in->coord, mol_c, W.nl.mol_start, N, n_mol, in->cell, n_cell, in->charge, nq, m.ext_coord,
                              m.ext_charge, m.n_ext, mp.accuracy, b, pb, mp.status));
    EmbedBuffers bp = b;  // the seed pass reads the periodic partials: the real-space slots, then the reciprocal-space slot
    bp.part = pb.part;
    RC(launch_embed_seed(s, P.grad, q_fin, N, m.n_ext, m.potential, m.potential_grad, bp, W.ecoul, W.qbar, W.fgrad, W.nl.mol_start,
                         n_mol, m.energy, 1));
    return launch_embed_pbc_site_pass(s, q_fin, W.nl.mol_start, N, n_mol, m.ext_charge, m.n_ext, b, pb, m.ext_forces,
                                      m.ext_potential);
  }
  RC(launch_embed_sites(s, m.ext_mol_idx, m.n_ext, n_mol, b, out->status + 6));
  RC(launch_embed_field(s, in->coord, mol_c, N, n_mol, m.ext_coord, m.ext_charge, m.n_ext, b));
  RC(launch_embed_seed(s, P.grad, q_fin, N, m.n_ext, m.potential, m.potential_grad, b, W.ecoul, W.qbar, W.fgrad, W.nl.mol_start,
                       n_mol, m.energy));
  return launch_embed_site_pass(s, in->coord, q_fin, W.nl.mol_start, n_mol, m.ext_coord, m.ext_charge, m.n_ext, b, m.ext_forces,
                                m.ext_potential);
}

// The results of the Coulomb block (ecoul, qbar / fgrad / virial seeds, qtot) are first needed here (energy only) or in front of
// the first conv backward.  The molecule energies are outputs only: where the plan lets their sums (and the copy of the charges)
// ride on the launches of finalize, nothing is launched here.
int Eval::join() {
  RC(prof_mark(e, s, FAM_POINTWISE));
  if (P.energy != EnergySum::OwnLaunch) return 0;
  const PairMapRider pmap = pair_map();
  return launch_energy_reduce(s, W.e_atom, W.ecoul, in->numbers, e->sae, W.nl.mol_start, n_mol, W.S, W.part, out->energy,
                              q_fin, P.charges == ChargesBy::EnergyLaunch ? out->charges : nullptr, N,  // + the charges output
                              P.rev_lookup == RevLookup::OnEnergyLaunch ? &pmap : nullptr,  // + the lookup of the reverse-pair map
                              out->status + 6);
}

// backward of the unfused energy head: zb0 holds the seed written by the head rider; leaves the adjoint of the last MLP's output in
// zcur, in the split form the MLP sweeps read (the fused head has left it in zb0 already)
int Eval::head_bwd(float*& zcur, float*& znext) {
  const int sfmt = P.layout.split_format;
  const int nh = (int)e->head.size();
  int ld = e->head[nh - 2].k_out;
  RC(prof_mark(e, s, FAM_GEMM));
  for (int l = nh - 2; l >= 0; --l) {
    const Layer& L = e->head[l];
    float* dprev = l > 0 ? W.hD[l - 1] : W.D[np - 1][e->mlp[np - 1].size() - 1];  // aim = GELU(z_last) of the last MLP
    RC(mlp_gemm(e, s, dprev ? EPI_MUL : EPI_NONE, zcur, ld, L, false, 0, 0, N, L.k_in, L.k_out, nullptr, znext, dprev, L.k_in));
    std::swap(zcur, znext);
    ld = L.k_in;
  }
  if (sfmt == SPLIT_NONE) return 0;
  // (the head runs on fp32 operands; its adjoint is split for the MLP backward)
  if (sfmt == SPLIT_H2) RC(launch_split_h2(s, zcur, ld, N, ld, reinterpret_cast<unsigned short*>(znext), 2 * ld, H2_ACT));
  else RC(launch_split_bf3(s, zcur, ld, N, ld, reinterpret_cast<unsigned short*>(znext), 3 * ld));
  std::swap(zcur, znext);
  return 0;
}

// NSE adjoint of pass p (the molecule sums of qbar . y, then the adjoint zbar of its MLP output into znext)
int Eval::nse_bwd(int p, float* znext) {
  const int sfmt = P.layout.split_format;
  const std::vector<Layer>& Lq = e->mlp[p];
  const int nlq = (int)Lq.size();
  const float* y = W.H[p][nlq - 1];
  const int ldy = Lq[nlq - 1].k_out;
  const float* dlast = e->arch.last_linear[p] ? nullptr : W.D[p][nlq - 1];
  RC(prof_mark(e, s, FAM_POINTWISE));
  switch (P.nse) {
    case NseAdjoint::Decomposed:  // domain decomposition: the adjoint sums run over every local atom and are all-reduced over the ranks
      RC(launch_nse_bwd_reduce(s, W.qbar, y, ldy, nq, W.nl.mol_start, n_mol, N, 1, (float*)W.part));
      if (dd->fn(dd->ctx, AIMNET_DD_SUM, W.part, (int64_t)nq * n_mol, (void*)s) != 0) {
        set_last_error("eval: the domain-decomposition exchange function failed (NSE adjoint sums)");
        return AIMNET_E_INVALID;
      }
      return launch_build_zbar(s, W.qbar, W.abar, y, ldy, dlast, W.Fm[p], W.Dm[p], (const float*)W.part, 1, mol_c, N, n_mol, 256, nq,
                               p > 0, znext, W.qbar, sfmt, nullptr, dd->owned);
    case NseAdjoint::Merged:  // small systems: the molecule sums inside build_zbar, one launch instead of two
      RC(launch_build_zbar(s, W.qbar, W.abar, y, ldy, dlast, W.Fm[p], W.Dm[p], nullptr, 1, mol_c, N, n_mol, 256, nq, p > 0, znext,
                           W.qbar2, sfmt, W.nl.mol_start));
      std::swap(W.qbar, W.qbar2);
      return 0;
    case NseAdjoint::Sliced:
      RC(launch_nse_bwd_reduce(s, W.qbar, y, ldy, nq, W.nl.mol_start, n_mol, N, W.S, (float*)W.part));
      return launch_build_zbar(s, W.qbar, W.abar, y, ldy, dlast, W.Fm[p], W.Dm[p], (const float*)W.part, W.S, mol_c, N, n_mol, 256,
                               nq, p > 0, znext, W.qbar, sfmt);
  }
  return 0;
}

int Eval::backward() {
  const int cap = P.layout.cap, sfmt = P.layout.split_format;
  const bool want_s = P.want_s, xe = P.layout.xe;
  float* zcur = W.zb0;
  float* znext = W.zb1;
  if (!P.head_fused) RC(head_bwd(zcur, znext));
  for (int p = np - 1; p >= 0; --p) {
    const bool p0m = p == 0 && P.p0_moments;
    const int ld = e->mlp[p][0].k_in;
    // zcur = adjoint of the last layer's pre-activation (GELU' already applied) -> zcur = xbar_p (N x k_in of the first layer;
    // pass-0 moments: only its conv columns 256.. are consumed - the embedding is a constant)
    RC(prof_mark(e, s, FAM_GEMM));
    RC(mlp_sweep_bwd(e, s, sfmt, p, N, p0m, zcur, znext, W.D[p], e->gemm_chain != 0));
    // the conv backward below is the first consumer of the Coulomb block's qbar / dE/dx / virial seeds
    if (p == np - 1) RC(join());
    RC(prof_mark(e, s, FAM_UNCONCAT));
    if (p0m) {
      RC(launch_unconcat_p0(s, zcur, ld, W.V[0], e->agh_a, e->afv, e->z_of_slot, e->nslots, W.present_part, W.n_part, W.Sbar, N));
      RC(prof_mark(e, s, FAM_CONV_BWD));
      RC(launch_conv_bwd_p0(s, want_s, W.Sbar, e->nslots, W.aslot, W.nb_idx, W.nb_cnt, W.pg, cap, e->bp, W.fgrad, W.virial_atom, N,
                            order, P.rev_hash ? W.pairbuf : nullptr));
      break;
    }
    RC(launch_unconcat(s, p > 0 ? nq : 0, zcur, ld, W.V[p], W.Vq[p], e->agh_a, e->agh_q, W.Sbar, W.Sqbar, N));
    RC(prof_mark(e, s, FAM_CONV_BWD));
    RC(launch_conv_bwd(s, p > 0 ? nq : 0, p > 0, want_s, p == 0 ? e->afv : W.a[p], p == 0 ? in->numbers : nullptr,
                       p > 0 ? W.q[p - 1] : nullptr, W.Sbar, W.Sqbar, W.nb_idx, W.nb_cnt, W.pg, cap, e->bp, zcur, ld,
                       (p < np - 1) ? W.abar : nullptr, W.abar, W.qbar, W.qbar, W.fgrad, W.virial_atom, N, order,
                       (xe && p > 0) ? W.pairbuf : nullptr, p < np - 1, e->split_max));
    if (p == 0) break;
    RC(nse_bwd(p - 1, znext));
    std::swap(zcur, znext);
  }
  return 0;
}

// forces, stress and whatever the plan deferred to these launches
int Eval::finalize() {
  const int cap = P.layout.cap;
  RC(prof_mark(e, s, FAM_POINTWISE));
  // reverse-pair form: the pair buffer holds F1 of both passes; its gather is the last contribution to dE/dx and writes the forces
  // (with a stress request the force gather rides on the launch of the virial sums: independent work, one kernel boundary less)
  const PairForceRider pfr{W.nb_idx, W.nb_cnt, W.rev, W.pairbuf, cap, out->forces, ceil_div(N, 4)};
  const EnergyRider erd{W.e_atom, W.ecoul, in->numbers, e->sae, W.part_e, out->energy, n_mol,
                        q_fin, P.charges == ChargesBy::ForceRider ? out->charges : nullptr, N};
  if (P.rev_hash && !P.pair_force_rides)
    RC(launch_pair_force(s, W.nb_idx, W.nb_cnt, W.rev, W.pairbuf, cap, N, W.fgrad, out->forces, out->status + 6));
  // (domain decomposition: no cell - the virial sums are divided by the volume of a unit cube, i.e. the `stress` output takes the
  // rank's share of dE/d(strain) itself; the caller adds the ranks' shares and divides by the cell volume)
  return launch_finalize(s, W.fgrad, W.virial_atom, W.nl.mol_start, dd ? e->unit_cell : in->cell, dd ? 1 : n_cell, n_mol, N,
                         W.S, W.part, (P.want_f && !P.layout.xe) ? out->forces : nullptr, P.want_s ? out->stress : nullptr,
                         P.pair_force_rides ? &pfr : nullptr, P.energy != EnergySum::OwnLaunch ? &erd : nullptr, e->sums_whole != 0,
                         out->status + 6);
}

// the plain values eval_plan.h works on
LayoutRequest layout_request(const aimnet_engine* e, int N, int n_mol, const aimnet_eval_options* opt) {
  LayoutRequest r{};
  r.N = N; r.n_mol = n_mol; r.n_pass = e->arch.n_pass;
  r.flags = opt->flags; r.coulomb = opt->coulomb; r.dftd3 = opt->dftd3;
  r.d3_same_cutoff = opt->d3_cutoff == opt->dsf_rc;
  r.max_nb = opt->max_nb; r.max_nb_lr = opt->max_nb_lr; r.max_nb_d3 = opt->max_nb_d3;
  r.ewald_max_k = opt->ewald_max_k; r.pme_max_mesh = opt->pme_max_mesh;
  r.ewald_kb = EWALD_KB; r.pme_part = PME_PART;
  r.conv_xe = e->conv_xe; r.split_max = e->split_max;
  r.pair_rev_ok = pair_rev_supported(N, std::max(1, opt->max_nb));
  r.split_format = split_format(e, N);
  r.split_planes = split_planes(r.split_format);
  return r;
}
EvalRequest eval_request(const aimnet_engine* e, const aimnet_inputs* in, const aimnet_eval_options* opt, const aimnet_outputs* out) {
  EvalRequest r{};
  const int N = in->n_atoms, n_mol = in->n_mol;
  r.L = layout_request(e, N, n_mol, opt);
  r.pbc = in->cell != nullptr;
  r.n_cell = in->n_cell; r.nq = e->nq;
  r.has_stress_out = out->stress != nullptr; r.has_forces_out = out->forces != nullptr; r.has_spin_out = out->spin_charges != nullptr;
  r.ewald_args = (opt->coulomb == AIMNET_COULOMB_EWALD || opt->coulomb == AIMNET_COULOMB_PME) ? ewald_args_check(in, opt) : 0;
  r.nbmat = in->nbmat != nullptr; r.shifts = in->shifts != nullptr;
  r.nbmat_lr = in->nbmat_lr != nullptr; r.shifts_lr = in->shifts_lr != nullptr;
  r.nbmat_d3 = in->nbmat_d3 != nullptr; r.shifts_d3 = in->shifts_d3 != nullptr;
  r.nbmat_width = in->nbmat_width; r.nbmat_lr_width = in->nbmat_lr_width; r.nbmat_d3_width = in->nbmat_d3_width;
  r.dd = e->dd.owned != nullptr;
  r.d3_tables = e->d3.ns != 0;
  r.prep_fused = e->prep_fused; r.energy_rides = e->energy_rides; r.status_rides = e->status_rides; r.setup_rides = e->setup_rides;
  r.status_owned = e->status_owned; r.nse_merged = e->nse_merged; r.d3_cn_rides = e->d3_cn_rides; r.dsf_np_walk = e->dsf_np_walk;
  r.p0_moments = e->p0_moments; r.spatial_order = e->spatial_order;
  r.prep_small_ok = prep_small_applies(N, n_mol, r.pbc);
  r.cell_setup_ok = cell_setup_rides(N, n_mol);
  r.bbox_ok = bbox_applies(N, n_mol);
  r.head_fusable = head_fusable(e);
  if (e->emb_on) {
    const aimnet_embedding& m = e->emb;
    r.emb = 1;
    r.emb_n_ext = m.n_ext;
    r.emb_sites_ok = m.n_ext <= 0 || (m.ext_coord && m.ext_charge);
    r.emb_ext_mol_idx = m.ext_mol_idx != nullptr;
    r.emb_potential = m.potential != nullptr;
    r.emb_potential_grad = m.potential_grad != nullptr;
    r.emb_scratch_ok = m.scratch && m.n_ext >= 0 && m.scratch_bytes >= aimnet_embedding_scratch_bytes(N, n_mol, m.n_ext);
    if (e->emb_periodic_on) {
      const aimnet_embedding_periodic& mp = e->emb_periodic;
      r.emb_periodic = 1;
      r.emb_pbc_full = !in->pbc_sys && in->pbc[0] && in->pbc[1] && in->pbc[2];
      r.emb_periodic_accuracy = mp.accuracy;
      r.emb_periodic_max_k = mp.max_k;
      r.emb_periodic_status = mp.status != nullptr;
      r.emb_periodic_scratch_ok = mp.scratch && m.n_ext >= 0 && mp.max_k > 0 &&
                                  mp.scratch_bytes >= aimnet_embedding_periodic_scratch_bytes(N, n_mol, m.n_ext, mp.max_k);
    }
  }
  return r;
}

}  // namespace

// ================================================================================================
extern "C" {

int aimnet_abi_version(void) { return AIMNET_ABI_VERSION; }

const char* aimnet_last_error(void) { return g_err; }

int aimnet_engine_create(const aimnet_arch* arch, const aimnet_weights* w, int device, aimnet_engine** out) {
  if (!arch || !w || !out) return AIMNET_E_INVALID;
  if (arch->nfeature != 16 || arch->nshifts != 16 || arch->ncomb_v != 12) {
    set_last_error("unsupported architecture: kernels are specialised for nfeature=16, nshifts=16, ncomb_v=12 (got %d,%d,%d)",
                   arch->nfeature, arch->nshifts, arch->ncomb_v);
    return AIMNET_E_INVALID;
  }
  if (arch->n_pass < 2 || arch->n_pass > AIMNET_MAX_PASS || arch->head_n_layers < 2 || arch->head_n_layers > AIMNET_MAX_LAYERS) {
    set_last_error("unsupported architecture: n_pass=%d head layers=%d", arch->n_pass, arch->head_n_layers);
    return AIMNET_E_INVALID;
  }
  if (arch->n_charge_channels < 0 || arch->n_charge_channels > 2) {
    set_last_error("unsupported architecture: n_charge_channels=%d (1 closed shell, 2 NSE)", arch->n_charge_channels);
    return AIMNET_E_INVALID;
  }
  AIMNET_HIP_CHECK(hipSetDevice(device));
  aimnet_engine* e = new aimnet_engine();
  e->arch = *arch;
  e->nq = std::max(1, arch->n_charge_channels);
  e->device = device;
  int rc = 0;
  const int AG = 256;
  if ((rc = dev_upload(e, w->afv, (size_t)64 * AG, &e->afv))) goto fail;
  {
    int soz[64], zos[64];
    int ns = 0, bad_row = -1;
    for (int z = 0; z < 64; ++z) {
      bool ok = true;
      for (int k = 0; k < AG; ++k) ok = ok && std::isfinite(w->afv[(size_t)z * AG + k]);
      if (ok) { soz[z] = ns; zos[ns++] = z; } else { soz[z] = -1; if (bad_row < 0) bad_row = z; }
    }
    if (bad_row >= 0) {
      for (int z = 0; z < 64; ++z) if (soz[z] < 0) soz[z] = ns;
      zos[ns++] = bad_row;
    }
    e->nslots = ns;
    e->z_of_slot_h.assign(zos, zos + ns);
    if ((rc = dev_upload(e, soz, (size_t)64, &e->slot_of_z))) goto fail;
    if ((rc = dev_upload(e, zos, (size_t)ns, &e->z_of_slot))) goto fail;
    apply_env_options(e);
  }
  if ((rc = dev_upload(e, w->agh_a, (size_t)16 * 16 * 12, &e->agh_a))) goto fail;
  if ((rc = dev_upload(e, w->agh_q, (size_t)e->nq * 16 * 12, &e->agh_q))) goto fail;
  if ((rc = dev_upload(e, w->sae, (size_t)64, &e->sae))) goto fail;
  for (int p = 0; p < arch->n_pass; ++p) {
    const int nl = arch->n_layers[p];
    if (nl < 1 || nl > AIMNET_MAX_LAYERS) { rc = AIMNET_E_INVALID; set_last_error("bad n_layers[%d]=%d", p, nl); goto fail; }
    const int n_in_expect = (p == 0) ? 704 : 704 + 29 * e->nq;  // [a | conv_a] (+ [q | conv_q] per charge channel)
    const int n_out_expect = (p < arch->n_pass - 1) ? 256 + 2 * e->nq : arch->layer_dims[p][nl];
    if (arch->layer_dims[p][0] != n_in_expect || arch->layer_dims[p][nl] != n_out_expect) {
      rc = AIMNET_E_INVALID;
      set_last_error("pass %d MLP dims %d->%d do not match the feature layout (%d->%d)", p, arch->layer_dims[p][0],
                     arch->layer_dims[p][nl], n_in_expect, n_out_expect);
      goto fail;
    }
    for (int l = 0; l < nl; ++l) {
      Layer L;
      if ((rc = upload_layer(e, w->mlp_w[p][l], w->mlp_b[p][l], arch->layer_dims[p][l], arch->layer_dims[p][l + 1], &L,
                             (p == 0 && l == 0 && arch->layer_dims[p][l] >= AG) ? AG : 0)))
        goto fail;
      e->mlp[p].push_back(L);
      if (p == 0 && l == 0 && L.n_in >= AG) {  // the embedding block of the first layer as a per-element bias table
        std::vector<float> tab((size_t)64 * L.k_out, 0.0f);
        for (int z = 0; z < 64; ++z)
          for (int o = 0; o < L.n_out; ++o) {
            double acc = (double)w->mlp_b[p][l][o];
            for (int k = 0; k < AG; ++k) acc += (double)w->mlp_w[p][l][(size_t)o * L.n_in + k] * (double)w->afv[(size_t)z * AG + k];
            tab[(size_t)z * L.k_out + o] = (float)acc;
          }
        if ((rc = dev_upload(e, tab.data(), tab.size(), &e->emb_bias0))) goto fail;
      }
    }
  }
  if (arch->head_dims[0] != arch->layer_dims[arch->n_pass - 1][arch->n_layers[arch->n_pass - 1]] ||
      arch->head_dims[arch->head_n_layers] != 1) {
    rc = AIMNET_E_INVALID;
    set_last_error("energy head dims do not chain from the last MLP / do not end in 1");
    goto fail;
  }
  for (int l = 0; l + 1 < arch->head_n_layers; ++l) {
    Layer L;
    if ((rc = upload_layer(e, w->head_w[l], w->head_b[l], arch->head_dims[l], arch->head_dims[l + 1], &L))) goto fail;
    e->head.push_back(L);
  }
  {
    const int l = arch->head_n_layers - 1;
    Layer L{};  // vector form of the final (k -> 1) layer
    L.n_in = arch->head_dims[l];
    L.n_out = 1;
    L.k_in = pad32(L.n_in);
    L.k_out = 1;
    e->head.push_back(L);
    if ((rc = dev_upload(e, w->head_w[l], (size_t)L.n_in, &e->head_w_last))) goto fail;
    if ((rc = dev_upload(e, w->head_b[l], (size_t)1, &e->head_b_last))) goto fail;
    {
      static const float unit[9] = {1.f, 0.f, 0.f, 0.f, 1.f, 0.f, 0.f, 0.f, 1.f};
      if ((rc = dev_upload(e, unit, (size_t)9, &e->unit_cell))) goto fail;
    }
  }
  if (e->h2_fits) {  // one-launch MLP sweeps (gemm_chain.hip) where the layer sizes match an instantiated shape
    for (int p = 0; p < arch->n_pass; ++p) {
      if ((rc = chain_plan_fwd(e, e->mlp[p], 0, &e->chain_fwd[p][0]))) goto fail;
      if ((rc = chain_plan_bwd(e, e->mlp[p], 0, &e->chain_bwd[p][0]))) goto fail;
      if (p == 0 && e->emb_bias0 && (rc = chain_plan_fwd(e, e->mlp[p], AG, &e->chain_fwd[p][1]))) goto fail;
      if (p == 0 && (rc = chain_plan_bwd(e, e->mlp[p], AG, &e->chain_bwd[p][1]))) goto fail;
    }
  }
  for (int p = 0; p < arch->n_pass; ++p)
    for (Layer& L : e->mlp[p]) {
      std::vector<unsigned short>().swap(L.h_w2a);
      std::vector<unsigned short>().swap(L.h_wt2a);
    }
  for (Layer& L : e->head) {
    std::vector<unsigned short>().swap(L.h_w2a);
    std::vector<unsigned short>().swap(L.h_wt2a);
  }
  e->bp.rc = arch->rc;
  e->bp.eta = arch->eta;
  for (int g = 0; g < 16; ++g) e->bp.shifts[g] = arch->shifts[g];
  if ((rc = gemm_set_attributes())) goto fail;
  if ((rc = gemm_bf3_set_attributes())) goto fail;
  if ((rc = gemm_split_set_attributes())) goto fail;  // AIMNET_BF3A_TILE / AIMNET_H2_TILE / AIMNET_H2_DEEP (gemm_h2.hip)
  *out = e;
  return AIMNET_OK;
fail:
  aimnet_engine_destroy(e);
  return rc;
}

void aimnet_engine_destroy(aimnet_engine* e) {
  if (!e) return;
  for (void* p : e->allocs) (void)hipFree(p);
  for (hipEvent_t ev : e->prof_ev) (void)hipEventDestroy(ev);
  delete e;
}

int aimnet_engine_set_profiling(aimnet_engine* e, int level) {
  if (!e || level < 0 || level > 2) return AIMNET_E_INVALID;
  e->prof_level = level;
  e->prof_used = 0;
  e->prof_last = -2;
  e->prof_evals = e->prof_sampled = 0;
  return AIMNET_OK;
}

int aimnet_engine_set_profile_sampling(aimnet_engine* e, int every) {
  if (!e || every < 1) return AIMNET_E_INVALID;
  e->prof_every = every;
  return AIMNET_OK;
}

int aimnet_engine_profile_read(aimnet_engine* e, double* ms, int n_families, int reset) {
  if (!e || !ms || n_families < FAM_COUNT) return AIMNET_E_INVALID;
  for (int k = 0; k < n_families; ++k) ms[k] = 0.0;
  if (e->prof_used > 0) AIMNET_HIP_CHECK(hipEventSynchronize(e->prof_ev[e->prof_used - 1]));
  for (size_t k = 0; k + 1 < e->prof_used; ++k) {
    const int fam = e->prof_fam[k];
    if (fam < 0) continue;  // gap between two evals
    float t = 0.f;
    AIMNET_HIP_CHECK(hipEventElapsedTime(&t, e->prof_ev[k], e->prof_ev[k + 1]));
    ms[fam] += (double)t;
  }
  if (n_families > FAM_COUNT) ms[FAM_COUNT] = (double)e->prof_sampled;  // evaluations the sums above cover
  if (reset) {
    e->prof_used = 0;
    e->prof_last = -2;
    e->prof_evals = e->prof_sampled = 0;
  }
  return AIMNET_OK;
}

int aimnet_engine_set_option(aimnet_engine* e, const char* name, int value) {
  if (!e || !name) return AIMNET_E_INVALID;
  const OptionRow* r = find_option(name);
  if (!r) {
    set_last_error("set_option: unknown option '%s'", name);
    return AIMNET_E_INVALID;
  }
  if (r->kind == OPT_RETIRED) {
    if (value == 0) return AIMNET_OK;
    set_last_error("%s was removed (%s)", r->name, r->env);
    return AIMNET_E_INVALID;
  }
  e->*r->field = option_value(*r, value);
  return AIMNET_OK;
}

int aimnet_engine_get_option(const aimnet_engine* e, const char* name, int* value) {
  if (!e || !name || !value) return AIMNET_E_INVALID;
  const OptionRow* r = find_option(name);
  if (!r) {
    set_last_error("get_option: unknown option '%s'", name);
    return AIMNET_E_INVALID;
  }
  *value = r->kind == OPT_RETIRED ? 0 : e->*r->field;
  if (r->field == &aimnet_engine::gemm_h2) *value = e->gemm_h2 && e->h2_fits;  // what eval() runs (split_format)
  return AIMNET_OK;
}

int aimnet_engine_set_dd(aimnet_engine* e, const float* owned, aimnet_dd_exchange_fn fn, void* ctx) {
  if (!e || (owned && !fn)) {
    set_last_error("set_dd: an owned-atom mask needs an exchange function");
    return AIMNET_E_INVALID;
  }
  e->dd = aimnet::DdLink{owned, owned ? fn : nullptr, owned ? ctx : nullptr};
  return AIMNET_OK;
}

size_t aimnet_embedding_scratch_bytes(int32_t n_atoms, int32_t n_mol, int32_t n_ext) {
  if (n_atoms <= 0 || n_mol <= 0 || n_ext < 0) return 0;
  aimnet::EmbedBuffers b;
  aimnet::embed_carve(b, nullptr, n_atoms, n_mol, n_ext);
  return b.total;
}

int aimnet_engine_set_embedding(aimnet_engine* e, const aimnet_embedding* emb) {
  if (!e) return AIMNET_E_INVALID;
  e->emb_tangent_on = false;  // a new embedding, or none, starts unarmed (aimnet_engine_set_embedding_tangent)
  e->emb_tangent = aimnet_embedding_tangent{};
  e->emb_periodic_on = false;  // (likewise: aimnet_engine_set_embedding_periodic)
  e->emb_periodic = aimnet_embedding_periodic{};
  if (!emb) {
    e->emb_on = false;
    e->emb = aimnet_embedding{};
    return AIMNET_OK;
  }
  if (emb->n_ext < 0 || (emb->n_ext > 0 && (!emb->ext_coord || !emb->ext_charge))) {
    set_last_error("set_embedding: n_ext >= 0, and n_ext > 0 needs ext_coord and ext_charge");
    return AIMNET_E_INVALID;
  }
  if (!emb->scratch) {
    set_last_error("set_embedding: scratch is required (aimnet_embedding_scratch_bytes)");
    return AIMNET_E_INVALID;
  }
  e->emb = *emb;  // (checked against the problem size by every evaluation, eval_plan.h)
  e->emb_on = true;
  return AIMNET_OK;
}

size_t aimnet_embedding_tangent_scratch_bytes(int32_t n_atoms, int32_t n_mol, int32_t n_ext) {
  if (n_atoms <= 0 || n_mol <= 0 || n_ext < 0) return 0;
  aimnet::EmbedBuffers b;
  aimnet::embed_carve(b, nullptr, n_atoms, n_mol, n_ext, true);
  return b.total;
}

int aimnet_engine_set_embedding_tangent(aimnet_engine* e, const aimnet_embedding_tangent* t) {
  if (!e) return AIMNET_E_INVALID;
  if (!t) {
    e->emb_tangent_on = false;
    e->emb_tangent = aimnet_embedding_tangent{};
    return AIMNET_OK;
  }
  if (!e->emb_on) {
    set_last_error("set_embedding_tangent: no embedding is set (aimnet_engine_set_embedding first)");
    return AIMNET_E_INVALID;
  }
  if (!t->scratch) {
    set_last_error("set_embedding_tangent: scratch is required (aimnet_embedding_tangent_scratch_bytes)");
    return AIMNET_E_INVALID;
  }
  e->emb_tangent = *t;  // (checked against the problem size by every aimnet_engine_hvp call, tangent_plan.h)
  e->emb_tangent_on = true;
  return AIMNET_OK;
}

size_t aimnet_embedding_periodic_scratch_bytes(int32_t n_atoms, int32_t n_mol, int32_t n_ext, int32_t max_k) {
  if (n_atoms <= 0 || n_mol <= 0 || n_ext < 0 || max_k <= 0) return 0;
  aimnet::EmbedPbcBuffers b;
  aimnet::embed_pbc_carve(b, nullptr, n_atoms, n_mol, n_ext, max_k);
  return b.total;
}

int aimnet_engine_set_embedding_periodic(aimnet_engine* e, const aimnet_embedding_periodic* p) {
  if (!e) return AIMNET_E_INVALID;
  if (!p) {
    e->emb_periodic_on = false;
    e->emb_periodic = aimnet_embedding_periodic{};
    return AIMNET_OK;
  }
  if (!e->emb_on) {
    set_last_error("set_embedding_periodic: no embedding is set (aimnet_engine_set_embedding first)");
    return AIMNET_E_INVALID;
  }
  if (!p->scratch) {
    set_last_error("set_embedding_periodic: scratch is required (aimnet_embedding_periodic_scratch_bytes)");
    return AIMNET_E_INVALID;
  }
  e->emb_periodic = *p;  // (checked against the problem size by every aimnet_engine_eval call, eval_plan.h)
  e->emb_periodic_on = true;
  return AIMNET_OK;
}

int aimnet_engine_set_pme_tangent(aimnet_engine* e, int32_t on) {
  if (!e) return AIMNET_E_INVALID;
  e->pme_tangent_on = on != 0;
  return AIMNET_OK;
}

int aimnet_engine_set_dftd3_tangent(aimnet_engine* e, int32_t on) {
  if (!e) return AIMNET_E_INVALID;
  e->d3_tangent_on = on != 0;
  return AIMNET_OK;
}

int aimnet_engine_set_dftd3(aimnet_engine* e, const aimnet_dftd3_tables* t) {
  if (!e || !t || t->n_z <= 0 || !t->c6ab || !t->cn_ref || !t->rcov || !t->r4r2) {
    set_last_error("set_dftd3: null argument");
    return AIMNET_E_INVALID;
  }
  AIMNET_HIP_CHECK(hipSetDevice(e->device));
  const int ns = e->nslots, nz = t->n_z;
  auto at = [&](const float* tab, int zi, int zj, int a, int b) { return tab[(((size_t)zi * nz + zj) * 5 + a) * 5 + b]; };
  std::vector<float> c6((size_t)ns * ns * 25, 0.0f), cnref((size_t)ns * 5, 0.0f), rcov(ns, 0.0f), r4r2(ns, 0.0f);
  std::vector<int> nref(ns, 0);
  for (int si = 0; si < ns; ++si) {
    const int zi = e->z_of_slot_h[si];
    if (zi >= nz || zi <= 0) continue;  // outside the table: all-zero rows (no dispersion for that slot)
    rcov[si] = t->rcov[zi];
    r4r2[si] = t->r4r2[zi];
    int n = 0;
    while (n < 5 && at(t->c6ab, zi, zi, n, n) != 0.0f) ++n;
    nref[si] = n;
    for (int a = 0; a < n; ++a) cnref[(size_t)si * 5 + a] = at(t->cn_ref, zi, zi, a, 0);
  }
  for (int si = 0; si < ns; ++si)
    for (int sj = 0; sj < ns; ++sj) {
      const int zi = e->z_of_slot_h[si], zj = e->z_of_slot_h[sj];
      if (zi >= nz || zj >= nz || zi <= 0 || zj <= 0) continue;
      for (int a = 0; a < 5; ++a)
        for (int b = 0; b < 5; ++b) {
          const float v = at(t->c6ab, zi, zj, a, b);
          const bool expect = a < nref[si] && b < nref[sj];
          if ((v != 0.0f) != expect || (expect && at(t->cn_ref, zi, zj, a, b) != cnref[(size_t)si * 5 + a])) {
            set_last_error("set_dftd3: the C6/CN table of Z = %d, %d does not factorise (ref %d, %d)", zi, zj, a, b);
            return AIMNET_E_INVALID;
          }
          c6[(((size_t)si * ns + sj) * 5 + a) * 5 + b] = v;
        }
    }
  int rc;
  float *d_c6, *d_cn, *d_rc, *d_r4;
  int* d_nr;
  if ((rc = dev_upload(e, c6.data(), c6.size(), &d_c6))) return rc;
  if ((rc = dev_upload(e, cnref.data(), cnref.size(), &d_cn))) return rc;
  if ((rc = dev_upload(e, nref.data(), nref.size(), &d_nr))) return rc;
  if ((rc = dev_upload(e, rcov.data(), rcov.size(), &d_rc))) return rc;
  if ((rc = dev_upload(e, r4r2.data(), r4r2.size(), &d_r4))) return rc;
  e->d3 = D3Tables{ns, d_c6, d_cn, d_nr, d_rc, d_r4};
  return AIMNET_OK;
}

size_t aimnet_engine_workspace_bytes(const aimnet_engine* e, int32_t n_atoms, int32_t n_mol, int32_t n_cell,
                                     const aimnet_eval_options* opt) {
  (void)n_cell;
  if (!e || !opt || n_atoms <= 0 || n_mol <= 0) return 0;
  Workspace W;
  layout(e, n_atoms, n_mol, opt, layout_plan(layout_request(e, n_atoms, n_mol, opt)), nullptr, W, nullptr);
  return W.total;
}

int aimnet_engine_debug_view(const aimnet_engine* e, const char* name, size_t* byte_offset, size_t* n_elem,
                             int32_t* elem_size, int32_t* row_stride) {
  if (!e || !name) return AIMNET_E_INVALID;
  auto it = e->views.find(name);
  if (it == e->views.end()) return AIMNET_E_INVALID;
  if (byte_offset) *byte_offset = it->second.off;
  if (n_elem) *n_elem = it->second.n_elem;
  if (elem_size) *elem_size = it->second.elem_size;
  if (row_stride) *row_stride = it->second.row_stride;
  return AIMNET_OK;
}

int aimnet_engine_eval(aimnet_engine* e, const aimnet_inputs* in, const aimnet_eval_options* opt,
                       const aimnet_outputs* out, void* workspace, size_t workspace_bytes, void* hip_stream) {
  if (!e || !in || !opt || !out || !workspace) return AIMNET_E_INVALID;
  const int N = in->n_atoms, n_mol = in->n_mol;
  if (N <= 0 || n_mol <= 0 || !in->coord || !in->numbers || !in->mol_idx || !in->charge || !out->energy ||
      !out->charges || !out->status) {
    set_last_error("eval: null or empty input/output");
    return AIMNET_E_INVALID;
  }
  // validate, plan, lay out
  const EvalRequest rq = eval_request(e, in, opt, out);
  RC(eval_validate(rq, g_err, sizeof(g_err)));
  const EvalPlan P = eval_plan(rq);
  hipStream_t s = (hipStream_t)hip_stream;
  AIMNET_HIP_CHECK(hipSetDevice(e->device));
  Workspace W;
  e->views.clear();
  layout(e, N, n_mol, opt, P.layout, (char*)workspace, W, &e->views);
  if (W.total > workspace_bytes) {
    set_last_error("eval: workspace too small (%zu < %zu)", workspace_bytes, W.total);
    return AIMNET_E_WORKSPACE;
  }
  RC(eval_validate_lists(rq, P.layout, g_err, sizeof(g_err)));
  const int np = e->arch.n_pass;
  Eval ev{e, s, in, opt, out, W, P, N, n_mol, rq.pbc ? in->n_cell : 0, np, e->nq, rq.pbc, rq.dd ? &e->dd : nullptr,
          W.nl.mol_c, P.bin_order ? W.nl.sorted : nullptr, e->nq == 2 ? W.qtot : W.q[np - 2]};

  e->prof_on = e->prof_level > 0 && (e->prof_evals++ % e->prof_every) == 0;
  if (e->prof_on) e->prof_sampled++;
  RC(prof_mark(e, s, FAM_NLIST));
  RC(ev.prepare());
  RC(P.ext ? ev.lists_imported() : ev.lists_built());
  RC(prof_mark(e, s, FAM_GEOM));
  RC(ev.forward());
  SrRiders head_rider{};  // the last energy-head layer, unless the head is fused
  RC(ev.head(head_rider));
  RC(prof_mark(e, s, FAM_COULOMB));
  RC(ev.coulomb(head_rider));
  if (P.grad) {
    RC(ev.backward());  // (runs join() in front of its first conv backward)
    RC(ev.finalize());
  } else {
    RC(ev.join());
  }
  RC(prof_mark(e, s, -1));
  return AIMNET_OK;
}

// ---- stand-alone entry points --------------------------------------------------------------------
size_t aimnet_neighbor_list_workspace_bytes(int32_t n_atoms, int32_t n_mol, int32_t max_nb) {
  if (n_atoms <= 0 || n_mol <= 0 || max_nb <= 0) return 0;
  return align_up(nlist_scratch_bytes(n_atoms, n_mol), 256) + align_up((size_t)n_atoms * (size_t)max_nb * sizeof(int), 256);
}

__global__ void expand_shifts_kernel(const int* __restrict__ code, size_t n, int* __restrict__ out) {
  const size_t e = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (e >= n) return;
  int sx, sy, sz;
  unpack_shift(code[e], sx, sy, sz);
  out[3 * e] = sx;
  out[3 * e + 1] = sy;
  out[3 * e + 2] = sz;
}

int aimnet_neighbor_list(const float* coord, const int32_t* mol_idx, int32_t n_atoms, int32_t n_mol,
                         const float* cell, int32_t n_cell, const int32_t pbc[3], float cutoff, int32_t max_nb,
                         int32_t fill_value, int32_t* nbmat, int32_t* shifts, int32_t* num_nb, int32_t* status,
                         float* coord_wrapped, void* workspace, size_t workspace_bytes, void* hip_stream) {
  if (!coord || !mol_idx || !nbmat || !num_nb || !status || !workspace || n_atoms <= 0 || n_mol <= 0 || max_nb <= 0)
    return AIMNET_E_INVALID;
  if (cell && !shifts) {
    set_last_error("neighbor_list: periodic input needs a shifts buffer");
    return AIMNET_E_INVALID;
  }
  if (cell && !(n_cell == 1 || n_cell == n_mol)) {
    set_last_error("neighbor_list: n_cell must be 1 or n_mol");
    return AIMNET_E_INVALID;
  }
  const size_t need = aimnet_neighbor_list_workspace_bytes(n_atoms, n_mol, max_nb);
  if (workspace_bytes < need) {
    set_last_error("neighbor_list: workspace too small (%zu < %zu)", workspace_bytes, need);
    return AIMNET_E_WORKSPACE;
  }
  hipStream_t s = (hipStream_t)hip_stream;
  NlistBuffers nl;
  nlist_carve(nl, (char*)workspace, n_atoms, n_mol);
  int* codes = (int*)((char*)workspace + align_up(nlist_scratch_bytes(n_atoms, n_mol), 256));
  const int pz[3] = {1, 1, 1};
  const int* pb = pbc ? pbc : pz;
  AIMNET_HIP_CHECK(hipMemsetAsync(status, 0, 2 * sizeof(int), s));
  RC(launch_mol_start(s, mol_idx, n_atoms, n_mol, nl.mol_start, nl.mol_c));
  mol_idx = nl.mol_c;  // clamped to [0, n_mol)
  RC(launch_wrap(s, coord, mol_idx, n_atoms, n_mol, cell, cell ? n_cell : 0, pb, nl));
  if (!cell && bbox_applies(n_atoms, n_mol)) RC(launch_bbox(s, n_mol, nl));
  RC(launch_nlist(s, n_atoms, n_mol, mol_idx, cell, cell ? n_cell : 0, pb, cutoff, cutoff, max_nb, fill_value, 1, nl, nbmat,
                  codes, num_nb, status + 0, status + 1));
  if (cell) {
    const size_t n_pairs = (size_t)n_atoms * max_nb;
    hipLaunchKernelGGL(expand_shifts_kernel, dim3((unsigned)((n_pairs + 255) / 256)), dim3(256), 0, s, codes, n_pairs, shifts);
    AIMNET_LAUNCH_CHECK();
  }
  if (coord_wrapped)
    AIMNET_HIP_CHECK(hipMemcpyAsync(coord_wrapped, nl.xw, (size_t)n_atoms * 3 * sizeof(float), hipMemcpyDeviceToDevice, s));
  return AIMNET_OK;
}

int aimnet_debug_gemm(int cfg, int epi, const float* A, int lda, const float* Bt, int ldb, int M, int N, int K,
                      const float* bias, float* C, float* D, int ldc, void* hip_stream) {
  static bool attr = false;
  if (!attr) {
    int rc = gemm_set_attributes();
    if (rc) return rc;
    attr = true;
  }
  return launch_gemm_nt_cfg((hipStream_t)hip_stream, cfg, epi, A, lda, Bt, ldb, M, N, K, bias, C, D, ldc);
}

int aimnet_debug_split_bf3(const float* src, int ld, int M, int K, void* dst, int ldd, int neg_from_block, void* hip_stream) {
  if (!src || !dst || M <= 0 || K <= 0 || ldd < 3 * pad32(K) || ldd % 96 || (neg_from_block < 0 && neg_from_block != aimnet::BF3_ALT))
    return AIMNET_E_INVALID;
  return launch_split_bf3((hipStream_t)hip_stream, src, ld, M, K, (unsigned short*)dst, ldd, neg_from_block);
}

int aimnet_debug_gemm_bf3(int cfg, int epi, const float* A, int lda, const void* Bt3, int ldb, int M, int N, int K,
                          const float* bias, float* C, float* D, int ldc, int kneg, void* hip_stream) {
  static bool attr = false;
  if (!attr) {
    int rc = gemm_bf3_set_attributes();
    if (rc) return rc;
    attr = true;
  }
  return launch_gemm_bf3_cfg((hipStream_t)hip_stream, cfg, epi, A, lda, (const unsigned short*)Bt3, ldb, M, N, K, bias, C, D, ldc,
                             nullptr, 0, kneg < 0 ? BF3_NO_NEG : kneg);
}

// the two split formats' debug entry points: one launcher (gemm_split.h)
static int debug_gemm_split(int fmt, int cfg, int epi, int out, const void* A3, int lda3, const void* Bt, int ldb, int M, int N, int K,
                            const float* bias, float* C, void* C3, int ldc3, float* D, int ldc, int alt, void* hip_stream) {
  using namespace aimnet;
  if (alt < 0 || alt > 2) return AIMNET_E_INVALID;
  static bool once = false;
  if (!once) {
    int rc = gemm_split_set_attributes();
    if (rc) return rc;
    once = true;
  }
  return launch_gemm_split_cfg((hipStream_t)hip_stream, fmt, cfg, epi, out != 0,
                               SplitArgs{(const unsigned short*)A3, lda3, (const unsigned short*)Bt, ldb, M, N, K, bias, C,
                                         (unsigned short*)C3, ldc3, D, ldc, nullptr, 0, alt});
}
int aimnet_debug_gemm_bf3a(int cfg, int epi, int out3, const void* A3, int lda3, const void* Bt3, int ldb, int M, int N, int K,
                           const float* bias, float* C, void* C3, int ldc3, float* D, int ldc, int alt, void* hip_stream) {
  return debug_gemm_split(aimnet::SPLIT_BF3, cfg, epi, out3, A3, lda3, Bt3, ldb, M, N, K, bias, C, C3, ldc3, D, ldc, alt, hip_stream);
}
int aimnet_debug_split_h2(const float* src, int ld, int M, int K, void* dst, int ldd, int mode, void* hip_stream) {
  if (!src || !dst || M <= 0 || K <= 0 || ldd < 2 * pad32(K) || ldd % 64 || mode < 0 || mode > 2) return AIMNET_E_INVALID;
  return aimnet::launch_split_h2((hipStream_t)hip_stream, src, ld, M, K, (unsigned short*)dst, ldd, mode);
}

int aimnet_debug_gemm_h2(int cfg, int epi, int out2, const void* A2, int lda2, const void* Bt2, int ldb, int M, int N, int K,
                         const float* bias, float* C, void* C2, int ldc2, float* D, int ldc, int alt, void* hip_stream) {
  return debug_gemm_split(aimnet::SPLIT_H2, cfg, epi, out2, A2, lda2, Bt2, ldb, M, N, K, bias, C, C2, ldc2, D, ldc, alt, hip_stream);
}
int aimnet_engine_debug_mlp_sweep(aimnet_engine* e, int pass, int backward, int chain, int flag, const void* x2, int M,
                                  const int32_t* numbers, float* const* H, float* const* D, float* const* zb, int* which,
                                  void* hip_stream) {
  using namespace aimnet;
  if (!e || pass < 0 || pass >= e->arch.n_pass || M <= 0 || !D) return AIMNET_E_INVALID;
  if (!(e->gemm_h2 && e->h2_fits)) {
    set_last_error("debug_mlp_sweep: the fp16x2 operand form is off");
    return AIMNET_E_INVALID;
  }
  hipStream_t s = (hipStream_t)hip_stream;
  if (!backward) {
    if (!x2 || !H) return AIMNET_E_INVALID;
    return mlp_sweep_fwd(e, s, SPLIT_H2, pass, M, numbers, reinterpret_cast<const float*>(x2), H, D, flag != 0, chain != 0);
  }
  if (!zb || !zb[0] || !zb[1] || !which) return AIMNET_E_INVALID;
  float *zcur = zb[0], *znext = zb[1];
  const int rc = mlp_sweep_bwd(e, s, SPLIT_H2, pass, M, flag != 0, zcur, znext, D, chain != 0);
  *which = zcur == zb[0] ? 0 : 1;
  return rc;
}

int aimnet_debug_pme_recip(const float* xw, const float* q, const int* order, const float* cell, float total_charge, int n_atoms,
                           float accuracy,
                           int max_mesh, double* e_atom, float* qbar, float* fgrad, float* virial_atom, double* host_info,
                           void* hip_stream) {
  using namespace aimnet;
  if (!xw || !q || !cell || !e_atom || !qbar || !fgrad || !virial_atom || !host_info || n_atoms <= 0 || max_mesh < 512)
    return AIMNET_E_INVALID;
  hipStream_t st = (hipStream_t)hip_stream;
  EwaldBuffers b{};
  b.max_mesh = max_mesh;
  b.max_parts = ceil_div(max_mesh, PME_PART);
  int *mol_idx = nullptr, *mol_start = nullptr, *status = nullptr;
  float* charge = nullptr;
  const int ms[2] = {0, n_atoms};
  int rc = 0;
#define PME_DBG(x)            \
  if ((x) != hipSuccess) {    \
    rc = AIMNET_E_HIP;        \
    goto done;                \
  }
  PME_DBG(hipMalloc(&b.sys, sizeof(EwaldSystem)));
  PME_DBG(hipMalloc(&b.meshq, sizeof(long long) * (size_t)max_mesh));
  PME_DBG(hipMalloc(&b.ma, sizeof(double) * 2 * (size_t)max_mesh));
  PME_DBG(hipMalloc(&b.mb, sizeof(double) * 2 * (size_t)max_mesh));
  PME_DBG(hipMalloc(&b.bmod, sizeof(double) * 3 * PME_MAX_AXIS));
  PME_DBG(hipMalloc(&b.vpart, sizeof(double) * 8 * (size_t)b.max_parts));
  PME_DBG(hipMalloc(&mol_idx, sizeof(int) * n_atoms));
  PME_DBG(hipMalloc(&mol_start, sizeof(int) * 2));
  PME_DBG(hipMalloc(&status, sizeof(int)));
  PME_DBG(hipMalloc(&charge, sizeof(float)));
  PME_DBG(hipMemsetAsync(mol_idx, 0, sizeof(int) * n_atoms, st));
  PME_DBG(hipMemcpyAsync(mol_start, ms, sizeof(ms), hipMemcpyHostToDevice, st));
  PME_DBG(hipMemcpyAsync(charge, &total_charge, sizeof(float), hipMemcpyHostToDevice, st));
  rc = launch_pme_setup(st, cell, 1, mol_start, charge, 1, 1, accuracy, b, status);
  if (!rc) rc = launch_pme_recip(st, true, true, xw, q, mol_idx, mol_start, order, n_atoms, 1, b, 1.0f, e_atom, qbar, fgrad, virial_atom);
  if (!rc) {
    EwaldSystem E;
    int need = 0;
    PME_DBG(hipMemcpyAsync(&E, b.sys, sizeof(E), hipMemcpyDeviceToHost, st));
    PME_DBG(hipMemcpyAsync(&need, status, sizeof(int), hipMemcpyDeviceToHost, st));
    PME_DBG(hipStreamSynchronize(st));
    host_info[0] = E.alpha; host_info[1] = E.rc; host_info[2] = E.mesh[0]; host_info[3] = E.mesh[1]; host_info[4] = E.mesh[2];
    host_info[5] = need; host_info[6] = E.phi_bg; host_info[7] = 0.0;
  }
done:
#undef PME_DBG
  (void)hipStreamSynchronize(st);
  (void)hipFree(b.sys); (void)hipFree(b.frac); (void)hipFree(b.meshq); (void)hipFree(b.ma); (void)hipFree(b.mb); (void)hipFree(b.bmod);
  (void)hipFree(b.vpart); (void)hipFree(mol_idx); (void)hipFree(mol_start); (void)hipFree(status); (void)hipFree(charge);
  return rc;
}

int aimnet_debug_pme_tangent(const float* xw, const float* q, const float* tq, const float* v, const int* order, const float* cell,
                             float total_charge, int n_atoms, int n_dir, float accuracy, int max_mesh, double* field, double* tphi,
                             double* tg, double* host_info, void* hip_stream) {
  using namespace aimnet;
  if (!xw || !q || !tq || !v || !cell || !field || !tphi || !tg || !host_info || n_atoms <= 0 || n_atoms >= (1 << 21) || n_dir <= 0 ||
      n_dir > 65535 || max_mesh < 512)
    return AIMNET_E_INVALID;
  hipStream_t st = (hipStream_t)hip_stream;
  EwaldBuffers b{};
  PmeTangentBuffers t{};
  b.max_mesh = max_mesh;
  b.max_parts = ceil_div(max_mesh, PME_PART);
  const size_t mm = (size_t)max_mesh, tm = mm * (size_t)n_dir;
  int *mol_idx = nullptr, *mol_start = nullptr, *status = nullptr;
  float* charge = nullptr;
  const int ms[2] = {0, n_atoms};
  std::vector<double> scales((size_t)n_dir);
  int rc = 0;
#define PME_DBG(x)            \
  if ((x) != hipSuccess) {    \
    rc = AIMNET_E_HIP;        \
    goto done;                \
  }
  PME_DBG(hipMalloc(&b.sys, sizeof(EwaldSystem)));
  PME_DBG(hipMalloc(&b.meshq, sizeof(long long) * mm));
  PME_DBG(hipMalloc(&b.ma, sizeof(double) * 2 * mm));
  PME_DBG(hipMalloc(&b.mb, sizeof(double) * 2 * mm));
  PME_DBG(hipMalloc(&b.bmod, sizeof(double) * 3 * PME_MAX_AXIS));
  PME_DBG(hipMalloc(&b.vpart, sizeof(double) * 8 * (size_t)b.max_parts));
  PME_DBG(hipMalloc(&t.tmeshq, sizeof(long long) * tm));
  PME_DBG(hipMalloc(&t.tma, sizeof(double) * 2 * tm));
  PME_DBG(hipMalloc(&t.tmb, sizeof(double) * 2 * tm));
  PME_DBG(hipMalloc(&t.sys_rep, sizeof(EwaldSystem) * (size_t)n_dir));
  PME_DBG(hipMalloc(&t.tscale, sizeof(double) * (size_t)n_dir));
  PME_DBG(hipMalloc(&mol_idx, sizeof(int) * n_atoms));
  PME_DBG(hipMalloc(&mol_start, sizeof(int) * 2));
  PME_DBG(hipMalloc(&status, sizeof(int)));
  PME_DBG(hipMalloc(&charge, sizeof(float)));
  t.field = field;
  PME_DBG(hipMemsetAsync(mol_idx, 0, sizeof(int) * n_atoms, st));
  PME_DBG(hipMemsetAsync(tphi, 0, sizeof(double) * (size_t)n_dir * n_atoms, st));
  PME_DBG(hipMemsetAsync(tg, 0, sizeof(double) * 3 * (size_t)n_dir * n_atoms, st));
  PME_DBG(hipMemcpyAsync(mol_start, ms, sizeof(ms), hipMemcpyHostToDevice, st));
  PME_DBG(hipMemcpyAsync(charge, &total_charge, sizeof(float), hipMemcpyHostToDevice, st));
  rc = launch_pme_setup(st, cell, 1, mol_start, charge, 1, 1, accuracy, b, status);
  if (!rc) rc = launch_pme_potential(st, xw, q, mol_idx, order, n_atoms, 1, b);
  if (!rc) rc = launch_pme_field(st, xw, mol_idx, n_atoms, b, field);
  if (!rc)
    rc = launch_pme_tangent(st, xw, q, tq, 1, v, mol_idx, order, n_atoms, 1, n_dir, b, t, 1.0f, nullptr, nullptr, nullptr, nullptr, tphi,
                            tg);
  if (!rc) {
    EwaldSystem E;
    int need = 0;
    PME_DBG(hipMemcpyAsync(&E, b.sys, sizeof(E), hipMemcpyDeviceToHost, st));
    PME_DBG(hipMemcpyAsync(&need, status, sizeof(int), hipMemcpyDeviceToHost, st));
    PME_DBG(hipMemcpyAsync(scales.data(), t.tscale, sizeof(double) * (size_t)n_dir, hipMemcpyDeviceToHost, st));
    PME_DBG(hipStreamSynchronize(st));
    double smax = scales[0];
    for (double sk : scales) smax = sk > smax ? sk : smax;
    host_info[0] = E.alpha; host_info[1] = E.rc; host_info[2] = E.mesh[0]; host_info[3] = E.mesh[1]; host_info[4] = E.mesh[2];
    host_info[5] = need; host_info[6] = E.phi_bg; host_info[7] = 1099511627776.0 / smax;
  }
done:
#undef PME_DBG
  (void)hipStreamSynchronize(st);
  (void)hipFree(b.sys); (void)hipFree(b.meshq); (void)hipFree(b.ma); (void)hipFree(b.mb); (void)hipFree(b.bmod); (void)hipFree(b.vpart);
  (void)hipFree(t.tmeshq); (void)hipFree(t.tma); (void)hipFree(t.tmb); (void)hipFree(t.sys_rep); (void)hipFree(t.tscale);
  (void)hipFree(mol_idx); (void)hipFree(mol_start); (void)hipFree(status); (void)hipFree(charge);
  return rc;
}

// ---- the engine's conv kernels, one launch at a time on caller-made buffers (tests/test_gpu_conv_kernels.py) ----------------
// row stride of x / xbar: the 704 (+ 29 per charge channel) columns in use, a multiple of 32, and at most the 64 pad columns the
// forward kernel zeroes
static bool debug_conv_ldx_ok(int nq, int ldx) { return ldx % 32 == 0 && ldx >= 704 + 29 * nq && ldx <= 768; }
static bool debug_conv_basis(float rc, float eta, const float* shifts, aimnet::BasisParams* bp) {
  if (!shifts || !(rc > 0.f) || !(eta > 0.f)) return false;
  bp->rc = rc;
  bp->eta = eta;
  for (int g = 0; g < 16; ++g) bp->shifts[g] = shifts[g];
  return true;
}

int aimnet_debug_conv_fwd(int nq, const float* a, const int32_t* row_of, const float* q, const int32_t* nb_idx,
                          const int32_t* nb_cnt, const float* pg, int cap, const float* agh_a, const float* agh_q, float rc,
                          float eta, const float* shifts, void* x, int ldx, float* Vsave, float* Vqsave, int n_atoms,
                          const int32_t* order, int species_moments, int split_max, int x_split, void* hip_stream) {
  aimnet::BasisParams bp;
  if (nq < 0 || nq > 2 || !a || !nb_idx || !nb_cnt || !pg || cap <= 0 || !agh_a || !x || !Vsave || n_atoms <= 0 || x_split < 0 ||
      x_split > 2 || !debug_conv_ldx_ok(nq, ldx) || !debug_conv_basis(rc, eta, shifts, &bp))
    return AIMNET_E_INVALID;
  if (nq > 0 && (!q || !agh_q || !Vqsave)) return AIMNET_E_INVALID;
  if (species_moments && (!row_of || nq != 0)) return AIMNET_E_INVALID;
  return launch_conv_fwd((hipStream_t)hip_stream, nq, a, row_of, q, nb_idx, nb_cnt, reinterpret_cast<const float4*>(pg), cap, agh_a,
                         agh_q, bp, reinterpret_cast<float*>(x), ldx, Vsave, Vqsave, n_atoms, order, species_moments != 0, split_max,
                         x_split);
}

int aimnet_debug_unconcat(int nq, const float* xbar, int ldx, const float* Vsave, const float* Vqsave, const float* agh_a,
                          const float* agh_q, float* Sbar, float* Sqbar, int n_atoms, void* hip_stream) {
  if (nq < 0 || nq > 2 || !xbar || !Vsave || !agh_a || !Sbar || n_atoms <= 0 || !debug_conv_ldx_ok(nq, ldx)) return AIMNET_E_INVALID;
  if (nq > 0 && (!Vqsave || !agh_q || !Sqbar)) return AIMNET_E_INVALID;
  return launch_unconcat((hipStream_t)hip_stream, nq, xbar, ldx, Vsave, Vqsave, agh_a, agh_q, Sbar, Sqbar, n_atoms);
}

int aimnet_debug_conv_bwd(int nq, int need_abar, int stress, const float* a, const int32_t* row_of, const float* q, const float* Sbar,
                          const float* Sqbar, const int32_t* nb_idx, const int32_t* nb_cnt, const float* pg, int cap, float rc,
                          float eta, const float* shifts, const float* xbar, int ldx, const float* abar_in, float* abar_out,
                          const float* qbar_in, float* qbar_out, float* fgrad, float* virial_atom, int n_atoms, const int32_t* order,
                          float* pairbuf, int pb_accum, int split_max, void* hip_stream) {
  aimnet::BasisParams bp;
  if (nq < 0 || nq > 2 || !a || !Sbar || !nb_idx || !nb_cnt || !pg || cap <= 0 || !xbar || !fgrad || n_atoms <= 0 ||
      !debug_conv_ldx_ok(nq, ldx) || !debug_conv_basis(rc, eta, shifts, &bp))
    return AIMNET_E_INVALID;
  if (nq > 0 && (!q || !Sqbar || !qbar_in || !qbar_out)) return AIMNET_E_INVALID;
  if ((need_abar && !abar_out) || (stress && !virial_atom)) return AIMNET_E_INVALID;
  return launch_conv_bwd((hipStream_t)hip_stream, nq, need_abar != 0, stress != 0, a, row_of, q, Sbar, Sqbar, nb_idx, nb_cnt,
                         reinterpret_cast<const float4*>(pg), cap, bp, xbar, ldx, abar_in, abar_out, qbar_in, qbar_out, fgrad,
                         virial_atom, n_atoms, order, reinterpret_cast<float4*>(pairbuf), pb_accum != 0, split_max);
}

int aimnet_debug_conv_bwd_p0(int stress, const float* xbar, int ldx, const float* Vsave, const float* agh_a, const float* afv,
                             const int32_t* z_of_slot, int nslots, const unsigned long long* present_part, int n_part,
                             const int32_t* aslot, const int32_t* nb_idx, const int32_t* nb_cnt, const float* pg, int cap, float rc,
                             float eta, const float* shifts, float* T, float* fgrad, float* virial_atom, int n_atoms,
                             const int32_t* order, float* pairbuf, void* hip_stream) {
  aimnet::BasisParams bp;
  if (!xbar || !Vsave || !agh_a || !afv || !z_of_slot || nslots <= 0 || nslots > 64 || !present_part || n_part <= 0 || !aslot ||
      !nb_idx || !nb_cnt || !pg || cap <= 0 || !T || !fgrad || n_atoms <= 0 || (stress && !virial_atom) ||
      !debug_conv_ldx_ok(0, ldx) || !debug_conv_basis(rc, eta, shifts, &bp))
    return AIMNET_E_INVALID;
  hipStream_t s = (hipStream_t)hip_stream;
  const int rc0 = launch_unconcat_p0(s, xbar, ldx, Vsave, agh_a, afv, z_of_slot, nslots, present_part, n_part, T, n_atoms);
  if (rc0) return rc0;
  return launch_conv_bwd_p0(s, stress != 0, T, nslots, aslot, nb_idx, nb_cnt, reinterpret_cast<const float4*>(pg), cap, bp, fgrad,
                            virial_atom, n_atoms, order, reinterpret_cast<float4*>(pairbuf));
}

int aimnet_debug_pair_force(const int32_t* nb_idx, const int32_t* nb_cnt, const int32_t* rev, const float* pairbuf, int cap,
                            int n_atoms, const float* fgrad, float* forces, void* hip_stream) {
  if (!nb_idx || !nb_cnt || !rev || !pairbuf || cap <= 0 || n_atoms <= 0 || !fgrad || !forces) return AIMNET_E_INVALID;
  return launch_pair_force((hipStream_t)hip_stream, nb_idx, nb_cnt, rev, reinterpret_cast<const float4*>(pairbuf), cap, n_atoms,
                           fgrad, forces, nullptr);
}

int aimnet_conv_sv_2d_sp_fwd(const float* a, const int32_t* idx, const float* g, float* out, int32_t B, int32_t A,
                             int32_t G, int32_t M, void* hip_stream) {
  if (!a || !idx || !g || !out || B < 0 || A <= 0 || G <= 0 || M <= 0) return AIMNET_E_INVALID;
  return launch_conv_sv_fwd((hipStream_t)hip_stream, a, idx, g, out, B, A, G, M);
}

int aimnet_conv_sv_2d_sp_bwd(const float* grad_out, const float* a, const int32_t* idx, const float* g,
                             float* grad_a, float* grad_g, int32_t B, int32_t A, int32_t G, int32_t M,
                             void* hip_stream) {
  if (!grad_out || !a || !idx || !g || !grad_a || !grad_g || B < 0 || A <= 0 || G <= 0 || M <= 0) return AIMNET_E_INVALID;
  return launch_conv_sv_bwd((hipStream_t)hip_stream, grad_out, a, idx, g, grad_a, grad_g, B, A, G, M);
}

int aimnet_conv_sv_2d_sp_bwd_bwd(const float* grad_out, const float* grad2_a, const float* grad2_g, const float* a,
                                 const int32_t* idx, const float* g, float* grad_grad_out, float* grad_a_double,
                                 float* grad_g_double, int32_t B, int32_t A, int32_t G, int32_t M, void* hip_stream) {
  if (!grad_out || !grad2_a || !grad2_g || !a || !idx || !g || !grad_grad_out || !grad_a_double || !grad_g_double || B < 0 ||
      A <= 0 || G <= 0 || M <= 0)
    return AIMNET_E_INVALID;
  return launch_conv_sv_bwd_bwd((hipStream_t)hip_stream, grad_out, grad2_a, grad2_g, a, idx, g, grad_grad_out, grad_a_double,
                                grad_g_double, B, A, G, M);
}

}  // extern "C"
