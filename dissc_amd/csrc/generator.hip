// dissc_gen_*: the unit/F0/speaker-conditioned HiFi-GAN generator on one MI355X.
// Orchestrates ~100 launches of conv_mfma_kernel per forward on the caller's stream;
// all activations live in the caller-provided workspace (no allocation here).
//
// Workspace = 4 buffers of B * max_i(C_i * ld_i) floats:
//   X   stage input (ConvTranspose output), read by the 3 resblocks
//   TMP conv1 output of the current (conv1, conv2) pair
//   XK  running x of the current resblock
//   ACC MRF accumulator; becomes the next stage's ConvTranspose input
// Activations are channels-first [B][C][ld] fp32 (time contiguous => coalesced tile
// loads and MFMA-row stores), ld = stage length rounded up to 4.
#include <algorithm>
#include <functional>
#include <map>
#include <mutex>
#include <string>
#include <tuple>
#include <vector>

#include "gen_plan.h"

using namespace dissc;

// option "graphs" (default 0): replay small forwards from a captured hipGraph.  OFF by default: measured on ROCm 7.2 / MI355X,
//   hipGraphLaunch of the ~85-node three-branch graph costs 1.3-1.8 ms MORE per forward than the plain three-stream launches
// option "graph_frames" (default 2048): largest B * Tmax that is graphed; g_graph_hits / g_graph_captures (common.h) count
// option "multistream" (default 1): concurrent ResBlock chains (read at create)

// The side streams of the concurrent ResBlock chains are shared by every generator handle of a device (created on first use, kept
// for the life of the process): HIP multiplexes streams onto a few hardware queues (4 by default), and a second handle with streams
// of its own would push the chains of both onto shared queues and serialise them (measured: +12 % per step for whichever handle was
// created second).  Work of different handles on a shared stream is ordered by the same events as before, so sharing changes no result.
static hipStream_t shared_aux_stream(int chain, int prio) {
  static std::mutex mu;
  static std::map<std::tuple<int, int, int>, hipStream_t> pool;
  int dev = 0;
  if (hipGetDevice(&dev) != hipSuccess) return nullptr;
  std::lock_guard<std::mutex> lock(mu);
  auto key = std::make_tuple(dev, chain, prio);
  auto it = pool.find(key);
  if (it != pool.end()) return it->second;
  hipStream_t st = nullptr;
  if (hipStreamCreateWithPriority(&st, hipStreamNonBlocking, prio) != hipSuccess) return nullptr;
  pool[key] = st;
  return st;
}

struct dissc_gen {
  Options opt;  // this handle's snapshot of the tuning options (common.h): every entry point that works on the handle runs under it
  DisscGenConfig cfg;
  int rb_type = 1;  // 1: ResBlock1, three (conv_d, conv_1) pairs per block (plan, rb1, rb2, pw, fused_*); 2: ResBlock2, two dilated
                    // convs per block, rb1[stage*nk*3 + j*3 + m], m = 0, 1, run in the form plan2 gives
  int hop = 1;
  DevConv conv_pre;
  std::vector<std::vector<DevConv>> ups;  // per stage: one conv per phase group
  std::vector<ChainPlan> plan;     // [stage*nk + j]: the kernel forms of ResBlock j of the stage
  std::vector<Rb2Form> plan2;      // ... of a ResBlock2 (rb_type 2)
  std::vector<DevConv> rb1, rb2;  // [stage*nk*3 + j*3 + m]: conv_d / conv_1 of pair m (forms direct, direct_dma, td, fused)
  std::vector<DevPairW> pw;       // same index: the pair as ONE transform-domain launch (form fused_td)
  std::vector<float*> fused_w, fused_b;  // [stage*nk + j]: 6 packed convs / biases of a split-bf16 ResBlock (bf3_* chains) or of a
                                         // one-launch F(2,3) chain (f23_chain)
  float* post_w = nullptr;
  float* post_b = nullptr;
  int post_C = 0, post_KS = 0;
  float* dict_w = nullptr;
  float* spkr_w = nullptr;
  std::vector<int> stage_C, stage_mul;  // channels / length multiplier after ups[i]
  // The num_kernels ResBlocks of a stage are independent until the MRF accumulate: they run as
  // concurrent chains (chain 0 on the caller's stream, the others on these) so bandwidth-bound
  // small-kernel layers overlap with matrix-bound large-kernel ones.
  hipStream_t aux[DISSC_MAX_RK] = {nullptr, nullptr, nullptr, nullptr};
  hipEvent_t ev_x = nullptr, ev_fin[DISSC_MAX_RK] = {nullptr, nullptr, nullptr, nullptr};
  // Opt-in (option "graphs"): small forwards (the reference's one-utterance-at-a-time mode: ~85 launches of a few us each
  // over three streams, 11 % of the period idle) captured once per (shapes, buffers) into a hipGraph and replayed.
  struct GraphEntry {
    const void *code, *f0, *spkr, *lengths, *out, *ws;
    int B, T;
    hipGraphExec_t exec;
    unsigned long long stamp;
  };
  std::vector<GraphEntry> graphs;
  hipStream_t cap_stream = nullptr;
  unsigned long long graph_clock = 0;
  int graph_failures = 0;  // captures that did not produce a graph: after two, this handle stops trying
  ~dissc_gen() {
    for (auto& e : graphs) (void)hipGraphExecDestroy(e.exec);
    if (cap_stream) (void)hipStreamDestroy(cap_stream);
    free_conv(conv_pre);
    for (auto& v : ups) for (auto& c : v) free_conv(c);
    for (auto& c : rb1) free_conv(c);
    for (auto& c : rb2) free_conv(c);
    for (auto& c : pw) free_pairw(c);
    for (float* p : fused_w) if (p) (void)hipFree(p);
    for (float* p : fused_b) if (p) (void)hipFree(p);
    if (post_w) (void)hipFree(post_w);
    if (post_b) (void)hipFree(post_b);
    for (int j = 0; j < DISSC_MAX_RK; ++j)  // aux[] streams belong to the process-wide pool
      if (ev_fin[j]) (void)hipEventDestroy(ev_fin[j]);
    if (ev_x) (void)hipEventDestroy(ev_x);
    if (dict_w) (void)hipFree(dict_w);
    if (spkr_w) (void)hipFree(spkr_w);
  }
};

static inline size_t round_up(size_t x, size_t m) { return (x + m - 1) / m * m; }

extern "C" {

int dissc_gen_create(const DisscGenConfig* cfg, const DisscTensor* weights, size_t n_weights,
                     dissc_gen_t* out) {
  return dissc_gen_create_ex(cfg, weights, n_weights, -1, out);
}

int dissc_gen_create_ex(const DisscGenConfig* cfg, const DisscTensor* weights, size_t n_weights, int precision,
                        dissc_gen_t* out) {
  return dissc_gen_create_rb(cfg, weights, n_weights, precision, 1, out);
}

int dissc_gen_create_rb(const DisscGenConfig* cfg, const DisscTensor* weights, size_t n_weights, int precision, int resblock,
                        dissc_gen_t* out) {
  if (resblock != 1 && resblock != 2) {
    set_error("dissc_gen_create_rb: resblock %d (use 1 = ResBlock1, 2 = ResBlock2)", resblock);
    return DISSC_EINVAL;
  }
  if (precision < -1 || precision > 1) {
    set_error("dissc_gen_create_ex: precision %d (use -1 = process option, 0 = fp32, 1 = split-bf16)", precision);
    return DISSC_EINVAL;
  }
  const int prec = precision < 0 ? g_defaults.precision : precision;  // this handle's arithmetic, fixed from here on
  if (!cfg || !weights || !out) {
    set_error("dissc_gen_create: null argument");
    return DISSC_EINVAL;
  }
  if (cfg->num_upsamples < 1 || cfg->num_upsamples > DISSC_MAX_UPS || cfg->num_kernels < 1 ||
      cfg->num_kernels > DISSC_MAX_RK) {
    set_error("dissc_gen_create: unsupported num_upsamples=%d / num_kernels=%d", cfg->num_upsamples,
              cfg->num_kernels);
    return DISSC_EINVAL;
  }
  std::map<std::string, const DisscTensor*> byname;
  for (size_t i = 0; i < n_weights; ++i) byname[weights[i].name] = &weights[i];
  auto get = [&](const std::string& name, std::initializer_list<int64_t> shape,
                 const float** p) -> int {
    auto it = byname.find(name);
    if (it == byname.end()) {
      set_error("dissc_gen_create: missing tensor '%s'", name.c_str());
      return DISSC_ENOTFOUND;
    }
    const DisscTensor* t = it->second;
    size_t d = 0;
    bool ok = (size_t)t->ndim == shape.size();
    for (int64_t s : shape) {
      if (ok && t->shape[d] != s) ok = false;
      ++d;
    }
    if (!ok) {
      set_error("dissc_gen_create: tensor '%s' has the wrong shape", name.c_str());
      return DISSC_EINVAL;
    }
    *p = t->data;
    return DISSC_OK;
  };

  dissc_gen* g = new dissc_gen();
  g->opt = g_defaults;          // frozen here: later dissc_set_option calls do not reach this handle
  g->opt.precision = prec;
  OptScope opt_scope(&g->opt);
  g->cfg = *cfg;
  g->rb_type = resblock;
  PrecScope prec_scope(prec);  // only the generator's layers may be packed for split-bf16
  int rc = DISSC_OK;
  const float *w = nullptr, *b = nullptr;
  const int c0 = cfg->upsample_initial_channel;
  const int in_dim = cfg->model_in_dim;
  const int E = cfg->embedding_dim;
  auto fail = [&](int code) {
    delete g;
    return code;
  };
  // Packing a layer's weights (direct fragments, Toom-Cook transforms in double) is host work of ~60 ms for this model when done
  // one layer after the other: the layers are independent, so their make_* calls are collected as tasks and run on a few host
  // threads at the end (run_pack_tasks, pack_pool.hip).  Each task writes one pre-sized slot of the handle.
  std::vector<std::function<int()>> tasks;
  if (in_dim != E + (cfg->has_f0 ? 1 : 0) + (cfg->has_spkr ? E : 0)) {
    set_error("dissc_gen_create: model_in_dim %d != embedding_dim %d (+1 f0) (+%d spkr)", in_dim, E, E);
    return fail(DISSC_EINVAL);
  }
  if ((rc = get("conv_pre.weight", {c0, in_dim, 7}, &w))) return fail(rc);
  if ((rc = get("conv_pre.bias", {c0}, &b))) return fail(rc);
  tasks.push_back([=]() { return make_conv(w, b, c0, in_dim, 7, 1, g->conv_pre); });

  int ch = c0, mul = 1;
  g->ups.resize(cfg->num_upsamples);
  const int nk = cfg->num_kernels;
  g->plan.resize((size_t)cfg->num_upsamples * nk);
  g->plan2.assign((size_t)cfg->num_upsamples * nk, Rb2Form::two_launch);
  g->rb1.resize((size_t)cfg->num_upsamples * nk * 3);
  g->rb2.resize((size_t)cfg->num_upsamples * nk * 3);
  g->pw.resize((size_t)cfg->num_upsamples * nk * 3);
  g->fused_w.assign((size_t)cfg->num_upsamples * nk, nullptr);
  g->fused_b.assign((size_t)cfg->num_upsamples * nk, nullptr);
  for (int i = 0; i < cfg->num_upsamples; ++i) {
    const int s = cfg->upsample_rates[i], k = cfg->upsample_kernel_sizes[i];
    if (s < 1 || k < s || (k - s) % 2 != 0) {  // L_out = s * L_in needs k - s even
      set_error("dissc_gen_create: upsample k=%d s=%d unsupported", k, s);
      return fail(DISSC_EINVAL);
    }
    const int cout = ch / 2;
    char name[96];
    snprintf(name, sizeof(name), "ups.%d.weight", i);
    if ((rc = get(name, {ch, cout, k}, &w))) return fail(rc);
    snprintf(name, sizeof(name), "ups.%d.bias", i);
    if ((rc = get(name, {cout}, &b))) return fail(rc);
    tasks.push_back([=]() { return make_convT(w, b, ch, cout, k, s, g->ups[i]); });
    ch = cout;
    mul *= s;
    g->stage_C.push_back(ch);
    g->stage_mul.push_back(mul);
    for (int j = 0; j < nk; ++j) {
      const int rk = cfg->resblock_kernel_sizes[j];
      if (rk % 2 != 1) {
        set_error("dissc_gen_create: even resblock kernel size %d unsupported", rk);
        return fail(DISSC_EINVAL);
      }
      const int* dl = cfg->resblock_dilations[j];
      const size_t cj = (size_t)i * nk + j;
      if (resblock == 2) {  // each conv by make_conv's per-layer rule (fp32, or split-bf16 where that rule grants an instance)
        for (int m = 0; m < 2; ++m) {
          const int d = dl[m];
          if (d < 1 || (rk - 1) * d > RB_TAP_SPAN) {
            set_error("dissc_gen_create_rb: resblock_dilation_sizes[%d][%d] = %d with kernel size %d: (k - 1) x dilation must be in 0 .. %d",
                      j, m, d, rk, RB_TAP_SPAN);
            return fail(DISSC_EINVAL);
          }
          snprintf(name, sizeof(name), "resblocks.%d.convs.%d.weight", (int)cj, m);
          if ((rc = get(name, {ch, ch, rk}, &w))) return fail(rc);
          snprintf(name, sizeof(name), "resblocks.%d.convs.%d.bias", (int)cj, m);
          if ((rc = get(name, {ch}, &b))) return fail(rc);
          tasks.push_back([=]() { return make_conv(w, b, ch, ch, rk, d, g->rb1[cj * 3 + m]); });
        }
        g->plan2[cj] = plan_resblock2(ch, rk, dl[0], dl[1], prec);
        continue;
      }
      const ChainPlan& cp = g->plan[cj] = plan_chain(ch, rk, dl, prec);
      const float* w6[6];  // conv_d / conv_1 of the three pairs
      const float* b6[6];
      for (int l = 0; l < 6; ++l) {
        snprintf(name, sizeof(name), "resblocks.%d.convs%d.%d.weight", (int)cj, 1 + l % 2, l / 2);
        if ((rc = get(name, {ch, ch, rk}, &w6[l]))) return fail(rc);
        snprintf(name, sizeof(name), "resblocks.%d.convs%d.%d.bias", (int)cj, 1 + l % 2, l / 2);
        if ((rc = get(name, {ch}, &b6[l]))) return fail(rc);
      }
      if (cp.form == ChainForm::f23_chain) {  // the six convs transformed and packed together
        const std::vector<const float*> wv(w6, w6 + 6), bv(b6, b6 + 6);
        tasks.push_back([=]() { return make_chain_f23(wv.data(), bv.data(), ch, &g->fused_w[cj], &g->fused_b[cj]); });
        continue;
      }
      if (cp.form != ChainForm::pairs) {  // split-bf16: the six convs packed together
        std::vector<float> fw, fb;
        pack_resblock_bf3(ch, rk, w6, fw);
        for (const float* bl : b6) fb.insert(fb.end(), bl, bl + ch);
        if ((rc = upload(fw, &g->fused_w[cj]))) return fail(rc);
        if ((rc = upload(fb, &g->fused_b[cj]))) return fail(rc);
        continue;
      }
      for (int m = 0; m < 3; ++m) {
        const PairPlan p = cp.pair[m];
        const size_t idx = cj * 3 + m;
        const int d = dl[m];
        const float *w1 = w6[2 * m], *b1 = b6[2 * m], *w2 = w6[2 * m + 1], *b2 = b6[2 * m + 1];
        if (p.form == PairForm::fused_td) {
          tasks.push_back([=]() { return make_pairw(w1, b1, w2, b2, ch, rk, d, p.reg_form, g->pw[idx]); });
        } else {
          tasks.push_back([=]() { return make_pair_conv(p.conv[0], w1, b1, ch, rk, d, g->rb1[idx]); });
          tasks.push_back([=]() { return make_pair_conv(p.conv[1], w2, b2, ch, rk, 1, g->rb2[idx]); });
        }
      }
    }
  }
  g->hop = mul;
  if ((rc = get("conv_post.weight", {1, ch, 7}, &w))) return fail(rc);
  if ((rc = get("conv_post.bias", {1}, &b))) return fail(rc);
  g->post_C = ch;
  g->post_KS = 7;
  if ((rc = upload(std::vector<float>(w, w + ch * 7), &g->post_w))) return fail(rc);
  if ((rc = upload(std::vector<float>(b, b + 1), &g->post_b))) return fail(rc);
  if ((rc = get("dict.weight", {cfg->num_embeddings, E}, &w))) return fail(rc);
  if ((rc = upload(std::vector<float>(w, w + (size_t)cfg->num_embeddings * E), &g->dict_w)))
    return fail(rc);
  if (cfg->has_spkr) {
    if ((rc = get("spkr.weight", {cfg->num_speakers, E}, &w))) return fail(rc);
    if ((rc = upload(std::vector<float>(w, w + (size_t)cfg->num_speakers * E), &g->spkr_w)))
      return fail(rc);
  }
  if ((rc = run_pack_tasks(tasks, pack_thread_count(), g->opt, prec))) return fail(rc);
  if (opts().multistream && nk > 1) {
    if (hipEventCreateWithFlags(&g->ev_x, hipEventDisableTiming) != hipSuccess) return fail(DISSC_EHIP);
    for (int j = 0; j < nk; ++j) {
      if (hipEventCreateWithFlags(&g->ev_fin[j], hipEventDisableTiming) != hipSuccess) return fail(DISSC_EHIP);
      // later chains have larger kernels (k = 3 < 7 < 11): the longest one is the stage's critical
      // path, so it gets the highest stream priority and the short chains fill in around it
      int lo = 0, hi = 0;
      (void)hipDeviceGetStreamPriorityRange(&lo, &hi);  // lo = least urgent, hi = most urgent (numerically lower)
      const int prio = lo + (hi - lo) * j / (nk - 1);
      if (j > 0 && !(g->aux[j] = shared_aux_stream(j, prio))) return fail(DISSC_EHIP);
    }
  }
  *out = g;
  return DISSC_OK;
}

void dissc_gen_destroy(dissc_gen_t g) { delete g; }

int dissc_gen_hop(dissc_gen_t g) { return g ? g->hop : 0; }

constexpr size_t BUF_GUARD = 64;  // floats in front of the chains' scratch buffers (their last ZERO_TAIL are kept zero)
static size_t gen_buf_floats(const dissc_gen* g, int B, int Tmax) {
  // rows may carry a zero tail (EPI_STORE_ACT layout): ZERO_TAIL extra columns
  size_t per = (size_t)g->cfg.upsample_initial_channel * round_up(Tmax + ZERO_TAIL, 4);
  per = std::max(per, (size_t)g->cfg.model_in_dim * round_up(Tmax + ZERO_TAIL, 4));
  for (size_t i = 0; i < g->stage_C.size(); ++i)
    per = std::max(per, (size_t)g->stage_C[i] * round_up((size_t)Tmax * g->stage_mul[i] + ZERO_TAIL, 4));
  return round_up(per * B + BUF_GUARD + 512, 64);  // + slack: LDS-DMA windows run up to ~130 floats past a row
}

size_t dissc_gen_workspace_bytes(dissc_gen_t g, int B, int Tmax) {
  if (!g || B <= 0 || Tmax <= 0) return 0;
  OptScope opt_scope(&g->opt);
  return (size_t)(2 + 2 * g->cfg.num_kernels) * gen_buf_floats(g, B, Tmax) * sizeof(float) + 256;
}

// multiply-adds per input frame: algorithmic, or (executed) what the matrix pipe executes -- the transform-domain forms do fewer
static double gen_macs(const dissc_gen* g, bool executed) {
  double macs = g->conv_pre.macs_per_t;
  int mul = 1;
  const int nk = g->cfg.num_kernels;
  for (int i = 0; i < g->cfg.num_upsamples; ++i) {
    for (auto& c : g->ups[i]) macs += c.macs_per_t * mul;
    mul = g->stage_mul[i];
    for (int j = 0; j < nk; ++j) {
      const int C = g->stage_C[i], rk = g->cfg.resblock_kernel_sizes[j];
      macs += (g->rb_type == 2 ? 2.0 * C * C * rk  // two direct convs: executed = algorithmic
                               : chain_macs(g->plan[(size_t)i * nk + j], C, rk, executed)) * mul;
    }
  }
  macs += (double)g->post_C * g->post_KS * mul;
  return macs;
}

double dissc_gen_flops(dissc_gen_t g, int64_t frames) { return g ? 2.0 * gen_macs(g, false) * (double)frames : 0; }

double dissc_gen_flops_executed(dissc_gen_t g, int64_t frames) { return g ? 2.0 * gen_macs(g, true) * (double)frames : 0; }

static int gen_forward_body(dissc_gen_t g, const int64_t* code, const float* f0, const int64_t* spkr,
                            const int32_t* lengths, int B, int Tmax, float* wav_out, void* workspace,
                            hipStream_t stream);

int dissc_gen_forward(dissc_gen_t g, const int64_t* code, const float* f0, const int64_t* spkr,
                      const int32_t* lengths, int B, int Tmax, float* wav_out, void* workspace,
                      size_t workspace_bytes, void* stream_) {
  if (!g || !code || !wav_out || !workspace || (g->cfg.has_f0 && !f0) ||
      (g->cfg.has_spkr && !spkr)) {
    set_error("dissc_gen_forward: null argument");
    return DISSC_EINVAL;
  }
  OptScope opt_scope(&g->opt);  // the forward reads this handle's options only
  if (B <= 0 || Tmax <= 0) {
    set_error("dissc_gen_forward: B=%d Tmax=%d", B, Tmax);
    return DISSC_EINVAL;
  }
  if ((long long)Tmax * g->hop > 2000000000LL) {
    set_error("dissc_gen_forward: Tmax=%d too long", Tmax);
    return DISSC_EINVAL;
  }
  if (workspace_bytes < dissc_gen_workspace_bytes(g, B, Tmax)) {
    set_error("dissc_gen_forward: workspace %zu < %zu bytes", workspace_bytes,
              dissc_gen_workspace_bytes(g, B, Tmax));
    return DISSC_ENOMEM;
  }
  hipStream_t stream = (hipStream_t)stream_;
#if !DISSC_EXPERIMENTAL  // hipGraph replay failed its gate (slower than plain launches on ROCm 7.2): DISSC_EXPERIMENTAL=1 builds only
  return gen_forward_body(g, code, f0, spkr, lengths, B, Tmax, wav_out, workspace, stream);
#else
  if (!opts().graphs || g->graph_failures >= 2 || (long long)B * Tmax > opts().graph_frames)
    return gen_forward_body(g, code, f0, spkr, lengths, B, Tmax, wav_out, workspace, stream);
  // ---- small forward: replay (or first capture) its hipGraph ----
  for (auto& e : g->graphs)
    if (e.code == code && e.f0 == f0 && e.spkr == spkr && e.lengths == lengths && e.out == wav_out && e.ws == workspace &&
        e.B == B && e.T == Tmax) {
      e.stamp = ++g->graph_clock;
      ++g_graph_hits;
      DISSC_HIP_CHECK(hipGraphLaunch(e.exec, stream));
      return DISSC_OK;
    }
  if (!g->cap_stream && hipStreamCreateWithFlags(&g->cap_stream, hipStreamNonBlocking) != hipSuccess) {
    (void)hipGetLastError();
    return gen_forward_body(g, code, f0, spkr, lengths, B, Tmax, wav_out, workspace, stream);
  }
  // capture on the handle's own stream (the caller's may be the legacy default stream, which cannot capture); the side
  // streams join the capture through the events the body records and waits on, and all rejoin before it ends
  hipGraph_t graph = nullptr;
  hipGraphExec_t exec = nullptr;
  int rc = DISSC_EHIP;
  if (hipStreamBeginCapture(g->cap_stream, hipStreamCaptureModeThreadLocal) == hipSuccess) {
    rc = gen_forward_body(g, code, f0, spkr, lengths, B, Tmax, wav_out, workspace, g->cap_stream);
    const hipError_t e = hipStreamEndCapture(g->cap_stream, &graph);
    if (rc == DISSC_OK && (e != hipSuccess || !graph)) rc = DISSC_EHIP;
    if (rc == DISSC_OK && hipGraphInstantiate(&exec, graph, nullptr, nullptr, 0) != hipSuccess) rc = DISSC_EHIP;
    if (graph) (void)hipGraphDestroy(graph);
  }
  if (rc != DISSC_OK) {  // anything the capture cannot express: run it the plain way
    (void)hipGetLastError();
    ++g->graph_failures;
    return gen_forward_body(g, code, f0, spkr, lengths, B, Tmax, wav_out, workspace, stream);
  }
  // keep the eight most recently used graphs (the handle's options are frozen: a captured graph never goes stale)
  if (g->graphs.size() >= 8) {
    size_t old = 0;
    for (size_t i = 1; i < g->graphs.size(); ++i)
      if (g->graphs[i].stamp < g->graphs[old].stamp) old = i;
    (void)hipGraphExecDestroy(g->graphs[old].exec);
    g->graphs.erase(g->graphs.begin() + old);
  }
  ++g_graph_captures;
  g->graphs.push_back({code, f0, spkr, lengths, wav_out, workspace, B, Tmax, exec, ++g->graph_clock});
  DISSC_HIP_CHECK(hipGraphLaunch(exec, stream));
  return DISSC_OK;
#endif
}

static int gen_forward_body(dissc_gen_t g, const int64_t* code, const float* f0, const int64_t* spkr,
                            const int32_t* lengths, int B, int Tmax, float* wav_out, void* workspace,
                            hipStream_t stream) {
  const size_t nbuf = gen_buf_floats(g, B, Tmax);
  float* base = (float*)round_up((size_t)workspace, 256);
  float* X = base;
  float* ACC = base + nbuf;
  float* TMPj[DISSC_MAX_RK];
  float* XKj[DISSC_MAX_RK];
  ZeroSpans zs;
  for (int j = 0; j < g->cfg.num_kernels; ++j) {
    TMPj[j] = base + (size_t)(2 + 2 * j) * nbuf + BUF_GUARD;
    XKj[j] = base + (size_t)(3 + 2 * j) * nbuf;
    // the floats right in front of a scratch buffer are the left halo of its first row when a conv stages it by LDS-DMA:
    // zeroed by the forward's first kernel (embed_concat, on `stream` before the chains fork)
    zs.p[j] = TMPj[j] - ZERO_TAIL;
  }
  zs.n = g->cfg.num_kernels;
  float* TMP = TMPj[0];
  const bool multi = g->ev_x != nullptr;
  const DisscGenConfig& c = g->cfg;
  int rc;

  // 1. conditioning -> TMP [B, in_dim, ld0]
  const int ld0 = (int)round_up(Tmax, 4);
  launch_embed_concat(code, f0, spkr, g->dict_w, g->spkr_w, lengths, B, Tmax, c.embedding_dim,
                      c.has_f0, c.has_spkr, c.num_embeddings, c.num_speakers, TMP, ld0, zs, stream);
  // 2. conv_pre -> ACC [B, c0, ld0]
  Batch bt = batch_of(lengths, 1, B, Tmax);  // the batch at the current stage's rate
  if ((rc = run_conv(g->conv_pre, TMP, ACC, bt, EpiSpec(), c.model_in_dim, ld0, ld0, 1.0f, stream))) return rc;
  int ch = c.upsample_initial_channel, mul = 1, ld = ld0;
  const int nk = c.num_kernels;
  for (int i = 0; i < c.num_upsamples; ++i) {
    const int s = c.upsample_rates[i];
    const int ch_out = ch / 2, mul_out = mul * s;
    const int ld_out = (int)round_up((size_t)Tmax * mul_out, 4);
    // lrelu(0.1) -> ConvTranspose: ACC [B,ch,ld] -> X [B,ch_out,ld_out]
    // (phase groups write disjoint output phases: with side streams they run concurrently, which
    // fills the CUs better than two or three small grids one after the other)
    const int ngrp = (int)g->ups[i].size();
    const bool par_ups = multi && ngrp > 1 && ngrp <= nk;
    if (par_ups) DISSC_HIP_CHECK(hipEventRecord(g->ev_x, stream));  // ACC is complete
    for (int gi = 0; gi < ngrp; ++gi) {
      hipStream_t sg = (par_ups && gi > 0) ? g->aux[gi] : stream;
      if (par_ups && gi > 0) DISSC_HIP_CHECK(hipStreamWaitEvent(sg, g->ev_x, 0));
      if ((rc = run_conv(g->ups[i][gi], ACC, X, bt, EpiSpec(), ch, ld, ld_out, 0.1f, sg))) return rc;
      if (par_ups && gi > 0) {
        DISSC_HIP_CHECK(hipEventRecord(g->ev_fin[gi], sg));
        DISSC_HIP_CHECK(hipStreamWaitEvent(stream, g->ev_fin[gi], 0));
      }
    }
    ch = ch_out; mul = mul_out; ld = ld_out;
    bt = batch_of(lengths, mul, B, Tmax * mul);
    if (multi) DISSC_HIP_CHECK(hipEventRecord(g->ev_x, stream));  // X is ready
    for (int j = 0; j < nk; ++j) {
      hipStream_t sj = (multi && j > 0) ? g->aux[j] : stream;
      if (multi && j > 0) DISSC_HIP_CHECK(hipStreamWaitEvent(sj, g->ev_x, 0));
      const size_t cj = (size_t)i * nk + j;
      const ChainPlan& cp = g->plan[cj];
      const int rk = c.resblock_kernel_sizes[j];
      const int* dl = c.resblock_dilations[j];
      Bf3Block bf3;  // (bf3_* chains)
      bf3.C = ch; bf3.KS = rk; bf3.dil = dl; bf3.wpack = g->fused_w[cj]; bf3.bias = g->fused_b[cj];
      float* TMPc = multi ? TMPj[j] : TMPj[0];
      float* XKc = multi ? XKj[j] : XKj[0];
      const EpiSpec mrf = epi_of(mrf_epi(j, nk), nullptr, ACC, (float)nk);  // the chain's last launch (a two-conv pair adds its residual x_k)
      // the chains run concurrently up to the MRF update: the one launch of a chain that updates ACC waits for the previous chain
      auto acc_turn = [&]() -> int {
        if (multi && j > 0) DISSC_HIP_CHECK(hipStreamWaitEvent(sj, g->ev_fin[j - 1], 0));
        return DISSC_OK;
      };
      if (g->rb_type == 2) {
        // ResBlock2: x_1 = x + conv_d0(lrelu(x)) -> XK (a conv cannot run in place: its neighbours read the halo), then the
        // block's output x_1 + conv_d1(lrelu(x_1)) goes straight into the MRF update
        if (g->plan2[cj] == Rb2Form::fused) {  // the whole block in one launch, x_1 on the CU
          if ((rc = acc_turn()) || (rc = launch_resblock2(g->rb1[cj * 3], g->rb1[cj * 3 + 1], X, nullptr, bt, mrf, ld, 0.1f, sj))) return rc;
          if (multi) DISSC_HIP_CHECK(hipEventRecord(g->ev_fin[j], sj));
          continue;
        }
        if ((rc = run_conv(g->rb1[cj * 3], X, XKc, bt, epi_of(EPI_RES, X), ch, ld, ld, 0.1f, sj))) return rc;
        if ((rc = acc_turn()) ||
            (rc = run_conv(g->rb1[cj * 3 + 1], XKc, TMPc, bt, epi_of(mrf.epi, XKc, ACC, (float)nk), ch, ld, ld, 0.1f, sj)))
          return rc;
        if (multi) DISSC_HIP_CHECK(hipEventRecord(g->ev_fin[j], sj));
        continue;
      }
      if (cp.form == ChainForm::bf3_block) {  // the whole ResBlock in one launch
        if ((rc = acc_turn()) || (rc = launch_resblock_bf3(bf3, X, bt, mrf, ld, 0.1f, 0, 3, sj))) return rc;
        if (multi) DISSC_HIP_CHECK(hipEventRecord(g->ev_fin[j], sj));
        continue;
      }
      if (cp.form == ChainForm::f23_chain) {  // the whole ResBlock in one launch, x_1 / x_2 on the CU
        if ((rc = acc_turn()) || (rc = launch_reschain_f23(g->fused_w[cj], g->fused_b[cj], ch, X, nullptr, bt, mrf, ld, 0.1f, sj))) return rc;
        if (multi) DISSC_HIP_CHECK(hipEventRecord(g->ev_fin[j], sj));
        continue;
      }
      const float* x = X;  // the chain's running x_k: X -> XK -> TMP -> MRF update of ACC where pairs are one launch each
      for (int m = 0; m < 3; ++m) {
        const size_t idx = cj * 3 + m;
        const bool last = m == 2;
        float* nxt = x == XKc ? TMPc : XKc;  // (a one-launch pair cannot run in place: its neighbours read the halo)
        const PairForm pf = cp.pair[m].form;
        if (cp.form == ChainForm::bf3_pairs) {
          if (last && (rc = acc_turn())) return rc;
          rc = launch_resblock_bf3(bf3, x, bt, last ? mrf : epi_of(EPI_STORE, nullptr, nxt), ld, 0.1f, m, m + 1, sj);
          x = nxt;
        } else if (pf == PairForm::fused || pf == PairForm::fused_td) {
          if (last && (rc = acc_turn())) return rc;
          float* out = last ? nullptr : nxt;
          const EpiSpec ep = last ? mrf : epi_of(EPI_RES, nullptr, ACC, (float)nk);
          rc = pf == PairForm::fused_td ? launch_respair_wino(g->pw[idx], x, out, bt, ep, ld, 0.1f, sj)
                                        : launch_respair(g->rb1[idx], g->rb2[idx], x, out, bt, ep, ld, 0.1f, sj);
          x = nxt;
        } else {  // two conv launches, t through TMP, x_k updated in place
          const bool dma = pf == PairForm::direct_dma;
          const int ldt = dma ? (int)round_up((size_t)bt.Lmax + ZERO_TAIL, 4) : ld;
          EpiSpec ep_t = epi_of(dma ? EPI_STORE_ACT : EPI_STORE);  // t = conv_d(lrelu(x_k)), stored activated for the DMA form
          ep_t.out_slope = 0.1f;
          if ((rc = run_conv(g->rb1[idx], x, TMPc, bt, ep_t, ch, ld, ldt, 0.1f, sj))) return rc;
          if (last && (rc = acc_turn())) return rc;
          rc = run_conv(g->rb2[idx], TMPc, XKc, bt, epi_of(last ? mrf.epi : EPI_RES, x, ACC, (float)nk), ch, ldt, ld, dma ? 1.0f : 0.1f,
                        sj, dma ? 1 : 0);
          x = XKc;
        }
        if (rc) return rc;
      }
      if (multi) DISSC_HIP_CHECK(hipEventRecord(g->ev_fin[j], sj));
    }
    if (multi) DISSC_HIP_CHECK(hipStreamWaitEvent(stream, g->ev_fin[nk - 1], 0));  // stage output complete
  }
  // tail: lrelu(0.01) -> conv_post -> tanh
  launch_conv_post(ACC, g->post_w, g->post_b, lengths, mul, B, ch, g->post_KS, Tmax * mul, ld,
                   (long long)ch * ld, 0.01f, wav_out, Tmax * mul, stream);
  DISSC_HIP_CHECK(hipGetLastError());
  return DISSC_OK;
}

int dissc_wav_postprocess(float* wav, const int32_t* n_samples, int B, int ld, void* stream) {
  if (!wav || !n_samples || B <= 0) {
    set_error("dissc_wav_postprocess: bad argument");
    return DISSC_EINVAL;
  }
  launch_wav_postprocess(wav, n_samples, B, ld, (hipStream_t)stream);
  DISSC_HIP_CHECK(hipGetLastError());
  return DISSC_OK;
}

}  // extern "C"
