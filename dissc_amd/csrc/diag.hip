// Stand-alone entry points for tests and diagnostics: one conv, one transposed conv, one residual pair, one split-bf16 ResBlock per
// call (weights packed per call), what a shape would launch, and the per-launch benchmarks.  Host only: no kernel here.
#include <stdlib.h>

#include <algorithm>
#include <vector>

#include "gen_plan.h"

using namespace dissc;

namespace {

// What one entry packs and allocates on the device, released on every way out: up to two convs and a one-launch pair, scratch
// buffers, the two events of a benchmark.
struct DiagScope {
  DevConv c1, c2;
  DevPairW pw;
  DevS2tc tc;
  std::vector<float*> bufs;
  hipEvent_t e0 = nullptr, e1 = nullptr;
  hipError_t alloc(float** p, size_t n) {
    const hipError_t e = hipMalloc((void**)p, n * sizeof(float));
    if (e == hipSuccess) bufs.push_back(*p);
    return e;
  }
  hipError_t events() {
    const hipError_t e = hipEventCreate(&e0);
    return e != hipSuccess ? e : hipEventCreate(&e1);
  }
  ~DiagScope() {
    if (e0) (void)hipEventDestroy(e0);
    if (e1) (void)hipEventDestroy(e1);
    for (float* q : bufs) (void)hipFree(q);
    free_conv(c1);
    free_conv(c2);
    free_pairw(pw);
    free_s2tc(tc);
  }
};

// the synthetic data of the benchmarks: one LCG stream per call, weights then input
struct Lcg {
  uint32_t s = 12345u;
  void fill(std::vector<float>& v, float scale, float centre = 0.5f) {
    for (auto& x : v) {
      s = s * 1664525u + 1013904223u;
      x = ((s >> 8) / 16777216.0f - centre) * scale;
    }
  }
};

// warm twice, then the average ms of `iters` launches between the scope's two events
template <class Once>
int time_launches(const DiagScope& d, int iters, Once once, float* ms_out) {
  int rc = DISSC_OK;
  for (int it = 0; it < 2 && !rc; ++it) rc = once();
  if (rc) return rc;
  DISSC_HIP_CHECK(hipEventRecord(d.e0, nullptr));
  for (int it = 0; it < iters && !rc; ++it) rc = once();
  DISSC_HIP_CHECK(hipEventRecord(d.e1, nullptr));
  const hipError_t e = hipEventSynchronize(d.e1);
  float ms = 0.f;
  (void)hipEventElapsedTime(&ms, d.e0, d.e1);
  *ms_out = ms / iters;
  if (rc) return rc;
  DISSC_HIP_CHECK(e);
  return DISSC_OK;
}

// DISSC_TIMELINE: `bytes` of a device buffer into that file
void dump_timeline(const char* path, const float* dev, size_t bytes) {
  std::vector<char> hb(bytes);
  if (hipMemcpy(hb.data(), dev, hb.size(), hipMemcpyDeviceToHost) == hipSuccess)
    if (FILE* f = fopen(path, "wb")) {
      fwrite(hb.data(), 1, hb.size(), f);
      fclose(f);
    }
}

}  // namespace

extern "C" {

// ---- stand-alone conv entry points (weights packed per call: tests only) ----------------
// what a synchronous entry returns: its launches' code, or the error the drained stream reports
static int drained(int rc, hipStream_t stream) {
  const hipError_t e = hipStreamSynchronize(stream);
  if (rc) return rc;
  DISSC_HIP_CHECK(e);
  return DISSC_OK;
}

static int conv_once(DevConv& dc, const float* x, float* y, const Batch& bt, int ldx, int ldo, float in_slope, hipStream_t stream) {
  const int rc = drained(run_conv(dc, x, y, bt, EpiSpec(), dc.CIN, ldx, ldo, in_slope, stream), stream);
  free_conv(dc);
  return rc;
}

// prec = 1: the layer must come out of conv_geometry under PrecScope(1) as a split-bf16 one -- the very function make_conv packs
// by -- or the entry refuses, before anything is packed or uploaded: a test of conv_bf3_kernel never runs fp32 unnoticed
static int prec_available(const char* who, int prec, int Cout, int Cin, int k, int dilation) {
  if (prec != 1) return DISSC_OK;
  DevConv dc;  // geometry only
  PrecScope prec_scope(1);
  conv_geometry(dc, Cout, Cin, k, dilation, 1, 1, -1);
  if (dc.prec != 1) {
    set_error("%s: no split-bf16 instance for %d rows, k = %d, dilation %d (>= 32 rows, taps spanning <= %d columns, not the big "
              "1x1 layers)", who, dc.M, dc.KS, dc.dil, MAX_TAP_SPAN);
    return DISSC_EINVAL;
  }
  return DISSC_OK;
}

int dissc_conv1d_prec(const float* x, const float* w_host, const float* bias_host, float* y, const int32_t* lengths, int B, int Cin,
                      int Cout, int k, int dilation, int ldx, int ldo, int Lmax, float in_slope, int prec, void* stream) {
  if (!x || !w_host || !y || k % 2 != 1 || dilation < 1 || (prec != 0 && prec != 1)) {
    set_error("dissc_conv1d: bad argument (prec %d: 0 = fp32, 1 = split-bf16)", prec);
    return DISSC_EINVAL;
  }
  int rc = prec_available("dissc_conv1d_prec", prec, Cout, Cin, k, dilation);
  if (rc) return rc;
  // "wino" / "wino8" / "wino8_r4" = 2: this entry takes the transform-domain forms too (tests)
  DevConv dc;
  {
    PrecScope prec_scope(prec);
    if (!prec && opts().wino8 >= 2 && wino8_supported(Cout, Cin, k, dilation))
      rc = make_wino8(w_host, bias_host, Cout, k, dilation, dc, opts().wino8_r4 >= 2 && wino8_r4_supported(Cout, k, dilation) ? 4 : 3);
    else if (!prec && opts().wino >= 2 && wino_supported(Cout, Cin, k, dilation))
      rc = make_wino(w_host, bias_host, Cout, k, dilation, dc);
    else
      rc = make_conv(w_host, bias_host, Cout, Cin, k, dilation, dc);
  }
  if (rc) return rc;
  return conv_once(dc, x, y, batch_of(lengths, 1, B, Lmax), ldx, ldo, in_slope, (hipStream_t)stream);
}

int dissc_conv1d(const float* x, const float* w_host, const float* bias_host, float* y, const int32_t* lengths, int B, int Cin,
                 int Cout, int k, int dilation, int ldx, int ldo, int Lmax, float in_slope, void* stream) {
  return dissc_conv1d_prec(x, w_host, bias_host, y, lengths, B, Cin, Cout, k, dilation, ldx, ldo, Lmax, in_slope, 0, stream);
}

// Diagnostics / tests: ONE residual pair y = x + conv_1(lrelu(conv_d(lrelu(x)))) (or its MRF modes) on device data with
// host weights, through a chosen implementation: mode 0 = two direct conv launches, 1 = the fused direct pair
// (respair.hip), 2 = two conv_wino launches, 3 = the fused transform-domain pair (pair_host.hip), 4 = two transform-domain
// launches in the forms the plan gives a PairForm::td pair of the shape (td_conv_form), 5 = two direct launches packed for
// split-bf16 (conv_bf3_kernel: how the 128- and 256-channel pairs run under "precision" = 1).  Synchronous.
static int pair_run(int mode, const DiagScope& d, const float* x, float* tmp, float* y, const Batch& bt, const EpiSpec& ep, int C,
                    int ld, float slope, hipStream_t st) {
  int rc;
  switch (mode) {
    case 0: case 2: case 4: case 5:  // two launches, t through tmp
      if ((rc = run_conv(d.c1, x, tmp, bt, EpiSpec(), C, ld, ld, slope, st))) return rc;
      return run_conv(d.c2, tmp, y, bt, epi_of(ep.epi, x, ep.acc, ep.mrf_div), C, ld, ld, slope, st);
    case 1:
      return launch_respair(d.c1, d.c2, x, y, bt, ep, ld, slope, st);
    case 3:
      return launch_respair_wino(d.pw, x, y, bt, ep, ld, slope, st);
    default:
      set_error("pair mode %d", mode);
      return DISSC_EINVAL;
  }
}

static int pair_make(int mode, const float* w1, const float* b1, const float* w2, const float* b2, int C, int k, int d, DiagScope& ds) {
  DevConv &c1 = ds.c1, &c2 = ds.c2;
  int rc;
  if (mode == 2) {
    if (!wino_supported(C, C, k, d) && !(C == 32 && (k == 3 || k == 7 || k == 11) && (d == 1 || d == 3 || d == 5))) {
      set_error("pair mode 2: no conv_wino instance for C = %d, k = %d, d = %d", C, k, d);
      return DISSC_EINVAL;
    }
    if ((rc = make_wino(w1, b1, C, k, d, c1))) return rc;
    return make_wino(w2, b2, C, k, 1, c2);
  }
  if (mode == 3) return make_pairw(w1, b1, w2, b2, C, k, d, pair_reg_form(C, k, d), ds.pw);
  if (mode == 4) {
    if (!wino_supported(C, C, k, d) || !wino_supported(C, C, k, 1)) {
      set_error("pair mode 4: no transform-domain conv instance for C = %d, k = %d, d = %d", C, k, d);
      return DISSC_EINVAL;
    }
    if ((rc = make_pair_conv(td_conv_form(C, k, d), w1, b1, C, k, d, c1))) return rc;
    return make_pair_conv(td_conv_form(C, k, 1), w2, b2, C, k, 1, c2);
  }
  if (mode == 5 && ((rc = prec_available("pair mode 5", 1, C, C, k, d)) || (rc = prec_available("pair mode 5", 1, C, C, k, 1)))) return rc;
  PrecScope prec_scope(mode == 5 ? 1 : 0);
  if ((rc = make_conv(w1, b1, C, C, k, d, c1))) return rc;
  return make_conv(w2, b2, C, C, k, 1, c2);
}

int dissc_respair1d(const float* x, const float* w1_host, const float* b1_host, const float* w2_host, const float* b2_host,
                    float* y, float* acc, const int32_t* lengths, int B, int C, int k, int dilation, int ld, int Lmax,
                    float slope, int epi, float mrf_div, int mode, void* stream) {
  if (!x || !w1_host || !w2_host || !y || k % 2 != 1 || dilation < 1 || B <= 0 || epi < EPI_RES || epi > EPI_MRF_DIV ||
      (epi != EPI_RES && !acc)) {
    set_error("dissc_respair1d: bad argument");
    return DISSC_EINVAL;
  }
  DiagScope ds;
  float* tmp = nullptr;
  int rc = pair_make(mode, w1_host, b1_host, w2_host, b2_host, C, k, dilation, ds);
  if (!rc && (mode == 0 || mode == 2 || mode == 4 || mode == 5) && ds.alloc(&tmp, (size_t)B * C * ld) != hipSuccess) {
    set_error("dissc_respair1d: hipMalloc");
    rc = DISSC_ENOMEM;
  }
  if (!rc)
    rc = pair_run(mode, ds, x, tmp, y, batch_of(lengths, 1, B, Lmax), epi_of(epi, nullptr, acc, mrf_div), C, ld, slope, (hipStream_t)stream);
  return drained(rc, (hipStream_t)stream);
}

// Diagnostics / tests: ONE ResBlock2, y1 = x + conv_d0(lrelu(x)), y2 = y1 + conv_d1(lrelu(y1)), on device data with host weights
// [C, C, k] and biases [C] packed per call: y (epi = EPI_RES) or acc (the MRF modes) = the block's output.  mode 0 = two direct
// conv launches, y1 through scratch; mode 1 = the one-launch kernel (resblock2.hip), which refuses a shape without an instance
// before anything is packed.  Synchronous.
static int rb2_run(int mode, const DiagScope& d, const float* x, float* y1, float* y, const Batch& bt, const EpiSpec& ep, int C, int ld,
                   float slope, hipStream_t st) {
  if (mode == 1) return launch_resblock2(d.c1, d.c2, x, y, bt, ep, ld, slope, st);
  if (int rc = run_conv(d.c1, x, y1, bt, epi_of(EPI_RES, x), C, ld, ld, slope, st)) return rc;
  return run_conv(d.c2, y1, y, bt, epi_of(ep.epi, y1, ep.acc, ep.mrf_div), C, ld, ld, slope, st);
}

int dissc_resblock2_1d(const float* x, const float* w1_host, const float* b1_host, const float* w2_host, const float* b2_host, float* y,
                       float* acc, const int32_t* lengths, int B, int C, int k, int d0, int d1, int ld, int Lmax, float slope, int epi,
                       float mrf_div, int mode, void* stream) {
  if (!x || !w1_host || !w2_host || !y || k % 2 != 1 || d0 < 1 || d1 < 1 || B <= 0 || C < 1 || epi < EPI_RES || epi > EPI_MRF_DIV ||
      (epi != EPI_RES && !acc) || (mode != 0 && mode != 1) || (k - 1) * std::max(d0, d1) > RB_TAP_SPAN) {
    set_error("dissc_resblock2_1d: bad argument (mode 0 = two launches, 1 = one launch; (k - 1) x dilation <= %d)", RB_TAP_SPAN);
    return DISSC_EINVAL;
  }
  if (mode == 1 && !resblock2_supported(C, k, d0, d1)) {
    set_error("dissc_resblock2_1d: no one-launch instance for C = %d, k = %d, dilations (%d, %d)", C, k, d0, d1);
    return DISSC_EINVAL;
  }
  DiagScope ds;
  float* y1 = nullptr;
  hipStream_t st = (hipStream_t)stream;
  const Batch bt = batch_of(lengths, 1, B, Lmax);
  int rc = make_conv(w1_host, b1_host, C, C, k, d0, ds.c1);
  if (!rc) rc = make_conv(w2_host, b2_host, C, C, k, d1, ds.c2);
  if (!rc && mode == 0 && ds.alloc(&y1, (size_t)B * C * ld) != hipSuccess) {
    set_error("dissc_resblock2_1d: hipMalloc");
    rc = DISSC_ENOMEM;
  }
  if (!rc) rc = rb2_run(mode, ds, x, y1, y, bt, epi_of(epi, nullptr, acc, mrf_div), C, ld, slope, st);
  return drained(rc, st);
}

// Per-launch benchmark of one ResBlock2 in either form (dissc_resblock2_1d's modes) on B synthetic utterances of L columns:
// dissc_pair_bench's method (two warm-up runs, then the average of `iters` runs between two events).  Synchronous.
int dissc_resblock2_bench(int B, int C, int k, int d0, int d1, int L, int epi, int iters, int mode, float* ms_out) {
  if (!ms_out || B <= 0 || L <= 0 || iters <= 0 || C < 1 || k % 2 != 1 || d0 < 1 || d1 < 1 || epi < EPI_RES || epi > EPI_MRF_DIV ||
      (mode != 0 && mode != 1) || (k - 1) * std::max(d0, d1) > RB_TAP_SPAN || (mode == 1 && !resblock2_supported(C, k, d0, d1))) {
    set_error("dissc_resblock2_bench: bad argument, or no one-launch instance for mode 1");
    return DISSC_EINVAL;
  }
  std::vector<float> w1((size_t)C * C * k), w2((size_t)C * C * k), bias(C, 0.1f);
  Lcg rnd;
  rnd.fill(w1, 0.05f);
  rnd.fill(w2, 0.05f);
  DiagScope ds;
  int rc = make_conv(w1.data(), bias.data(), C, C, k, d0, ds.c1);
  if (!rc) rc = make_conv(w2.data(), bias.data(), C, C, k, d1, ds.c2);
  if (rc) return rc;
  const int ld = (L + 3) / 4 * 4;
  const size_t n = (size_t)B * C * ld;
  float *x = nullptr, *y = nullptr, *t = nullptr, *a = nullptr;
  std::vector<float> hx(n);
  rnd.fill(hx, 2.f);
  if (ds.alloc(&x, n) != hipSuccess || ds.alloc(&y, n) != hipSuccess || ds.alloc(&t, n) != hipSuccess ||
      ds.alloc(&a, n) != hipSuccess || hipMemcpy(x, hx.data(), n * 4, hipMemcpyHostToDevice) != hipSuccess ||
      hipMemset(a, 0, n * 4) != hipSuccess || ds.events() != hipSuccess) {
    set_error("dissc_resblock2_bench: allocation failed");
    return DISSC_ENOMEM;
  }
  const Batch bt = batch_of(nullptr, 1, B, L);
  const EpiSpec ep = epi_of(epi, nullptr, a, 3.f);
  return time_launches(ds, iters, [&]() { return rb2_run(mode, ds, x, t, y, bt, ep, C, ld, 0.1f, nullptr); }, ms_out);
}

// Diagnostics: the form a (C; k; d0, d1) ResBlock2 takes in an fp32 generator handle created under the current option defaults
// (0 = two direct conv launches, 1 = one launch) and, for the one-launch form, the outputs a workgroup owns (else 0); DISSC_EINVAL
// for a block no handle takes.  Host only: no HIP call.
int dissc_resblock2_info(int C, int k, int d0, int d1, int* form_out, int* tile_out) {
  if (C < 1 || k < 1 || k % 2 != 1 || d0 < 1 || d1 < 1 || (k - 1) * std::max(d0, d1) > RB_TAP_SPAN) {
    set_error("dissc_resblock2_info: C = %d, k = %d, dilations (%d, %d): k odd, (k - 1) x dilation within 0 .. %d", C, k, d0, d1, RB_TAP_SPAN);
    return DISSC_EINVAL;
  }
  const int form = plan_resblock2(C, k, d0, d1, 0) == Rb2Form::fused ? 1 : 0;
  if (form_out) *form_out = form;
  if (tile_out) *tile_out = form ? resblock2_tile(k, d0, d1) : 0;
  return DISSC_OK;
}

// Diagnostics / tests: ONE k = 3 ResBlock -- three residual pairs, dilations dil3 -- on device data with host weights [C,C,k] and
// biases [C] in execution order (c1_0, c2_0, c1_1, c2_1, c1_2, c2_2): y (EPI_RES) or acc (the MRF modes) = the block's output.
// mode 0 = three launches, each pair in the one-launch form the generator gives it without "chain_f23" (the register-only form
// pair_reg_form names, else the direct fused pair), x_1 / x_2 through scratch; mode 1 = the one-launch F(2,3) chain
// (reschain32/16_f23_kernel), which refuses a shape without an instance before anything is packed or written.  Synchronous.
struct ChainDiag {
  DiagScope pair[3];
  int pmode[3] = {0, 0, 0};
  float *w = nullptr, *b = nullptr, *s1 = nullptr, *s2 = nullptr;
  ~ChainDiag() {
    for (float* q : {w, b, s1, s2})
      if (q) (void)hipFree(q);
  }
};
static int chain_make(int mode, const float* const* w6, const float* const* b6, int C, int k, const int* dil, size_t scratch_floats,
                      ChainDiag& cd) {
  if (mode == 1) {
    if (!chain_f23_supported(C, k, dil)) {
      set_error("chain mode 1: no instance for C = %d, k = %d, dilations (%d, %d, %d)", C, k, dil[0], dil[1], dil[2]);
      return DISSC_EINVAL;
    }
    return make_chain_f23(w6, b6, C, &cd.w, &cd.b);
  }
  if (mode != 0) {
    set_error("chain mode %d", mode);
    return DISSC_EINVAL;
  }
  for (int m = 0; m < 3; ++m) {
    cd.pmode[m] = pair_reg_form(C, k, dil[m]) ? 3 : 1;
    if (cd.pmode[m] == 1 && !respair_supported(C, k, dil[m])) {
      set_error("chain mode 0: no one-launch pair for C = %d, k = %d, dilation %d", C, k, dil[m]);
      return DISSC_EINVAL;
    }
    const int rc = pair_make(cd.pmode[m], w6[2 * m], b6[2 * m], w6[2 * m + 1], b6[2 * m + 1], C, k, dil[m], cd.pair[m]);
    if (rc) return rc;
  }
  if (hipMalloc(&cd.s1, scratch_floats * sizeof(float)) != hipSuccess || hipMalloc(&cd.s2, scratch_floats * sizeof(float)) != hipSuccess) {
    set_error("chain mode 0: hipMalloc");
    return DISSC_ENOMEM;
  }
  return DISSC_OK;
}
static int chain_run(int mode, const ChainDiag& cd, const float* x, float* y, const Batch& bt, const EpiSpec& ep, int C, int ld, float slope,
                     hipStream_t st) {
  if (mode == 1) return launch_reschain_f23(cd.w, cd.b, C, x, y, bt, ep, ld, slope, st);
  int rc = pair_run(cd.pmode[0], cd.pair[0], x, nullptr, cd.s1, bt, epi_of(EPI_RES), C, ld, slope, st);
  if (!rc) rc = pair_run(cd.pmode[1], cd.pair[1], cd.s1, nullptr, cd.s2, bt, epi_of(EPI_RES), C, ld, slope, st);
  if (!rc) rc = pair_run(cd.pmode[2], cd.pair[2], cd.s2, nullptr, y, bt, ep, C, ld, slope, st);
  return rc;
}

int dissc_reschain1d(const float* x, const float* const* w6_host, const float* const* b6_host, float* y, float* acc, const int32_t* lengths,
                     int B, int C, int k, const int32_t* dil3, int ld, int Lmax, float slope, int epi, float mrf_div, int mode,
                     void* stream) {
  if (!x || !w6_host || !b6_host || !dil3 || B <= 0 || Lmax <= 0 || ld < Lmax || epi < EPI_RES || epi > EPI_MRF_DIV ||
      (epi == EPI_RES ? !y || y == x : !acc || acc == x)) {
    set_error("dissc_reschain1d: bad argument");
    return DISSC_EINVAL;
  }
  for (int l = 0; l < 6; ++l)
    if (!w6_host[l] || !b6_host[l]) {
      set_error("dissc_reschain1d: weight or bias %d is null", l);
      return DISSC_EINVAL;
    }
  const int dil[3] = {dil3[0], dil3[1], dil3[2]};
  ChainDiag cd;
  int rc = chain_make(mode, w6_host, b6_host, C, k, dil, (size_t)B * C * ld, cd);
  if (!rc) rc = chain_run(mode, cd, x, y, batch_of(lengths, 1, B, Lmax), epi_of(epi, nullptr, acc, mrf_div), C, ld, slope, (hipStream_t)stream);
  return drained(rc, (hipStream_t)stream);
}

// Diagnostics: the geometry of the one-launch chain of a (C, k, dil3) block.  Host only: no HIP call.
int dissc_chain_info(int C, int k, const int32_t* dil3, DisscChainInfo* out) {
  ChainInfo ci;
  const int dil[3] = {dil3 ? dil3[0] : 0, dil3 ? dil3[1] : 0, dil3 ? dil3[2] : 0};
  if (!chain_f23_info(C, k, dil, ci)) {
    set_error("dissc_chain_info: no instance for C = %d, k = %d, dilations (%d, %d, %d)", C, k, dil[0], dil[1], dil[2]);
    return DISSC_EINVAL;
  }
  if (out) {
    out->wout = ci.wout; out->span = ci.span; out->halo = ci.halo; out->lds_bytes = ci.lds_bytes; out->tiles_per_wave = ci.tiles_per_wave;
  }
  return DISSC_OK;
}

// Diagnostics: average ms of `iters` launches of one k = 3, dilations (1, 3, 5) block (modes as dissc_reschain1d) on synthetic data.
int dissc_chain_bench(int B, int C, int L, int epi, int iters, int mode, float* ms_out) {
  if (!ms_out || B <= 0 || L <= 0 || iters <= 0 || epi < EPI_RES || epi > EPI_MRF_DIV) {
    set_error("dissc_chain_bench: bad argument");
    return DISSC_EINVAL;
  }
  const int k = 3, dil[3] = {1, 3, 5};
  std::vector<float> w[6], bias(C, 0.1f);
  const float *w6[6], *b6[6];
  Lcg rnd;
  for (int l = 0; l < 6; ++l) {
    w[l].resize((size_t)C * C * k);
    rnd.fill(w[l], 0.05f);
    w6[l] = w[l].data();
    b6[l] = bias.data();
  }
  const int ld = (L + 3) / 4 * 4;
  const size_t n = (size_t)B * C * ld;
  ChainDiag cd;
  int rc = chain_make(mode, w6, b6, C, k, dil, n, cd);
  if (rc) return rc;
  DiagScope ds;
  float *x = nullptr, *y = nullptr, *a = nullptr;
  std::vector<float> hx(n);
  rnd.fill(hx, 2.f);
  if (ds.alloc(&x, n) != hipSuccess || ds.alloc(&y, n) != hipSuccess || ds.alloc(&a, n) != hipSuccess ||
      hipMemcpy(x, hx.data(), n * 4, hipMemcpyHostToDevice) != hipSuccess || hipMemset(a, 0, n * 4) != hipSuccess ||
      ds.events() != hipSuccess) {
    set_error("dissc_chain_bench: allocation failed");
    return DISSC_ENOMEM;
  }
  const Batch bt = batch_of(nullptr, 1, B, L);
  const EpiSpec ep = epi_of(epi, nullptr, a, 3.f);
  return time_launches(ds, iters, [&]() { return chain_run(mode, cd, x, y, bt, ep, C, ld, 0.1f, nullptr); }, ms_out);
}

// Diagnostics / tests: residual pairs [m0, m1) of ONE ResBlock1 in split-bf16 arithmetic on resblock_bf3_kernel, as the generator
// launches it under "precision" = 1: the whole block (m0 = 0, m1 = 3) or a pair at a time, chained through EPI_STORE.  x / acc on
// the device, the six weights [C,C,k] and biases [C] on the host in execution order (c1_0, c2_0, c1_1, c2_1, c1_2, c2_2).  Synchronous.
int dissc_resblock1d_bf3(const float* x, const float* const* w6_host, const float* const* b6_host, float* acc, const int32_t* lengths,
                         int B, int C, int k, const int32_t* dil3, int ld, int Lmax, float slope, int epi, float mrf_div, int m0, int m1,
                         void* stream) {
  if (!x || !w6_host || !b6_host || !acc || !dil3 || x == acc) {
    set_error("dissc_resblock1d_bf3: bad argument (null pointer, or acc aliasing x)");
    return DISSC_EINVAL;
  }
  for (int l = 0; l < 6; ++l)
    if (!w6_host[l] || !b6_host[l]) {
      set_error("dissc_resblock1d_bf3: weight or bias %d is null", l);
      return DISSC_EINVAL;
    }
  const int dil[3] = {dil3[0], dil3[1], dil3[2]};
  ResblockBf3Plan plan;  // refuses an unsupported (C, k, dil) or [m0, m1) before anything is packed or uploaded
  int rc = resblock_bf3_plan(C, k, dil, m0, m1, plan);
  if (rc) return rc;
  std::vector<float> fw, fb;
  pack_resblock_bf3(C, k, w6_host, fw);
  for (int l = 0; l < 6; ++l) fb.insert(fb.end(), b6_host[l], b6_host[l] + C);
  DiagScope ds;
  float *dw = nullptr, *db = nullptr;
  if (ds.alloc(&dw, fw.size()) != hipSuccess || ds.alloc(&db, fb.size()) != hipSuccess) {
    set_error("dissc_resblock1d_bf3: hipMalloc");
    return DISSC_ENOMEM;
  }
  DISSC_HIP_CHECK(hipMemcpy(dw, fw.data(), fw.size() * sizeof(float), hipMemcpyHostToDevice));
  DISSC_HIP_CHECK(hipMemcpy(db, fb.data(), fb.size() * sizeof(float), hipMemcpyHostToDevice));
  Bf3Block blk;
  blk.C = C; blk.KS = k; blk.dil = dil; blk.wpack = dw; blk.bias = db;
  rc = launch_resblock_bf3(blk, x, batch_of(lengths, 1, B, Lmax), epi_of(epi, nullptr, acc, mrf_div), ld, slope, m0, m1,
                           (hipStream_t)stream);
  return drained(rc, (hipStream_t)stream);
}

// Diagnostics: what the split-bf16 kernels of the generator would launch, from the planning functions the launches themselves call.
// dil3 == NULL: the conv_bf3_kernel tile of a Cin -> Cout conv of k taps and `dilation` (for a ConvTranspose phase group: its GEMM
// rows and taps, dissc_conv_info) on B utterances of at most Lmax columns under the current option defaults; DISSC_EINVAL where
// the layer gets no split-bf16 instance.  dil3 != NULL: the resblock_bf3_kernel window of pairs [m0, m1) of a block of C = Cout
// channels.  Host only: no HIP call.
int dissc_bf3_info(int Cout, int Cin, int k, int dilation, int B, int Lmax, const int32_t* dil3, int m0, int m1, DisscBf3Info* out) {
  DisscBf3Info o = {};
  if (!dil3) {
    if (Cin < 1 || Cout < 1 || k < 1 || dilation < 1) {
      set_error("dissc_bf3_info: bad argument");
      return DISSC_EINVAL;
    }
    int rc = prec_available("dissc_bf3_info", 1, Cout, Cin, k, dilation);
    ConvBf3Plan p;
    if (!rc) rc = conv_bf3_plan(Cout, k, dilation, 1, B, Lmax, p);
    if (rc) return rc;
    o.bm = p.BM; o.bn = p.BN; o.small_grid = p.small; o.tile = p.tile;
  } else {
    const int dil[3] = {dil3[0], dil3[1], dil3[2]};
    ResblockBf3Plan p;
    const int rc = resblock_bf3_plan(Cout, k, dil, m0, m1, p);
    if (rc) return rc;
    o.bn = p.BN; o.cols = p.COLS; o.h4 = p.H4; o.pad = p.PAD;
  }
  if (out) *out = o;
  return DISSC_OK;
}

// Diagnostics: the form and tile of what mode 3 of dissc_respair1d / dissc_pair_bench builds under the current option
// defaults.  Host only: no HIP call.
int dissc_pair_info(int C, int k, int dilation, int* form_out, int* tile_out) {
  const int form = pair_reg_form(C, k, dilation);
  if (!pair_form_supported(form, C, k, dilation)) {
    set_error("dissc_pair_info: no instance for C = %d, k = %d, dilation %d", C, k, dilation);
    return DISSC_EINVAL;
  }
  if (form_out) *form_out = form;
  if (tile_out) *tile_out = pair_reg_tile(form, C, k, dilation);
  return DISSC_OK;
}

// Diagnostics: the launches dissc_conv1d (up == 1) / dissc_conv_transpose1d (up > 1: k taps, stride up) make for a layer on a
// batch of B utterances of at most Lmax_out columns per launch, under the current option defaults: the planning functions of
// make_conv / make_convT / run_conv / launch_conv themselves, without packing or uploading anything.  Host only: no HIP call.
int dissc_conv_info(int Cin, int Cout, int k, int dilation, int up, int B, int Lmax_out, DisscConvLaunch* out, int max_out,
                    int* n_out) {
  if (Cin < 1 || Cout < 1 || k < 1 || dilation < 1 || up < 1 || B < 1 || Lmax_out < 1 || max_out < 0 || (max_out && !out) ||
      (up == 1 && k % 2 != 1) || (up > 1 && ((k - up) % 2 != 0 || k < up || dilation != 1))) {
    set_error("dissc_conv_info: bad argument");
    return DISSC_EINVAL;
  }
  std::vector<ConvTGroup> plan;
  if (up > 1) convT_groups(Cout, k, up, plan);
  else plan.push_back(ConvTGroup{0, 1, 0, k});
  int n = 0;
  for (const ConvTGroup& g : plan) {
    DevConv dc;  // geometry only: nothing is uploaded, nothing to free
    conv_geometry(dc, Cout * g.np, Cin, g.ntap, up > 1 ? 1 : dilation, 1, 1, up > 1 ? -g.dlo : -1);
    int family, cfg, bm, bn;
    const int rc = conv_launch_info(dc, B, Lmax_out, &family, &cfg, &bm, &bn);
    if (rc) return rc;
    if (n < max_out) {
      DisscConvLaunch& o = out[n];
      o.family = family; o.cfg = cfg; o.bm = bm; o.bn = bn; o.rows = dc.M;
      o.p0 = g.p0; o.np = g.np; o.ntap = g.ntap;
      o.pad_left = dc.pad_left >= 0 ? dc.pad_left : ((dc.KS - 1) * dc.dil) / 2;
    }
    ++n;
  }
  if (n_out) *n_out = n;
  return DISSC_OK;
}

// Diagnostics: the conv_wino8_kernel instance and grid a k = 7 / 11 (or the k = 3) conv of C channels launches as F(6,3) (R = 3) or
// F(5,4) (R = 4) on a batch of B utterances of at most Lmax columns, under the current option defaults: wino8_plan, which
// run_wino8 launches from.  Host only: no HIP call.
int dissc_wino8_info(int C, int k, int dilation, int R, int B, int Lmax, DisscWino8Plan* out) {
  Wino8Plan p;
  const int rc = wino8_plan(C, k, dilation, R, B, Lmax, p);
  if (rc) return rc;
  if (out) {
    out->mi = p.MI; out->ni = p.NI; out->wps = p.WPS; out->r = p.R; out->ns = p.NS;
    out->unit = p.unit; out->ot = p.OT; out->cpr = p.CPR; out->gx = p.gx; out->gy = p.gy;
  }
  return DISSC_OK;
}

// Diagnostics: which form of that instance the launch takes under the current option defaults ("wino8_sv"): 1 = the transform shared
// between the waves (conv_wino8_kernel<.., SHV = true>), 0 = private V tiles.  wino8_plan_shared, which run_wino8 launches from.  Host only.
int dissc_wino8_form(int C, int k, int dilation, int R, int B, int Lmax, int* shared_out) {
  Wino8Plan p;
  const int rc = wino8_plan(C, k, dilation, R, B, Lmax, p);
  if (rc) return rc;
  if (shared_out) *shared_out = wino8_plan_shared(p) ? 1 : 0;
  return DISSC_OK;
}

// Diagnostics: the conv_wino_kernel instance and grid a C -> C conv of (k, dilation) launches in its six-point F(4,3) form on a batch of
// B utterances of at most Lmax columns, under the current option defaults: wino_plan, which run_wino launches from.  Host only: no
// HIP call.
int dissc_wino_info(int C, int k, int dilation, int B, int Lmax, DisscWinoPlan* out) {
  WinoPlan p;
  const int rc = wino_plan(C, k, dilation, B, Lmax, p);
  if (rc) return rc;
  if (out) {
    out->ns = p.NS; out->dilation = p.dil; out->cpr = p.CPR; out->rh = p.RH; out->tw = p.TW; out->shv = p.SHV;
    out->unit = p.unit; out->ot = p.OT; out->gx = p.gx; out->gy = p.gy; out->wgs = p.wgs; out->lds_bytes = p.lds_bytes;
  }
  return DISSC_OK;
}

// Diagnostics: average ms of `iters` launches of one residual pair (modes as dissc_respair1d) on synthetic data.
int dissc_pair_bench(int B, int C, int k, int dilation, int L, int epi, int iters, int mode, float* ms_out) {
  if (!ms_out || B <= 0 || L <= 0 || iters <= 0 || epi < EPI_RES || epi > EPI_MRF_DIV) {
    set_error("dissc_pair_bench: bad argument");
    return DISSC_EINVAL;
  }
  std::vector<float> w1((size_t)C * C * k), w2((size_t)C * C * k), bias(C, 0.1f);
  Lcg rnd;
  rnd.fill(w1, 0.05f);
  rnd.fill(w2, 0.05f);
  DiagScope ds;
  int rc = pair_make(mode, w1.data(), bias.data(), w2.data(), bias.data(), C, k, dilation, ds);
  if (rc) return rc;
  const int ld = (L + 3) / 4 * 4;
  const size_t n = (size_t)B * C * ld;
  float *x = nullptr, *y = nullptr, *t = nullptr, *a = nullptr;
  std::vector<float> hx(n);
  rnd.fill(hx, 2.f);
  if (ds.alloc(&x, n) != hipSuccess || ds.alloc(&y, n) != hipSuccess || ds.alloc(&t, n) != hipSuccess ||
      ds.alloc(&a, n) != hipSuccess || hipMemcpy(x, hx.data(), n * 4, hipMemcpyHostToDevice) != hipSuccess ||
      hipMemset(a, 0, n * 4) != hipSuccess || ds.events() != hipSuccess) {
    set_error("dissc_pair_bench: allocation failed");
    return DISSC_ENOMEM;
  }
  const Batch bt = batch_of(nullptr, 1, B, L);
  const EpiSpec ep = epi_of(epi, nullptr, a, 3.f);
  return time_launches(ds, iters, [&]() { return pair_run(mode, ds, x, t, y, bt, ep, C, ld, 0.1f, nullptr); }, ms_out);
}

int dissc_conv_transpose1d_prec(const float* x, const float* w_host, const float* bias_host, float* y, const int32_t* lengths, int B,
                                int Cin, int Cout, int k, int stride, int ldx, int ldo, int Lmax, float in_slope, int prec,
                                void* stream) {
  if (!x || !w_host || !y || stride < 1 || (k - stride) % 2 != 0 || (prec != 0 && prec != 1)) {
    set_error("dissc_conv_transpose1d: bad argument (prec %d: 0 = fp32, 1 = split-bf16)", prec);
    return DISSC_EINVAL;
  }
  std::vector<ConvTGroup> plan;
  convT_groups(Cout, k, stride, plan);
  int rc = DISSC_OK;
  for (const ConvTGroup& g : plan)  // every phase group, before anything is packed
    if (!rc) rc = prec_available("dissc_conv_transpose1d_prec", prec, Cout * g.np, Cin, g.ntap, 1);
  if (rc) return rc;
  std::vector<DevConv> grp;
  {
    PrecScope prec_scope(prec);
    rc = make_convT(w_host, bias_host, Cin, Cout, k, stride, grp);
  }
  for (auto& dc : grp) {
    int r2 = rc ? rc : conv_once(dc, x, y, batch_of(lengths, 1, B, Lmax), ldx, ldo, in_slope, (hipStream_t)stream);
    if (rc) free_conv(dc);
    rc = rc ? rc : r2;
  }
  return rc;
}

int dissc_conv_transpose1d(const float* x, const float* w_host, const float* bias_host, float* y, const int32_t* lengths, int B,
                           int Cin, int Cout, int k, int stride, int ldx, int ldo, int Lmax, float in_slope, void* stream) {
  return dissc_conv_transpose1d_prec(x, w_host, bias_host, y, lengths, B, Cin, Cout, k, stride, ldx, ldo, Lmax, in_slope, 0, stream);
}

// Diagnostics: average ms of `iters` launches of one conv layer on synthetic data.
int dissc_conv_bench(int B, int Cin, int Cout, int k, int dilation, int L, int epi, int iters, int flags, float* ms_out) {
  if (!ms_out || B <= 0 || L <= 0 || iters <= 0) {
    set_error("dissc_conv_bench: bad argument");
    return DISSC_EINVAL;
  }
  std::vector<float> w((size_t)Cout * Cin * k), bias(Cout, 0.1f);
  Lcg rnd;
  rnd.fill(w, 0.05f);
  // flags bit 5 (0x20): zero-filled operands (the chip clocks to its power budget: how much of a launch's time is the data's
  // switching activity, not the schedule?  never a number to quote)
  if (flags & 0x20) std::fill(w.begin(), w.end(), 0.f);
  DiagScope ds;
  DevConv& dc = ds.c1;
  const bool w8 = (flags & 4) && wino8_supported(Cout, Cin, k, dilation);
  const bool wino = w8 || ((flags & 2) && wino_supported(Cout, Cin, k, dilation));
  int rc;
  {
    PrecScope prec_scope(opts().precision);  // diagnostics follow the "precision" option like the generator does
    rc = w8 ? make_wino8(w.data(), bias.data(), Cout, k, dilation, dc, (flags & 8) && wino8_r4_supported(Cout, k, dilation) ? 4 : 3)
            : wino ? make_wino(w.data(), bias.data(), Cout, k, dilation, dc)
                   : make_conv(w.data(), bias.data(), Cout, Cin, k, dilation, dc);
  }
  if (rc) return rc;
  const int ld = (L + 3) / 4 * 4;
  const size_t nx = (size_t)B * Cin * ld, no = (size_t)B * Cout * ld;
  float *x = nullptr, *y = nullptr, *r = nullptr, *a = nullptr;
  std::vector<float> hx(nx);
  rnd.fill(hx, 2.f);
  if (flags & 0x20) std::fill(hx.begin(), hx.end(), 0.f);
  DISSC_HIP_CHECK(ds.alloc(&x, nx));
  DISSC_HIP_CHECK(ds.alloc(&y, no));
  DISSC_HIP_CHECK(ds.alloc(&r, no));
  DISSC_HIP_CHECK(ds.alloc(&a, no));
  DISSC_HIP_CHECK(hipMemcpy(x, hx.data(), nx * 4, hipMemcpyHostToDevice));
  DISSC_HIP_CHECK(hipMemset(r, 0, no * 4));
  DISSC_HIP_CHECK(hipMemset(a, 0, no * 4));
  DISSC_HIP_CHECK(ds.events());
  const int saved_cls = (flags >> 16) & 0xf;
  if (flags & 0x8000) conv_set_cfg(saved_cls, (flags >> 8) & 0x3f);
  const Batch bt = batch_of(nullptr, 1, B, L);
  const EpiSpec ep = epi_of(epi, r, a, 3.f);
  rc = time_launches(ds, iters, [&]() { return run_conv(dc, x, y, bt, ep, Cin, ld, ld, (flags & 1) ? 1.0f : 0.1f, nullptr); }, ms_out);
  // diagnostics: the head of the accumulator buffer (a kernel's timeline stamps)
  if (const char* tlp = getenv("DISSC_TIMELINE")) dump_timeline(tlp, a, std::min<size_t>(no * 4, (size_t)4096 * 64));
  return rc;
}

// Diagnostics: average ms of `iters` launches of one stride-2, k = 3 conv (C -> C channels, L input samples per utterance,
// GELU fused) on synthetic data; form as dissc_conv1d_s2 (hubert.hip).
int dissc_conv_s2_bench(int B, int C, int L, int form, int iters, float* ms_out) {
  if (!ms_out || B <= 0 || L < 3 || iters <= 0 || (form != 0 && form != 1)) {
    set_error("dissc_conv_s2_bench: bad argument");
    return DISSC_EINVAL;
  }
  std::vector<float> w((size_t)C * C * 3);
  Lcg rnd;
  rnd.fill(w, 0.1f);
  const int Lo = (L - 3) / 2 + 1;
  const int ldx = (L + 3) / 4 * 4, ldo = (Lo + 3) / 4 * 4;
  const size_t nx = (size_t)B * C * ldx, no = (size_t)B * C * ldo;
  std::vector<float> hx(nx);
  rnd.fill(hx, 2.f, 0.3f);
  DiagScope ds;
  float *x = nullptr, *y = nullptr;
  DISSC_HIP_CHECK(ds.alloc(&x, nx));
  DISSC_HIP_CHECK(ds.alloc(&y, no));
  DISSC_HIP_CHECK(hipMemcpy(x, hx.data(), nx * 4, hipMemcpyHostToDevice));
  DevS2tc& tc = ds.tc;
  DevConv& dc = ds.c1;
  int rc = form == 1 ? make_s2tc(w.data(), nullptr, C, C, tc) : make_conv(w.data(), nullptr, C, C, 3, 1, dc, 1, 2, 0);
  if (rc) return rc;
  tc.act = 1;
  dc.act = 1;
  Batch bt;
  bt.len_default = L; bt.olen_default = Lo; bt.B = B; bt.Lmax = Lo;
  float* tlbuf = nullptr;  // diagnostics (DISSC_TIMELINE): a kernel's timeline stamps, handed over as the accumulator pointer
  const char* tlp = getenv("DISSC_TIMELINE");
  if (tlp) {
    DISSC_HIP_CHECK(ds.alloc(&tlbuf, (size_t)1024 * 64));
    DISSC_HIP_CHECK(hipMemset(tlbuf, 0, (size_t)4096 * 64));
  }
  DISSC_HIP_CHECK(ds.events());
  rc = time_launches(ds, iters, [&]() {
    return form == 1 ? run_s2tc(tc, x, y, bt, ldx, ldo, nullptr)
                     : run_conv(dc, x, y, bt, epi_of(EPI_STORE, nullptr, tlbuf), C, ldx, ldo, 1.0f, nullptr);
  }, ms_out);
  if (tlbuf) dump_timeline(tlp, tlbuf, (size_t)4096 * 64);
  return rc;
}

}  // extern "C"
