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
#include <stdarg.h>
#include <stdlib.h>
#include <string.h>

#include <atomic>
#include <exception>
#include <functional>
#include <map>
#include <mutex>
#include <string>
#include <thread>
#include <tuple>
#include <vector>

#include <algorithm>

#include "common.h"

namespace dissc {

static thread_local char g_err[512] = "";
void set_error(const char* fmt, ...) {
  va_list ap;
  va_start(ap, fmt);
  vsnprintf(g_err, sizeof(g_err), fmt, ap);
  va_end(ap);
}

Options g_defaults;
thread_local const Options* t_opts = nullptr;

}  // namespace dissc

using namespace dissc;

// option "graphs" (default 0): replay small forwards from a captured hipGraph.  OFF by default:
                                  // measured on ROCm 7.2 / MI355X, hipGraphLaunch of the ~85-node three-branch graph costs
                                  // 1.3-1.8 ms MORE per forward than the plain three-stream launches (tools/graph_ab.py)
// option "graph_frames" (default 2048): largest B * Tmax that is graphed
[[maybe_unused]] static int g_graph_hits = 0, g_graph_captures = 0;  // diagnostics (dissc_get_option)
// option "multistream" (default 1): concurrent ResBlock chains (read at create)

// ---- the ResBlock plan -------------------------------------------------------------------------------------------------------
// Each ResBlock is a chain of three residual pairs x = x + conv_1(lrelu(conv_d(lrelu(x)))).  Which kernels run a chain and its
// pairs is decided ONCE per handle, by plan_chain() under the handle's options when it is created: packing follows the plan, and
// the plan is all that the forward and the executed-FLOP count read.  The policy below is the only code that reads the form
// options (wino, wino8*, pair_*) and the handle's precision; the kernel files only say which instances exist
// (*_supported).
enum class ChainForm : uint8_t {
  pairs,      // three pair launches or launch pairs, each in its own PairForm
  bf3_block,  // split-bf16: the whole block in one launch (resblock_bf3.hip)
  bf3_pairs,  // split-bf16: the block as three pair launches of the same kernel
};
enum class PairForm : uint8_t {
  direct,      // two direct convs, t through the chain's TMP buffer
  direct_dma,  // ... the first stores lrelu(t) with zero tails (EPI_STORE_ACT): the second stages its windows by LDS-DMA
  td,          // two transform-domain convs (PairPlan::conv)
  fused,       // one launch, direct, t in LDS (respair.hip)
  fused_td,    // one launch, both convs in the transform domain (PairPlan::reg_form)
};
enum class ConvForm : uint8_t { direct, f43, f63, f54 };  // f43: conv_wino.hip; f63 / f54: conv_wino8.hip with 3 / 4-tap sub-filters
struct PairPlan {
  PairForm form = PairForm::direct;
  ConvForm conv[2] = {ConvForm::direct, ConvForm::direct};  // conv_d, conv_1
  // fused_td: DevPairW::form -- 1 / 2 the register-only F(2,3) / six-point F(3,4) kernels (respair_f23.hip); 0 F(4,3)
  // (respair_wino.hip, experimental)
  uint8_t reg_form = 0;
};
struct ChainPlan {
  ChainForm form = ChainForm::pairs;
  PairPlan pair[3];
};

// option "wino" (default 1): 1 = the ResBlock convs of the stages with C >= WINO_MIN_C (at C = 64 those with
//   k >= WINO_C64_KMIN) run in the Toom-Cook transform domain; 0 = all direct (and no fused transform-domain pairs either);
//   2 = dissc_conv1d too (tests)
constexpr int WINO_MIN_C = 64;    // narrowest stage on the transform-domain kernels
constexpr int WINO_C64_KMIN = 3;  // C = 64: k = 3 / 7 gain 2 % per forward, in isolation break-even against the DMA-staged direct pair
static bool wino_wanted(int C, int KS) {
  if (!opts().wino || C < WINO_MIN_C) return false;
  if (C < 128 && KS < WINO_C64_KMIN) return false;
  return wino_supported(C, C, KS, 1);
}

// option "wino8" (default 1): 1 = the transform-domain convs "wino8_mask" names run on conv_wino8.hip's eight
//   points instead of conv_wino's F(4,3) form; 0 = none; 2 = dissc_conv1d too (tests).  Per launch 3-17 % faster than F(4,3) on 26
//   of the 36 (C, k, d, epilogue) shapes of the generator (tools/wino8_gate.py), 4-9 % slower on the d = 1 shapes of the
//   128-channel stage (864 workgroups = 3.4 rounds of 256 CUs where the F(4,3) tiles make exactly 5.0): the default mask leaves
//   that stage alone.  Whole forward 35.17 / 35.27 -> 34.84 / 34.91 ms, in-run parity rms 5.5e-7 -> 6.5e-7.
// option "wino8_mask" (default 0450770550): one bit per SHAPE, from per-launch measurements and same-box
//   forward A/Bs (tools/opt_ab.sh): bit 9 cls + 3 ki + di with cls = 0 / 1 / 2 for C = 64 / 128 / >= 256, ki = 0 / 1 / 2 for
//   k = 3 / 7 / 11, di = 0 / 1 / 2 for dilation 1 / 3 / 5 -- in octal three digits per class (k = 11, k = 7, k = 3 from the left),
//   each digit = the dilations d5 d3 d1.  Speed alone picked every k = 7 / 11 shape and k = 3, d = 1 at C = 64 (0770770771);
//   on trained-like weights and inputs (tests/test_gpu_trained_like.py, profiles/trained_like_error.md) seven of those shapes
//   rounded above 3x the direct kernel's rms error in their eight-point form and stay on F(4,3): C >= 256 k = 7 d = 3 and
//   k = 11 d = 1 / 3 (F(5,4)), C = 64 k = 3 d = 1, k = 7 d = 3 and k = 11 d = 3 (F(6,3)).
// option "wino8_r4" (default 1): 1 = the shapes "wino8_r4_mask" (same layout, k = 3 bits ignored; default every
//   k = 7 / 11 shape of the C >= 128 stages and k = 7, d = 1 at C = 64) run as F(5,4) instead of F(6,3); 2 = dissc_conv1d too
//   (tests); 0 = never
static int w8_shape_bit(int C, int KS, int dil) {
  const int cls = C >= 256 ? 2 : C >= 128 ? 1 : 0;
  return 9 * cls + 3 * (KS == 11 ? 2 : KS == 7 ? 1 : 0) + (dil == 1 ? 0 : dil == 3 ? 1 : 2);
}
static ConvForm td_conv_form(int C, int KS, int dil) {
  if (!opts().wino8 || !wino8_supported(C, C, KS, dil) || !((opts().wino8_mask >> w8_shape_bit(C, KS, dil)) & 1))
    return ConvForm::f43;
  const bool r4 = opts().wino8_r4 && wino8_r4_supported(C, KS, dil) && ((opts().wino8_r4_mask >> w8_shape_bit(C, KS, dil)) & 1);
  return r4 ? ConvForm::f54 : ConvForm::f63;
}

// option "pair_f23" (default 3), a bit mask: 1 = the C = 32, k = 11 pairs run as register-only F(2,3)
//   (respair_f23.hip; per launch 857 / 894 / 924 us at d = 1 / 3 / 5 against 1 042 / 1 037 / 1 052 for the direct pair,
//   B = 32 x 10 s), 2 = the C = 16, k = 11 pairs (respair16_f23.hip: 525 against 604 us at d = 1); 4 / 8 = the k = 3 pairs of the
//   two stages (C = 32: 365 against 417 us, C = 16: 262 against 263; forward 33.11 -> 33.09 ms: off).  Bits 1 / 2 are the
//   per-stage switch of the register-only transform-domain pairs: which form a (stage, k) takes is "pair_tc6"'s choice.
// option "pair_tc6" (default 3), a bit mask honoured only for a stage whose "pair_f23" bit is set: 1 = the C = 32, k = 7
//   pairs, 2 = the C = 32, k = 11 pairs run on six points as F(3,4) (respair32_tc6_kernel: 4 / 6 products per output where the
//   direct pair executes 7 and F(2,3) 8).  Per launch at d = 1 / 3 / 5, B = 32 x 10 s, 1 000 alternated launches: k = 7
//   478 / 482 / 538 us against 655 / 658 / 690 for the direct pair, k = 11 705 / 701 / 796 against 797 / 834 / 898 for F(2,3);
//   forward 32.84-33.00 -> 32.10-32.23 ms (five alternated runs), bit 1 alone 32.30-32.79, bit 2 alone 32.64-32.77 against
//   32.74-32.89 (profiles/r07).  Rounding on trained-like data <= 1.4 x the direct pair's rms (bar 3).  4 / 8 = the same for
//   C = 16: no instance, ignored.  The two options together also pick the form of dissc_respair1d's mode 3.
// option "pair_f23_c64" (default 1), honoured only while "pair_f23" != 0: the k = 3 pairs of the 64-channel stage run as ONE
//   register-only F(2,3) launch each (respair64_f23_kernel in respair_f23.hip: 2 C^2 products per output and conv where the two
//   conv_wino launches it replaces execute 1.5 C^2, for two tensor passes instead of five); 0 = two transform-domain launches.
//   Measurements: profiles/r09.
// option "pair_tc6_c64" (default 1), a bit mask honoured only while "pair_f23" != 0, independent of "pair_tc6" and
//   "pair_f23_c64": 1 = the k = 7 pairs, 2 = the k = 11 pairs of the 64-channel stage run as ONE register-only six-point launch
//   each (respair64_tc6_kernel in respair_f23.hip: 4 / 6 C^2 products per output and conv, two tensor passes instead of five);
//   0 = two transform-domain launches in the forms td_conv_form() gives.  Per launch at d = 1 / 3 / 5, B = 32 x 40 000: k = 7
//   810 / 869 / 950 us against 979 / 1 117 / 1 095 for the two launches, forward 31.89-32.06 -> 31.43-31.65 ms (five alternated
//   runs); k = 11 1 210 / 1 307 / 1 465 against 1 251 / 1 318 / 1 317, forward slower with bit 2 than without: off
//   (profiles/r10).
// the register-only form of a pair (DevPairW::form: 1 F(2,3), 2 six points), or 0
static int pair_reg_form(int C, int KS, int dil) {
  if (C == 64) {
    if (opts().pair_f23 == 0) return 0;
    if (KS == 3) return opts().pair_f23_c64 && pair_f23_supported(C, KS, dil) ? 1 : 0;
    const int bit = KS == 7 ? 1 : KS == 11 ? 2 : 0;
    return (opts().pair_tc6_c64 & bit) && pair_tc6_supported(C, KS, dil) ? 2 : 0;
  }
  if (C != 16 && C != 32) return 0;
  const int stage = C == 32 ? 1 : 2;
  if (KS == 3) return pair_f23_supported(C, KS, dil) && (opts().pair_f23 & (stage << 2)) ? 1 : 0;
  if (!(opts().pair_f23 & stage)) return 0;
  const int tc6_bit = (C == 32 ? 1 : 4) << (KS == 11 ? 1 : 0);
  if ((KS == 7 || KS == 11) && (opts().pair_tc6 & tc6_bit) && pair_tc6_supported(C, KS, dil)) return 2;
  return pair_f23_supported(C, KS, dil) ? 1 : 0;
}
// option "pair_wino" (default 0; experimental builds): 1 = the pairs respair_wino.hip's F(4,3) kernel measured
//   faster for (tools/pair_gate.py, B = 32 x 10 s: C = 32, k = 11, d = 1 / 3: 895 / 988 us against 1 042 / 1 047 for the direct
//   fused pair; C = 64, k = 3, d = 1: 624 against 658 for two conv_wino launches) run on it; 2 = every shape with an instance
//   (tests); 0 = none.  Off: its gate failed (whole forward 35.36 against 35.42 ms, executed-FLOP utilisation 0.619 -> 0.602).
static bool pairw_wanted(int C, int KS, int dil) {
  if (pair_reg_form(C, KS, dil)) return true;
  if (!opts().pair_wino || !pairw_supported(C, KS, dil)) return false;
  if (opts().pair_wino >= 2) return true;
  if (C == 32) return KS == 11 && dil <= 3;
  return C == 64 && KS == 3 && dil == 1;
}

// option "pair_max_c" (default 32): widest stage whose pairs run as one launch each (0 = off)
// option "pair_dma" (default 1): the direct pairs of the wide stages hand t over in the EPI_STORE_ACT layout
static ChainPlan plan_chain(int C, int KS, const int* dil, int prec) {
  ChainPlan cp;
  if (prec == 1 && resblock_bf3_supported(C, KS, dil)) {
    // split-bf16 blocks of >= 64 channels run as three pair launches.  With 64 channels the LDS holds 256-column windows only,
    // and the 120-column halo of a whole 11-tap block would be recomputed ~2x; a pair's halo is 10-30 columns, at the price of
    // two more read+write passes of x_k per block.
    cp.form = C >= 64 ? ChainForm::bf3_pairs : ChainForm::bf3_block;
    return cp;
  }
  // the direct fused pair needs fp32 weights in its layout (16x16x4 at C = 16, 32x32x2 at C = 32: make_conv's choice)
  bool fused = prec == 0 && (C < 32 || opts().use_mfma32) && C <= opts().pair_max_c;
  for (int m = 0; m < 3; ++m) fused = fused && respair_supported(C, KS, dil[m]);
  // ... or when every pair of the chain takes a one-launch transform-domain form: x_k then ping-pongs X -> XK -> TMP -> ACC
  bool all_td = prec == 0 && opts().wino && C > 32 && wino_wanted(C, KS);
  for (int m = 0; m < 3; ++m) all_td = all_td && wino_supported(C, C, KS, dil[m]) && pairw_wanted(C, KS, dil[m]);
  for (int m = 0; m < 3; ++m) {
    PairPlan& p = cp.pair[m];
    const int d = dil[m];
    const bool td = prec == 0 && wino_wanted(C, KS) && wino_supported(C, C, KS, d);
    // a fused transform-domain pair writes a new x_k: at C = 64 (where the other pairs update x_k in place) and in a chain whose
    // pairs do not all fuse, only the first pair of the chain takes it
    const bool fuse_td = prec == 0 && opts().wino && pairw_wanted(C, KS, d) && (C > 32 ? td : C <= opts().pair_max_c) &&
                         (fused || all_td || m == 0);
    if (fuse_td) {
      p.form = PairForm::fused_td;
      p.reg_form = (uint8_t)pair_reg_form(C, KS, d);
    } else if (fused) {
      p.form = PairForm::fused;
    } else if (td) {
      p.form = PairForm::td;
      p.conv[0] = td_conv_form(C, KS, d);
      p.conv[1] = td_conv_form(C, KS, 1);
    } else if (opts().pair_dma && prec == 0 && opts().use_mfma32 && C >= 32 && C % KC == 0) {  // both convs on the 32x32x2 kernel, fp32
      p.form = PairForm::direct_dma;
    }
  }
  return cp;
}

// multiply-adds per output position of one pair: algorithmic, or what the matrix pipe executes
static double pair_macs(const PairPlan& p, int C, int KS, bool executed) {
  const double direct = (double)C * C * KS;
  auto conv = [&](ConvForm f) {
    return f == ConvForm::f43 ? wino_executed_macs_per_t(C, KS)
         : f == ConvForm::f63 ? wino8_executed_macs_per_t(C, KS, 3)
         : f == ConvForm::f54 ? wino8_executed_macs_per_t(C, KS, 4) : direct;
  };
  if (executed && p.form == PairForm::fused_td) {  // F(2,3): 4 products per 2 outputs and sub-filter; six points: 6 per 3
    if (p.reg_form == 2) return 2.0 * C * C * 2.0 * ((KS + 3) / 4);
    return p.reg_form == 1 ? 2.0 * C * C * 2.0 * ((KS + 2) / 3) : 2.0 * wino_executed_macs_per_t(C, KS);
  }
  return executed ? conv(p.conv[0]) + conv(p.conv[1]) : direct + direct;
}

// a transform-domain or direct conv of a pair, packed for its form
static int make_pair_conv(ConvForm f, const float* w, const float* b, int C, int KS, int dil, DevConv& dc) {
  switch (f) {
    case ConvForm::f43: return make_wino(w, b, C, KS, dil, dc);
    case ConvForm::f63: return make_wino8(w, b, C, KS, dil, dc, 3);
    case ConvForm::f54: return make_wino8(w, b, C, KS, dil, dc, 4);
    default: return make_conv(w, b, C, C, KS, dil, dc);
  }
}

// The MRF epilogue of chain j's last launch: xs = r_0; xs += r_j; x = (xs + r_last) / nk
static int mrf_epi(int j, int nk) { return j == nk - 1 ? EPI_MRF_DIV : j == 0 ? EPI_MRF_SET : EPI_MRF_ADD; }

// The side streams of the concurrent ResBlock chains are shared by every generator handle of a
// device (created on first use, kept for the life of the process): HIP multiplexes streams onto a
// few hardware queues (4 by default), and a second handle with streams of its own would push the
// chains of both onto shared queues and serialise them (measured: +12 % per step for whichever
// handle was created second).  Work of different handles on a shared stream is ordered by the same
// events as before, so sharing changes no result.
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
  int hop = 1;
  DevConv conv_pre;
  std::vector<std::vector<DevConv>> ups;  // per stage: one conv per phase group
  std::vector<ChainPlan> plan;     // [stage*nk + j]: the kernel forms of ResBlock j of the stage
  std::vector<DevConv> rb1, rb2;  // [stage*nk*3 + j*3 + m]: conv_d / conv_1 of pair m (forms direct, direct_dma, td, fused)
  std::vector<DevPairW> pw;       // same index: the pair as ONE transform-domain launch (form fused_td)
  std::vector<float*> fused_w, fused_b;  // [stage*nk + j]: 6 packed convs / biases of a split-bf16 ResBlock (bf3_* chains)
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

const char* dissc_last_error(void) { return g_err; }
int dissc_abi_version(void) { return 7; }

int dissc_device_count(void) {
  int n = 0;
  if (hipGetDeviceCount(&n) != hipSuccess) return 0;
  return n;
}

int dissc_device_name(int dev, char* buf, size_t buflen) {
  hipDeviceProp_t p;
  DISSC_HIP_CHECK(hipGetDeviceProperties(&p, dev));
  snprintf(buf, buflen, "%s (%s, %d CUs)", p.name, p.gcnArchName, p.multiProcessorCount);
  return DISSC_OK;
}

int dissc_gen_create(const DisscGenConfig* cfg, const DisscTensor* weights, size_t n_weights,
                     dissc_gen_t* out) {
  return dissc_gen_create_ex(cfg, weights, n_weights, -1, out);
}

int dissc_gen_create_ex(const DisscGenConfig* cfg, const DisscTensor* weights, size_t n_weights, int precision,
                        dissc_gen_t* out) {
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
  struct PrecScope {  // only the generator's layers may be packed for split-bf16
    explicit PrecScope(int p) { g_conv_prec = p; }
    ~PrecScope() { g_conv_prec = 0; }
  } prec_scope(prec);
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
  // threads at the end (run_pack_tasks; DISSC_PACK_THREADS, default min(8, cores); 1 = in place).  Each task writes one
  // pre-sized slot of the handle; a worker carries the creating thread's device, options snapshot and packing precision.
  std::vector<std::function<int()>> tasks;
  auto run_pack_tasks = [&]() -> int {
    // default: min(8, the CPUs this process may really use / ranks on the node) -- hardware_concurrency() knows neither the cgroup
    // CPU quota (the GPU boxes: 16 of 256 logical CPUs) nor that 8 ranks create handles at once
    int nthr = 8;
    {
      double cpus = (double)std::thread::hardware_concurrency();
      if (FILE* f = fopen("/sys/fs/cgroup/cpu.max", "r")) {
        char q[32] = {0};
        long long per = 0;
        if (fscanf(f, "%31s %lld", q, &per) == 2 && strcmp(q, "max") != 0 && per > 0) {
          const double quota = atof(q) / (double)per;
          if (quota >= 1.0 && (cpus <= 0 || quota < cpus)) cpus = quota;
        }
        fclose(f);
      }
      int ranks = 1;
      if (const char* e = getenv("LOCAL_WORLD_SIZE")) {
        const long v = strtol(e, nullptr, 10);
        if (v >= 1 && v <= 1024) ranks = (int)v;
      }
      if (cpus >= 1.0 && nthr > (int)(cpus / ranks)) nthr = (int)(cpus / ranks) > 1 ? (int)(cpus / ranks) : 1;
    }
    if (const char* e = getenv("DISSC_PACK_THREADS")) {  // explicit override, validated
      char* end = nullptr;
      const long v = strtol(e, &end, 10);
      if (end != e && *end == 0 && v >= 1 && v <= 256) nthr = (int)v;
    }
    if (nthr > (int)tasks.size()) nthr = (int)tasks.size();
    if (nthr <= 1) {
      for (auto& t : tasks)
        if (int r = t()) return r;
      return DISSC_OK;
    }
    int dev = 0;
    DISSC_HIP_CHECK(hipGetDevice(&dev));
    std::atomic<size_t> next{0};
    std::atomic<int> first_rc{DISSC_OK};
    std::mutex err_mu;
    std::string err_msg;
    auto worker = [&]() {
      if (hipSetDevice(dev) != hipSuccess) {
        first_rc = DISSC_EHIP;
        return;
      }
      OptScope scope(&g->opt);
      g_conv_prec = prec;
      for (size_t i = next++; i < tasks.size() && first_rc == DISSC_OK; i = next++) {
        int r;
        try {
          r = tasks[i]();
        } catch (const std::exception& e) {  // (an exception leaving a std::thread would terminate the process)
          set_error("dissc_gen_create: packing a layer failed: %s", e.what());
          r = DISSC_ENOMEM;
        } catch (...) {
          set_error("dissc_gen_create: packing a layer failed (unknown exception)");
          r = DISSC_ENOMEM;
        }
        if (r != DISSC_OK) {
          std::lock_guard<std::mutex> lk(err_mu);
          if (first_rc == DISSC_OK) {
            first_rc = r;
            err_msg = g_err;  // the worker's thread-local message
          }
        }
      }
      g_conv_prec = 0;
    };
    std::vector<std::thread> pool;
    try {
      for (int t = 0; t + 1 < nthr; ++t) pool.emplace_back(worker);
    } catch (const std::exception&) {  // no more threads to be had: whoever started shares the tasks with this thread
    }
    worker();  // the creating thread packs too (and alone, if no thread could be started)
    for (auto& t : pool) t.join();
    g_conv_prec = prec;  // (worker() cleared this thread's copy; the bf3 tail below and PrecScope's exit expect it set)
    if (first_rc != DISSC_OK) set_error("%s", err_msg.empty() ? "dissc_gen_create: a packing thread failed" : err_msg.c_str());
    return first_rc;
  };
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
      const ChainPlan& cp = g->plan[cj] = plan_chain(ch, rk, dl, prec);
      const float* w6[6];  // conv_d / conv_1 of the three pairs
      const float* b6[6];
      for (int l = 0; l < 6; ++l) {
        snprintf(name, sizeof(name), "resblocks.%d.convs%d.%d.weight", (int)cj, 1 + l % 2, l / 2);
        if ((rc = get(name, {ch, ch, rk}, &w6[l]))) return fail(rc);
        snprintf(name, sizeof(name), "resblocks.%d.convs%d.%d.bias", (int)cj, 1 + l % 2, l / 2);
        if ((rc = get(name, {ch}, &b6[l]))) return fail(rc);
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
  if ((rc = run_pack_tasks())) return fail(rc);
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
    for (int j = 0; j < nk; ++j)
      for (const PairPlan& p : g->plan[(size_t)i * nk + j].pair)
        macs += pair_macs(p, g->stage_C[i], g->cfg.resblock_kernel_sizes[j], executed) * mul;
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
  if ((rc = run_conv(g->conv_pre, TMP, ACC, nullptr, nullptr, lengths, Tmax, 1, B, c.model_in_dim,
                     ld0, ld0, Tmax, 1.0f, EPI_STORE, 1.f, stream)))
    return rc;
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
      if ((rc = run_conv(g->ups[i][gi], ACC, X, nullptr, nullptr, lengths, Tmax * mul, mul, B, ch, ld,
                         ld_out, Tmax * mul, 0.1f, EPI_STORE, 1.f, sg)))
        return rc;
      if (par_ups && gi > 0) {
        DISSC_HIP_CHECK(hipEventRecord(g->ev_fin[gi], sg));
        DISSC_HIP_CHECK(hipStreamWaitEvent(stream, g->ev_fin[gi], 0));
      }
    }
    ch = ch_out; mul = mul_out; ld = ld_out;
    const int L = Tmax * mul;
    if (multi) DISSC_HIP_CHECK(hipEventRecord(g->ev_x, stream));  // X is ready
    for (int j = 0; j < nk; ++j) {
      hipStream_t sj = (multi && j > 0) ? g->aux[j] : stream;
      if (multi && j > 0) DISSC_HIP_CHECK(hipStreamWaitEvent(sj, g->ev_x, 0));
      const size_t cj = (size_t)i * nk + j;
      const ChainPlan& cp = g->plan[cj];
      const int rk = c.resblock_kernel_sizes[j];
      const int* dl = c.resblock_dilations[j];
      const float* fw = g->fused_w[cj];
      const float* fb = g->fused_b[cj];
      float* TMPc = multi ? TMPj[j] : TMPj[0];
      float* XKc = multi ? XKj[j] : XKj[0];
      const int mrf = mrf_epi(j, nk);
      // the chains run concurrently up to the MRF update: the one launch of a chain that updates ACC waits for the previous chain
      auto acc_turn = [&]() -> int {
        if (multi && j > 0) DISSC_HIP_CHECK(hipStreamWaitEvent(sj, g->ev_fin[j - 1], 0));
        return DISSC_OK;
      };
      if (cp.form == ChainForm::bf3_block) {  // the whole ResBlock in one launch
        if ((rc = acc_turn()) ||
            (rc = launch_resblock_bf3(ch, X, ACC, fw, fb, lengths, L, mul, rk, dl, B, L, ld, 0.1f, mrf, (float)nk, 0, 3, sj)))
          return rc;
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
          rc = launch_resblock_bf3(ch, x, last ? ACC : nxt, fw, fb, lengths, L, mul, rk, dl, B, L, ld, 0.1f, last ? mrf : EPI_STORE,
                                   last ? (float)nk : 1.f, m, m + 1, sj);
          x = nxt;
        } else if (pf == PairForm::fused || pf == PairForm::fused_td) {
          if (last && (rc = acc_turn())) return rc;
          float* out = last ? nullptr : nxt;
          const int epi = last ? mrf : EPI_RES;
          rc = pf == PairForm::fused_td
                   ? launch_respair_wino(g->pw[idx], x, out, ACC, lengths, L, mul, B, L, ld, 0.1f, epi, (float)nk, sj)
                   : launch_respair(g->rb1[idx], g->rb2[idx], x, out, ACC, lengths, L, mul, B, L, ld, 0.1f, epi, (float)nk, sj);
          x = nxt;
        } else {  // two conv launches, t through TMP, x_k updated in place
          const bool dma = pf == PairForm::direct_dma;
          const int ldt = dma ? (int)round_up((size_t)L + ZERO_TAIL, 4) : ld;
          if ((rc = run_conv(g->rb1[idx], x, TMPc, nullptr, nullptr, lengths, L, mul, B, ch, ld, ldt, L, 0.1f,
                             dma ? EPI_STORE_ACT : EPI_STORE, 1.f, sj, 0.1f, 0)))
            return rc;
          if (last && (rc = acc_turn())) return rc;
          rc = run_conv(g->rb2[idx], TMPc, XKc, x, ACC, lengths, L, mul, B, ch, ldt, ld, L, dma ? 1.0f : 0.1f, last ? mrf : EPI_RES,
                        (float)nk, sj, 0.f, dma ? 1 : 0);
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

// ---- stand-alone conv entry points (weights packed per call: tests only) ----------------
static int conv_once(DevConv& dc, const float* x, float* y, const int32_t* lengths, int B,
                     int ldx, int ldo, int Lmax, float in_slope, hipStream_t stream) {
  int rc = run_conv(dc, x, y, nullptr, nullptr, lengths, Lmax, 1, B, dc.CIN, ldx, ldo, Lmax,
                    in_slope, EPI_STORE, 1.f, stream);
  hipError_t e = hipStreamSynchronize(stream);
  free_conv(dc);
  if (rc) return rc;
  DISSC_HIP_CHECK(e);
  return DISSC_OK;
}

int dissc_conv1d(const float* x, const float* w_host, const float* bias_host, float* y,
                 const int32_t* lengths, int B, int Cin, int Cout, int k, int dilation, int ldx,
                 int ldo, int Lmax, float in_slope, void* stream) {
  if (!x || !w_host || !y || k % 2 != 1 || dilation < 1) {
    set_error("dissc_conv1d: bad argument");
    return DISSC_EINVAL;
  }
  // "wino" / "wino8" / "wino8_r4" = 2: this entry takes the transform-domain forms too (tests)
  DevConv dc;
  int rc;
  if (opts().wino8 >= 2 && wino8_supported(Cout, Cin, k, dilation))
    rc = make_wino8(w_host, bias_host, Cout, k, dilation, dc, opts().wino8_r4 >= 2 && wino8_r4_supported(Cout, k, dilation) ? 4 : 3);
  else if (opts().wino >= 2 && wino_supported(Cout, Cin, k, dilation))
    rc = make_wino(w_host, bias_host, Cout, k, dilation, dc);
  else
    rc = make_conv(w_host, bias_host, Cout, Cin, k, dilation, dc);
  if (rc) return rc;
  return conv_once(dc, x, y, lengths, B, ldx, ldo, Lmax, in_slope, (hipStream_t)stream);
}

// Diagnostics / tests: ONE residual pair y = x + conv_1(lrelu(conv_d(lrelu(x)))) (or its MRF modes) on device data with
// host weights, through a chosen implementation: mode 0 = two direct conv launches, 1 = the fused direct pair
// (respair.hip), 2 = two conv_wino launches, 3 = the fused transform-domain pair (pair_host.hip), 4 = two transform-domain
// launches in the forms the plan gives a PairForm::td pair of the shape (td_conv_form).  Synchronous.
static int pair_run(int mode, const DevConv& c1, const DevConv& c2, const DevPairW& pw, const float* x, float* tmp, float* y,
                    float* acc, const int32_t* lengths, int B, int C, int ld, int Lmax, float slope, int epi, float mrf_div,
                    hipStream_t st) {
  int rc;
  switch (mode) {
    case 0:
    case 2:
    case 4:
      if ((rc = run_conv(c1, x, tmp, nullptr, nullptr, lengths, Lmax, 1, B, C, ld, ld, Lmax, slope, EPI_STORE, 1.f, st))) return rc;
      return run_conv(c2, tmp, y, x, acc, lengths, Lmax, 1, B, C, ld, ld, Lmax, slope, epi, mrf_div, st);
    case 1:
      return launch_respair(c1, c2, x, y, acc, lengths, Lmax, 1, B, Lmax, ld, slope, epi, mrf_div, st);
    case 3:
      return launch_respair_wino(pw, x, y, acc, lengths, Lmax, 1, B, Lmax, ld, slope, epi, mrf_div, st);
    default:
      set_error("pair mode %d", mode);
      return DISSC_EINVAL;
  }
}

static int pair_make(int mode, const float* w1, const float* b1, const float* w2, const float* b2, int C, int k, int d,
                     DevConv& c1, DevConv& c2, DevPairW& pw) {
  int rc;
  if (mode == 2) {
    if (!wino_supported(C, C, k, d) && !(C == 32 && (k == 3 || k == 7 || k == 11) && (d == 1 || d == 3 || d == 5))) {
      set_error("pair mode 2: no conv_wino instance for C = %d, k = %d, d = %d", C, k, d);
      return DISSC_EINVAL;
    }
    if ((rc = make_wino(w1, b1, C, k, d, c1))) return rc;
    return make_wino(w2, b2, C, k, 1, c2);
  }
  if (mode == 3) return make_pairw(w1, b1, w2, b2, C, k, d, pair_reg_form(C, k, d), pw);
  if (mode == 4) {
    if (!wino_supported(C, C, k, d) || !wino_supported(C, C, k, 1)) {
      set_error("pair mode 4: no transform-domain conv instance for C = %d, k = %d, d = %d", C, k, d);
      return DISSC_EINVAL;
    }
    if ((rc = make_pair_conv(td_conv_form(C, k, d), w1, b1, C, k, d, c1))) return rc;
    return make_pair_conv(td_conv_form(C, k, 1), w2, b2, C, k, 1, c2);
  }
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
  DevConv c1, c2;
  DevPairW pw;
  float* tmp = nullptr;
  int rc = pair_make(mode, w1_host, b1_host, w2_host, b2_host, C, k, dilation, c1, c2, pw);
  if (!rc && (mode == 0 || mode == 2 || mode == 4) && hipMalloc((void**)&tmp, (size_t)B * C * ld * sizeof(float)) != hipSuccess) {
    set_error("dissc_respair1d: hipMalloc");
    rc = DISSC_ENOMEM;
  }
  if (!rc) rc = pair_run(mode, c1, c2, pw, x, tmp, y, acc, lengths, B, C, ld, Lmax, slope, epi, mrf_div, (hipStream_t)stream);
  const hipError_t e = hipStreamSynchronize((hipStream_t)stream);
  if (tmp) (void)hipFree(tmp);
  free_conv(c1);
  free_conv(c2);
  free_pairw(pw);
  if (rc) return rc;
  DISSC_HIP_CHECK(e);
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
// make_conv / make_convT / run_conv_ex / launch_conv themselves, without packing or uploading anything.  Host only: no HIP call.
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

// Diagnostics: average ms of `iters` launches of one residual pair (modes as dissc_respair1d) on synthetic data.
int dissc_pair_bench(int B, int C, int k, int dilation, int L, int epi, int iters, int mode, float* ms_out) {
  if (!ms_out || B <= 0 || L <= 0 || iters <= 0 || epi < EPI_RES || epi > EPI_MRF_DIV) {
    set_error("dissc_pair_bench: bad argument");
    return DISSC_EINVAL;
  }
  std::vector<float> w1((size_t)C * C * k), w2((size_t)C * C * k), bias(C, 0.1f);
  uint32_t s = 12345u;
  auto rnd = [&]() {
    s = s * 1664525u + 1013904223u;
    return (s >> 8) / 16777216.0f - 0.5f;
  };
  for (auto& v : w1) v = rnd() * 0.05f;
  for (auto& v : w2) v = rnd() * 0.05f;
  DevConv c1, c2;
  DevPairW pw;
  int rc = pair_make(mode, w1.data(), bias.data(), w2.data(), bias.data(), C, k, dilation, c1, c2, pw);
  const int ld = (L + 3) / 4 * 4;
  const size_t n = (size_t)B * C * ld;
  float *x = nullptr, *y = nullptr, *t = nullptr, *a = nullptr;
  hipEvent_t e0 = nullptr, e1 = nullptr;
  hipError_t e = hipSuccess;
  float ms = 0.f;
  if (!rc) {
    std::vector<float> hx(n);
    for (auto& v : hx) v = rnd() * 2.f;
    if (hipMalloc((void**)&x, n * 4) != hipSuccess || hipMalloc((void**)&y, n * 4) != hipSuccess ||
        hipMalloc((void**)&t, n * 4) != hipSuccess || hipMalloc((void**)&a, n * 4) != hipSuccess ||
        hipMemcpy(x, hx.data(), n * 4, hipMemcpyHostToDevice) != hipSuccess || hipMemset(a, 0, n * 4) != hipSuccess ||
        hipEventCreate(&e0) != hipSuccess || hipEventCreate(&e1) != hipSuccess) {
      set_error("dissc_pair_bench: allocation failed");
      rc = DISSC_ENOMEM;
    }
  }
  auto once = [&]() { return pair_run(mode, c1, c2, pw, x, t, y, a, nullptr, B, C, ld, L, 0.1f, epi, 3.f, nullptr); };
  for (int it = 0; it < 2 && !rc; ++it) rc = once();
  if (!rc) {
    (void)hipEventRecord(e0, nullptr);
    for (int it = 0; it < iters && !rc; ++it) rc = once();
    (void)hipEventRecord(e1, nullptr);
    e = hipEventSynchronize(e1);
    (void)hipEventElapsedTime(&ms, e0, e1);
    *ms_out = ms / iters;
  }
  if (e0) (void)hipEventDestroy(e0);
  if (e1) (void)hipEventDestroy(e1);
  for (float* q : {x, y, t, a})
    if (q) (void)hipFree(q);
  free_conv(c1);
  free_conv(c2);
  free_pairw(pw);
  if (rc) return rc;
  DISSC_HIP_CHECK(e);
  return DISSC_OK;
}

int dissc_conv_transpose1d(const float* x, const float* w_host, const float* bias_host, float* y,
                           const int32_t* lengths, int B, int Cin, int Cout, int k, int stride,
                           int ldx, int ldo, int Lmax, float in_slope, void* stream) {
  if (!x || !w_host || !y || stride < 1 || (k - stride) % 2 != 0) {
    set_error("dissc_conv_transpose1d: bad argument");
    return DISSC_EINVAL;
  }
  std::vector<DevConv> grp;
  int rc = make_convT(w_host, bias_host, Cin, Cout, k, stride, grp);
  for (auto& dc : grp) {
    int r2 = rc ? rc : conv_once(dc, x, y, lengths, B, ldx, ldo, Lmax, in_slope, (hipStream_t)stream);
    if (rc) free_conv(dc);
    rc = rc ? rc : r2;
  }
  return rc;
}

// The DEFAULTS (what handles created later start from), whatever handle the calling thread may be working for
int dissc_get_option(const char* key, int* value) {
  if (!key || !value) return DISSC_EINVAL;
  if (strcmp(key, "graph_hits") == 0) { *value = g_graph_hits; return DISSC_OK; }
  if (strcmp(key, "graph_captures") == 0) { *value = g_graph_captures; return DISSC_OK; }
  if (strcmp(key, "experimental") == 0) { *value = DISSC_EXPERIMENTAL; return DISSC_OK; }
  // the tile-shape tables, under the keys dissc_set_option takes: "conv_cfg_bm16|32|64|128|256", "conv32_cfg_bm32|64|128|256"
  for (int cls = 0; cls < 5; ++cls) {
    char name[32];
    snprintf(name, sizeof name, "conv_cfg_bm%d", 16 << cls);
    if (strcmp(key, name) == 0) { *value = g_defaults.cfg_for_bm[cls]; return DISSC_OK; }
    snprintf(name, sizeof name, "conv32_cfg_bm%d", 32 << cls);
    if (cls < 4 && strcmp(key, name) == 0) { *value = g_defaults.cfg32_for_bm[cls]; return DISSC_OK; }
  }
#define DISSC_OPT_GET(f, d, k) if (strcmp(key, k) == 0) { *value = g_defaults.f; return DISSC_OK; }
  DISSC_OPTION_LIST(DISSC_OPT_GET)
#undef DISSC_OPT_GET
  set_error("dissc_get_option: unknown key %s", key);
  return DISSC_EINVAL;
}

int dissc_set_option(const char* key, int value) {
  if (!key) return DISSC_EINVAL;
  if (strncmp(key, "conv_cfg_bm", 11) == 0) {  // "conv_cfg_bm16|32|64|128|256" -> tile config id
    const int bm = atoi(key + 11);
    int cls = 0;
    while ((16 << cls) < bm) ++cls;
    conv_set_cfg(cls, value);
    return DISSC_OK;
  }
  if (strncmp(key, "conv32_cfg_bm", 13) == 0) {
    const int bm = atoi(key + 13);
    int cls = 0;
    while ((32 << cls) < bm) ++cls;
    conv32_set_cfg(cls, value);
    return DISSC_OK;
  }
  if (strcmp(key, "pairw_chv") == 0) value = value == 2 ? 2 : 1;
#define DISSC_OPT_SET(f, d, k) if (strcmp(key, k) == 0) { g_defaults.f = value; return DISSC_OK; }
  DISSC_OPTION_LIST(DISSC_OPT_SET)
#undef DISSC_OPT_SET
  set_error("dissc_set_option: unknown key %s", key);
  return DISSC_EINVAL;
}

// Diagnostics: average ms of `iters` launches of one conv layer on synthetic data.
int dissc_conv_bench(int B, int Cin, int Cout, int k, int dilation, int L, int epi, int iters,
                     int flags, float* ms_out) {
  if (!ms_out || B <= 0 || L <= 0 || iters <= 0) {
    set_error("dissc_conv_bench: bad argument");
    return DISSC_EINVAL;
  }
  std::vector<float> w((size_t)Cout * Cin * k), bias(Cout, 0.1f);
  uint32_t s = 12345u;
  for (auto& v : w) {
    s = s * 1664525u + 1013904223u;
    v = ((s >> 8) / 16777216.0f - 0.5f) * 0.05f;
  }
  // flags bit 5 (0x20): zero-filled operands (the chip clocks to its power budget: how much of a launch's time is the data's
  // switching activity, not the schedule?  never a number to quote)
  if (flags & 0x20) std::fill(w.begin(), w.end(), 0.f);
  DevConv dc;
  g_conv_prec = opts().precision;  // diagnostics follow the "precision" option like the generator does
  const bool w8 = (flags & 4) && wino8_supported(Cout, Cin, k, dilation);
  const bool wino = w8 || ((flags & 2) && wino_supported(Cout, Cin, k, dilation));
  int rc = w8 ? make_wino8(w.data(), bias.data(), Cout, k, dilation, dc, (flags & 8) && wino8_r4_supported(Cout, k, dilation) ? 4 : 3)
              : wino ? make_wino(w.data(), bias.data(), Cout, k, dilation, dc)
                     : make_conv(w.data(), bias.data(), Cout, Cin, k, dilation, dc);
  g_conv_prec = 0;
  if (rc) return rc;
  const int ld = (L + 3) / 4 * 4;
  const size_t nx = (size_t)B * Cin * ld, no = (size_t)B * Cout * ld;
  float *x = nullptr, *y = nullptr, *r = nullptr, *a = nullptr;
  std::vector<float> hx(nx);
  for (auto& v : hx) {
    s = s * 1664525u + 1013904223u;
    v = ((s >> 8) / 16777216.0f - 0.5f) * 2.f;
  }
  if (flags & 0x20) std::fill(hx.begin(), hx.end(), 0.f);
  DISSC_HIP_CHECK(hipMalloc((void**)&x, nx * 4));
  DISSC_HIP_CHECK(hipMalloc((void**)&y, no * 4));
  DISSC_HIP_CHECK(hipMalloc((void**)&r, no * 4));
  DISSC_HIP_CHECK(hipMalloc((void**)&a, no * 4));
  DISSC_HIP_CHECK(hipMemcpy(x, hx.data(), nx * 4, hipMemcpyHostToDevice));
  DISSC_HIP_CHECK(hipMemset(r, 0, no * 4));
  DISSC_HIP_CHECK(hipMemset(a, 0, no * 4));
  hipEvent_t e0, e1;
  DISSC_HIP_CHECK(hipEventCreate(&e0));
  DISSC_HIP_CHECK(hipEventCreate(&e1));
  const int saved_cls = (flags >> 16) & 0xf;
  if (flags & 0x8000) conv_set_cfg(saved_cls, (flags >> 8) & 0x3f);
  auto once = [&]() { return run_conv(dc, x, y, r, a, nullptr, L, 1, B, Cin, ld, ld, L, (flags & 1) ? 1.0f : 0.1f, epi, 3.f, nullptr); };
  for (int it = 0; it < 2 && !rc; ++it) rc = once();
  DISSC_HIP_CHECK(hipEventRecord(e0, nullptr));
  for (int it = 0; it < iters && !rc; ++it) rc = once();
  DISSC_HIP_CHECK(hipEventRecord(e1, nullptr));
  hipError_t e = hipEventSynchronize(e1);
  float ms = 0.f;
  (void)hipEventElapsedTime(&ms, e0, e1);
  *ms_out = ms / iters;
  (void)hipEventDestroy(e0);
  (void)hipEventDestroy(e1);
  if (const char* tlp = getenv("DISSC_TIMELINE")) {  // diagnostics: the head of the accumulator buffer (a kernel's timeline stamps)
    std::vector<char> hb(std::min<size_t>(no * 4, (size_t)4096 * 64));
    if (hipMemcpy(hb.data(), a, hb.size(), hipMemcpyDeviceToHost) == hipSuccess)
      if (FILE* f = fopen(tlp, "wb")) {
        fwrite(hb.data(), 1, hb.size(), f);
        fclose(f);
      }
  }
  (void)hipFree(x); (void)hipFree(y); (void)hipFree(r); (void)hipFree(a);
  free_conv(dc);
  if (rc) return rc;
  DISSC_HIP_CHECK(e);
  return DISSC_OK;
}

}  // extern "C"
