// The ResBlock plan policy (gen_plan.h): the form options and what they choose.  Host only: no kernel here.
#include "gen_plan.h"

namespace dissc {

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
ConvForm td_conv_form(int C, int KS, int dil) {
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
// option "chain_f23" (default 3), a bit mask honoured only for fp32 handles while "wino" != 0, "pair_f23" != 0 and the stage is within
//   "pair_max_c" (a chain is a one-launch form like the pairs it replaces): 1 = the
//   k = 3, dilations (1, 3, 5) ResBlock of the 32-channel stage, 2 = that of the 16-channel stage runs as ONE register-only F(2,3)
//   launch (reschain32_f23_kernel in respair_f23.hip, reschain16_f23_kernel in respair16_f23.hip): 2 C^2 products per output and
//   conv where the three direct pairs it replaces execute 3 C^2, x_1 / x_2 and the residuals never leave the CU.  0 = three
//   one-launch pairs in the forms pair_reg_form() gives.  A chain-level choice: it does not enter pair_reg_form or dissc_pair_info.
//   Measurements: profiles/r14.
static bool chain_f23_wanted(int C, int KS, const int* dil, int prec) {
  const int bit = C == 32 ? 1 : C == 16 ? 2 : 0;
  return prec == 0 && opts().wino && opts().pair_f23 && C <= opts().pair_max_c && (opts().chain_f23 & bit) && chain_f23_supported(C, KS, dil);
}

int pair_reg_form(int C, int KS, int dil) {
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
ChainPlan plan_chain(int C, int KS, const int* dil, int prec) {
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
  if (chain_f23_wanted(C, KS, dil, prec)) cp.form = ChainForm::f23_chain;
  return cp;
}

// option "rb2_fused" (default 59), a bit mask honoured only for fp32 handles: the ResBlock2 blocks of the 32-channel stage with
//   k = 3 / 5 / 7 (bits 1 / 2 / 4) and of the 16-channel stage (bits 8 / 16 / 32) run as ONE launch each with x_1 in LDS
//   (resblock2_32_kernel / resblock2_16_kernel; instances: HiFi-GAN V3's (3; 1, 2), (5; 2, 6), (7; 3, 12)), bit-identical to
//   the two direct launches it replaces.  The mask holds the (C, k) whose one-launch form measured faster than its two launches
//   by more than the spread between blocks of the same form (tools/resblock2_bench.py, B = 32 x 10 s, medians of seven alternated
//   blocks, two launches -> one): C = 32: k = 3 584 -> 496 us, k = 5 709 -> 681, k = 7 877 -> 1 020 (it recomputes 72 of 256
//   columns of the first conv: OFF); C = 16: k = 3 496 -> 313, k = 5 562 -> 404, k = 7 676 -> 570.  Forward of the V3-block VCTK
//   model, 32 x 10 s: 14.23 ms all off, 13.80 all on.  profiles/resblock2.md.
static int rb2_bit(int C, int KS) { return (KS == 3 ? 1 : KS == 5 ? 2 : KS == 7 ? 4 : 0) << (C == 16 ? 3 : 0); }
Rb2Form plan_resblock2(int C, int KS, int d0, int d1, int prec) {
  const bool fused = prec == 0 && (C == 16 || opts().use_mfma32) && resblock2_supported(C, KS, d0, d1) && (opts().rb2_fused & rb2_bit(C, KS));
  return fused ? Rb2Form::fused : Rb2Form::two_launch;
}

double chain_macs(const ChainPlan& cp, int C, int KS, bool executed) {
  if (executed && cp.form == ChainForm::f23_chain) return 3 * 2 * 2.0 * C * C;  // F(2,3): 4 products per 2 outputs, six convs
  double macs = 0;
  for (const PairPlan& p : cp.pair) macs += pair_macs(p, C, KS, executed);
  return macs;
}

double pair_macs(const PairPlan& p, int C, int KS, bool executed) {
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

int make_pair_conv(ConvForm f, const float* w, const float* b, int C, int KS, int dil, DevConv& dc) {
  switch (f) {
    case ConvForm::f43: return make_wino(w, b, C, KS, dil, dc);
    case ConvForm::f63: return make_wino8(w, b, C, KS, dil, dc, 3);
    case ConvForm::f54: return make_wino8(w, b, C, KS, dil, dc, 4);
    default: return make_conv(w, b, C, C, KS, dil, dc);
  }
}

}  // namespace dissc
