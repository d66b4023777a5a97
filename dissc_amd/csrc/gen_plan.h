// The ResBlock plan of a generator handle: which kernels run each chain and its pairs (gen_plan.hip).  Host only.
#pragma once
#include "common.h"

namespace dissc {

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
  f23_chain,  // fp32: the k = 3 block in one register-only F(2,3) launch (reschain32/16_f23_kernel); pair[] = the plan without it
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

ConvForm td_conv_form(int C, int KS, int dil);  // the transform-domain form of one conv of a PairForm::td pair
int pair_reg_form(int C, int KS, int dil);      // the register-only form of a pair (DevPairW::form: 1 F(2,3), 2 six points), or 0
ChainPlan plan_chain(int C, int KS, const int* dil, int prec);
double pair_macs(const PairPlan& p, int C, int KS, bool executed);  // multiply-adds per output position of one pair: algorithmic, or executed
double chain_macs(const ChainPlan& cp, int C, int KS, bool executed);  // ... of a whole chain in its form
int make_pair_conv(ConvForm f, const float* w, const float* b, int C, int KS, int dil, DevConv& dc);  // packed for its form
// ---- a ResBlock2 chain (two dilated convs, x = x + conv_d(lrelu(x)) twice): decided once per handle like plan_chain ----
enum class Rb2Form : uint8_t {
  two_launch,  // two direct conv launches, x_1 through the chain's XK buffer, the second with the MRF epilogue
  fused,       // one launch, x_1 in LDS (resblock2.hip)
};
Rb2Form plan_resblock2(int C, int KS, int d0, int d1, int prec);
// The MRF epilogue of chain j's last launch: xs = r_0; xs += r_j; x = (xs + r_last) / nk
inline int mrf_epi(int j, int nk) { return j == nk - 1 ? EPI_MRF_DIV : j == 0 ? EPI_MRF_SET : EPI_MRF_ADD; }

}  // namespace dissc
