// Host side of the one-launch residual pairs in the Toom-Cook transform domain: which shapes have an instance, packing, dispatch.
//   form 1: the register-only F(2,3) pairs (respair_f23.hip, respair16_f23.hip) -- the default for k = 11 at C = 16, and the
//           k = 3 pairs at C = 64 (respair64_f23_kernel, option "pair_f23_c64");
//   form 2: the register-only six-point F(3,4) pairs (respair_f23.hip) -- the default for k = 7 / 11 at C = 32, and the
//           k = 7 / 11 pairs at C = 64 (respair64_tc6_kernel, option "pair_tc6_c64");
//   chains: the k = 3 ResBlocks of the 16- / 32-channel stages as ONE register-only F(2,3) launch (reschain16_f23_kernel,
//           reschain32_f23_kernel; option "chain_f23"): make_chain_f23, launch_reschain_f23, chain_f23_info;
//   form 0: the F(4,3) pair kernel with the Y exchange through LDS (experimental/csrc/respair_wino.hip: its gate FAILED in round 4,
//           it is in DISSC_EXPERIMENTAL=1 builds only; experimental_stubs.hip answers for it otherwise).
#include <string.h>

#include <algorithm>
#include <vector>

#include "common.h"
#include "respair_f23.h"

namespace dissc {

// shapes with an instance.  Register-only F(2,3): k = 11 at C = 16 / 32 (k = 3 in DISSC_EXPERIMENTAL=1 builds), k = 3 at C = 64;
// six points: k = 7 / 11 at C = 32 / 64; the F(4,3) kernel: a point's weights must fit 64 registers per lane (C^2 NS / 64 <= 64)
bool pair_f23_supported(int C, int KS, int dil) {
  if (!(dil == 1 || dil == 3 || dil == 5)) return false;
  if (C == 64) return KS == 3;
  return (C == 16 || C == 32) && (KS == 11 || (KS == 3 && DISSC_EXPERIMENTAL));
}
bool pair_tc6_supported(int C, int KS, int dil) { return (C == 32 || C == 64) && (KS == 7 || KS == 11) && (dil == 1 || dil == 3 || dil == 5); }
bool pairw_supported(int C, int KS, int dil) {
  if (!pairw43_built()) return false;  // (the kernel is in DISSC_EXPERIMENTAL=1 builds only)
  if (!(dil == 1 || dil == 3 || dil == 5)) return false;
  if (C == 32) return KS == 7 || KS == 11;
  if (C == 64) return KS == 3;
  return false;
}
bool pair_form_supported(int form, int C, int KS, int dil) {
  return form == 2 ? pair_tc6_supported(C, KS, dil) : form == 1 ? pair_f23_supported(C, KS, dil) : pairw_supported(C, KS, dil);
}

// ---- weights of the register-only kernels ----
// F(2,3) weight transform at the points 0, 1, -1, inf
static const double kF23G[4][3] = {{1.0, 0.0, 0.0}, {0.5, 0.5, 0.5}, {0.5, -0.5, 0.5}, {0.0, 0.0, 1.0}};
// F(3,4) weight transform at the points 0, 1, -1, 2, -2, inf
static const double kTc6G[6][4] = {{1.0 / 4, 0.0, 0.0, 0.0},
                                   {-1.0 / 6, -1.0 / 6, -1.0 / 6, -1.0 / 6},
                                   {-1.0 / 6, 1.0 / 6, -1.0 / 6, 1.0 / 6},
                                   {1.0 / 24, 2.0 / 24, 4.0 / 24, 8.0 / 24},
                                   {1.0 / 24, -2.0 / 24, 4.0 / 24, -8.0 / 24},
                                   {0.0, 0.0, 0.0, 1.0}};

// w: [C][C][KS] -> U[p][co][ci][j] = sum_i G[p][i] w[co][ci][j + NS i] for the NS = ceil(KS / taps) sub-filters j (taps beyond
// KS are zeros): each sum in double over ascending i, rounded once
static std::vector<float> transform_taps(const float* w, int C, int KS, const double* G, int points, int taps) {
  const int NS = (KS + taps - 1) / taps;
  std::vector<float> U((size_t)points * C * C * NS);
  size_t o = 0;
  for (int p = 0; p < points; ++p)
    for (int cc = 0; cc < C * C; ++cc)
      for (int j = 0; j < NS; ++j) {
        double u = 0.0;
        for (int i = 0; i < taps; ++i)
          if (j + NS * i < KS) u += G[p * taps + i] * (double)w[(size_t)cc * KS + j + NS * i];
        U[o++] = (float)u;
      }
  return U;
}

static int pack_pair_reg(const float* w, float** dev, int C, int KS, int form) {
  if ((form != 1 && form != 2) || (C != 16 && C != 32 && C != 64) || (form == 2 && C == 16) || (form == 1 && C == 64 && KS != 3)) {
    // (a layout loop exists for these only)
    set_error("pack_pair_reg: no layout for form %d, C = %d", form, C);
    return DISSC_EINVAL;
  }
  const int points = form == 2 ? 6 : 4, taps = form == 2 ? 4 : 3, NS = (KS + taps - 1) / taps;
  const std::vector<float> U = transform_taps(w, C, KS, form == 2 ? &kTc6G[0][0] : &kF23G[0][0], points, taps);
  auto u = [&](int p, int co, int ci, int j) { return U[(((size_t)p * C + co) * C + ci) * NS + j]; };
  std::vector<float> packed(U.size());
  size_t o = 0;
  if (C == 16) {
    // respair16_f23_kernel: [sub-filter][point][lane][k-step]; lane l, k-step cq -> U_p[l & 15][4 cq + (l >> 4)][j]
    for (int j = 0; j < NS; ++j)
      for (int p = 0; p < 4; ++p)
        for (int lane = 0; lane < 64; ++lane)
          for (int cq = 0; cq < 4; ++cq) packed[o++] = u(p, lane & 15, 4 * cq + (lane >> 4), j);
  } else if (C == 64 && form == 2) {
    // respair64_tc6_kernel: respair32_tc6_kernel's map below with four chunks, one slab per 32-row block (a wave streams its own
    // slab, 6 KB per step): [row block 2][chunk 4][sub-filter][half 2][point 6][64 lanes][4 k-steps]
    for (int mi = 0; mi < 2; ++mi)
      for (int c = 0; c < 4; ++c)
        for (int j = 0; j < NS; ++j)
          for (int hf = 0; hf < 2; ++hf)
            for (int p = 0; p < 6; ++p)
              for (int lane = 0; lane < 64; ++lane)
                for (int e = 0; e < 4; ++e) packed[o++] = u(p, 32 * mi + (lane & 31), 16 * c + 2 * (4 * hf + e) + (lane >> 5), j);
  } else if (C == 64) {
    // respair64_f23_kernel (one sub-filter): [8-channel step 8][point 4][row block 2][64 lanes][4 k-steps]; lane l, k-step e ->
    // U_p[32 mi + (l & 31)][8 s + 2 e + (l >> 5)]
    for (int st = 0; st < 8; ++st)
      for (int p = 0; p < 4; ++p)
        for (int mi = 0; mi < 2; ++mi)
          for (int lane = 0; lane < 64; ++lane)
            for (int e = 0; e < 4; ++e) packed[o++] = u(p, 32 * mi + (lane & 31), 8 * st + 2 * e + (lane >> 5), 0);
  } else if (form == 1) {
    // respair32_f23_kernel: [chunk 2][sub-filter][point 4][half 2][64 lanes][4 k-steps]; lane l, k-step 4 hf + e ->
    // U_p[l & 31][16 chunk + 2 (4 hf + e) + (l >> 5)][j]
    for (int c = 0; c < 2; ++c)
      for (int j = 0; j < NS; ++j)
        for (int p = 0; p < 4; ++p)
          for (int hf = 0; hf < 2; ++hf)
            for (int lane = 0; lane < 64; ++lane)
              for (int e = 0; e < 4; ++e) packed[o++] = u(p, lane & 31, 16 * c + 2 * (4 * hf + e) + (lane >> 5), j);
  } else {
    // respair32_tc6_kernel: the same map with the half outside the point: [chunk 2][sub-filter][half 2][point 6][64 lanes][4 k-steps]
    for (int c = 0; c < 2; ++c)
      for (int j = 0; j < NS; ++j)
        for (int hf = 0; hf < 2; ++hf)
          for (int p = 0; p < 6; ++p)
            for (int lane = 0; lane < 64; ++lane)
              for (int e = 0; e < 4; ++e) packed[o++] = u(p, lane & 31, 16 * c + 2 * (4 * hf + e) + (lane >> 5), j);
  }
  return upload(packed, dev);
}

// ---- the k = 3 chains (reschain32_f23_kernel, reschain16_f23_kernel): six convs and six biases in one buffer each ----
bool chain_f23_supported(int C, int KS, const int* dil) {
  return (C == 16 || C == 32) && KS == 3 && dil && dil[0] == 1 && dil[1] == 3 && dil[2] == 5;
}

bool chain_f23_info(int C, int KS, const int* dil, ChainInfo& ci) {
  if (!chain_f23_supported(C, KS, dil)) return false;
  auto fill = [&](auto geo) {
    using G = decltype(geo);
    ci.wout = G::WOUT; ci.span = G::NP; ci.halo = G::HALO; ci.lds_bytes = (int)sizeof(float) * G::C * G::XW; ci.tiles_per_wave = G::NI;
  };
  if (C == 32) fill(F23ChainGeo32());
  else fill(F23ChainGeo16());
  return true;
}

int make_chain_f23(const float* const* w6, const float* const* b6, int C, float** dev_w, float** dev_b) {
  if (C != 16 && C != 32) {
    set_error("make_chain_f23: no instance for C = %d", C);
    return DISSC_EINVAL;
  }
  std::vector<float> packed, bias((size_t)6 * C, 0.f);
  packed.reserve((size_t)6 * 4 * C * C);
  for (int l = 0; l < 6; ++l) {
    const std::vector<float> U = transform_taps(w6[l], C, 3, &kF23G[0][0], 4, 3);  // one sub-filter
    auto u = [&](int p, int co, int ci) { return U[((size_t)p * C + co) * C + ci]; };
    if (C == 16) {
      // reschain16_f23_kernel: [conv 6][point 4][64 lanes][4 k-steps]; lane l, k-step cq -> U_p[l & 15][4 cq + (l >> 4)]
      for (int p = 0; p < 4; ++p)
        for (int lane = 0; lane < 64; ++lane)
          for (int cq = 0; cq < 4; ++cq) packed.push_back(u(p, lane & 15, 4 * cq + (lane >> 4)));
    } else {
      // reschain32_f23_kernel: [conv 6][8-channel step 4][point 4][64 lanes][4 k-steps]; lane l, k-step e ->
      // U_p[l & 31][8 st + 2 e + (l >> 5)]
      for (int st = 0; st < 4; ++st)
        for (int p = 0; p < 4; ++p)
          for (int lane = 0; lane < 64; ++lane)
            for (int e = 0; e < 4; ++e) packed.push_back(u(p, lane & 31, 8 * st + 2 * e + (lane >> 5)));
    }
    if (b6 && b6[l]) memcpy(bias.data() + (size_t)l * C, b6[l], C * sizeof(float));
  }
  int rc = upload(packed, dev_w);
  if (!rc) rc = upload(bias, dev_b);
  return rc;
}

int make_pairw(const float* w1, const float* b1, const float* w2, const float* b2, int C, int KS, int dil, int form, DevPairW& pw) {
  pw.form = form;
  if (!pair_form_supported(form, C, KS, dil)) {
    set_error("make_pairw: no instance for C = %d, k = %d, dilation %d", C, KS, dil);
    return DISSC_EINVAL;
  }
  pw.C = C; pw.KS = KS; pw.dil = dil;
  auto pack = [&](const float* w, float** dev) {
    return form ? pack_pair_reg(w, dev, C, KS, form) : pack_pairw43(w, C, KS, dev);
  };
  int rc = pack(w1, &pw.w1);
  if (!rc) rc = pack(w2, &pw.w2);
  std::vector<float> bb(C, 0.f);
  if (b1) memcpy(bb.data(), b1, C * sizeof(float));
  if (!rc) rc = upload(bb, &pw.b1);
  std::fill(bb.begin(), bb.end(), 0.f);
  if (b2) memcpy(bb.data(), b2, C * sizeof(float));
  if (!rc) rc = upload(bb, &pw.b2);
  return rc;
}

void free_pairw(DevPairW& pw) {
  for (float** q : {&pw.w1, &pw.w2, &pw.b1, &pw.b2}) {
    if (*q) (void)hipFree(*q);
    *q = nullptr;
  }
}

// ---- launches of the register-only kernels ----
// grid from Geo::WOUT, the one LDS buffer [C][XW] as dynamic shared memory; want_max_lds: the buffer exceeds the 64 KB a kernel
// gets without the attribute (once per device and instance: DeviceOnce, common.h)
template <auto Kernel, class Geo>
static int launch_pair_reg(const PairArgs& a, int B, int Lmax, hipStream_t stream, bool want_max_lds) {
  static DeviceOnce attr_once;
  if (want_max_lds) DISSC_HIP_CHECK(attr_once.max_lds(reinterpret_cast<const void*>(Kernel), 160 * 1024));
  dim3 grid((Lmax + Geo::WOUT - 1) / Geo::WOUT, B);
  hipLaunchKernelGGL(Kernel, grid, dim3(256), sizeof(float) * Geo::C * Geo::XW, stream, a);
  DISSC_HIP_CHECK(hipGetLastError());
  return DISSC_OK;
}

// every register-only instance, as DISSC_CASE(form, C, kernel, Geo, want_max_lds, k, dilation)
#define DISSC_TC6(K_, D_) DISSC_CASE(2, 32, respair32_tc6_kernel, Tc6Geo, true, K_, D_)
#define DISSC_TC6_64(K_, D_) DISSC_CASE(2, 64, respair64_tc6_kernel, Tc6Geo64, false, K_, D_)
#define DISSC_F23_32(K_, D_) DISSC_CASE(1, 32, respair32_f23_kernel, F23Geo32, true, K_, D_)
#define DISSC_F23_16(K_, D_) DISSC_CASE(1, 16, respair16_f23_kernel, F23Geo16, false, K_, D_)
#define DISSC_F23_64(K_, D_) DISSC_CASE(1, 64, respair64_f23_kernel, F23Geo64, true, K_, D_)
#define DISSC_PAIR_REG_INSTANCES                                                                          \
  DISSC_PAIR_TC6_SHAPES(DISSC_TC6) DISSC_PAIR_F23_SHAPES(DISSC_F23_32) DISSC_PAIR_F23_SHAPES(DISSC_F23_16) \
  DISSC_PAIR_F23_C64_SHAPES(DISSC_F23_64) DISSC_PAIR_TC6_SHAPES(DISSC_TC6_64)

// outputs a workgroup of the instance owns (the Geo::WOUT its launch sizes the grid by); 0: no register-only instance
int pair_reg_tile(int form, int C, int KS, int dil) {
#define DISSC_CASE(FORM_, C_, KERNEL_, GEO_, MAX_LDS_, K_, D_) \
  if (form == FORM_ && C == C_ && KS == K_ && dil == D_) return GEO_<K_, D_>::WOUT;
  DISSC_PAIR_REG_INSTANCES
#undef DISSC_CASE
  return 0;
}

int launch_respair_wino(const DevPairW& pw, const float* x, float* out, const Batch& bt, const EpiSpec& ep, int ld, float slope,
                        hipStream_t stream) {
  const int B = bt.B, Lmax = bt.Lmax;
  if (!pw.w1 || ep.epi == EPI_STORE || x == out || ld < 4 || ld % 4 || misaligned16(x) || misaligned16(out) || misaligned16(ep.acc) ||
      B <= 0 || Lmax <= 0) {
    set_error("launch_respair_wino: bad argument (C=%d k=%d d=%d ld=%d epi=%d)", pw.C, pw.KS, pw.dil, ld, ep.epi);
    return DISSC_EINVAL;
  }
  if (!pw.form) {
    if (pairw43_built()) return launch_pairw43(pw, x, out, bt, ep, ld, slope, stream);
    set_error("launch_respair_wino: no instance (the F(4,3) pair kernel is only in DISSC_EXPERIMENTAL=1 builds)");
    return DISSC_EINVAL;
  }
  PairArgs a;
  a.x = x; a.out = out; a.acc = ep.acc; a.w1 = pw.w1; a.w2 = pw.w2; a.b1 = pw.b1; a.b2 = pw.b2;
  a.lengths = bt.lengths; a.len_default = bt.len_default; a.len_mul = bt.len_mul; a.ld = ld;
  a.bstride = (long long)pw.C * ld; a.slope = slope; a.mrf_div = ep.mrf_div; a.epi = ep.epi; a.dbg = opts().kernel_dbg;
#define DISSC_CASE(FORM_, C_, KERNEL_, GEO_, MAX_LDS_, K_, D_)       \
  if (pw.form == FORM_ && pw.C == C_ && pw.KS == K_ && pw.dil == D_) \
    return launch_pair_reg<KERNEL_<K_, D_>, GEO_<K_, D_>>(a, B, Lmax, stream, MAX_LDS_);
  DISSC_PAIR_REG_INSTANCES
#undef DISSC_CASE
  set_error("launch_pair_f23: no instance of form %d for C = %d, k = %d, dilation %d", pw.form, pw.C, pw.KS, pw.dil);
  return DISSC_EINVAL;
}

template <class Geo, auto Kernel, auto KernelDbg>
static int launch_chain(const PairArgs& a, int B, int Lmax, hipStream_t stream) {
  dim3 grid((Lmax + Geo::WOUT - 1) / Geo::WOUT, B);
  // (the instance with the knock-outs only while "kernel_dbg" asks for one; the buffer is below the 64 KB a kernel gets unasked)
  hipLaunchKernelGGL(a.dbg ? KernelDbg : Kernel, grid, dim3(256), sizeof(float) * Geo::C * Geo::XW, stream, a);
  DISSC_HIP_CHECK(hipGetLastError());
  return DISSC_OK;
}

int launch_reschain_f23(const float* w, const float* bias, int C, const float* x, float* out, const Batch& bt, const EpiSpec& ep, int ld,
                        float slope, hipStream_t stream) {
  const int B = bt.B, Lmax = bt.Lmax;
  if (!w || !bias || !x || (C != 16 && C != 32) || ep.epi == EPI_STORE || (ep.epi == EPI_RES ? !out || x == out : !ep.acc || x == ep.acc) ||
      ld < 4 || ld % 4 || misaligned16(x) || misaligned16(out) || misaligned16(ep.acc) || B <= 0 || Lmax <= 0) {
    set_error("launch_reschain_f23: bad argument (C=%d ld=%d epi=%d)", C, ld, ep.epi);
    return DISSC_EINVAL;
  }
  PairArgs a;
  a.x = x; a.out = out; a.acc = ep.acc; a.w1 = w; a.w2 = nullptr; a.b1 = bias; a.b2 = nullptr;
  a.lengths = bt.lengths; a.len_default = bt.len_default; a.len_mul = bt.len_mul; a.ld = ld;
  a.bstride = (long long)C * ld; a.slope = slope; a.mrf_div = ep.mrf_div; a.epi = ep.epi; a.dbg = opts().kernel_dbg;
  if (C == 32) return launch_chain<F23ChainGeo32, reschain32_f23_kernel<false>, reschain32_f23_kernel<true>>(a, B, Lmax, stream);
  return launch_chain<F23ChainGeo16, reschain16_f23_kernel<false>, reschain16_f23_kernel<true>>(a, B, Lmax, stream);
}

}  // namespace dissc
