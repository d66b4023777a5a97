// resblock2_16_kernel / resblock2_32_kernel: one ResBlock2 (HiFi-GAN V3's light block, reference sr/models.py:50-65) of the
// generator's narrow stages,
//
//     y1 = x  + conv_d0(lrelu(x))            y2 = y1 + conv_d1(lrelu(y1))            (k taps each)
//
// in ONE launch, exact fp32 on the matrix pipe, followed by the epilogue modes of the pair kernels (EPI_RES to out, or the
// MRF modes on acc).  At C = 32 / 16 a stride-1 conv launch is HBM-bound (respair.hip): the block as two conv launches moves six
// activation passes (read x twice, write y1, read y1 twice, write y2) where this kernel moves two and a re-read of x from L2.
// Built on respair.hip: its window stage, ragged tile walk, weight packings (16x16x4 at C = 16, 32x32x2 at C = 32: what make_conv
// produces) and store tail; the differences are the second conv's dilation and what is kept of the intermediate.
//
// y1 on the CU.  A workgroup computes y1 on SLOTS = 256 columns [o0 - P1, o0 - P1 + SLOTS), P1 = d1 (k - 1) / 2, from the x
// window [o0 - P1 - P0, ...), P0 = d0 (k - 1) / 2, and y2 on [o0, o0 + SLOTS), of which it owns the first WOUT = SLOTS - 2 P1:
// the (7; 3, 12) block recomputes a 36-column halo of the first conv per side (WOUT = 184 of 256 columns).  Two images of y1 go to
// LDS when the first conv's accumulators are final: lrelu(y1) with exact zeros left of column 0 and from `len` on (the reference's
// zero padding of y1 -- not bias + conv(zeros)), over the x window it replaces, and the raw y1 of the columns from o0 on, the
// second conv's residual.  Activation and masks are applied once per element, there; the tap loops hold LDS reads and MFMAs only.
//
// Bit-level: every output element sees the MFMA sequence of the two-launch path (taps outer, k-steps inner; (acc + bias) +
// residual; the MRF ops of ragged_epi.h), so the two forms are bit-identical; tests/test_gpu_resblock2.py holds them to that.
#include "common.h"
#include "respair_f23.h"

namespace dissc {

template <int KS, int D0, int D1>
struct Rb2Geo {
  static constexpr int NW = 4, NT = 64 * NW, SLOTS = 256;
  static constexpr int P0 = D0 * (KS - 1) / 2, P1 = D1 * (KS - 1) / 2;
  static constexpr int WOUT = (SLOTS - 2 * P1) & ~3;       // columns of y2 a workgroup owns
  static constexpr int XW1 = round32_16(3 + SLOTS + 2 * P0);  // lrelu(x) window
  static constexpr int XW2 = round32_16(SLOTS + 2 * P1);      // lrelu(y1): conv_d1's last slots read up to 2 P1 beyond it
  static constexpr int XW = XW1 > XW2 ? XW1 : XW2;            // one buffer: the x window, then lrelu(y1), then the patches
  static constexpr int YW = SLOTS + 4;                        // raw y1 from column o0 on: slot u at u - P1
  static_assert(WOUT > 0 && WOUT % 4 == 0 && P1 % 2 == 0, "owned quads are whole");
};

// the raw x of one accumulator element, for y1's residual (L2-hot: this workgroup staged the window a moment ago)
__device__ __forceinline__ float rb2_x_at(const float* xrow, int t, bool inside) {
  const float v = xrow[inside ? t : 0];  // an unconditional, in-bounds load
  return inside ? v : 0.f;
}

// ---- C = 16: v_mfma_f32_16x16x4_f32, each conv's weights in registers ------------------------------------------------------
template <int KS, int D0, int D1>
__global__ void __launch_bounds__(256) resblock2_16_kernel(const PairArgs a) {
  using G = Rb2Geo<KS, D0, D1>;
  constexpr int C = 16, NI = 4, NW = G::NW, NT = G::NT, SLOTS = G::SLOTS, P0 = G::P0, P1 = G::P1, WOUT = G::WOUT;
  constexpr int XW1 = G::XW1, XW2 = G::XW2, XW = G::XW, YW = G::YW;
  constexpr int CW = 16 * NI + 4;
  constexpr int LPR = 4 * NI, RPP = 64 / LPR;
  static_assert(16 * NI * NW == SLOTS && NW * 16 * CW <= C * XW, "the epilogue patches fit the buffer");
  __shared__ __attribute__((aligned(16))) float Xs[C * XW];  // lrelu(x) window, then lrelu(y1), then the epilogue patches
  __shared__ __attribute__((aligned(16))) float Yr[C * YW];  // raw y1 on [o0, o0 + SLOTS - P1)

  int b, len, o0;
  if (!pair_tile<WOUT>(a, gridDim.y, b, len, o0)) return;
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int l15 = lane & 15, g = lane >> 4;
  const int tin0 = o0 - P1 - P0;
  const int tb = tin0 & ~3, sh = tin0 - tb;
  const float slope = a.slope;
  const float* xb = a.x + (size_t)b * a.bstride;

  f32x4 wa[KS];
  {
    const __amdgpu_buffer_rsrc_t w1r = wave_rsrc(a.w1, 0x7ffffff0u);  // scalar-base loads (common.h)
#pragma unroll
    for (int j = 0; j < KS; ++j) wa[j] = rsrc_load16(w1r, lane * 16u, j * 1024u);
  }
  const f32x4 bias1 = *reinterpret_cast<const f32x4*>(a.b1 + 4 * g);
  pair_stage_window<C, XW1, NT>(a, xb, Xs, tb, len, tid);
  __syncthreads();

  // ---- conv_d0 on slots u <-> columns o0 - P1 + u ----
  f32x4 acc[NI];
#pragma unroll
  for (int ni = 0; ni < NI; ++ni) acc[ni] = f32x4{0.f, 0.f, 0.f, 0.f};
  {
    const float* bj = Xs + g * XW1 + sh + wave * (16 * NI) + l15;
#pragma unroll
    for (int j = 0; j < KS; ++j) {
#pragma unroll
      for (int cq = 0; cq < 4; ++cq)
#pragma unroll
        for (int ni = 0; ni < NI; ++ni)
          acc[ni] = __builtin_amdgcn_mfma_f32_16x16x4f32(wa[j][cq], bj[cq * 4 * XW1 + ni * 16 + j * D0], acc[ni], 0, 0, 0);
      if (j & 1) __builtin_amdgcn_sched_barrier(0);  // bounds how far the LDS reads are hoisted (register pressure)
    }
  }
  // conv_d1's weights take over the registers of conv_d0's
  {
    const __amdgpu_buffer_rsrc_t w2r = wave_rsrc(a.w2, 0x7ffffff0u);
#pragma unroll
    for (int j = 0; j < KS; ++j) wa[j] = rsrc_load16(w2r, lane * 16u, j * 1024u);
  }
  // y1 = (conv + b1) + x, the order of the two-launch path's EPI_RES.  C/D layout: col = lane & 15, row = 4 (lane >> 4) + r.
#pragma unroll
  for (int ni = 0; ni < NI; ++ni) {
    const int t = o0 - P1 + wave * (16 * NI) + ni * 16 + l15;
    const bool inside = t >= 0 && t < len;
#pragma unroll
    for (int r = 0; r < 4; ++r) acc[ni][r] = (acc[ni][r] + bias1[r]) + rb2_x_at(xb + (size_t)(4 * g + r) * a.ld, t, inside);
  }
  __syncthreads();  // every wave is done reading the x window lrelu(y1) is about to overwrite
#pragma unroll
  for (int ni = 0; ni < NI; ++ni) {
    const int u = wave * (16 * NI) + ni * 16 + l15;
    const int t = o0 - P1 + u;
    const bool inside = t >= 0 && t < len;
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      const float y1 = acc[ni][r];
      Xs[(4 * g + r) * XW2 + u] = inside ? lrelu(y1, slope) : 0.f;
      if (u >= P1) Yr[(4 * g + r) * YW + u - P1] = y1;
    }
  }
  __syncthreads();

  // ---- conv_d1 on slots u <-> columns o0 + u; the first WOUT of them are this workgroup's output ----
#pragma unroll
  for (int ni = 0; ni < NI; ++ni) acc[ni] = f32x4{0.f, 0.f, 0.f, 0.f};
  {
    const float* bt = Xs + g * XW2 + wave * (16 * NI) + l15;
#pragma unroll
    for (int j = 0; j < KS; ++j) {
#pragma unroll
      for (int cq = 0; cq < 4; ++cq)
#pragma unroll
        for (int ni = 0; ni < NI; ++ni)
          acc[ni] = __builtin_amdgcn_mfma_f32_16x16x4f32(wa[j][cq], bt[cq * 4 * XW2 + ni * 16 + j * D1], acc[ni], 0, 0, 0);
      if (j & 1) __builtin_amdgcn_sched_barrier(0);
    }
  }
  __syncthreads();  // lrelu(y1) is dead: the wave-private patches take its place
  float* patch = Xs + wave * (16 * CW);
#pragma unroll
  for (int ni = 0; ni < NI; ++ni)
#pragma unroll
    for (int r = 0; r < 4; ++r) patch[(4 * g + r) * CW + ni * 16 + l15] = acc[ni][r];
  __builtin_amdgcn_wave_barrier();
  const int prow = lane / LPR, pc4 = lane % LPR;
  const int ncol = wave * (16 * NI) + 4 * pc4;  // column within the slots
  const int tcol = o0 + ncol;
  const size_t ob = (size_t)b * a.bstride;
  if (ncol < WOUT && tcol < len) {
    const int n = len - tcol;
#pragma unroll
    for (int p = 0; p < NI; ++p) {
      const int row = p * RPP + prow;
      f32x4 v = *reinterpret_cast<const f32x4*>(patch + row * CW + 4 * pc4);
      const f32x4 res = *reinterpret_cast<const f32x4*>(Yr + row * YW + ncol);
      const float bz = a.b2[row];
#pragma unroll
      for (int e = 0; e < 4; ++e) v[e] = (v[e] + bz) + res[e];
      chain_store_tail(a, a.epi, ob + (size_t)row * a.ld + tcol, v, n);
    }
  }
}

// ---- C = 32: v_mfma_f32_32x32x2_f32 (64-cycle form), weights streamed tap by tap from L2 as in respair32_kernel ---------------
typedef float rb2_f32x16 __attribute__((ext_vector_type(16)));

template <int KS, int D0, int D1>
__global__ void __launch_bounds__(256) resblock2_32_kernel(const PairArgs a) {
  using G = Rb2Geo<KS, D0, D1>;
  constexpr int C = 32, NI = 2, NW = G::NW, NT = G::NT, SLOTS = G::SLOTS, P0 = G::P0, P1 = G::P1, WOUT = G::WOUT;
  constexpr int XW1 = G::XW1, XW2 = G::XW2, XW = G::XW, YW = G::YW;
  constexpr int CW = 32 * NI + 4;
  constexpr int LPR = 8 * NI, RPP = 64 / LPR, NPASS = 8 / RPP;
  static_assert(32 * NI * NW == SLOTS, "four waves of 64 columns");
  static_assert(NW * 8 * CW <= C * XW, "the epilogue patches fit the buffer");
  extern __shared__ __attribute__((aligned(16))) float rb2_lds[];  // 66-75 KB (above the static limit): two workgroups per CU
  float* const Xs = rb2_lds;               // [C][XW]  lrelu(x) window, then lrelu(y1), then the epilogue patches [NW][8][CW]
  float* const Yr = Xs + C * XW;           // [C][YW]  raw y1 on [o0, o0 + SLOTS - P1)
  float* const Ps = Xs;

  int b, len, o0;
  if (!pair_tile<WOUT>(a, gridDim.y, b, len, o0)) return;
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int l31 = lane & 31, h = lane >> 5;
  const int tin0 = o0 - P1 - P0;
  const int tb = tin0 & ~3, sh = tin0 - tb;
  const float slope = a.slope;
  const float* xb = a.x + (size_t)b * a.bstride;
  const __amdgpu_buffer_rsrc_t w1p = wave_rsrc(a.w1, 0x7ffffff0u), w2p = wave_rsrc(a.w2, 0x7ffffff0u);
  const unsigned lane16 = lane * 16u;
  f32x4 av[2], avn[2];
  av[0] = rsrc_load16(w1p, lane16, 0);
  av[1] = rsrc_load16(w1p, lane16, 1024u);

  pair_stage_window<C, XW1, NT, 2>(a, xb, Xs, tb, len, tid);
  __syncthreads();

  rb2_f32x16 acc[NI];
#pragma unroll
  for (int ni = 0; ni < NI; ++ni)
#pragma unroll
    for (int e = 0; e < 16; ++e) acc[ni][e] = 0.f;

  // step q = c * KS + j (chunk outer, tap inner: the order of conv_mfma32_kernel) = 8 k-steps = 2 float4, the next step's
  // fragments fetched behind the current 8 NI MFMAs (respair32_kernel's loop with the tap step a parameter)
#define DISSC_RB2_TAPS(WP, BASE, XWD, STEP, NEXT_WP)                                                        \
  _Pragma("unroll") for (int q = 0; q < 2 * KS; ++q) {                                                     \
    if (q + 1 < 2 * KS) {                                                                                  \
      avn[0] = rsrc_load16(WP, lane16, ((q + 1) * 2 + 0) * 1024u);                                         \
      avn[1] = rsrc_load16(WP, lane16, ((q + 1) * 2 + 1) * 1024u);                                         \
    } else {                                                                                               \
      avn[0] = rsrc_load16(NEXT_WP, lane16, 0);                                                            \
      avn[1] = rsrc_load16(NEXT_WP, lane16, 1024u);                                                        \
    }                                                                                                      \
    __builtin_amdgcn_sched_barrier(0);                                                                     \
    _Pragma("unroll") for (int hf = 0; hf < 2; ++hf)                                                       \
      _Pragma("unroll") for (int e = 0; e < 4; ++e)                                                        \
        _Pragma("unroll") for (int ni = 0; ni < NI; ++ni)                                                  \
          acc[ni] = __builtin_amdgcn_mfma_f32_32x32x2f32(                                                  \
              av[hf][e], BASE[((q / KS) * 16 + 2 * (4 * hf + e)) * XWD + ni * 32 + (q % KS) * STEP], acc[ni], 0, 0, 0); \
    __builtin_amdgcn_sched_barrier(0);                                                                     \
    av[0] = avn[0];                                                                                        \
    av[1] = avn[1];                                                                                        \
  }

  {
    const float* bj = Xs + h * XW1 + sh + wave * (32 * NI) + l31;
    DISSC_RB2_TAPS(w1p, bj, XW1, D0, w2p)  // leaves conv_d1's first tap in av
  }
  // y1 = (conv + b1) + x.  D layout: col = lane & 31, row = (r & 3) + 8 (r >> 2) + 4 (lane >> 5).
#pragma unroll
  for (int ni = 0; ni < NI; ++ni) {
    const int t = o0 - P1 + wave * (32 * NI) + ni * 32 + l31;
    const bool inside = t >= 0 && t < len;
#pragma unroll
    for (int r = 0; r < 16; ++r) {
      const int row = (r & 3) + 8 * (r >> 2) + 4 * h;
      acc[ni][r] = (acc[ni][r] + a.b1[row]) + rb2_x_at(xb + (size_t)row * a.ld, t, inside);
    }
  }
  __syncthreads();  // every wave is done reading the x window lrelu(y1) is about to overwrite
#pragma unroll
  for (int ni = 0; ni < NI; ++ni) {
    const int u = wave * (32 * NI) + ni * 32 + l31;
    const int t = o0 - P1 + u;
    const bool inside = t >= 0 && t < len;
#pragma unroll
    for (int r = 0; r < 16; ++r) {
      const int row = (r & 3) + 8 * (r >> 2) + 4 * h;
      const float y1 = acc[ni][r];
      Xs[row * XW2 + u] = inside ? lrelu(y1, slope) : 0.f;
      if (u >= P1) Yr[row * YW + u - P1] = y1;
    }
  }
  __syncthreads();
#pragma unroll
  for (int ni = 0; ni < NI; ++ni)
#pragma unroll
    for (int e = 0; e < 16; ++e) acc[ni][e] = 0.f;
  {
    const float* bt = Xs + h * XW2 + wave * (32 * NI) + l31;
    DISSC_RB2_TAPS(w2p, bt, XW2, D1, w2p)  // (the last prefetch re-reads tap 0: harmless)
  }
#undef DISSC_RB2_TAPS
  __syncthreads();  // lrelu(y1) is dead: the wave-private patches take its place
  // epilogue: 8 rows at a time through a wave-private patch [8][CW] -> 16 B per lane
  float* ep = Ps + wave * (8 * CW);
  const int prow = lane / LPR, pc4 = lane % LPR;
  const int ncol = wave * (32 * NI) + 4 * pc4;
  const int tcol = o0 + ncol;
  const size_t ob = (size_t)b * a.bstride;
  const bool live = ncol < WOUT && tcol < len;
  const int n = len - tcol;
#pragma unroll
  for (int qd = 0; qd < 4; ++qd) {  // rows 8 qd .. 8 qd + 7
    __builtin_amdgcn_wave_barrier();
#pragma unroll
    for (int ni = 0; ni < NI; ++ni)
#pragma unroll
      for (int r = 0; r < 4; ++r) ep[(r + 4 * h) * CW + ni * 32 + l31] = acc[ni][4 * qd + r];
    __builtin_amdgcn_wave_barrier();
#pragma unroll
    for (int p = 0; p < NPASS; ++p) {
      const int prw = p * RPP + prow;
      f32x4 v = *reinterpret_cast<const f32x4*>(ep + prw * CW + 4 * pc4);
      if (!live) continue;
      const int row = 8 * qd + prw;
      const f32x4 res = *reinterpret_cast<const f32x4*>(Yr + row * YW + ncol);
      const float bz = a.b2[row];
#pragma unroll
      for (int e = 0; e < 4; ++e) v[e] = (v[e] + bz) + res[e];
      chain_store_tail(a, a.epi, ob + (size_t)row * a.ld + tcol, v, n);
    }
  }
}

// ---- host side ----------------------------------------------------------------------------------------------------------------
// the instances: HiFi-GAN V3's three blocks (k; d0, d1) at both widths
#define DISSC_RB2_SHAPES(X) X(3, 1, 2) X(5, 2, 6) X(7, 3, 12)

bool resblock2_supported(int C, int KS, int d0, int d1) {
  if (C != 16 && C != 32) return false;
#define DISSC_RB2_IS(K, A, B) if (KS == K && d0 == A && d1 == B) return true;
  DISSC_RB2_SHAPES(DISSC_RB2_IS)
#undef DISSC_RB2_IS
  return false;
}

int resblock2_tile(int KS, int d0, int d1) {
#define DISSC_RB2_W(K, A, B) if (KS == K && d0 == A && d1 == B) return Rb2Geo<K, A, B>::WOUT;
  DISSC_RB2_SHAPES(DISSC_RB2_W)
#undef DISSC_RB2_W
  return 0;
}

template <int KS, int D0, int D1>
static int launch_rb2(const PairArgs& a, int C, int B, int Lmax, hipStream_t stream) {
  constexpr int WOUT = Rb2Geo<KS, D0, D1>::WOUT;
  dim3 grid((Lmax + WOUT - 1) / WOUT, B);
  if (C == 16) {
    hipLaunchKernelGGL((resblock2_16_kernel<KS, D0, D1>), grid, dim3(256), 0, stream, a);
  } else {
    using G = Rb2Geo<KS, D0, D1>;
    constexpr size_t lds = ((size_t)32 * G::XW + (size_t)32 * G::YW) * sizeof(float);
    static_assert(2 * lds <= 160 * 1024, "two workgroups per CU");
    static DeviceOnce attr_once;  // per device (common.h)
    DISSC_HIP_CHECK(attr_once.max_lds(reinterpret_cast<const void*>(&resblock2_32_kernel<KS, D0, D1>), (int)lds));
    hipLaunchKernelGGL((resblock2_32_kernel<KS, D0, D1>), grid, dim3(256), lds, stream, a);
  }
  DISSC_HIP_CHECK(hipGetLastError());
  return DISSC_OK;
}

// c1 / c2: the DevConvs of conv_d0 and conv_d1 (fp32, the packing make_conv gives the width)
int launch_resblock2(const DevConv& c1, const DevConv& c2, const float* x, float* out, const Batch& bt, const EpiSpec& ep, int ld,
                     float slope, hipStream_t stream) {
  const int C = c1.M, B = bt.B, Lmax = bt.Lmax;
  if (!resblock2_supported(C, c1.KS, c1.dil, c2.dil) || c2.KS != c1.KS || c1.m32 != (C == 32) || c2.m32 != (C == 32) || c1.prec ||
      c2.prec || c1.wino || c2.wino || c1.CIN != C || c2.CIN != C || c2.M != C || ep.epi == EPI_STORE || ep.epi > EPI_MRF_DIV ||
      x == out || (ld & 3) || misaligned16(x) || misaligned16(out) || misaligned16(ep.acc)) {
    set_error("launch_resblock2: unsupported block (C = %d, k = %d, dilations %d, %d)", C, c1.KS, c1.dil, c2.dil);
    return DISSC_EINVAL;
  }
  if (B <= 0 || Lmax <= 0) return DISSC_OK;
  if (B > 65535) {
    set_error("launch_resblock2: batch %d exceeds the grid limit", B);
    return DISSC_EINVAL;
  }
  PairArgs a;
  a.x = x; a.out = out; a.acc = ep.acc; a.w1 = c1.wpack; a.w2 = c2.wpack; a.b1 = c1.bias; a.b2 = c2.bias;
  a.lengths = bt.lengths; a.len_default = bt.len_default; a.len_mul = bt.len_mul; a.ld = ld;
  a.bstride = (long long)C * ld; a.slope = slope; a.mrf_div = ep.mrf_div; a.epi = ep.epi; a.dbg = 0;
#define DISSC_RB2_LAUNCH(K, A, B_) if (c1.KS == K && c1.dil == A && c2.dil == B_) return launch_rb2<K, A, B_>(a, C, B, Lmax, stream);
  DISSC_RB2_SHAPES(DISSC_RB2_LAUNCH)
#undef DISSC_RB2_LAUNCH
  set_error("launch_resblock2: no instance");
  return DISSC_EINVAL;
}

}  // namespace dissc
