// respair16_f23_kernel: the k = 11 residual pairs of the 16-channel stage as register-only Toom-Cook F(2,3) -- respair_f23.hip's
// scheme (four points held by one wave, B^T one addition per B operand, A^T three additions per output in registers, no V
// tiles, no exchange) on v_mfma_f32_16x16x4_f32: M = 16 rows, a k-step is 4 channels, the 16 channels of a conv are 4 k-steps.
// Both convs' transform-domain weights live in registers like respair16_kernel's taps do: 4 sub-filters x 4 points = 16 float4
// per conv (64 registers, loaded per conv) where the direct form holds 11; 8 products per output instead of 11.
// A wave's 4 column tiles x 16 columns = 64 output PAIRS = 128 outputs; geometry (F23Geo16) in respair_f23.h, weights and
// launch in pair_host.hip.
#include "common.h"
#include "respair_f23.h"

namespace dissc {

template <int KS_, int DIL>
__global__ void __launch_bounds__(256, 3) respair16_f23_kernel(const PairArgs a) {
  using G = F23Geo16<KS_, DIL>;
  constexpr int C = G::C, NW = G::NW, NT = 64 * NW, NS = G::NS, P2 = G::P2, P1 = G::P1, D1 = G::D1, D2 = G::D2, XW = G::XW,
                W1 = G::W1, NC1 = G::NC1, NC2 = G::NC2, WOUT = G::WOUT, PW = G::PW, NI = 4;
  extern __shared__ __attribute__((aligned(16))) float xs[];  // [C][XW]

  int b, len, o0;
  if (!pair_tile<WOUT>(a, gridDim.y, b, len, o0)) return;
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int l15 = lane & 15, g = lane >> 4;
  const int tin0 = o0 - P2 - P1;
  const int tb = tin0 & ~3, sh = tin0 - tb;
  const float slope = a.slope;
  const float* xb = a.x + (size_t)b * a.bstride;

  pair_stage_window<C, XW, NT>(a, xb, xs, tb, len, tid);

  // this lane's four columns of each conv: column -> (unit tau, phase rho) -> first sample 2 D tau + rho
  int base1[NI], base2[NI];
#pragma unroll
  for (int ni = 0; ni < NI; ++ni) {
    const int c = wave * 64 + ni * 16 + l15;
    const int c1 = c < NC1 ? c : NC1 - 1, c2 = c < NC2 ? c : NC2 - 1;
    base1[ni] = 2 * D1 * (c1 / D1) + (c1 % D1);
    base2[ni] = 2 * D2 * (c2 / D2) + (c2 % D2);
  }
  f32x4 acc[4][NI];
  auto clear = [&]() __attribute__((always_inline)) {
#pragma unroll
    for (int p = 0; p < 4; ++p)
#pragma unroll
      for (int ni = 0; ni < NI; ++ni)
#pragma unroll
        for (int e = 0; e < 4; ++e) acc[p][ni][e] = 0.f;
  };
  // one conv: 4 sub-filters x 4 k-steps x 4 column tiles x 4 points = 256 MFMAs fed by 256 fragment reads and 256 additions;
  // the conv's 16 weight fragments [sub-filter][point] (one float4 = the 4 k-steps) stay in registers
  auto taps = [&](const float* wq, const float* src, const int (&base)[NI], int off0, int dstep, int dunit) __attribute__((always_inline)) {
    const __amdgpu_buffer_rsrc_t wr = wave_rsrc(wq, 0x7ffffff0u);  // scalar-base loads (common.h), constant offsets
    f32x4 u[NS][4];
#pragma unroll
    for (int j = 0; j < NS; ++j)
#pragma unroll
      for (int p = 0; p < 4; ++p) u[j][p] = rsrc_load16(wr, lane * 16u, (j * 4 + p) * 1024u);
#pragma unroll
    for (int j = 0; j < NS; ++j) {
#pragma unroll
      for (int cq = 0; cq < 4; ++cq) {
        const int row = 4 * cq + g;
        float bq[4][NI];
#pragma unroll
        for (int ni = 0; ni < NI; ++ni) {
          const float* q = src + row * XW + off0 + base[ni] + j * dstep;
          const float x0 = q[0], x1 = q[dunit], x2 = q[2 * dunit], x3 = q[3 * dunit];
          bq[0][ni] = x0 - x2;
          bq[1][ni] = x1 + x2;
          bq[2][ni] = x2 - x1;
          bq[3][ni] = x1 - x3;
        }
#pragma unroll
        for (int p = 0; p < 4; ++p)
#pragma unroll
          for (int ni = 0; ni < NI; ++ni)
            acc[p][ni] = __builtin_amdgcn_mfma_f32_16x16x4f32(u[j][p][cq], bq[p][ni], acc[p][ni], 0, 0, 0);
      }
      __builtin_amdgcn_sched_barrier(0);
    }
  };

  __syncthreads();
  clear();
  if (!(a.dbg & 1)) taps(a.w1, xs, base1, sh, DIL, D1);

  // ---- T = lrelu(conv_d + b1) inside the utterance, 0 outside, into the same buffer.  D layout: col = lane & 15, row = 4 g + r ----
  __syncthreads();
  pair_zero_beyond_t<C, XW, W1, NT>(xs, tid);
#pragma unroll
  for (int ni = 0; ni < NI; ++ni) {
    const int c = wave * 64 + ni * 16 + l15;
    if (c < NC1 && !(a.dbg & 2)) {
      const int pe = 2 * D1 * (c / D1) + (c % D1), po = pe + D1;
      const int te = o0 - P2 + pe, to = te + D1;
      const bool ine = te >= 0 && te < len, ino = to >= 0 && to < len;
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const int row = 4 * g + r;
        const float bz = a.b1[row];
        const float y0 = acc[0][ni][r], y1 = acc[1][ni][r], y2 = acc[2][ni][r], y3 = acc[3][ni][r];
        float ve = (y0 + y1) + y2 + bz, vo = (y1 - y2) - y3 + bz;
        ve = ve > 0.f ? ve : ve * slope;
        vo = vo > 0.f ? vo : vo * slope;
        xs[row * XW + pe] = ine ? ve : 0.f;
        xs[row * XW + po] = ino ? vo : 0.f;
      }
    }
  }
  __syncthreads();
  clear();
  if (!(a.dbg & 1)) taps(a.w2, xs, base2, 0, 1, D2);

  // ---- epilogue: y = x + conv_1 + b2 (or an MRF mode) through a wave-private patch [16][PW] -> 16 B per lane ----
  __syncthreads();
  float* ep = xs + wave * (16 * PW);
  const int prow = lane >> 5, pc4 = lane & 31;
  const int ncol = wave * 128 + 4 * pc4;
  const int tcol = o0 + ncol;
  const size_t ob = (size_t)b * a.bstride;
  const bool live = ncol < WOUT && tcol < len;
  const int epi = a.epi;
  const bool rmw = epi != EPI_RES && epi != EPI_MRF_SET;
  if (a.dbg & 4) {
    if (acc[0][0][0] == 123.f) a.out[0] = 1.f;
    return;
  }
  f32x4 rv[8], pa[8];
#pragma unroll
  for (int p = 0; p < 8; ++p) {
    const int row = 2 * p + prow;
    const int tc = tcol > a.ld - 4 ? a.ld - 4 : tcol;
    rv[p] = *reinterpret_cast<const f32x4*>(a.x + ob + (size_t)row * a.ld + tc);
    if (rmw && live && tcol + 4 <= len) pa[p] = *reinterpret_cast<const f32x4*>(a.acc + ob + (size_t)row * a.ld + tcol);
  }
#pragma unroll
  for (int ni = 0; ni < NI; ++ni) {
    const int cl = ni * 16 + l15;
    const int pe = 2 * D2 * (cl / D2) + (cl % D2);
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      const float y0 = acc[0][ni][r], y1 = acc[1][ni][r], y2 = acc[2][ni][r], y3 = acc[3][ni][r];
      ep[(4 * g + r) * PW + pe] = (y0 + y1) + y2;
      ep[(4 * g + r) * PW + pe + D2] = (y1 - y2) - y3;
    }
  }
  __builtin_amdgcn_wave_barrier();
#pragma unroll
  for (int p = 0; p < 8; ++p) {
    const int row = 2 * p + prow;
    f32x4 v = *reinterpret_cast<const f32x4*>(ep + row * PW + 4 * pc4);
    if (!live) continue;
    const float bz = a.b2[row];
    const size_t idx = ob + (size_t)row * a.ld + tcol;
    pair_store_tail(a, epi, idx, v, bz, rv[p], [&] { return pa[p]; }, 0, len - tcol < 4 ? len - tcol : 4);
  }
}

#define DISSC_INSTANCE(K_, D_) template __global__ void respair16_f23_kernel<K_, D_>(const PairArgs);
DISSC_PAIR_F23_SHAPES(DISSC_INSTANCE)
#undef DISSC_INSTANCE

}  // namespace dissc
