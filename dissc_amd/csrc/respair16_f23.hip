// respair16_f23_kernel: the k = 11 residual pairs of the 16-channel stage as register-only Toom-Cook F(2,3) -- respair_f23.hip's
// scheme (four points held by one wave, B^T one addition per B operand, A^T three additions per output in registers, no V
// tiles, no exchange) on v_mfma_f32_16x16x4_f32: M = 16 rows, a k-step is 4 channels, the 16 channels of a conv are 4 k-steps.
// Both convs' transform-domain weights live in registers like respair16_kernel's taps do: 4 sub-filters x 4 points = 16 float4
// per conv (64 registers, loaded per conv) where the direct form holds 11; 8 products per output instead of 11.
// A wave's 4 column tiles x 16 columns = 64 output PAIRS = 128 outputs; geometry (F23Geo16) in respair_f23.h, weights and
// launch in pair_host.hip.  Further down: reschain16_f23_kernel, the whole k = 3 ResBlock of this stage in one launch.
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

// ---------------------------------------------------------------------------------------------
// reschain16_f23_kernel: the whole k = 3 ResBlock of the 16-channel stage -- three residual pairs, dilations (1, 3, 5) -- in one
// launch: reschain32_f23_kernel's scheme (respair_f23.hip) on v_mfma_f32_16x16x4_f32.  A wave holds the four points of four
// 16-column tiles (64 accumulators) and the raw x_k of its 128 outputs in conv_1's accumulator layout (32 registers); a conv's
// transform-domain weights are four float4 per lane, fetched one conv ahead.  The computed span is the same 512 outputs in every
// pair, of which the middle 488 are valid after the third (F23ChainGeo16).
// ---------------------------------------------------------------------------------------------
template <bool DBG>
__global__ void __launch_bounds__(256, 3) reschain16_f23_kernel(const PairArgs a) {
  using G = F23ChainGeo16;
  constexpr int C = G::C, NW = G::NW, NT = 64 * NW, XW = G::XW, PADL = G::PADL, HALO = G::HALO, WOUT = G::WOUT, PW = G::PW, NI = G::NI;
  static_assert(NI == 4, "four column tiles per wave");
  extern __shared__ __attribute__((aligned(16))) float xs[];  // [C][XW]

  int b, len, o0;
  if (!pair_tile<WOUT>(a, gridDim.y, b, len, o0)) return;
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int l15 = lane & 15, g = lane >> 4;
  const int t00 = o0 - HALO;  // the time of buffer coordinate 0
  const float slope = a.slope;
  const int dbg = DBG ? a.dbg : 0;  // (the knock-out branches around the tap loops cost the instance without them registers: two instances)
  const size_t ob = (size_t)b * a.bstride;
  const float* xb = a.x + ob;
  typedef float f32x2f __attribute__((ext_vector_type(2)));

  // a conv's weights: [point 4][64 lanes][4 k-steps], fetched one conv ahead
  const __amdgpu_buffer_rsrc_t wr = wave_rsrc(a.w1, 0x7ffffff0u);  // scalar-base loads (common.h), constant offsets
  f32x4 u[4];
  auto load_w = [&](int ci) __attribute__((always_inline)) {
#pragma unroll
    for (int p = 0; p < 4; ++p) u[p] = rsrc_load16(wr, lane * 16u, (unsigned)((ci * 4 + p) * 1024));
  };
  load_w(0);
  pair_stage_window<C, XW, NT>(a, xb, xs, t00 - PADL, len, tid);
  // (this and the bare fences below: without them loads and index math of later phases are hoisted into earlier ones and the
  // instance without knock-outs spills 16 registers at three workgroups per CU)
  __builtin_amdgcn_sched_barrier(0);

  // the wave's outputs: column col0 + 16 ni <-> buffer coordinates 2 col, 2 col + 1; their raw x_0 in conv_1's accumulator layout
  const int col0 = wave * 64 + l15;
  f32x2f res[NI][4];
#pragma unroll
  for (int ni = 0; ni < NI; ++ni) {
    const int tc0 = t00 + 2 * (col0 + 16 * ni);
    const int tcl = tc0 < 0 ? 0 : (tc0 > a.ld - 2 ? a.ld - 2 : tc0);  // (clamped: such outputs are neither stored nor fed on)
#pragma unroll
    for (int r = 0; r < 4; ++r) res[ni][r] = *reinterpret_cast<const f32x2f*>(xb + (size_t)(4 * g + r) * a.ld + tcl);
  }
  // one conv: per column tile 4 k-steps x 4 points = 16 MFMAs fed by 16 fragment reads and 16 additions, then A^T at once: the
  // tile's 16 accumulators become 8 outputs y[ni][r] = (even, odd) before the next tile starts (all four tiles' accumulators
  // held to the end do not fit three workgroups per CU next to the residual)
  f32x2f y[NI][4];
  auto taps = [&](const float* src, const int (&off)[NI], int dunit) __attribute__((always_inline)) {
#pragma unroll
    for (int ni = 0; ni < NI; ++ni) {
      f32x4 acc[4];
#pragma unroll
      for (int p = 0; p < 4; ++p)
#pragma unroll
        for (int e = 0; e < 4; ++e) acc[p][e] = 0.f;
#pragma unroll
      for (int cq = 0; cq < 4; ++cq) {
        const float* q = src + (4 * cq + g) * XW + off[ni];
        float x0, x1, x2, x3;
        if (dunit == 1) {  // (src + off is even in floats: 8-byte aligned)
          const f32x2f lo = *reinterpret_cast<const f32x2f*>(q), hi = *reinterpret_cast<const f32x2f*>(q + 2);
          x0 = lo[0]; x1 = lo[1]; x2 = hi[0]; x3 = hi[1];
        } else {
          x0 = q[0]; x1 = q[dunit]; x2 = q[2 * dunit]; x3 = q[3 * dunit];
        }
        float bq[4];
        bq[0] = x0 - x2;
        bq[1] = x1 + x2;
        bq[2] = x2 - x1;
        bq[3] = x1 - x3;
#pragma unroll
        for (int p = 0; p < 4; ++p) acc[p] = __builtin_amdgcn_mfma_f32_16x16x4f32(u[p][cq], bq[p], acc[p], 0, 0, 0);
      }
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        y[ni][r][0] = (acc[0][r] + acc[1][r]) + acc[2][r];
        y[ni][r][1] = (acc[1][r] - acc[2][r]) - acc[3][r];
      }
    }
  };
  auto clear = [&]() __attribute__((always_inline)) {  // (what a knocked-out tap loop leaves)
#pragma unroll
    for (int ni = 0; ni < NI; ++ni)
#pragma unroll
      for (int r = 0; r < 4; ++r) y[ni][r][0] = y[ni][r][1] = 0.f;
  };
  int pc[NI];
#pragma unroll
  for (int ni = 0; ni < NI; ++ni) pc[ni] = 2 * (col0 + 16 * ni);

#pragma unroll
  for (int m = 0; m < 3; ++m) {
    const int d = G::dil(m), T0 = G::t0(m), NC1 = G::nc1(m);
    int pe[NI], offd[NI];  // conv_d's columns: T at buffer coordinates pe, pe + d
#pragma unroll
    for (int ni = 0; ni < NI; ++ni) {
      const int c = col0 + 16 * ni, c1 = c < NC1 ? c : NC1 - 1;
      pe[ni] = T0 + 2 * d * (c1 / d) + (c1 % d);
      offd[ni] = pe[ni] - d;
    }
    __syncthreads();  // lrelu(x_m) is in place
    __builtin_amdgcn_sched_barrier(0);
    if (dbg & 1) clear();
    else taps(xs + PADL, offd, d);
    __builtin_amdgcn_sched_barrier(0);  // (not above the tap loop: into the registers it has just released)
    load_w(2 * m + 1);

    // ---- T = lrelu(conv_d + b1) inside the utterance, 0 outside, at LDS column PADL + 1 + p.  D layout: col = lane & 15, row = 4 g + r ----
    __syncthreads();  // every wave is done reading lrelu(x_m)
    __builtin_amdgcn_sched_barrier(0);
#pragma unroll
    for (int ni = 0; ni < NI; ++ni) {
      if (col0 + 16 * ni < NC1 && !(dbg & 2)) {
        const int te = t00 + pe[ni], to = te + d;
        const bool ine = te >= 0 && te < len, ino = to >= 0 && to < len;
#pragma unroll
        for (int r = 0; r < 4; ++r) {
          const int row = 4 * g + r;
          const float bz = a.b1[(2 * m) * C + row];
          float ve = y[ni][r][0] + bz, vo = y[ni][r][1] + bz;
          ve = ve > 0.f ? ve : ve * slope;
          vo = vo > 0.f ? vo : vo * slope;
          xs[row * XW + PADL + 1 + pe[ni]] = ine ? ve : 0.f;
          xs[row * XW + PADL + 1 + pe[ni] + d] = ino ? vo : 0.f;
        }
      }
    }
    __syncthreads();
    __builtin_amdgcn_sched_barrier(0);
    if (dbg & 1) clear();
    else taps(xs + PADL, pc, 1);  // (T of p - 1 .. p + 2)
    __builtin_amdgcn_sched_barrier(0);
    if (m < 2) load_w(2 * m + 2);

    // ---- x_m+1 = (conv_1 + b2) + x_m, in registers ----
#pragma unroll
    for (int ni = 0; ni < NI; ++ni)
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const float bz = a.b1[(2 * m + 1) * C + 4 * g + r];
        res[ni][r][0] = (y[ni][r][0] + bz) + res[ni][r][0];
        res[ni][r][1] = (y[ni][r][1] + bz) + res[ni][r][1];
      }
    __syncthreads();  // every wave is done reading T
    __builtin_amdgcn_sched_barrier(0);
    if (m < 2 && !(dbg & 2)) {  // lrelu(x_m+1), 0 outside the utterance, to the wave's own columns
#pragma unroll
      for (int ni = 0; ni < NI; ++ni) {
        const int tc0 = t00 + pc[ni];
        const bool in_e = tc0 >= 0 && tc0 < len, in_o = tc0 + 1 >= 0 && tc0 + 1 < len;
#pragma unroll
        for (int r = 0; r < 4; ++r) {
          f32x2f v;
          v[0] = in_e ? (res[ni][r][0] > 0.f ? res[ni][r][0] : res[ni][r][0] * slope) : 0.f;
          v[1] = in_o ? (res[ni][r][1] > 0.f ? res[ni][r][1] : res[ni][r][1] * slope) : 0.f;
          *reinterpret_cast<f32x2f*>(xs + (4 * g + r) * XW + PADL + pc[ni]) = v;
        }
      }
    }
  }

  // ---- epilogue: x_3 (or an MRF mode of it) through a wave-private patch [16][PW] -> 16 B per lane ----
  if (dbg & 4) {
    if (res[0][0][0] == 123.f && a.acc) a.acc[0] = 1.f;
    return;
  }
  float* ep = xs + wave * (16 * PW);
  const int prow = lane >> 5, pc4 = lane & 31;
  const int pq = wave * 128 + 4 * pc4;  // this lane's quad in buffer coordinates
  const int tq = t00 + pq;
  const bool live = pq >= HALO && pq < HALO + WOUT && tq < len;
  const int epi = a.epi;
#pragma unroll
  for (int ni = 0; ni < NI; ++ni)
#pragma unroll
    for (int r = 0; r < 4; ++r) *reinterpret_cast<f32x2f*>(ep + (4 * g + r) * PW + 2 * (16 * ni + l15)) = res[ni][r];
  __builtin_amdgcn_wave_barrier();
#pragma unroll
  for (int p = 0; p < 8; ++p) {
    const int row = 2 * p + prow;
    const f32x4 v = *reinterpret_cast<const f32x4*>(ep + row * PW + 4 * pc4);
    if (!live) continue;
    chain_store_tail(a, epi, ob + (size_t)row * a.ld + tq, v, len - tq);
  }
}

template __global__ void reschain16_f23_kernel<false>(const PairArgs);
template __global__ void reschain16_f23_kernel<true>(const PairArgs);
#define DISSC_INSTANCE(K_, D_) template __global__ void respair16_f23_kernel<K_, D_>(const PairArgs);
DISSC_PAIR_F23_SHAPES(DISSC_INSTANCE)
#undef DISSC_INSTANCE

}  // namespace dissc
