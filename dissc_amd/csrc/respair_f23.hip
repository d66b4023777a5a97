// respair32_f23_kernel: one residual pair y = x + conv_1(lrelu(conv_d(lrelu(x)))) of the 32-channel stage, k = 11 (reference
// sr/models.py:34-41), with BOTH convs in the Toom-Cook F(2,3) transform domain and NOTHING exchanged between waves.
//
// Why F(2,3) here when the wider stages use six and eight points (conv_wino.hip, conv_wino8.hip): what makes the transform
// domain lose at C <= 32 is not its arithmetic but the traffic around it -- V tiles written and re-read through LDS, Y_p
// exchanged between the waves that own the points.  With FOUR points (0, 1, -1, inf) one wave can hold all of them for its
// own columns (4 points x 2 column tiles x 16 accumulators = 128 registers at M = 32 rows), so
//   * B^T (entries 0 / +-1) is one subtraction or addition per B operand on the way from LDS to the MFMA:
//       b0 = x0 - x2, b1 = x1 + x2, b2 = x2 - x1, b3 = x1 - x3           (x_q = window sample at + q D)
//   * A^T is three additions per output, in registers: y_even = Y0 + Y1 + Y2, y_odd = Y1 - Y2 - Y3
//   * G (host, pair_host.hip): U_p = G w per triple of taps, rows (1, 0, 0), (1/2, 1/2, 1/2), (1/2, -1/2, 1/2), (0, 0, 1)
// and the kernel keeps the shape of respair32_kernel (respair.hip): window of lrelu(x) in LDS, conv_d, T = lrelu(. + b1) back
// into the same LDS, conv_1, wave-private epilogue patches.  The k = 11 taps are four sub-filters of three taps with tap
// stride NS = 4 (tap 11 is a zero: its samples still enter the transforms, so the window holds real data there); an MFMA
// column is an output PAIR (t, t + D), D = d NS: 4 products per 2 outputs and sub-filter = 8 per output instead of 11, and 4
// LDS fragment reads where the direct form makes 6.  A wave's 64 columns are 128 outputs, the workgroup's 256 columns 512
// (480 / 504 for d = 5 / 3, whose units of 2 D outputs do not divide 512).
// fp32 operands, fp32 products, fp32 accumulation on v_mfma_f32_32x32x2_f32; not bit-identical to the direct pair.
// Further down: the six-point pairs (respair32_tc6_kernel, respair64_tc6_kernel), the C = 64 F(2,3) pair (respair64_f23_kernel) and
// reschain32_f23_kernel, the whole k = 3 ResBlock of this stage in one launch.
// Geometry (F23Geo32, F23Geo64, F23ChainGeo, Tc6Geo) and what every pair kernel shares: respair_f23.h; weights, launch and dispatch: pair_host.hip.
#include "common.h"
#include "respair_f23.h"

namespace dissc {

template <int KS_, int DIL>
__global__ void __launch_bounds__(256, 2) respair32_f23_kernel(const PairArgs a) {
  using G = F23Geo32<KS_, DIL>;
  constexpr int C = G::C, NW = G::NW, NT = 64 * NW, NS = G::NS, P2 = G::P2, P1 = G::P1, D1 = G::D1, D2 = G::D2, XW = G::XW,
                W1 = G::W1, NC1 = G::NC1, NC2 = G::NC2, WOUT = G::WOUT, PW = G::PW;
  extern __shared__ __attribute__((aligned(16))) float xs[];  // [C][XW]

  int b, len, o0;
  if (!pair_tile<WOUT>(a, gridDim.y, b, len, o0)) return;
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int l31 = lane & 31, h = lane >> 5;
  const int tin0 = o0 - P2 - P1;
  const int tb = tin0 & ~3, sh = tin0 - tb;
  const float slope = a.slope;
  const float* xb = a.x + (size_t)b * a.bstride;

  pair_stage_window<C, XW, NT>(a, xb, xs, tb, len, tid);

  // this lane's two columns of each conv: column -> (unit tau, phase rho) -> first sample 2 D tau + rho
  int base1[2], base2[2];
#pragma unroll
  for (int ni = 0; ni < 2; ++ni) {
    int c = wave * 64 + ni * 32 + l31;
    const int c1 = c < NC1 ? c : NC1 - 1, c2 = c < NC2 ? c : NC2 - 1;
    base1[ni] = 2 * D1 * (c1 / D1) + (c1 % D1);
    base2[ni] = 2 * D2 * (c2 / D2) + (c2 % D2);
  }
  typedef float f32x16f __attribute__((ext_vector_type(16)));
  f32x16f acc[4][2];
  auto clear = [&]() __attribute__((always_inline)) {
#pragma unroll
    for (int p = 0; p < 4; ++p)
#pragma unroll
      for (int ni = 0; ni < 2; ++ni)
#pragma unroll
        for (int e = 0; e < 16; ++e) acc[p][ni][e] = 0.f;
  };
  // one conv: chunks of 16 channels x 4 sub-filters; per (chunk, sub-filter) 8 k-steps x 2 column tiles x 4 points = 64 MFMAs fed
  // by 64 fragment reads and 64 additions
  auto taps = [&](const float* wq, const float* src, const int (&base)[2], int off0, int dstep, int dunit) __attribute__((always_inline)) {
    const __amdgpu_buffer_rsrc_t wr = wave_rsrc(wq, 0x7ffffff0u);  // scalar-base loads (common.h), constant offsets
    const unsigned lane16 = lane * 16u;
    f32x4 av[4][2], avn[4][2];
#pragma unroll
    for (int p = 0; p < 4; ++p) {
      av[p][0] = rsrc_load16(wr, lane16, (p * 2 + 0) * 1024u);
      av[p][1] = rsrc_load16(wr, lane16, (p * 2 + 1) * 1024u);
    }
#pragma unroll
    for (int s = 0; s < 2 * NS; ++s) {  // s = chunk * NS + sub-filter
      const int sn = s + 1 < 2 * NS ? s + 1 : s;
#pragma unroll
      for (int p = 0; p < 4; ++p) {
        avn[p][0] = rsrc_load16(wr, lane16, ((sn * 4 + p) * 2 + 0) * 1024u);
        avn[p][1] = rsrc_load16(wr, lane16, ((sn * 4 + p) * 2 + 1) * 1024u);
      }
      __builtin_amdgcn_sched_barrier(0);
      const int chunk = s / NS, j = s % NS;
#pragma unroll
      for (int hf = 0; hf < 2; ++hf)
#pragma unroll
        for (int e = 0; e < 4; ++e) {
          const int row = 16 * chunk + 2 * (4 * hf + e) + h;
          float bq[4][2];
#pragma unroll
          for (int ni = 0; ni < 2; ++ni) {
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
            for (int ni = 0; ni < 2; ++ni)
              acc[p][ni] = __builtin_amdgcn_mfma_f32_32x32x2f32(av[p][hf][e], bq[p][ni], acc[p][ni], 0, 0, 0);
        }
      __builtin_amdgcn_sched_barrier(0);
#pragma unroll
      for (int p = 0; p < 4; ++p) {
        av[p][0] = avn[p][0];
        av[p][1] = avn[p][1];
      }
    }
  };

  __syncthreads();
  clear();
  if (!(a.dbg & 1)) taps(a.w1, xs, base1, sh, DIL, D1);

  // ---- T = lrelu(conv_d + b1) inside the utterance, 0 outside, into the same buffer: positions [0, W1) <-> times o0 - P2 + . ----
  __syncthreads();  // every wave is done reading the x window
  pair_zero_beyond_t<C, XW, W1, NT>(xs, tid);
#pragma unroll
  for (int ni = 0; ni < 2; ++ni) {
    const int c = wave * 64 + ni * 32 + l31;
    if (c < NC1 && !(a.dbg & 2)) {
      const int pe = 2 * D1 * (c / D1) + (c % D1), po = pe + D1;
      const int te = o0 - P2 + pe, to = te + D1;
      const bool ine = te >= 0 && te < len, ino = to >= 0 && to < len;
#pragma unroll
      for (int r = 0; r < 16; ++r) {
        const int row = (r & 3) + 8 * (r >> 2) + 4 * h;
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

  // ---- epilogue: y = x + conv_1 + b2 (or an MRF mode), 8 rows at a time through a wave-private patch [8][PW] ----
  __syncthreads();  // every wave is done reading T, which the patches overwrite
  float* ep = xs + wave * (8 * PW);
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
#pragma unroll
  for (int qd = 0; qd < 4; ++qd) {  // rows 8 qd .. 8 qd + 7
    f32x4 rv[4], pa[4];
#pragma unroll
    for (int p = 0; p < 4; ++p) {
      const int row = 8 * qd + 2 * p + prow;
      const int tc = tcol > a.ld - 4 ? a.ld - 4 : tcol;
      rv[p] = *reinterpret_cast<const f32x4*>(a.x + ob + (size_t)row * a.ld + tc);
      if (rmw && live && tcol + 4 <= len) pa[p] = *reinterpret_cast<const f32x4*>(a.acc + ob + (size_t)row * a.ld + tcol);
    }
    __builtin_amdgcn_wave_barrier();
#pragma unroll
    for (int ni = 0; ni < 2; ++ni) {
      const int cl = ni * 32 + l31;
      const int pe = 2 * D2 * (cl / D2) + (cl % D2);
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const int rr = 4 * qd + r;
        const float y0 = acc[0][ni][rr], y1 = acc[1][ni][rr], y2 = acc[2][ni][rr], y3 = acc[3][ni][rr];
        ep[(r + 4 * h) * PW + pe] = (y0 + y1) + y2;
        ep[(r + 4 * h) * PW + pe + D2] = (y1 - y2) - y3;
      }
    }
    __builtin_amdgcn_wave_barrier();
#pragma unroll
    for (int p = 0; p < 4; ++p) {
      const int prw = 2 * p + prow;
      f32x4 v = *reinterpret_cast<const f32x4*>(ep + prw * PW + 4 * pc4);
      if (!live) continue;
      const int row = 8 * qd + prw;
      const float bz = a.b2[row];
      const size_t idx = ob + (size_t)row * a.ld + tcol;
      pair_store_tail(a, epi, idx, v, bz, rv[p], [&] { return pa[p]; }, 0, len - tcol < 4 ? len - tcol : 4);
    }
  }
}

// ---------------------------------------------------------------------------------------------
// respair32_tc6_kernel: the same pair on SIX points (0, +-1, +-2, inf) used as F(3,4) -- three outputs of a four-tap sub-filter,
// still register-only.  k = 7 is NS = 2 sub-filters (taps j, j + 2, j + 4, j + 6; tap 7 is a zero), k = 11 is NS = 3: 6 products
// per 3 outputs and sub-filter = 4 per output at k = 7 (direct: 7) and 6 at k = 11 (F(2,3): 8).
//   * an MFMA column is a unit's phase: outputs t, t + D, t + 2 D (D = d NS; NS for conv_1) from the samples x_q at t + j d + q D
//   * B^T (conv_wino.hip's F(4,3) matrix) on the way from LDS to the MFMA, 8 fused multiply-adds and 4 additions per 6 operands:
//       b0 = 4 x0 - 5 x2 + x4      b1 = (x4 - 4 x2) + (x3 - 4 x1)      b3 = (x4 - x2) + 2 (x3 - x1)
//       b5 = 4 x1 - 5 x3 + x5      b2 = (x4 - 4 x2) - (x3 - 4 x1)      b4 = (x4 - x2) - 2 (x3 - x1)
//   * A^T in registers: y0 = Y0 + Y1 + Y2 + Y3 + Y4, y1 = (Y1 - Y2) + 2 (Y3 - Y4), y2 = (Y1 + Y2) + 4 (Y3 + Y4) + Y5
//   * G (host, kTc6G in pair_host.hip): U_p = G w per quadruple of taps
// Six points x 16 accumulators leave room for ONE 32-column tile per wave (two spill), and the weights of a (chunk,
// sub-filter) come one 8-channel half at a time, double-buffered (6 x 16 bytes per lane and step).  conv_d's columns are dealt
// over the workgroup's 128; conv_1's per wave (32 / D2 whole units, 96 outputs at k = 7 and 90 at k = 11), so that a wave's
// outputs are one contiguous range and its epilogue patch stays private.  At k = 11 that range starts 2 mod 4 in the odd
// waves: the patch is laid out from the 16-byte boundary below it and the two quads that straddle a neighbour's range are
// stored element by element.
// ---------------------------------------------------------------------------------------------
template <class G>
__device__ __forceinline__ void pair_tc6_body(const PairArgs a) {
  constexpr int C = G::C, NW = G::NW, NT = 64 * NW, NS = G::NS, P2 = G::P2, P1 = G::P1, D1 = G::D1, D2 = G::D2, XW = G::XW,
                W1 = G::W1, NC1 = G::NC1, NCW2 = G::NCW2, OW = G::OW, WOUT = G::WOUT, PW = G::PW, RB = G::RB, DIL = G::DIL;
  extern __shared__ __attribute__((aligned(16))) float xs[];  // [C][XW]

  int b, len, o0;
  if (!pair_tile<WOUT>(a, gridDim.y, b, len, o0)) return;
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int l31 = lane & 31, h = lane >> 5;
  const int ct = wave / RB, mrow = 32 * (wave % RB);  // the wave's column tile and the first row of its 32-row block
  const int tin0 = o0 - P2 - P1;
  const int tb = tin0 & ~3, sh = tin0 - tb;
  const float slope = a.slope;
  const float* xb = a.x + (size_t)b * a.bstride;

  pair_stage_window<C, XW, NT, RB>(a, xb, xs, tb, len, tid);

  // this lane's column of each conv: column -> (unit tau, phase rho) -> first sample 3 D tau + rho
  int base1, base2;
  {
    const int c = ct * 32 + l31;
    const int c1 = c < NC1 ? c : NC1 - 1, c2 = l31 < NCW2 ? l31 : NCW2 - 1;
    base1 = 3 * D1 * (c1 / D1) + (c1 % D1);
    base2 = ct * OW + 3 * D2 * (c2 / D2) + (c2 % D2);
  }
  typedef float f32x16f __attribute__((ext_vector_type(16)));
  f32x16f acc[6];
  auto clear = [&]() __attribute__((always_inline)) {
#pragma unroll
    for (int p = 0; p < 6; ++p)
#pragma unroll
      for (int e = 0; e < 16; ++e) acc[p][e] = 0.f;
  };
  // one conv: per (chunk of 16 channels, sub-filter, half of 8 channels) 4 k-steps x 6 points = 24 MFMAs fed by 24 fragment
  // reads and 48 transform instructions
  auto taps = [&](const float* wq, const float* src, int base, int dstep, int dunit) __attribute__((always_inline)) {
    const __amdgpu_buffer_rsrc_t wr = wave_rsrc(wq, 0x7ffffff0u);  // scalar-base loads (common.h), constant offsets
    const unsigned lane16 = lane * 16u;
    constexpr int NST = C / 16 * NS * 2;  // step = (chunk * NS + sub-filter) * 2 + half
    const unsigned wstep = (a.dbg & 8) ? 0u : 6 * 1024u;  // (knock-out: every step re-reads the first step's 6 KB)
    f32x4 av[6], avn[6];
#pragma unroll
    for (int p = 0; p < 6; ++p) av[p] = rsrc_load16(wr, lane16, p * 1024u);
#pragma unroll
    for (int st = 0; st < NST; ++st) {
      const int sn = st + 1 < NST ? st + 1 : st;
#pragma unroll
      for (int p = 0; p < 6; ++p) avn[p] = rsrc_load16(wr, lane16, sn * wstep + p * 1024u);
      __builtin_amdgcn_sched_barrier(0);
      const int chunk = (st >> 1) / NS, j = (st >> 1) % NS, hf = st & 1;
#pragma unroll
      for (int e = 0; e < 4; ++e) {
        const int row = 16 * chunk + 2 * (4 * hf + e) + h;
        const float* q = src + row * XW + base + j * dstep;
        const float x0 = q[0], x1 = q[dunit], x2 = q[2 * dunit], x3 = q[3 * dunit], x4 = q[4 * dunit], x5 = q[5 * dunit];
        const float pe = __builtin_fmaf(-4.f, x2, x4), po = __builtin_fmaf(-4.f, x1, x3), re = x4 - x2, ro = x3 - x1;
        float bq[6];
        bq[0] = __builtin_fmaf(4.f, x0, __builtin_fmaf(-5.f, x2, x4));
        bq[1] = pe + po;
        bq[2] = pe - po;
        bq[3] = __builtin_fmaf(2.f, ro, re);
        bq[4] = __builtin_fmaf(-2.f, ro, re);
        bq[5] = __builtin_fmaf(4.f, x1, __builtin_fmaf(-5.f, x3, x5));
#pragma unroll
        for (int p = 0; p < 6; ++p) acc[p] = __builtin_amdgcn_mfma_f32_32x32x2f32(av[p][e], bq[p], acc[p], 0, 0, 0);
      }
      __builtin_amdgcn_sched_barrier(0);
#pragma unroll
      for (int p = 0; p < 6; ++p) av[p] = avn[p];
    }
  };
  // A^T of accumulator element r: the unit's three outputs
  auto outs = [&](int r, float& y0, float& y1, float& y2) __attribute__((always_inline)) {
    const float s12 = acc[1][r] + acc[2][r], d12 = acc[1][r] - acc[2][r];
    const float s34 = acc[3][r] + acc[4][r], d34 = acc[3][r] - acc[4][r];
    y0 = (acc[0][r] + s12) + s34;
    y1 = __builtin_fmaf(2.f, d34, d12);
    y2 = __builtin_fmaf(4.f, s34, s12) + acc[5][r];
  };

  const int wslab = (wave % RB) * (C / 16 * NS * 2 * 6 * 256);  // the row block's slab of either conv's weights
  __syncthreads();
  clear();
  if (!(a.dbg & 1)) taps(a.w1 + wslab, xs + sh, base1, DIL, D1);

  // ---- T = lrelu(conv_d + b1) inside the utterance, 0 outside, into the same buffer: positions [0, W1) <-> times o0 - P2 + . ----
  __syncthreads();  // every wave is done reading the x window
  pair_zero_beyond_t<C, XW, W1, NT>(xs, tid);
  {
    const int c = ct * 32 + l31;
    if (c < NC1 && !(a.dbg & 2)) {
      const int p0 = 3 * D1 * (c / D1) + (c % D1);
      const int t0 = o0 - P2 + p0;
      const bool in0 = t0 >= 0 && t0 < len, in1 = t0 + D1 >= 0 && t0 + D1 < len, in2 = t0 + 2 * D1 >= 0 && t0 + 2 * D1 < len;
#pragma unroll
      for (int r = 0; r < 16; ++r) {
        const int row = mrow + (r & 3) + 8 * (r >> 2) + 4 * h;
        const float bz = a.b1[row];
        float v0, v1, v2;
        outs(r, v0, v1, v2);
        v0 += bz; v1 += bz; v2 += bz;
        v0 = v0 > 0.f ? v0 : v0 * slope;
        v1 = v1 > 0.f ? v1 : v1 * slope;
        v2 = v2 > 0.f ? v2 : v2 * slope;
        xs[row * XW + p0] = in0 ? v0 : 0.f;
        xs[row * XW + p0 + D1] = in1 ? v1 : 0.f;
        xs[row * XW + p0 + 2 * D1] = in2 ? v2 : 0.f;
      }
    }
  }
  __syncthreads();
  clear();
  if (!(a.dbg & 1)) taps(a.w2 + wslab, xs, base2, 1, D2);

  // ---- epilogue: y = x + conv_1 + b2 (or an MRF mode), 8 rows at a time through a wave-private patch [8][PW] ----
  __syncthreads();  // every wave is done reading T, which the patches overwrite
  float* ep = xs + wave * (8 * PW);
  const int prow = lane >> 5, pc4 = lane & 31;
  const int ws = ct * OW, woff = ws & 3;          // the wave's outputs [ws, ws + OW) of the tile
  const int ncol = ws - woff + 4 * pc4;           // this lane's quad
  const int tcol = o0 + ncol;
  const size_t ob = (size_t)b * a.bstride;
  const int wend = ws + OW < WOUT ? ws + OW : WOUT;
  const int elo = ncol < ws ? ws - ncol : 0;      // elements [elo, ehi) of the quad are this wave's, owned and inside the utterance
  const int ehi = (wend - ncol < len - tcol ? wend - ncol : len - tcol) < 4 ? (wend - ncol < len - tcol ? wend - ncol : len - tcol) : 4;
  const bool live = ehi > elo;
  const int epi = a.epi;
  const bool rmw = epi != EPI_RES && epi != EPI_MRF_SET;
  if (a.dbg & 4) {
    if (acc[0][0] == 123.f) a.out[0] = 1.f;
    return;
  }
  const int cl = l31 < NCW2 ? l31 : NCW2 - 1;  // (the lanes beyond the wave's columns rewrite its last one)
  const int pcol = woff + 3 * D2 * (cl / D2) + (cl % D2);
#pragma unroll
  for (int qd = 0; qd < 4; ++qd) {  // rows 8 qd .. 8 qd + 7
    __builtin_amdgcn_sched_barrier(0);  // (the loads of a later trip hoisted above this one spill: 96 accumulators are live)
    f32x4 rv[4], pa[4];  // (both from the clamped quad, unconditionally: used by the lanes whose quad is `full`)
    const int tc = tcol > a.ld - 4 ? a.ld - 4 : tcol;
#pragma unroll
    for (int p = 0; p < 4; ++p) rv[p] = *reinterpret_cast<const f32x4*>(a.x + ob + (size_t)(mrow + 8 * qd + 2 * p + prow) * a.ld + tc);
    if (rmw) {
#pragma unroll
      for (int p = 0; p < 4; ++p) pa[p] = *reinterpret_cast<const f32x4*>(a.acc + ob + (size_t)(mrow + 8 * qd + 2 * p + prow) * a.ld + tc);
    }
    __builtin_amdgcn_wave_barrier();
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      float y0, y1, y2;
      outs(4 * qd + r, y0, y1, y2);
      ep[(r + 4 * h) * PW + pcol] = y0;
      ep[(r + 4 * h) * PW + pcol + D2] = y1;
      ep[(r + 4 * h) * PW + pcol + 2 * D2] = y2;
    }
    __builtin_amdgcn_wave_barrier();
#pragma unroll
    for (int p = 0; p < 4; ++p) {
      const int prw = 2 * p + prow;
      f32x4 v = *reinterpret_cast<const f32x4*>(ep + prw * PW + (4 * pc4 < PW - 4 ? 4 * pc4 : PW - 4));
      if (!live) continue;
      const int row = mrow + 8 * qd + prw;
      const float bz = a.b2[row];
      const size_t idx = ob + (size_t)row * a.ld + tcol;
      pair_store_tail(a, epi, idx, v, bz, rv[p], [&] { return pa[p]; }, elo, ehi);
    }
  }
}

template <int KS_, int DIL>
__global__ void __launch_bounds__(256, (Tc6Geo<KS_, DIL>::OCC)) respair32_tc6_kernel(const PairArgs a) {
  pair_tc6_body<Tc6Geo<KS_, DIL>>(a);
}
template <int KS_, int DIL>
__global__ void __launch_bounds__(256, (Tc6Geo64<KS_, DIL>::OCC)) respair64_tc6_kernel(const PairArgs a) {
  pair_tc6_body<Tc6Geo64<KS_, DIL>>(a);
}

// ---------------------------------------------------------------------------------------------
// respair64_f23_kernel: the k = 3 residual pairs of the 64-channel stage in the same F(2,3) scheme with the roles of rows and
// columns swapped: a wave holds the four points of ONE 32-column tile under BOTH 32-row blocks (4 x 2 x 16 accumulators), so a B
// operand -- one LDS read and one addition -- feeds two MFMAs, and the weights come one 8-channel step at a time,
// double-buffered (4 points x 2 row blocks x 16 bytes per lane and step).  k = 3 is one sub-filter (NS = 1): a column is the
// output pair (t, t + d) of conv_d and (t, t + 1) of conv_1, whose four samples are two aligned 8-byte LDS reads.  A wave's 32
// columns are 64 outputs, the workgroup's 128 columns 256 (252 / 250 for d = 3 / 5); 252 / 248 / 248 of them are owned
// (F23Geo64).  The summation order over the input channels is ascending in steps of two, whatever the grid.
// ---------------------------------------------------------------------------------------------
template <int KS_, int DIL>
__global__ void __launch_bounds__(256, 2) respair64_f23_kernel(const PairArgs a) {
  using G = F23Geo64<KS_, DIL>;
  constexpr int C = G::C, NW = G::NW, NT = 64 * NW, P2 = G::P2, P1 = G::P1, D1 = G::D1, D2 = G::D2, XW = G::XW, W1 = G::W1,
                NC1 = G::NC1, NC2 = G::NC2, WOUT = G::WOUT, PW = G::PW;
  static_assert(G::NS == 1 && D2 == 1 && XW % 2 == 0, "one sub-filter; conv_1's samples pair up into 8-byte reads");
  extern __shared__ __attribute__((aligned(16))) float xs[];  // [C][XW]

  int b, len, o0;
  if (!pair_tile<WOUT>(a, gridDim.y, b, len, o0)) return;
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int l31 = lane & 31, h = lane >> 5;
  const int tin0 = o0 - P2 - P1;
  const int tb = tin0 & ~3, sh = tin0 - tb;
  const float slope = a.slope;
  const float* xb = a.x + (size_t)b * a.bstride;

  pair_stage_window<C, XW, NT, 2>(a, xb, xs, tb, len, tid);

  // this lane's column of each conv: column -> (unit tau, phase rho) -> first sample 2 D tau + rho
  const int col = wave * 32 + l31;
  const int c1 = col < NC1 ? col : NC1 - 1, c2 = col < NC2 ? col : NC2 - 1;
  const int base1 = 2 * D1 * (c1 / D1) + (c1 % D1), base2 = 2 * D2 * (c2 / D2) + (c2 % D2);
  typedef float f32x16f __attribute__((ext_vector_type(16)));
  typedef float f32x2f __attribute__((ext_vector_type(2)));
  f32x16f acc[4][2];
  auto clear = [&]() __attribute__((always_inline)) {
#pragma unroll
    for (int p = 0; p < 4; ++p)
#pragma unroll
      for (int mi = 0; mi < 2; ++mi)
#pragma unroll
        for (int e = 0; e < 16; ++e) acc[p][mi][e] = 0.f;
  };
  // one conv: 8 steps of 8 channels; per step 4 k-steps x 4 points x 2 row blocks = 32 MFMAs fed by 16 fragment reads (8 of 8
  // bytes where the samples are neighbours) and 16 additions
  auto taps = [&](const float* wq, const float* src, int dunit) __attribute__((always_inline)) {
    const __amdgpu_buffer_rsrc_t wr = wave_rsrc(wq, 0x7ffffff0u);  // scalar-base loads (common.h), constant offsets
    const unsigned lane16 = lane * 16u;
    constexpr int NST = C / 8;
    f32x4 av[4][2], avn[4][2];
#pragma unroll
    for (int p = 0; p < 4; ++p)
#pragma unroll
      for (int mi = 0; mi < 2; ++mi) av[p][mi] = rsrc_load16(wr, lane16, (p * 2 + mi) * 1024u);
#pragma unroll
    for (int st = 0; st < NST; ++st) {
      const int sn = st + 1 < NST ? st + 1 : st;
#pragma unroll
      for (int p = 0; p < 4; ++p)
#pragma unroll
        for (int mi = 0; mi < 2; ++mi) avn[p][mi] = rsrc_load16(wr, lane16, ((sn * 4 + p) * 2 + mi) * 1024u);
      __builtin_amdgcn_sched_barrier(0);
#pragma unroll
      for (int e = 0; e < 4; ++e) {
        const float* q = src + (8 * st + 2 * e + h) * XW;
        float x0, x1, x2, x3;
        if (dunit == 1) {  // (src + base is even in floats: 8-byte aligned)
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
        for (int p = 0; p < 4; ++p)
#pragma unroll
          for (int mi = 0; mi < 2; ++mi)
            acc[p][mi] = __builtin_amdgcn_mfma_f32_32x32x2f32(av[p][mi][e], bq[p], acc[p][mi], 0, 0, 0);
      }
      __builtin_amdgcn_sched_barrier(0);
#pragma unroll
      for (int p = 0; p < 4; ++p)
#pragma unroll
        for (int mi = 0; mi < 2; ++mi) av[p][mi] = avn[p][mi];
    }
  };

  __syncthreads();
  clear();
  if (!(a.dbg & 1)) taps(a.w1, xs + sh + base1, D1);

  // ---- T = lrelu(conv_d + b1) inside the utterance, 0 outside, into the same buffer: positions [0, W1) <-> times o0 - P2 + . ----
  __syncthreads();  // every wave is done reading the x window
  pair_zero_beyond_t<C, XW, W1, NT>(xs, tid);
  if (col < NC1 && !(a.dbg & 2)) {
    const int pe = base1, po = pe + D1;
    const int te = o0 - P2 + pe, to = te + D1;
    const bool ine = te >= 0 && te < len, ino = to >= 0 && to < len;
#pragma unroll
    for (int mi = 0; mi < 2; ++mi)
#pragma unroll
      for (int r = 0; r < 16; ++r) {
        const int row = 32 * mi + (r & 3) + 8 * (r >> 2) + 4 * h;
        const float bz = a.b1[row];
        const float y0 = acc[0][mi][r], y1 = acc[1][mi][r], y2 = acc[2][mi][r], y3 = acc[3][mi][r];
        float ve = (y0 + y1) + y2 + bz, vo = (y1 - y2) - y3 + bz;
        ve = ve > 0.f ? ve : ve * slope;
        vo = vo > 0.f ? vo : vo * slope;
        xs[row * XW + pe] = ine ? ve : 0.f;
        xs[row * XW + po] = ino ? vo : 0.f;
      }
  }
  __syncthreads();
  clear();
  if (!(a.dbg & 1)) taps(a.w2, xs + base2, D2);

  // ---- epilogue: y = x + conv_1 + b2 (or an MRF mode), 8 rows at a time through a wave-private patch [8][PW] ----
  __syncthreads();  // every wave is done reading T, which the patches overwrite
  float* ep = xs + wave * (8 * PW);
  const int prow = lane >> 4, pc4 = lane & 15;
  const int ncol = wave * 64 + 4 * pc4;
  const int tcol = o0 + ncol;
  const size_t ob = (size_t)b * a.bstride;
  const bool live = ncol < WOUT && tcol < len;
  const int epi = a.epi;
  const bool rmw = epi != EPI_RES && epi != EPI_MRF_SET;
  if (a.dbg & 4) {
    if (acc[0][0][0] == 123.f) a.out[0] = 1.f;
    return;
  }
  const int pcol = 2 * l31;  // (D2 = 1: the column's outputs are neighbours)
#pragma unroll
  for (int mq = 0; mq < 8; ++mq) {  // rows 8 mq .. 8 mq + 7
    const int mi = mq >> 2, qd = mq & 3;
    __builtin_amdgcn_sched_barrier(0);  // (the loads of a later trip hoisted above this one spill: 128 accumulators are live)
    f32x4 rv[2], pa[2];
    const int tc = tcol > a.ld - 4 ? a.ld - 4 : tcol;
#pragma unroll
    for (int p = 0; p < 2; ++p) {
      const int row = 8 * mq + 4 * p + prow;
      rv[p] = *reinterpret_cast<const f32x4*>(a.x + ob + (size_t)row * a.ld + tc);
      if (rmw && live && tcol + 4 <= len) pa[p] = *reinterpret_cast<const f32x4*>(a.acc + ob + (size_t)row * a.ld + tcol);
    }
    __builtin_amdgcn_wave_barrier();
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      const int rr = 4 * qd + r;
      const float y0 = acc[0][mi][rr], y1 = acc[1][mi][rr], y2 = acc[2][mi][rr], y3 = acc[3][mi][rr];
      f32x2f v;
      v[0] = (y0 + y1) + y2;
      v[1] = (y1 - y2) - y3;
      *reinterpret_cast<f32x2f*>(ep + (r + 4 * h) * PW + pcol) = v;
    }
    __builtin_amdgcn_wave_barrier();
#pragma unroll
    for (int p = 0; p < 2; ++p) {
      const int prw = 4 * p + prow;
      f32x4 v = *reinterpret_cast<const f32x4*>(ep + prw * PW + 4 * pc4);
      if (!live) continue;
      const int row = 8 * mq + prw;
      const float bz = a.b2[row];
      const size_t idx = ob + (size_t)row * a.ld + tcol;
      pair_store_tail(a, epi, idx, v, bz, rv[p], [&] { return pa[p]; }, 0, len - tcol < 4 ? len - tcol : 4);
    }
  }
}

// ---------------------------------------------------------------------------------------------
// reschain32_f23_kernel: the WHOLE k = 3 ResBlock of the 32-channel stage -- three residual pairs, dilations (1, 3, 5) -- in one
// launch, each conv in the F(2,3) scheme above (one sub-filter: a column is the output pair (t, t + d) of conv_d, (t, t + 1) of
// conv_1).  x_1 and x_2 never leave the CU and the residual is read once:
//   * a wave holds the four points of ONE 32-column tile (64 accumulators) and, in conv_1's accumulator layout, the raw x_k of
//     its 64 outputs (32 registers): conv_1's column map does not depend on d, so a wave owns the same outputs in every pair;
//   * x_k+1 = (A^T acc + b2) + x_k replaces those registers, and lrelu(x_k+1), zero outside the utterance, goes back into the
//     one LDS buffer for the next pair's conv_d;
//   * the computed span is the same 256 outputs in every pair, of which the middle 232 are valid after the third (F23ChainGeo);
//   * the 16 KB of a conv's weights are fetched while the epilogue before it runs.
// Per output and conv 2 C^2 products where three direct pairs execute 3 C^2, and one read of x plus one write of the result
// where they make three reads of x_k, three of the residual and three writes.
// ---------------------------------------------------------------------------------------------
template <bool DBG>
__global__ void __launch_bounds__(256, 2) reschain32_f23_kernel(const PairArgs a) {
  using G = F23ChainGeo32;
  constexpr int C = G::C, NW = G::NW, NT = 64 * NW, XW = G::XW, PADL = G::PADL, HALO = G::HALO, WOUT = G::WOUT, PW = G::PW;
  extern __shared__ __attribute__((aligned(16))) float xs[];  // [C][XW]

  int b, len, o0;
  if (!pair_tile<WOUT>(a, gridDim.y, b, len, o0)) return;
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int l31 = lane & 31, h = lane >> 5;
  const int t00 = o0 - HALO;  // the time of buffer coordinate 0
  const float slope = a.slope;
  const int dbg = DBG ? a.dbg : 0;  // (the knock-out branches around the tap loops cost the instance without them registers: two instances)
  const size_t ob = (size_t)b * a.bstride;
  const float* xb = a.x + ob;
  typedef float f32x16f __attribute__((ext_vector_type(16)));
  typedef float f32x2f __attribute__((ext_vector_type(2)));

  // a conv's weights: [8-channel step 4][point 4][64 lanes][4 k-steps], fetched one conv ahead
  const __amdgpu_buffer_rsrc_t wr = wave_rsrc(a.w1, 0x7ffffff0u);  // scalar-base loads (common.h), constant offsets
  const unsigned lane16 = lane * 16u;
  f32x4 wv[4][4];
  auto load_w = [&](int ci) __attribute__((always_inline)) {
#pragma unroll
    for (int st = 0; st < 4; ++st)
#pragma unroll
      for (int p = 0; p < 4; ++p) wv[st][p] = rsrc_load16(wr, lane16, (unsigned)(((ci * 4 + st) * 4 + p) * 1024));
  };
  load_w(0);

  pair_stage_window<C, XW, NT>(a, xb, xs, t00 - PADL, len, tid);

  // the wave's outputs: column col <-> buffer coordinates pc, pc + 1; their raw x_0 in conv_1's accumulator layout
  const int col = wave * 32 + l31, pc = 2 * col, tc0 = t00 + pc;
  const bool in_e = tc0 >= 0 && tc0 < len, in_o = tc0 + 1 >= 0 && tc0 + 1 < len;
  f32x2f res[16];
  {
    const int tcl = tc0 < 0 ? 0 : (tc0 > a.ld - 2 ? a.ld - 2 : tc0);  // (clamped: such outputs are neither stored nor fed on)
#pragma unroll
    for (int r = 0; r < 16; ++r)
      res[r] = *reinterpret_cast<const f32x2f*>(xb + (size_t)((r & 3) + 8 * (r >> 2) + 4 * h) * a.ld + tcl);
  }
  f32x16f acc[4];
  auto clear = [&]() __attribute__((always_inline)) {
#pragma unroll
    for (int p = 0; p < 4; ++p)
#pragma unroll
      for (int e = 0; e < 16; ++e) acc[p][e] = 0.f;
  };
  // one conv: 4 steps of 8 channels x 4 k-steps x 4 points = 64 MFMAs fed by 64 fragment reads (32 of 8 bytes where the samples
  // are neighbours) and 64 additions
  auto taps = [&](const float* src, int dunit) __attribute__((always_inline)) {
#pragma unroll
    for (int st = 0; st < 4; ++st)
#pragma unroll
      for (int e = 0; e < 4; ++e) {
        const float* q = src + (8 * st + 2 * e + h) * XW;
        float x0, x1, x2, x3;
        if (dunit == 1) {  // (src is even in floats: 8-byte aligned)
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
        for (int p = 0; p < 4; ++p) acc[p] = __builtin_amdgcn_mfma_f32_32x32x2f32(wv[st][p][e], bq[p], acc[p], 0, 0, 0);
      }
  };

#pragma unroll
  for (int m = 0; m < 3; ++m) {
    const int d = G::dil(m), T0 = G::t0(m), NC1 = G::nc1(m);
    const int c1 = col < NC1 ? col : NC1 - 1;
    const int pe = T0 + 2 * d * (c1 / d) + (c1 % d);  // conv_d's column: T at buffer coordinates pe, pe + d
    __syncthreads();  // lrelu(x_m) is in place
    clear();
    if (!(dbg & 1)) taps(xs + PADL + pe - d, d);
    load_w(2 * m + 1);

    // ---- T = lrelu(conv_d + b1) inside the utterance, 0 outside, at LDS column PADL + 1 + p ----
    __syncthreads();  // every wave is done reading lrelu(x_m)
    if (col < NC1 && !(dbg & 2)) {
      const int te = t00 + pe, to = te + d;
      const bool ine = te >= 0 && te < len, ino = to >= 0 && to < len;
#pragma unroll
      for (int r = 0; r < 16; ++r) {
        const int row = (r & 3) + 8 * (r >> 2) + 4 * h;
        const float bz = a.b1[(2 * m) * C + row];
        const float y0 = acc[0][r], y1 = acc[1][r], y2 = acc[2][r], y3 = acc[3][r];
        float ve = (y0 + y1) + y2 + bz, vo = (y1 - y2) - y3 + bz;
        ve = ve > 0.f ? ve : ve * slope;
        vo = vo > 0.f ? vo : vo * slope;
        xs[row * XW + PADL + 1 + pe] = ine ? ve : 0.f;
        xs[row * XW + PADL + 1 + pe + d] = ino ? vo : 0.f;
      }
    }
    __syncthreads();
    clear();
    if (!(dbg & 1)) taps(xs + PADL + pc, 1);  // (T of p - 1 .. p + 2)
    if (m < 2) load_w(2 * m + 2);

    // ---- x_m+1 = (conv_1 + b2) + x_m, in registers ----
#pragma unroll
    for (int r = 0; r < 16; ++r) {
      const float bz = a.b1[(2 * m + 1) * C + (r & 3) + 8 * (r >> 2) + 4 * h];
      const float y0 = acc[0][r], y1 = acc[1][r], y2 = acc[2][r], y3 = acc[3][r];
      res[r][0] = (((y0 + y1) + y2) + bz) + res[r][0];
      res[r][1] = (((y1 - y2) - y3) + bz) + res[r][1];
    }
    __syncthreads();  // every wave is done reading T
    if (m < 2 && !(dbg & 2)) {  // lrelu(x_m+1), 0 outside the utterance, to the wave's own columns
#pragma unroll
      for (int r = 0; r < 16; ++r) {
        f32x2f v;
        v[0] = in_e ? (res[r][0] > 0.f ? res[r][0] : res[r][0] * slope) : 0.f;
        v[1] = in_o ? (res[r][1] > 0.f ? res[r][1] : res[r][1] * slope) : 0.f;
        *reinterpret_cast<f32x2f*>(xs + ((r & 3) + 8 * (r >> 2) + 4 * h) * XW + PADL + pc) = v;
      }
    }
  }

  // ---- epilogue: x_3 (or an MRF mode of it), 8 rows at a time through a wave-private patch [8][PW] -> 16 B per lane ----
  if (dbg & 4) {
    if (res[0][0] == 123.f && a.acc) a.acc[0] = 1.f;
    return;
  }
  float* ep = xs + wave * (8 * PW);
  const int prow = lane >> 4, pc4 = lane & 15;
  const int pq = wave * 64 + 4 * pc4;  // this lane's quad in buffer coordinates
  const int tq = t00 + pq;
  const bool live = pq >= HALO && pq < HALO + WOUT && tq < len;
  const int epi = a.epi;
#pragma unroll
  for (int mq = 0; mq < 4; ++mq) {  // rows 8 mq .. 8 mq + 7
    __builtin_amdgcn_wave_barrier();
#pragma unroll
    for (int r = 0; r < 4; ++r) *reinterpret_cast<f32x2f*>(ep + (r + 4 * h) * PW + 2 * l31) = res[4 * mq + r];
    __builtin_amdgcn_wave_barrier();
#pragma unroll
    for (int p = 0; p < 2; ++p) {
      const int prw = 4 * p + prow;
      const f32x4 v = *reinterpret_cast<const f32x4*>(ep + prw * PW + 4 * pc4);
      if (!live) continue;
      chain_store_tail(a, epi, ob + (size_t)(8 * mq + prw) * a.ld + tq, v, len - tq);
    }
  }
}

template __global__ void reschain32_f23_kernel<false>(const PairArgs);
template __global__ void reschain32_f23_kernel<true>(const PairArgs);
#define DISSC_INSTANCE(K_, D_) template __global__ void respair32_f23_kernel<K_, D_>(const PairArgs);
DISSC_PAIR_F23_SHAPES(DISSC_INSTANCE)
#undef DISSC_INSTANCE
#define DISSC_INSTANCE(K_, D_) template __global__ void respair32_tc6_kernel<K_, D_>(const PairArgs);
DISSC_PAIR_TC6_SHAPES(DISSC_INSTANCE)
#undef DISSC_INSTANCE
#define DISSC_INSTANCE(K_, D_) template __global__ void respair64_f23_kernel<K_, D_>(const PairArgs);
DISSC_PAIR_F23_C64_SHAPES(DISSC_INSTANCE)
#undef DISSC_INSTANCE
#define DISSC_INSTANCE(K_, D_) template __global__ void respair64_tc6_kernel<K_, D_>(const PairArgs);
DISSC_PAIR_TC6_SHAPES(DISSC_INSTANCE)
#undef DISSC_INSTANCE

}  // namespace dissc
