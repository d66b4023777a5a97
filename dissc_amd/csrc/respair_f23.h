// What the one-launch residual-pair kernels share -- the direct pairs (respair.hip) and the register-only Toom-Cook pairs, F(2,3)
// on four points and F(3,4) on six (respair_f23.hip at C = 32, respair16_f23.hip at C = 16): the argument struct, the tile finder,
// the staging of the lrelu(x) window into LDS, the zero fill beyond T and the store tail; and, for the register-only kernels, the
// geometry, the declarations and the instance lists that pair_host.hip launches from.
#pragma once
#include "common.h"
#include "ragged_epi.h"

namespace dissc {

struct PairArgs {
  const float* x;   // [B][C][ld] pair input x_k
  float* out;       // EPI_RES: x_k' (may not alias x: neighbouring workgroups still read x's halo)
  float* acc;       // EPI_MRF_*: the stage accumulator
  const float* w1;  // conv_d / conv_1 weights in the kernel's fragment order (direct: DevConv::wpack; register-only: pair_host.hip)
  const float* w2;
  const float* b1;  // [C]
  const float* b2;
  const int32_t* lengths;
  int len_default, len_mul;
  int ld;
  long long bstride;
  float slope, mrf_div;
  int epi;
  int dbg;  // diagnostics ("kernel_dbg" option; the direct kernels ignore it): knock-outs -- bit 0 the tap loops, 1 the T epilogue,
            // 2 the output epilogue, 3 (six-point kernel) the weight stream: every step loads the first step's 6 KB
};

// (b, len, first output column) of workgroup (blockIdx.x: tile, blockIdx.y: utterance); with lengths only the tiles that
// EXIST are enumerated (ragged_tile)
template <int WOUT>
__device__ __forceinline__ bool pair_tile(const PairArgs& a, int B, int& b, int& len, int& o0) {
  if (a.lengths == nullptr) {
    b = blockIdx.y;
    len = a.len_default;
    o0 = blockIdx.x * WOUT;
    return o0 < len;
  }
  int tile;
  if (!ragged_tile<WOUT>(blockIdx.y * gridDim.x + blockIdx.x, B, [&](int i) { return a.lengths[i] * a.len_mul; }, b, tile, len))
    return false;
  o0 = tile * WOUT;
  return true;
}

// lrelu(x) on [tb, tb + XW) of the C rows at xb into xs[C][XW], 16 bytes per lane and trip: every load of a batch first (clamped,
// unconditional: loads issued one per trip would be as many dependent round trips), then activation, zeros outside [0, len) and
// the stores.  tb and ld are multiples of 4, so a clamped quad lies wholly outside the utterance and is zeroed.  NBATCH = 2 halves
// the staging registers where a kernel is short of them.
template <int C, int XW, int NT, int NBATCH = 1>
__device__ __forceinline__ void pair_stage_window(const PairArgs& a, const float* xb, float* xs, int tb, int len, int tid) {
  constexpr int NV = XW / 4, NIT = ((C * NV + NT - 1) / NT + NBATCH - 1) / NBATCH;
  const float slope = a.slope;
#pragma unroll
  for (int nb = 0; nb < NBATCH; ++nb) {
    f32x4 sv[NIT];
#pragma unroll
    for (int it = 0; it < NIT; ++it) {
      const int i = tid + (nb * NIT + it) * NT;
      const int r = i / NV < C ? i / NV : C - 1, v = i - (i / NV) * NV;
      const int t = tb + 4 * v;
      const int tc = t < 0 ? 0 : (t > a.ld - 4 ? a.ld - 4 : t);
      sv[it] = *reinterpret_cast<const f32x4*>(xb + (size_t)r * a.ld + tc);
    }
#pragma unroll
    for (int it = 0; it < NIT; ++it) {
      const int i = tid + (nb * NIT + it) * NT;
      if (i >= C * NV) continue;
      const int r = i / NV, v = i - r * NV;
      const int t = tb + 4 * v;
      f32x4 val = sv[it];
#pragma unroll
      // (lrelu() spelled out: through the call the register-only kernels compile to other code, 0.2-1.3 % slower per launch at C = 32)
      for (int e = 0; e < 4; ++e) val[e] = ((t + e) >= 0 && (t + e) < len) ? (val[e] > 0.f ? val[e] : val[e] * slope) : 0.f;
      *reinterpret_cast<f32x4*>(xs + r * XW + 4 * v) = val;
    }
  }
}

// zeros in xs[r][W1 .. XW): what conv_1's last columns read beyond T
template <int C, int XW, int W1, int NT>
__device__ __forceinline__ void pair_zero_beyond_t(float* xs, int tid) {
  for (int i = tid; i < C * (XW - W1); i += NT) {
    const int r = i / (XW - W1), v = i - r * (XW - W1);
    xs[r * XW + W1 + v] = 0.f;
  }
}

// Store tail of one row quad at idx: v from the epilogue patch, (v + bz) + residual, then the epilogue mode -- on the whole quad
// when its elements [elo, ehi) are all four (rv: the residual quad fetched earlier; acc_old(): the accumulator's old quad),
// element by element otherwise (a ragged tail, a quad shared with the neighbouring wave).
template <class AccOld>
__device__ __forceinline__ void pair_store_tail(const PairArgs& a, int epi, size_t idx, f32x4 v, float bz, const f32x4& rv,
                                                AccOld acc_old, int elo, int ehi) {
  if (elo == 0 && ehi == 4) {
#pragma unroll
    for (int e = 0; e < 4; ++e) v[e] = (v[e] + bz) + rv[e];
    epi_store_res(epi, quad_at(a.out + idx), quad_at(a.acc + idx), v, acc_old, a.mrf_div);
  } else {
    for (int e = elo; e < ehi; ++e)
      epi_store_res(epi, a.out + idx + e, a.acc + idx + e, (v[e] + bz) + a.x[idx + e], [&] { return a.acc[idx + e]; }, a.mrf_div);
  }
}

// ---- the register-only kernels: geometry, declarations, instances ----
// F(2,3): respair32_f23_kernel (C = 32, patches of 8 rows), respair16_f23_kernel (C = 16, patches of 16 rows) and
// respair64_f23_kernel (C = 64, patches of 8 rows; WCOLS = 32: one 32-column tile per wave under two 32-row blocks)
template <int C_, int PROWS, int KS_, int DIL, int WCOLS = 64>
struct F23Geo {
  static constexpr int KS = KS_, NS = (KS_ + 2) / 3, C = C_, NW = 4;
  static constexpr int P2 = (KS - 1) / 2, P1 = P2 * DIL;
  static constexpr int D1 = DIL * NS, D2 = NS;
  static constexpr int NCOLS = WCOLS * NW;                            // pair-columns per conv and workgroup
  static constexpr int NU1 = NCOLS / D1, NC1 = NU1 * D1, W1 = 2 * NC1;  // positions of T conv_d produces: [o0 - P2, o0 - P2 + W1)
  static constexpr int NU2 = NCOLS / D2, NC2 = NU2 * D2, W2 = 2 * NC2;  // outputs conv_1 computes: [o0, o0 + W2)
  static constexpr int WOUT = ((W1 - 2 * P2) < W2 ? (W1 - 2 * P2) : W2) & ~3;  // outputs a workgroup owns
  static constexpr int REACH1 = (3 * NS - 1) * DIL, REACH2 = 3 * NS - 1;       // samples read beyond the last column's first
  static constexpr int XW1 = round32_16(3 + W1 + REACH1);
  static constexpr int XW2 = round32_16(W2 + REACH2 + 1);
  static constexpr int XW = XW1 > XW2 ? XW1 : XW2;  // row stride of the one LDS buffer (x window, then T, then the patches)
  static constexpr int PW = 2 * WCOLS + 4;          // patch row: a wave's 2 WCOLS outputs
  static_assert(NW * PROWS * PW <= C * XW, "the epilogue patches fit the buffer");
  static_assert(W1 <= XW && W2 + REACH2 < XW, "T fits the buffer");
};
template <int KS, int DIL> using F23Geo32 = F23Geo<32, 8, KS, DIL>;
template <int KS, int DIL> using F23Geo16 = F23Geo<16, 16, KS, DIL>;
template <int KS, int DIL> using F23Geo64 = F23Geo<64, 8, KS, DIL, 32>;

// F(2,3) chains: reschain32_f23_kernel (C = 32, one 32-column tile per wave) and reschain16_f23_kernel (C = 16, four 16-column
// tiles per wave) run the three pairs of a k = 3 ResBlock, dilations (1, 3, 5), in one launch.  Everything is in BUFFER
// COORDINATES p <-> time o0 - HALO + p: the workgroup computes conv_1's outputs p in [0, NP) in every pair and owns
// [HALO, HALO + WOUT); lrelu(x_k) sits at LDS column PADL + p (the staged window is p in [-PADL, XW - PADL)), T at PADL + 1 + p
// (so conv_1's four samples of an output pair are two aligned 8-byte reads).  Pair m's conv_d produces T on
// [t0(m), t0(m) + w1(m)): whole units of 2 d positions dealt over the NCOLS columns.  What a column outside a pair's valid range
// computes is arbitrary but finite, stays inside the buffer and feeds no valid output: covers() walks the ranges.
template <int C_, int PROWS, int WCOLS>
struct F23ChainGeo {
  static constexpr int C = C_, NW = 4, KS = 3, NI = WCOLS / (C_ == 16 ? 16 : 32);
  static constexpr int NCOLS = WCOLS * NW, NP = 2 * NCOLS;  // pair-columns per conv and workgroup; computed span
  static constexpr int HALO = 12, PADL = 4;                 // 2 + 4 + 6 per side: d for conv_d and 1 for conv_1 per pair
  static constexpr int WOUT = NP - 2 * HALO;                // outputs a workgroup owns
  static constexpr int XW = round32_16(PADL + NP + 8);      // row stride of the one LDS buffer (x window / T / x_k+1 / patches)
  static constexpr int PW = 2 * WCOLS + 4;                  // patch row: a wave's 2 WCOLS outputs
  static constexpr int dil(int m) { return 2 * m + 1; }
  static constexpr int t0(int m) { return m == 0 ? 1 : m == 1 ? 3 : 4; }
  static constexpr int nc1(int m) { return NCOLS / dil(m) * dil(m); }
  static constexpr int w1(int m) { return 2 * nc1(m); }
  // x_0 is valid on the whole staged window; T_m where its three samples are valid x_m; x_m+1 where its three samples are valid
  // T_m, and only on [0, NP): what is written.  true: every read stays in the row and the owned outputs are valid x_3.
  static constexpr bool covers() {
    int a = -PADL, b = XW - PADL;
    for (int m = 0; m < 3; ++m) {
      const int d = dil(m), lo = t0(m), hi = t0(m) + w1(m);
      if (lo - d < -PADL || hi + d > XW - PADL || hi + 1 > XW - PADL) return false;  // conv_d's reads, T's writes
      const int tlo = lo > a + d ? lo : a + d, thi = hi < b - d ? hi : b - d;
      a = tlo + 1 > 0 ? tlo + 1 : 0;
      b = thi - 1 < NP ? thi - 1 : NP;
    }
    return a <= HALO && b >= HALO + WOUT;
  }
  static_assert(WOUT % 4 == 0 && HALO % 4 == 0 && PADL % 4 == 0, "owned quads are whole");
  static_assert(PADL + NP + 3 <= XW, "conv_1's reads of T stay in the row");
  static_assert(NW * PROWS * PW <= C * XW, "the epilogue patches fit the buffer");
};
using F23ChainGeo32 = F23ChainGeo<32, 8, 32>;
using F23ChainGeo16 = F23ChainGeo<16, 16, 64>;
static_assert(F23ChainGeo32::covers() && F23ChainGeo16::covers(), "each pair's valid range covers what the next pair reads");

// Store tail of the chain kernels: x = conv + bias + residual is complete in registers; n of the quad's elements lie inside
// the utterance.
__device__ __forceinline__ void chain_store_tail(const PairArgs& a, int epi, size_t idx, const f32x4& x, int n) {
  if (n >= 4) {
    epi_store_res(epi, quad_at(a.out + idx), quad_at(a.acc + idx), x, [&] { return load_quad(a.acc + idx); }, a.mrf_div);
  } else {
    for (int e = 0; e < n; ++e)
      epi_store_res(epi, a.out + idx + e, a.acc + idx + e, x[e], [&] { return a.acc[idx + e]; }, a.mrf_div);
  }
}

// six points: respair32_tc6_kernel and respair64_tc6_kernel (the scheme is described in respair_f23.hip).  At C = 64 the two 32-row
// blocks of a column tile go to a wave pair (RB = 2): wave w has column tile w / RB and row block w % RB, so a workgroup holds
// NCT = 2 column tiles where C = 32 holds 4.
template <int C_, int KS_, int DIL_>
struct Tc6GeoC {
  static constexpr int KS = KS_, DIL = DIL_, NS = (KS_ + 3) / 4, C = C_, NW = 4, RB = C_ / 32, NCT = NW / RB;
  static constexpr int P2 = (KS - 1) / 2, P1 = P2 * DIL;
  static constexpr int D1 = DIL * NS, D2 = NS;
  static constexpr int NCOLS = 32 * NCT;                                // columns of conv_d per workgroup
  static constexpr int NU1 = NCOLS / D1, NC1 = NU1 * D1, W1 = 3 * NC1;  // positions of T conv_d produces: [o0 - P2, o0 - P2 + W1)
  static constexpr int NCW2 = 32 / D2 * D2, OW = 3 * NCW2, W2 = NCT * OW;  // conv_1: columns and outputs per column tile, outputs [o0, o0 + W2)
  static constexpr int WOUT = ((W1 - 2 * P2) < W2 ? (W1 - 2 * P2) : W2) & ~3;  // outputs a workgroup owns
  static constexpr int REACH1 = (4 * NS - 1) * DIL, REACH2 = 4 * NS - 1;  // samples read beyond the conv's last position
  // row stride of the one LDS buffer (x window, then T, then the patches): a multiple of 4 and no more -- the two halves of a
  // wave read different rows, but a 4-byte LDS read serves them in separate passes, so the stride's residue modulo the 32 banks
  // buys nothing here, and rounding it to 16 mod 32 as the F(2,3) kernel does would cost the d = 3 / 5 shapes a workgroup per CU
  static constexpr int XW1 = (3 + W1 + REACH1 + 3) & ~3;
  static constexpr int XW2 = (W2 + REACH2 + 3) & ~3;
  static constexpr int XW = XW1 > XW2 ? XW1 : XW2;
  static constexpr int PW = 96 + 4;                 // patch row: a wave's outputs from the 16-byte boundary below its first
  static constexpr int OCC = 3 * 4 * C * XW <= 160 * 1024 ? 3 : 2;  // workgroups per CU the LDS admits: the register budget follows
  static_assert(C == 32 || C == 64, "one or two 32-row blocks");
  static_assert(3 + OW <= PW - 1 && NW * 8 * PW <= C * XW, "the epilogue patches fit the buffer");
  static_assert(W1 <= XW && WOUT + 2 * P2 <= W1 && WOUT <= W2, "T fits the buffer and covers what the owned outputs read");
};
template <int KS, int DIL> using Tc6Geo = Tc6GeoC<32, KS, DIL>;
template <int KS, int DIL> using Tc6Geo64 = Tc6GeoC<64, KS, DIL>;

// Each kernel is defined and instantiated in its own file for the (k, dilation) listed here; pair_host.hip launches from the
// same lists.  k = 3 through the C = 16 / 32 F(2,3) kernels (one sub-filter, 2 products per output instead of 3) measured neutral
// in the forward (NOTES round 4): DISSC_EXPERIMENTAL=1 builds only.  At C = 64 k = 3 is the only shape (respair64_f23_kernel).
template <int KS, int DIL> __global__ void respair32_f23_kernel(const PairArgs a);
template <int KS, int DIL> __global__ void respair32_tc6_kernel(const PairArgs a);
template <int KS, int DIL> __global__ void respair16_f23_kernel(const PairArgs a);
template <int KS, int DIL> __global__ void respair64_f23_kernel(const PairArgs a);
template <int KS, int DIL> __global__ void respair64_tc6_kernel(const PairArgs a);
// the k = 3, dilations (1, 3, 5) chains: a.w1 = the six transformed weights, a.b1 = the six biases [6][C], in execution order;
// DBG = true: the instance that honours a.dbg (launched only while "kernel_dbg" != 0)
template <bool DBG> __global__ void reschain32_f23_kernel(const PairArgs a);
template <bool DBG> __global__ void reschain16_f23_kernel(const PairArgs a);
#if DISSC_EXPERIMENTAL
#define DISSC_PAIR_F23_SHAPES(X) X(11, 1) X(11, 3) X(11, 5) X(3, 1) X(3, 3) X(3, 5)
#else
#define DISSC_PAIR_F23_SHAPES(X) X(11, 1) X(11, 3) X(11, 5)
#endif
#define DISSC_PAIR_F23_C64_SHAPES(X) X(3, 1) X(3, 3) X(3, 5)
#define DISSC_PAIR_TC6_SHAPES(X) X(7, 1) X(7, 3) X(7, 5) X(11, 1) X(11, 3) X(11, 5)

}  // namespace dissc
