// A differentiable, ragged, GROUPED, strided, wide-tap Conv1d layer for training the vocoder's scale discriminator on the MI355X:
// the first six layers of every DiscriminatorS (reference sr/models.py:285-307), k = 15 and k = 41, stride 1, 2 or 4, 1 to 16
// groups, which none of conv_grad.hip, conv_grad_t.hip and conv_grad_s.hip can run (CG_MAX_K = 11 taps, no groups).
//
//   y[b,co,q] = bias[co] + sum_{ci in group(co)} sum_kk w[co,ci,kk] lrelu(x, in_slope)[b,ci,s q + kk - pad],   pad = (k - 1) / 2
//
// torch's F.conv1d(lrelu(x), w, b, stride=s, padding=pad, groups=g); w is [Cout][Cin / g][k].  x [B][Cin][ldx] with lengths[b]
// valid INPUT positions, y [B][Cout][ldo] with ceil(lengths[b] / s) valid output positions; what lies beyond is read as zero and
// never written.  Everything is per group: a group is a dense layer of cig = Cin / g inputs and cog = Cout / g outputs, and the
// group is one more grid index.  As in conv_grad_s.hip the long side x is seen as its s phase planes, plane_p[ci][q] =
// x[ci][s q + p], and tap kk touches ONE plane at one shift: o = kk - pad = s dl + p, 0 <= p < s.  The tap table of conv_grad.h is
// sized by CG_MAX_K, so this file computes (p, dl) itself: s is a power of two, p = o & (s - 1), dl = o >> log2(s).
//
// All three kernels run on v_mfma_f32_16x16x4_f32 (the same peak as 32x32x2): a group of convs.2 has 16 output channels and
// 8 input channels, which fill a 16-row tile and would leave half or three quarters of a 32-row one empty.
//   * Taps are indexed by o' = o + PO, PO = pad rounded up to 4, and packed four to a float4 (o' = 4 k4 + e).  Because s divides 4,
//     the plane of element e is e & (s - 1) whatever k4 is: the unrolled e picks its accumulator statically.
//   * Forward (convggrad_fwd_kernel): per group an implicit GEMM, rows co, columns q (64 a workgroup), reduction over (ci, o').
//     The x window of the tile is staged de-interleaved into the s planes with the leaky ReLU applied while staging, at most 32
//     channels at a time (s = 4: 32 x 336 floats = 43 KB, so two workgroups share a CU); a B fragment is 4 channels x 16
//     consecutive floats.  FOUR accumulators per output, one per e, added as (a0 + a1) + (a2 + a3) in the epilogue: the 2 624
//     products of a convs.5 output are four chains of 656, and two dependent MFMAs are never back to back.
//   * Data gradient (convggrad_dgrad_kernel): the phase-group forward of the transposed layer as one kernel, rows ci, columns t,
//     gx[ci][s t + p] = lrelu'(x) sum_{co, o = s dl + p} w[co][ci][o + pad] gy[co][t - dl].  The same four accumulators: with
//     s = 4 each is one output phase, with s = 2 phase p is a_p + a_{p + 2}, with s = 1 all four are one output.  The derivative
//     (torch's rule at x = 0: the slope) and the zeros from lengths[b] to the end of the row are the epilogue.
//   * Weight gradient (convggrad_wgrad_kernel): gw[co][ci][kk] = sum_b sum_q gy[co][q] plane_p(lrelu x)[ci][q + dl], per group,
//     on conv_grad.hip's chunks of 64 output positions with fixed-order partials (cg_launch_reduce) and the shared bias gradient.
//     A wave owns one 16 x 16 tile of (co, ci) and a block of GG_TB = 11 taps (44 accumulator registers); the (row tile, column
//     tile, tap block) units of a group are dealt four to a workgroup, all fed from one staged window (of which only the
//     tiles those four touch are loaded), so 41 taps are four units, not four passes.  The order of every sum is a function
//     of (B, Lmax, layer).
// Cin / g = 1 (convs.0, which reads the waveform) runs on the same kernels with zero-padded tiles: 4 staged channels in the
// forward, one 16-row tile in the gradients.
// LDS banks (ds_read_b32: 32 banks, lanes 0 - 31 and 32 - 63 apart): a B fragment of the forward and the data gradient is two
// rows of 16 consecutive floats per half-wave, the row stride is 16 mod 32; a fragment of the weight gradient is 16 rows x 2
// columns per half-wave, the row stride is 2 x an odd number.  Both conflict-free.
//
// dissc_mean_pool_fwd / _bwd, the AvgPool1d(4, 2, padding=2) between the scales, are at the end of the file.
#include <string.h>

#include <algorithm>

#include "conv_grad.h"

namespace dissc {

constexpr int GG_MAX_K = 41;
constexpr int GG_TN = 64;   // columns of a workgroup's tile, forward and data gradient
constexpr int GG_TB = 11;   // taps of a weight-gradient unit
constexpr size_t GG_WG_LDS = 80 * 1024;     // weight gradient: two workgroups per CU
constexpr size_t GG_WG_LDS1 = 160 * 1024;   // ... one, where 16 positions of the widest accepted group need more (they do not)
constexpr size_t GG_PART_BUDGET = (size_t)56 << 20;  // bytes of partials, as conv_grad.hip
constexpr int GG_TARGET_WG = 512;

// ---- the forward and the data gradient: one argument struct ---------------------------------------------------------------
struct GgConvArgs {
  const float* in;     // forward: x [B][Cin][ldx], before the activation; data gradient: gy [B][Cout][ldo]
  const float* apack;  // [G][RT][C4][K4][64 lanes][4]: lane (i, kq), element e = w[row 16 rt + i][reduction channel 4 c4 + kq][o' = 4 k4 + e]
  const float* bias;   // forward: [Cout]
  const float* x;      // data gradient: x, for the derivative
  const int32_t* lengths;
  float* out;          // y [B][Cout][ldo] / gx [B][Cin][ldx]
  int B, Cin, Cout, cig, cog;
  int S, ls, pad, PO, K4, halo;  // halo: output positions, >= ceil(pad / S), multiple of 4
  int Lmax, ldx, ldo;
  int RT;              // 16-row tiles of a group
  int WM;              // waves over row tiles; 4 / WM over columns, each WM column tiles of 16
  int CK, C4;          // reduction channels staged at a time; of a group, / 4
  int ldw, cst;        // LDS: floats per plane row; per channel (forward: S planes), 16 mod 32
  float slope;
};

typedef f32x4 gg_acc[4][4];  // [e][column tile]

// the MFMAs of one staged slab: rows of `lds` are reduction channels `cst` apart; element e of tap quad k4 is o = 4 k4 + e - PO and
// reads column `col + shift(o)`, shift = plane * ldw + dl (forward) or -dl (data gradient)
template <bool FWD>
__device__ __forceinline__ void gg_slab_mfma(const GgConvArgs& a, const f32x4* aps, const float* lds, int col, int kq, gg_acc& acc) {
  const int n = (a.CK / 4) * a.K4;
  f32x4 cur = aps[0];
  int c4 = 0, k4 = 0;
  for (int i = 0; i < n; ++i) {
    f32x4 nxt = cur;  // the A fragments of the next quad in flight behind this one's MFMAs
    if (i + 1 < n) nxt = aps[(size_t)(i + 1) * 64];
    const float* bp = lds + (4 * c4 + kq) * a.cst + col;
#pragma unroll
    for (int e = 0; e < 4; ++e) {
      const int o = 4 * k4 + e - a.PO;
      if (o < -a.pad || o > a.pad) continue;  // wave-uniform: not a tap
      const int dl = o >> a.ls;               // floor(o / S)
      const float* bq = FWD ? bp + (o & (a.S - 1)) * a.ldw + dl : bp - dl;
#pragma unroll
      for (int nt = 0; nt < 4; ++nt)
        if (nt < a.WM) acc[e][nt] = __builtin_amdgcn_mfma_f32_16x16x4f32(cur[e], bq[16 * nt], acc[e][nt], 0, 0, 0);
    }
    cur = nxt;
    if (++k4 == a.K4) {
      k4 = 0;
      ++c4;
    }
  }
}

__global__ void __launch_bounds__(256, 2) convggrad_fwd_kernel(GgConvArgs a) {
  extern __shared__ float gg_lds[];  // planes of the lrelu(x) window [CK][S][ldw], column c = output position q0 - halo + c
  const int S = a.S, ls = a.ls, halo = a.halo, W = GG_TN + 2 * halo;
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int j = lane & 15, kq = lane >> 4;
  const int wm = wave % a.WM, wn = wave / a.WM;
  const int RB = (a.RT + a.WM - 1) / a.WM;
  const int grp = blockIdx.y / RB, rt = (blockIdx.y - grp * RB) * a.WM + wm;
  const int b = blockIdx.z, q0 = blockIdx.x * GG_TN;
  int len = a.lengths ? a.lengths[b] : a.Lmax;
  len = len < 0 ? 0 : (len > a.Lmax ? a.Lmax : len);
  const int olen = (len + S - 1) >> ls;
  if (q0 >= olen) return;  // uniform over the workgroup: nothing is written at or beyond the output length
  const int cb = wn * 16 * a.WM;  // this wave's first column of the tile
  const bool live = rt < a.RT && q0 + cb < olen;  // wave-uniform
  gg_acc acc;
#pragma unroll
  for (int e = 0; e < 4; ++e)
#pragma unroll
    for (int nt = 0; nt < 4; ++nt) acc[e][nt] = f32x4{0.f, 0.f, 0.f, 0.f};
  // Bounds of the staging reads.  The window is the S W input columns from u0 = S (q0 - halo), a multiple of 4 (halo % 4 == 0,
  // q0 % 64 == 0), read as float4 at u = u0 + 4 v.  A load happens only for 0 <= u < len: u % 4 == 0, len <= Lmax <= ldx and
  // ldx % 4 == 0 give u + 3 < ldx, inside the row whatever the halo (20 columns at S = 4 reach 80 inputs either side) and
  // whatever the length; the row is one of the group's cig (ci0 + r < cig).  Everything else is stored as zero.
  const int nv = (W << ls) >> 2, u0 = (q0 - halo) * S;
  const f32x4* ap = reinterpret_cast<const f32x4*>(a.apack) + (size_t)(grp * a.RT + (rt < a.RT ? rt : 0)) * a.C4 * a.K4 * 64 + lane;
  for (int ci0 = 0; ci0 < 4 * a.C4; ci0 += a.CK) {
    __syncthreads();
    const float* xb = a.in + ((size_t)b * a.Cin + (size_t)grp * a.cig + ci0) * a.ldx;
    for (int i = tid; i < a.CK * nv; i += 256) {
      const int r = i / nv, v = i - r * nv, u = u0 + 4 * v;
      f32x4 x4 = {0.f, 0.f, 0.f, 0.f};
      if (u >= 0 && u < len && ci0 + r < a.cig) x4 = *reinterpret_cast<const f32x4*>(xb + (size_t)r * a.ldx + u);
#pragma unroll
      for (int qq = 0; qq < 4; ++qq) {
        const int c = 4 * v + qq;
        const float xv = x4[qq];
        gg_lds[r * a.cst + (c & (S - 1)) * a.ldw + (c >> ls)] = (u + qq < len) ? (xv > 0.f ? xv : xv * a.slope) : 0.f;
      }
    }
    __syncthreads();
    if (live) gg_slab_mfma<true>(a, ap + (size_t)(ci0 / 4) * a.K4 * 64, gg_lds, halo + cb + j, kq, acc);
  }
  if (!live) return;
#pragma unroll
  for (int nt = 0; nt < 4; ++nt) {
    const int q = q0 + cb + 16 * nt + j;
    if (nt >= a.WM || q >= olen) continue;
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      const int co = grp * a.cog + 16 * rt + 4 * kq + r;  // cog % 16 == 0: every row of a live tile is a channel
      a.out[((size_t)b * a.Cout + co) * a.ldo + q] = ((acc[0][nt][r] + acc[1][nt][r]) + (acc[2][nt][r] + acc[3][nt][r])) + a.bias[co];
    }
  }
}

__global__ void __launch_bounds__(256, 2) convggrad_dgrad_kernel(GgConvArgs a) {
  extern __shared__ float gg_lds[];  // the gy window [CK][ldw], column c = output position t0 - halo + c
  const int S = a.S, ls = a.ls, halo = a.halo, W = GG_TN + 2 * halo;
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int j = lane & 15, kq = lane >> 4;
  const int wm = wave % a.WM, wn = wave / a.WM;
  const int RB = (a.RT + a.WM - 1) / a.WM;
  const int grp = blockIdx.y / RB, rt = (blockIdx.y - grp * RB) * a.WM + wm;
  const int b = blockIdx.z, t0 = blockIdx.x * GG_TN;
  int len = a.lengths ? a.lengths[b] : a.Lmax;
  len = len < 0 ? 0 : (len > a.Lmax ? a.Lmax : len);
  const int olen = (len + S - 1) >> ls;
  const int cb = wn * 16 * a.WM;
  const bool live = rt < a.RT && t0 + cb < olen;  // wave-uniform; a wave at or beyond the output length writes zeros
  gg_acc acc;
#pragma unroll
  for (int e = 0; e < 4; ++e)
#pragma unroll
    for (int nt = 0; nt < 4; ++nt) acc[e][nt] = f32x4{0.f, 0.f, 0.f, 0.f};
  if (t0 < olen) {  // uniform over the workgroup
    // the staging reads: float4 at t = t0 - halo + 4 v, only for 0 <= t < olen; olen <= ceil(Lmax / S) <= ldo and ldo % 4 == 0
    // give t + 3 < ldo.  cog % CK == 0: every staged row is one of the group's channels.
    const int nv = W / 4;
    const f32x4* ap = reinterpret_cast<const f32x4*>(a.apack) + (size_t)(grp * a.RT + (rt < a.RT ? rt : 0)) * a.C4 * a.K4 * 64 + lane;
    for (int co0 = 0; co0 < a.cog; co0 += a.CK) {
      __syncthreads();
      const float* gyb = a.in + ((size_t)b * a.Cout + (size_t)grp * a.cog + co0) * a.ldo;
      for (int i = tid; i < a.CK * nv; i += 256) {
        const int r = i / nv, v = i - r * nv, t = t0 - halo + 4 * v;
        f32x4 g4 = {0.f, 0.f, 0.f, 0.f};
        if (t >= 0 && t < olen) g4 = *reinterpret_cast<const f32x4*>(gyb + (size_t)r * a.ldo + t);
#pragma unroll
        for (int qq = 0; qq < 4; ++qq) gg_lds[r * a.cst + 4 * v + qq] = (t + qq < olen) ? g4[qq] : 0.f;  // (t < 0: loaded as zero)
      }
      __syncthreads();
      if (live) gg_slab_mfma<false>(a, ap + (size_t)(co0 / 4) * a.K4 * 64, gg_lds, halo + cb + j, kq, acc);
    }
  }
  if (rt >= a.RT) return;
#pragma unroll
  for (int nt = 0; nt < 4; ++nt) {
    if (nt >= a.WM) continue;
    const int t = t0 + cb + 16 * nt + j;
#pragma unroll
    for (int p = 0; p < 4; ++p) {
      if (p >= S) continue;
      const int u = S * t + p;
      if (u >= a.ldx) continue;  // every column of gx up to ldx is written, none beyond
      // element e of a tap quad is plane e & (S - 1): the accumulators of output phase p
      const f32x4 s4 = S == 1 ? (acc[0][nt] + acc[1][nt]) + (acc[2][nt] + acc[3][nt])
                              : (S == 2 ? acc[p & 1][nt] + acc[(p & 1) + 2][nt] : acc[p][nt]);
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const int ci = 16 * rt + 4 * kq + r;
        if (ci >= a.cig) continue;
        const size_t i = ((size_t)b * a.Cin + (size_t)grp * a.cig + ci) * a.ldx + u;
        float v = 0.f;  // zero from lengths[b] to the end of the row
        if (u < len) v = a.x[i] > 0.f ? s4[r] : s4[r] * a.slope;
        a.out[i] = v;
      }
    }
  }
}

// ---- the weight gradient ------------------------------------------------------------------------------------------------
struct GgWgradArgs {
  const float* gy;   // [B][Cout][ldo]
  const float* x;    // [B][Cin][ldx], before the activation
  const int32_t* lengths;
  float* part;       // [P][Cout][cig][K]
  int B, Cout, Cin, cig, cog, K;
  int S, ls, pad, halo;
  int Lmax, ldo, ldx;  // Lmax: input positions
  int tsub;            // output positions staged at a time: CG_T, CG_T / 2 or CG_T / 4
  int RT, CT, NTB;     // of a group: 16-row tiles (co), 16-column tiles (ci), tap blocks; a unit is one of each
  int WPG;             // workgroups per group: ceil(RT CT NTB / 4)
  int nch, cpp;
  float slope;
};

__global__ void __launch_bounds__(256, 2) convggrad_wgrad_kernel(GgWgradArgs a) {
  extern __shared__ float gg_lds[];
  const int S = a.S, ls = a.ls, halo = a.halo, nrows = 16 * a.CT;
  const int ldd = a.tsub + 2, lda = a.tsub + 2 * halo + 2;  // 2 x odd (tsub % 16 == 0, halo % 4 == 0)
  float* ds = gg_lds;                // gy [cog][ldd], column c = output position ts0 + c
  float* as = gg_lds + a.cog * ldd;  // planes of lrelu(x) [S][16 CT][lda], column c = output position ts0 - halo + c
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int i16 = lane & 15, kq = lane >> 4;
  const int grp = blockIdx.x / a.WPG, unit = (blockIdx.x - grp * a.WPG) * 4 + wave;
  const bool live = unit < a.RT * a.CT * a.NTB;  // wave-uniform
  const int tb = unit % a.NTB, ct = (unit / a.NTB) % a.CT, rt = live ? unit / (a.NTB * a.CT) : 0;
  // the row tiles of gy and the column tiles of x that this workgroup's four units touch: only those are staged (the others'
  // LDS rows are never read).  convs.0 has 8 row tiles and a workgroup touches 2; convs.5 has 4 x 4 and it touches one of each.
  unsigned rmask = 0, cmask = 0;
  for (int w = 0; w < 4; ++w) {
    const int u = unit - wave + w;
    if (u < a.RT * a.CT * a.NTB) {
      rmask |= 1u << (u / (a.NTB * a.CT));
      cmask |= 1u << ((u / a.NTB) % a.CT);
    }
  }
  f32x4 acc[GG_TB];
  int boff[GG_TB];
#pragma unroll
  for (int g = 0; g < GG_TB; ++g) {
    acc[g] = f32x4{0.f, 0.f, 0.f, 0.f};
    const int kk = tb * GG_TB + g;
    const int o = (kk < a.K ? kk : a.K - 1) - a.pad;  // a slot beyond the last tap reads a valid address; it is never stored
    // B: plane_p[ci = 16 ct + i16][q + dl], q = ts0 + 4 step + kq
    boff[g] = ((o & (S - 1)) * nrows + 16 * ct + i16) * lda + halo + (o >> ls) + kq;
  }
  // the staging reads are bounded as the forward's and the data gradient's: x float4 at u = S (ts0 - halo) + 4 v (a multiple of 4:
  // ts0 % 16 == 0, halo % 4 == 0) only for 0 <= u < len <= ldx, rows r < cig; gy float4 at t = ts0 + 4 v only for t < olen <= ldo
  const int nv = ((a.tsub + 2 * halo) << ls) >> 2;  // float4 per row of the x slab
  const int gv = a.tsub / 4;                        // float4 per row of the gy tile
  const long long npair = (long long)a.B * a.nch;
  const long long pr0 = (long long)blockIdx.z * a.cpp, pr1 = pr0 + a.cpp < npair ? pr0 + a.cpp : npair;
  for (long long pr = pr0; pr < pr1; ++pr) {
    const int b = (int)(pr / a.nch), t0 = (int)(pr - (long long)b * a.nch) * CG_T;
    int len = a.lengths ? a.lengths[b] : a.Lmax;
    len = len < 0 ? 0 : (len > a.Lmax ? a.Lmax : len);
    const int olen = (len + S - 1) >> ls;
    const float* gyb = a.gy + ((size_t)b * a.Cout + (size_t)grp * a.cog) * a.ldo;
    const float* xb = a.x + ((size_t)b * a.Cin + (size_t)grp * a.cig) * a.ldx;
    for (int ts0 = t0; ts0 < t0 + CG_T && ts0 < olen; ts0 += a.tsub) {  // uniform over the workgroup
      __syncthreads();
      for (int i = tid; i < a.cog * gv; i += 256) {  // gy tile: cog rows x tsub positions
        const int r = i / gv, v = i - r * gv, t = ts0 + 4 * v;
        if (!((rmask >> (r >> 4)) & 1)) continue;
        f32x4 g4 = {0.f, 0.f, 0.f, 0.f};
        if (t < olen) g4 = *reinterpret_cast<const f32x4*>(gyb + (size_t)r * a.ldo + t);
#pragma unroll
        for (int qq = 0; qq < 4; ++qq) ds[r * ldd + 4 * v + qq] = (t + qq < olen) ? g4[qq] : 0.f;
      }
      const int u0 = (ts0 - halo) * S;
      for (int i = tid; i < nrows * nv; i += 256) {  // S (tsub + 2 halo) contiguous columns of x, de-interleaved
        const int r = i / nv, v = i - r * nv, u = u0 + 4 * v;
        if (!((cmask >> (r >> 4)) & 1)) continue;
        f32x4 x4 = {0.f, 0.f, 0.f, 0.f};
        if (u >= 0 && u < len && r < a.cig) x4 = *reinterpret_cast<const f32x4*>(xb + (size_t)r * a.ldx + u);
#pragma unroll
        for (int qq = 0; qq < 4; ++qq) {
          const int c = 4 * v + qq;
          const float xv = x4[qq];
          as[((c & (S - 1)) * nrows + r) * lda + (c >> ls)] = (u + qq < len) ? (xv > 0.f ? xv : xv * a.slope) : 0.f;
        }
      }
      __syncthreads();
      if (live) {
        const int nst = ((olen - ts0 < a.tsub ? olen - ts0 : a.tsub) + 3) >> 2;
        const float* ap = ds + (16 * rt + i16) * ldd + kq;  // A: gy[co = 16 rt + i16][ts0 + 4 step + kq]
        for (int s = 0; s < nst; ++s) {
          const float av = ap[4 * s];
#pragma unroll
          for (int g = 0; g < GG_TB; ++g) acc[g] = __builtin_amdgcn_mfma_f32_16x16x4f32(av, as[boff[g] + 4 * s], acc[g], 0, 0, 0);
        }
      }
    }
  }
  if (!live) return;
  const int ci = 16 * ct + i16;
  if (ci >= a.cig) return;
  float* pbase = a.part + (size_t)blockIdx.z * a.Cout * a.cig * a.K;
#pragma unroll
  for (int g = 0; g < GG_TB; ++g) {
    const int kk = tb * GG_TB + g;
    if (kk >= a.K) continue;
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      const int co = grp * a.cog + 16 * rt + 4 * kq + r;
      pbase[((size_t)co * a.cig + ci) * a.K + kk] = acc[g][r];
    }
  }
}

// ---- packing on the device ----------------------------------------------------------------------------------------------
struct GgPackArgs {
  const float* w;     // master weights [Cout][cig][K]
  const float* bias;  // [Cout] or nullptr
  float* fpack;       // the forward's GgConvArgs::apack
  float* bpack;       // the data gradient's
  float* bias_out;    // [Cout]
  int Cout, cig, cog, G, K, pad, PO, K4;
  int rtf, c4f, rtb, c4b;
};

// blockIdx.y == 0: the forward's A fragments (and the bias, zeros without one); 1: the data gradient's
__global__ void __launch_bounds__(256) convggrad_pack_kernel(GgPackArgs a) {
  const size_t idx = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  const bool fwd = blockIdx.y == 0;
  if (fwd && idx < (size_t)a.Cout) a.bias_out[idx] = a.bias ? a.bias[idx] : 0.f;
  const int rtn = fwd ? a.rtf : a.rtb, c4n = fwd ? a.c4f : a.c4b;
  const size_t total = (size_t)a.G * rtn * c4n * a.K4 * 256;
  if (idx >= total) return;
  const int e = idx & 3, lane = (idx >> 2) & 63;
  size_t r = idx >> 8;
  const int k4 = (int)(r % a.K4);
  r /= a.K4;
  const int c4 = (int)(r % c4n);
  r /= c4n;
  const int rt = (int)(r % rtn), grp = (int)(r / rtn);
  const int row = 16 * rt + (lane & 15), red = 4 * c4 + (lane >> 4);  // the tile's row, the reduction's channel, within the group
  const int co = fwd ? row : red, ci = fwd ? red : row;
  const int kk = 4 * k4 + e - a.PO + a.pad;
  (fwd ? a.fpack : a.bpack)[idx] =
      (co < a.cog && ci < a.cig && kk >= 0 && kk < a.K) ? a.w[((size_t)(grp * a.cog + co) * a.cig + ci) * a.K + kk] : 0.f;
}

// ---- the pool -----------------------------------------------------------------------------------------------------------
// out[j] = ((x[2 j - 2] + x[2 j - 1]) + (x[2 j] + x[2 j + 1])) / 4, j <= floor(n / 2), x zero outside [0, n): AvgPool1d(4, 2, 2)
__global__ void __launch_bounds__(256) mean_pool_fwd_kernel(const float* __restrict__ x, const int32_t* __restrict__ lengths, int C,
                                                            int T, int ldx, int ldo, float* __restrict__ out) {
  const int row = blockIdx.y, jj = blockIdx.x * blockDim.x + threadIdx.x;
  int n = lengths ? lengths[row / C] : T;
  n = n < 0 ? 0 : (n > T ? T : n);
  if (n == 0 || jj > n / 2) return;  // nothing is written beyond the output length
  const float* xr = x + (size_t)row * ldx;
  const int i = 2 * jj;
  const float x0 = i - 2 >= 0 ? xr[i - 2] : 0.f, x1 = i - 1 >= 0 ? xr[i - 1] : 0.f;  // (i - 1 <= n - 1)
  const float x2 = i < n ? xr[i] : 0.f, x3 = i + 1 < n ? xr[i + 1] : 0.f;
  out[(size_t)row * ldo + jj] = ((x0 + x1) + (x2 + x3)) * 0.25f;
}

// gx[i] = (gy[floor(i / 2)] + gy[floor(i / 2) + 1]) / 4, gy zero at and beyond the output length; zero from n to ldx
__global__ void __launch_bounds__(256) mean_pool_bwd_kernel(const float* __restrict__ gy, const int32_t* __restrict__ lengths, int C,
                                                            int T, int ldx, int ldo, float* __restrict__ gx) {
  const int row = blockIdx.y, i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= ldx) return;
  int n = lengths ? lengths[row / C] : T;
  n = n < 0 ? 0 : (n > T ? T : n);
  float g = 0.f;
  if (i < n) {
    const int no = n / 2 + 1, jj = i >> 1;  // jj <= (n - 1) / 2 < no
    const float* gr = gy + (size_t)row * ldo;
    g = 0.25f * (gr[jj] + (jj + 1 < no ? gr[jj + 1] : 0.f));
  }
  gx[(size_t)row * ldx + i] = g;
}

}  // namespace dissc

using namespace dissc;

struct dissc_convggrad : CgLayer {
  int s = 1, g = 1;
  float* fpack = nullptr;  // the forward's A fragments
  float* bpack = nullptr;  // the data gradient's
  float* bias = nullptr;   // [Cout]
  ~dissc_convggrad() {
    if (fpack) (void)hipFree(fpack);
    if (bpack) (void)hipFree(bpack);
    if (bias) (void)hipFree(bias);
  }
};

namespace {

struct GgGeom {
  int cig, cog;   // channels of a group
  int c4f, rtf;   // forward: reduction channels (cig rounded up to 4) / 4, row tiles cog / 16
  int c4b, rtb;   // data gradient: cog / 4, ceil(cig / 16)
  int ls, pad, PO, K4, halo;
};

GgGeom gg_geom(const dissc_convggrad* h) {
  GgGeom g;
  g.cig = h->Cin / h->g; g.cog = h->Cout / h->g;
  g.c4f = (g.cig + 3) / 4; g.rtf = g.cog / 16;
  g.c4b = g.cog / 4; g.rtb = (g.cig + 15) / 16;
  g.ls = h->s == 4 ? 2 : (h->s == 2 ? 1 : 0);
  g.pad = (h->k - 1) / 2;
  g.PO = (g.pad + 3) & ~3;
  g.K4 = (g.PO + g.pad) / 4 + 1;
  g.halo = ((g.pad + h->s - 1) / h->s + 3) & ~3;
  return g;
}

size_t gg_npack(const dissc_convggrad* h, int which) {
  const GgGeom g = gg_geom(h);
  return (size_t)h->g * (which ? g.rtb : g.rtf) * (which ? g.c4b : g.c4f) * g.K4 * 256;
}

// the smallest row stride >= n that is 16 mod 32
int gg_stride16(int n) { return (n + 15) / 32 * 32 + 16; }

// what the forward and the data gradient share: the taps, the wave grid over RT row tiles, the slab of `red` reduction channels
void gg_conv_args(const dissc_convggrad* h, const GgGeom& g, int B, int Lmax, int ldx, int ldo, const int32_t* lengths, float slope,
                  int RT, int red, GgConvArgs* a) {
  a->lengths = lengths;
  a->B = B; a->Cin = h->Cin; a->Cout = h->Cout; a->cig = g.cig; a->cog = g.cog;
  a->S = h->s; a->ls = g.ls; a->pad = g.pad; a->PO = g.PO; a->K4 = g.K4; a->halo = g.halo;
  a->Lmax = Lmax; a->ldx = ldx; a->ldo = ldo;
  a->RT = RT;
  a->WM = RT % 4 == 0 ? 4 : (RT % 2 == 0 ? 2 : 1);
  a->CK = red % 32 == 0 ? 32 : (red % 16 == 0 ? 16 : (red % 8 == 0 ? 8 : 4));
  a->C4 = red / 4;
  a->slope = slope;
}

struct GgPlan {
  CgPlan p;  // nch, P, cpp, gw; WT = 1
  int RT, CT, NTB, WPG;
};

// conv_grad.hip's chunks of CG_T output positions and its budget of partial bytes; P from this kernel's own workgroup count.  A
// function of the shape only.
GgPlan gg_plan(const dissc_convggrad* h, int B, int Lmax) {
  const GgGeom g = gg_geom(h);
  GgPlan q;
  q.p = cg_plan(g.cig, h->Cout, h->k, B, (Lmax + h->s - 1) / h->s);
  q.RT = g.rtf; q.CT = g.rtb; q.NTB = (h->k + GG_TB - 1) / GG_TB;
  q.WPG = (q.RT * q.CT * q.NTB + 3) / 4;
  q.p.WCI = 1; q.p.WT = 1; q.p.CIB = 16; q.p.TS = 1; q.p.NG = GG_TB;
  q.p.coT = h->g * q.WPG; q.p.ciS = 1;
  const long long N = (long long)B * q.p.nch;
  long long P = (GG_TARGET_WG + q.p.coT - 1) / q.p.coT;
  const long long cap = (long long)(GG_PART_BUDGET / (q.p.gw * sizeof(float)));
  P = std::min(P, std::max(cap, 1LL));
  P = std::max(1LL, std::min(P, N));
  q.p.cpp = (int)((N + P - 1) / P);
  q.p.P = (int)((N + q.p.cpp - 1) / q.p.cpp);  // no empty partial
  return q;
}

size_t gg_wgrad_lds(const GgGeom& g, int S, int CT, int tsub) {
  return ((size_t)g.cog * (tsub + 2) + (size_t)S * 16 * CT * (tsub + 2 * g.halo + 2)) * sizeof(float);
}

}  // namespace

extern "C" {

int dissc_convggrad_create(int Cin, int Cout, int k, int stride, int groups, dissc_convggrad_t* out) {
  const char* who = "dissc_convggrad_create";
  if (out) *out = nullptr;
  if (int rc = cg_check_create(who, out, Cin, Cout)) return rc;
  if (k < 3 || k > GG_MAX_K || k % 2 != 1) {
    set_error("%s: kernel size %d (odd, 3 .. %d)", who, k, GG_MAX_K);
    return DISSC_EINVAL;
  }
  if (stride != 1 && stride != 2 && stride != 4) {
    set_error("%s: stride %d (1, 2 or 4)", who, stride);
    return DISSC_EINVAL;
  }
  if (groups < 1 || Cin % groups || Cout % groups) {
    set_error("%s: %d groups must divide %d -> %d channels", who, groups, Cin, Cout);
    return DISSC_EINVAL;
  }
  const int cig = Cin / groups, cog = Cout / groups;
  if (!(cig == 1 || (cig % 8 == 0 && cig <= 64))) {
    set_error("%s: %d input channels per group (1, or a multiple of 8 up to 64)", who, cig);
    return DISSC_EINVAL;
  }
  if (cog % 16 || cog > 128) {
    set_error("%s: %d output channels per group (a multiple of 16 up to 128)", who, cog);
    return DISSC_EINVAL;
  }
  dissc_convggrad* h = new dissc_convggrad();
  h->opt = g_defaults;  // frozen here
  h->Cin = Cin; h->Cout = Cout; h->k = k; h->s = stride; h->g = groups;
  *out = h;
  return DISSC_OK;
}

void dissc_convggrad_destroy(dissc_convggrad_t h) { delete h; }

int dissc_convggrad_set_weights(dissc_convggrad_t h, const float* w_dev, const float* bias_dev, void* stream) {
  if (!h || !w_dev) {
    set_error("dissc_convggrad_set_weights: bad argument");
    return DISSC_EINVAL;
  }
  OptScope opt_scope(&h->opt);
  hipStream_t st = (hipStream_t)stream;
  const size_t nf = gg_npack(h, 0), nb = gg_npack(h, 1);
  if (!h->ready) {
    float *f = nullptr, *bk = nullptr, *bi = nullptr;  // handed to the handle only when all three are allocated
    if (hipMalloc((void**)&f, nf * sizeof(float)) != hipSuccess || hipMalloc((void**)&bk, nb * sizeof(float)) != hipSuccess ||
        hipMalloc((void**)&bi, (size_t)h->Cout * sizeof(float)) != hipSuccess) {
      if (f) (void)hipFree(f);
      if (bk) (void)hipFree(bk);
      set_error("dissc_convggrad_set_weights: cannot allocate %zu bytes", (nf + nb + h->Cout) * sizeof(float));
      return DISSC_ENOMEM;
    }
    h->fpack = f; h->bpack = bk; h->bias = bi;
    h->ready = true;
  }
  const GgGeom g = gg_geom(h);
  GgPackArgs a;
  a.w = w_dev; a.bias = bias_dev; a.fpack = h->fpack; a.bpack = h->bpack; a.bias_out = h->bias;
  a.Cout = h->Cout; a.cig = g.cig; a.cog = g.cog; a.G = h->g; a.K = h->k; a.pad = g.pad; a.PO = g.PO; a.K4 = g.K4;
  a.rtf = g.rtf; a.c4f = g.c4f; a.rtb = g.rtb; a.c4b = g.c4b;
  const size_t most = std::max(std::max(nf, nb), (size_t)h->Cout);
  hipLaunchKernelGGL(convggrad_pack_kernel, dim3((unsigned)((most + 255) / 256), 2), dim3(256), 0, st, a);
  DISSC_HIP_CHECK(hipGetLastError());
  return DISSC_OK;
}

long long dissc_convggrad_packed(dissc_convggrad_t h, int which, float* dst_dev, void* stream) {
  if (!h || which < 0 || which > 1) {
    set_error("dissc_convggrad_packed: bad argument");
    return DISSC_EINVAL;
  }
  const size_t n = gg_npack(h, which);
  if (!dst_dev) return (long long)n;
  if (!h->ready) {
    set_error("dissc_convggrad_packed: dissc_convggrad_set_weights first");
    return DISSC_EINVAL;
  }
  DISSC_HIP_CHECK(hipMemcpyAsync(dst_dev, which ? h->bpack : h->fpack, n * sizeof(float), hipMemcpyDeviceToDevice, (hipStream_t)stream));
  return (long long)n;
}

// Lmax: input positions; a row of y / gy holds ceil(Lmax / stride)
int dissc_convggrad_forward(dissc_convggrad_t h, const float* x, float* y, const int32_t* lengths, int B, int ldx, int ldo,
                            int Lmax, float in_slope, void* stream) {
  int rc = cg_check_call(h, "dissc_convggrad_forward", B, Lmax, 1, ldx, ldo, h ? h->s : 1);
  if (rc) return rc;
  if (!x || !y || ((uintptr_t)x & 15)) {
    set_error("dissc_convggrad_forward: bad argument (x must be a 16-byte aligned device pointer)");
    return DISSC_EINVAL;
  }
  OptScope opt_scope(&h->opt);
  const GgGeom g = gg_geom(h);
  GgConvArgs a;
  gg_conv_args(h, g, B, Lmax, ldx, ldo, lengths, in_slope, g.rtf, 4 * g.c4f, &a);
  a.in = x; a.apack = h->fpack; a.bias = h->bias; a.x = nullptr; a.out = y;
  a.ldw = GG_TN + 2 * g.halo;
  a.cst = gg_stride16(h->s * a.ldw);
  const int olmax = (Lmax + h->s - 1) / h->s, RB = (a.RT + a.WM - 1) / a.WM;
  hipLaunchKernelGGL(convggrad_fwd_kernel, dim3((olmax + GG_TN - 1) / GG_TN, h->g * RB, B), dim3(256),
                     (size_t)a.CK * a.cst * sizeof(float), (hipStream_t)stream, a);
  DISSC_HIP_CHECK(hipGetLastError());
  return DISSC_OK;
}

int dissc_convggrad_partials(dissc_convggrad_t h, int B, int Lmax, int* P, int* chunk) {
  if (int rc = cg_check_call(h, "dissc_convggrad_partials", B, Lmax)) return rc;
  const GgPlan q = gg_plan(h, B, Lmax);
  if (P) *P = q.p.P;
  if (chunk) *chunk = q.p.cpp;
  return DISSC_OK;
}

size_t dissc_convggrad_workspace_bytes(dissc_convggrad_t h, int B, int Lmax) {
  if (!h || B <= 0 || Lmax <= 0) return 0;
  return cg_workspace(gg_plan(h, B, Lmax).p, B, h->Cout).bytes;
}

int dissc_convggrad_backward(dissc_convggrad_t h, const float* x, const float* gy, const int32_t* lengths, int B, int ldx,
                             int ldo, int Lmax, float in_slope, float* gx, float* gw, float* gb, void* workspace,
                             size_t workspace_bytes, void* stream) {
  const char* who = "dissc_convggrad_backward";
  int rc = cg_check_call(h, who, B, Lmax, 1, ldx, ldo, h ? h->s : 1);
  if (rc) return rc;
  const GgPlan q = gg_plan(h, B, Lmax);
  float* part;
  double* bpart;
  if ((rc = cg_backward_begin(who, q.p, B, h->Cout, x, gy, gx, gw || gb, workspace, workspace_bytes, &part, &bpart))) return rc;
  OptScope opt_scope(&h->opt);
  hipStream_t st = (hipStream_t)stream;
  const GgGeom g = gg_geom(h);
  if (gw) {
    GgWgradArgs a;
    a.gy = gy; a.x = x; a.lengths = lengths; a.part = part;
    a.B = B; a.Cout = h->Cout; a.Cin = h->Cin; a.cig = g.cig; a.cog = g.cog; a.K = h->k;
    a.S = h->s; a.ls = g.ls; a.pad = g.pad; a.halo = g.halo;
    a.Lmax = Lmax; a.ldo = ldo; a.ldx = ldx;
    a.tsub = CG_T;
    while (a.tsub > CG_T / 4 && gg_wgrad_lds(g, h->s, q.CT, a.tsub) > GG_WG_LDS) a.tsub /= 2;
    const size_t lds = gg_wgrad_lds(g, h->s, q.CT, a.tsub);
    if (lds > GG_WG_LDS1) {
      set_error("%s: the weight gradient's window does not fit (%zu bytes)", who, lds);
      return DISSC_EINVAL;
    }
    a.RT = q.RT; a.CT = q.CT; a.NTB = q.NTB; a.WPG = q.WPG;
    a.nch = q.p.nch; a.cpp = q.p.cpp;
    a.slope = in_slope;
    static DeviceOnce attr_once;  // per device (common.h)
    DISSC_HIP_CHECK(attr_once.max_lds(reinterpret_cast<const void*>(&convggrad_wgrad_kernel), (int)GG_WG_LDS1));
    hipLaunchKernelGGL(convggrad_wgrad_kernel, dim3(h->g * q.WPG, 1, q.p.P), dim3(256), lds, st, a);
    cg_launch_reduce(part, q.p.P, q.p.gw, gw, st);
  }
  if (gb) cg_launch_bias(gy, lengths, 1, B, h->Cout, (Lmax + h->s - 1) / h->s, ldo, bpart, gb, st, h->s);
  if (gx) {
    GgConvArgs a;
    gg_conv_args(h, g, B, Lmax, ldx, ldo, lengths, in_slope, g.rtb, g.cog, &a);
    a.in = gy; a.apack = h->bpack; a.bias = nullptr; a.x = x; a.out = gx;
    a.ldw = a.cst = gg_stride16(GG_TN + 2 * g.halo);
    const int nt = ((ldx + h->s - 1) / h->s + GG_TN - 1) / GG_TN;  // every column of gx up to ldx is written
    const int RB = (a.RT + a.WM - 1) / a.WM;
    hipLaunchKernelGGL(convggrad_dgrad_kernel, dim3(nt, h->g * RB, B), dim3(256), (size_t)a.CK * a.cst * sizeof(float), st, a);
  }
  DISSC_HIP_CHECK(hipGetLastError());
  return DISSC_OK;
}

static int mean_pool_check(const char* who, const void* a, const void* b, int B, int C, int T, int ldx, int ldo) {
  if (!a || !b || B <= 0 || C <= 0 || (long long)B * C > 65535 || T <= 0 || ldx < T || ldo < T / 2 + 1) {
    set_error("%s: bad argument (B = %d, C = %d, T = %d, ldx = %d, ldo = %d; ldx >= T, ldo >= T / 2 + 1, B C <= 65535)", who, B, C,
              T, ldx, ldo);
    return DISSC_EINVAL;
  }
  return DISSC_OK;
}

int dissc_mean_pool_fwd(const float* x, float* out, const int32_t* lengths, int B, int C, int T, int ldx, int ldo, void* stream) {
  if (int rc = mean_pool_check("dissc_mean_pool_fwd", x, out, B, C, T, ldx, ldo)) return rc;
  hipLaunchKernelGGL(mean_pool_fwd_kernel, dim3((T / 2 + 1 + 255) / 256, B * C), dim3(256), 0, (hipStream_t)stream, x, lengths, C, T,
                     ldx, ldo, out);
  DISSC_HIP_CHECK(hipGetLastError());
  return DISSC_OK;
}

int dissc_mean_pool_bwd(const float* gy, float* gx, const int32_t* lengths, int B, int C, int T, int ldx, int ldo, void* stream) {
  if (int rc = mean_pool_check("dissc_mean_pool_bwd", gy, gx, B, C, T, ldx, ldo)) return rc;
  hipLaunchKernelGGL(mean_pool_bwd_kernel, dim3((ldx + 255) / 256, B * C), dim3(256), 0, (hipStream_t)stream, gy, lengths, C, T, ldx,
                     ldo, gx);
  DISSC_HIP_CHECK(hipGetLastError());
  return DISSC_OK;
}

}  // extern "C"
