// A differentiable, ragged, STRIDED Conv1d layer for training the vocoder's discriminators on the MI355X: the four
// Conv2d((5,1), stride (3,1), padding (2,0)) layers of every DiscriminatorP (reference sr/models.py:228-260), which on the
// period-major rows of dissc_period_fold_fwd are plain stride-3, k = 5 Conv1d layers, 1 -> 32 -> 128 -> 512 -> 1024.
//
//   y[b,co,q] = bias[co] + sum_{ci,kk} w[co,ci,kk] lrelu(x, in_slope)[b,ci,s q + kk - pad],   pad = (k - 1) / 2
//
// x [B][Cin][ldx] with lengths[b] valid INPUT positions, y [B][Cout][ldo] with ceil(lengths[b] / s) valid output positions; what
// lies beyond is read as zero and never written.  The layer is the adjoint of conv_grad_t.hip's ConvTranspose1d, and everything
// is phrased on the same s phase planes of the long side, here x: plane_p[ci][q] = x[ci][s q + p]; tap kk touches ONE plane at one
// shift, kk - pad = s dl + p (ct_taps, conv_grad.h), so that x[s q + kk - pad] = plane_p[q + dl].  k = 5, s = 3: (plane 1, -1),
// (plane 2, -1), (plane 0, 0), (plane 1, 0), (plane 2, 0): no zero taps.  The three kernels are the transposes of that file's:
//   * Forward (convsgrad_fwd_kernel; its convtgrad_dgrad_kernel): an implicit GEMM with rows co, columns q and the reduction over
//     (ci, kk) on v_mfma_f32_32x32x2_f32.  The x window of a column tile is staged de-interleaved into the s planes, with the leaky
//     ReLU applied while staging, so a B fragment is 32 consecutive floats of one plane; the bias is the epilogue.
//   * Weight gradient (convsgrad_wgrad_kernel; its convtgrad_wgrad_kernel with the roles of x and gy swapped):
//     gw[co][ci][kk] = sum_b sum_q gy[co][q] plane_p(kk)(lrelu x)[ci][q + dl(kk)].  A chunk is 64 OUTPUT positions = 64 s contiguous
//     columns of x, read once with float4 loads and de-interleaved in LDS (32 or 16 positions at a time where s planes of 128 rows
//     of a whole chunk do not fit); all k taps accumulate in one pass.  The plan, the fixed-order sum over the partials and the
//     bias gradient are conv_grad.hip's (conv_grad.h), as is the host side of the handle.
//   * Data gradient (convsgrad_dgrad_kernel<S>; the phase-group forward of a ConvTranspose1d as ONE kernel):
//     gx[ci][s t + p] = lrelu'(x) sum_{co, kk : p(kk) = p} w[co][ci][kk] gy[co][t - dl(kk)]: rows ci, columns t, one accumulator per
//     output phase p, all fed from one staged window of gy.  The derivative of the leaky ReLU (torch's rule at x = 0: the slope)
//     and the zeros from lengths[b] to the end of the row are the epilogue: no mask pass, no atomics.
// Cin = 1 (the discriminator's first layer, which reads the waveform) runs on the same kernels with zero-padded tiles: 8 staged
// channels a slab in the forward (one MFMA in four is spent on it), one 32-row block in the gradients (profiles/conv_strided_grad.md).
// Every summation order is a function of the layer alone: an utterance's y and gx bits depend neither on its batch nor on the
// row stride it is stored with.
// LDS banks: as conv_grad_t.hip.  Every fragment read is either 32 consecutive floats or 32 rows of odd stride: conflict-free; the
// de-interleaving writes of a float4 lane are s apart in column.
//
// dissc_period_fold_fwd / _bwd, the 1d -> 2d view in front of the first layer, are at the end of the file.
#include <string.h>

#include <algorithm>

#include "conv_grad.h"

namespace dissc {

constexpr size_t CS_WG_LDS = 80 * 1024;    // weight gradient: two workgroups per CU, as conv_grad.hip
constexpr size_t CS_WG_LDS1 = 160 * 1024;  // ... one, where 16 positions of s planes of 128 rows need more (s >= 7 with Cin > 64)
constexpr size_t CS_FW_LDS = 40 * 1024;    // forward: the staged slab of x

// ---- the forward --------------------------------------------------------------------------------------------------------
struct FwdSArgs {
  const float* x;      // [B][Cin][ldx], before the activation
  const float* apack;  // [Cout / 32][K][cip8][64 lanes][4]: lane (i, hh), element e = w[co = 32 blk + i][ci = 8 c8 + 2 e + hh][kk]
  const float* bias;   // [Cout]
  const int32_t* lengths;
  float* y;            // [B][Cout][ldo]
  int B, Cout, Cin, K, S, Lmax, ldo, ldx;
  int WM, WN;          // waves: WM blocks of 32 rows (co) x WN blocks of 32 columns (q)
  int CK;              // input channels staged at a time (8, 16 or 32)
  int cip8;            // Cin rounded up to 32, / 8
  float slope;
  CtTaps tp;
};

__global__ void __launch_bounds__(256, 2) convsgrad_fwd_kernel(FwdSArgs a) {
  extern __shared__ float cs_lds[];  // planes of the lrelu(x) window [CK][S][ldw], column c = position q0 - halo + c
  const int halo = a.tp.halo;
  const int TN = 32 * a.WN, W = TN + 2 * halo, ldw = W + 1;
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int l31 = lane & 31, h = lane >> 5;
  const int wm = wave % a.WM, wn = wave / a.WM;
  const int n8 = a.CK / 8;  // eights of a slab's channels, <= 4
  const int b = blockIdx.z, q0 = blockIdx.x * TN;
  const int blk = blockIdx.y * a.WM + wm;  // this wave's block of 32 output channels
  int len = a.lengths ? a.lengths[b] : a.Lmax;
  len = len < 0 ? 0 : (len > a.Lmax ? a.Lmax : len);
  const int olen = (len + a.S - 1) / a.S;
  if (q0 >= olen) return;  // uniform over the workgroup: nothing is written at or beyond the output length
  const bool live = blk * 32 < a.Cout && q0 + wn * 32 < olen;  // wave-uniform
  cg_f32x16 acc;
#pragma unroll
  for (int e = 0; e < 16; ++e) acc[e] = 0.f;
  const int nv = a.S * W / 4, u0 = a.S * (q0 - halo);  // u0 % 4 == 0: q0 % 32 == 0, halo % 4 == 0
  const f32x4* ap = reinterpret_cast<const f32x4*>(a.apack) + (size_t)blk * a.K * a.cip8 * 64 + lane;
  const int col = wn * 32 + l31 + halo;
  for (int ci0 = 0; ci0 < a.Cin; ci0 += a.CK) {
    __syncthreads();
    const float* xb = a.x + ((size_t)b * a.Cin + ci0) * a.ldx;
    for (int e = tid; e < a.CK * nv; e += 256) {
      const int r = e / nv, v = e - r * nv, u = u0 + 4 * v;
      f32x4 x4 = {0.f, 0.f, 0.f, 0.f};
      if (u >= 0 && u < len && ci0 + r < a.Cin) x4 = *reinterpret_cast<const f32x4*>(xb + (size_t)r * a.ldx + u);
#pragma unroll
      for (int qq = 0; qq < 4; ++qq) {
        const int c = 4 * v + qq, pos = c / a.S, p = c - pos * a.S;
        const float xv = x4[qq];
        cs_lds[(r * a.S + p) * ldw + pos] = (u + qq < len) ? (xv > 0.f ? xv : xv * a.slope) : 0.f;  // (u < 0: loaded as zero)
      }
    }
    __syncthreads();
    if (live) {
      const f32x4* apc = ap + (size_t)(ci0 / 8) * 64;
      f32x4 cur[4], nxt[4];  // the A fragments of tap kk, those of kk + 1 in flight behind its MFMAs
#pragma unroll
      for (int c = 0; c < 4; ++c) {
        cur[c] = nxt[c] = f32x4{0.f, 0.f, 0.f, 0.f};
        if (c < n8) cur[c] = apc[(size_t)c * 64];
      }
      for (int kk = 0; kk < a.K; ++kk) {
        if (kk + 1 < a.K) {
          const f32x4* apn = apc + (size_t)(kk + 1) * a.cip8 * 64;
#pragma unroll
          for (int c = 0; c < 4; ++c)
            if (c < n8) nxt[c] = apn[(size_t)c * 64];
        }
        // B: plane_p[ci = 8 c + 2 e + h][q + dl]
        const float* bp = cs_lds + (h * a.S + a.tp.p[kk]) * ldw + col + a.tp.dl[kk];
#pragma unroll
        for (int c = 0; c < 4; ++c)
          if (c < n8) {
#pragma unroll
            for (int e = 0; e < 4; ++e)
              acc = __builtin_amdgcn_mfma_f32_32x32x2f32(cur[c][e], bp[(c * 8 + 2 * e) * a.S * ldw], acc, 0, 0, 0);
          }
#pragma unroll
        for (int c = 0; c < 4; ++c) cur[c] = nxt[c];
      }
    }
  }
  if (!live) return;
  const int q = q0 + wn * 32 + l31;
  if (q >= olen) return;
#pragma unroll
  for (int r = 0; r < 16; ++r) {
    const int co = blk * 32 + (r & 3) + 8 * (r >> 2) + 4 * h;
    if (co < a.Cout) a.y[((size_t)b * a.Cout + co) * a.ldo + q] = acc[r] + a.bias[co];
  }
}

// ---- the weight gradient ------------------------------------------------------------------------------------------------
struct WgradSArgs {
  const float* gy;   // [B][Cout][ldo]
  const float* x;    // [B][Cin][ldx], before the activation
  const int32_t* lengths;
  float* part;       // [P * WT][Cout][Cin][K]
  int B, Cout, Cin, K, S, Lmax, ldo, ldx;  // Lmax: input positions
  int tsub;          // output positions staged at a time: CG_T, CG_T / 2 or CG_T / 4
  float slope;
  int WCI, WT, nch, cpp;
  CtTaps tp;
};

template <int NG>
__global__ void __launch_bounds__(256, 2) convsgrad_wgrad_kernel(WgradSArgs a) {
  extern __shared__ float cs_lds[];
  const int halo = a.tp.halo, nrows = 32 * a.WCI;
  const int ldd = a.tsub + 1, lda = a.tsub + 2 * halo + 1;  // odd row strides: a fragment read (32 rows x 1 column) is conflict-free
  float* ds = cs_lds;             // gy [32][ldd], column c = output position ts0 + c
  float* as = cs_lds + 32 * ldd;  // planes of lrelu(x) [S][32 WCI][lda], column c = position ts0 - halo + c
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int l31 = lane & 31, h = lane >> 5;
  const int wci = wave % a.WCI, wt = wave / a.WCI;
  const int co0 = blockIdx.x * 32, ci0 = blockIdx.y * 32 * a.WCI;
  const bool live = ci0 + wci * 32 < a.Cin;  // wave-uniform
  cg_f32x16 acc[NG];
  int boff[NG];
#pragma unroll
  for (int g = 0; g < NG; ++g) {
#pragma unroll
    for (int e = 0; e < 16; ++e) acc[g][e] = 0.f;
    // B: plane_p[ci = l31][q + dl], q = ts0 + 2 step + h
    boff[g] = (a.tp.p[g] * nrows + wci * 32 + l31) * lda + halo + a.tp.dl[g] + h;
  }
  const int nv = a.S * (a.tsub + 2 * halo) / 4;  // float4 per row of the x slab
  const int gv = a.tsub / 4;                     // float4 per row of the gy tile
  const int spw = (a.tsub / 2) / a.WT;           // MFMA k-steps per time slice
  const long long npair = (long long)a.B * a.nch;
  const long long pr0 = (long long)blockIdx.z * a.cpp, pr1 = pr0 + a.cpp < npair ? pr0 + a.cpp : npair;
  for (long long pr = pr0; pr < pr1; ++pr) {
    const int b = (int)(pr / a.nch), t0 = (int)(pr - (long long)b * a.nch) * CG_T;
    int len = a.lengths ? a.lengths[b] : a.Lmax;
    len = len < 0 ? 0 : (len > a.Lmax ? a.Lmax : len);
    const int olen = (len + a.S - 1) / a.S;
    const float* gyb = a.gy + ((size_t)b * a.Cout + co0) * a.ldo;
    const float* xb = a.x + ((size_t)b * a.Cin + ci0) * a.ldx;
    for (int ts0 = t0; ts0 < t0 + CG_T && ts0 < olen; ts0 += a.tsub) {  // uniform over the workgroup
      __syncthreads();
      for (int e = tid; e < 32 * gv; e += 256) {  // gy tile: 32 rows x tsub positions
        const int r = e / gv, v = e - r * gv, t = ts0 + 4 * v;
        f32x4 g4 = {0.f, 0.f, 0.f, 0.f};
        if (t < olen && co0 + r < a.Cout) g4 = *reinterpret_cast<const f32x4*>(gyb + (size_t)r * a.ldo + t);
#pragma unroll
        for (int qq = 0; qq < 4; ++qq) ds[r * ldd + 4 * v + qq] = (t + qq < olen) ? g4[qq] : 0.f;
      }
      const int u0 = a.S * (ts0 - halo);  // u0 % 4 == 0: ts0 % 16 == 0, halo % 4 == 0
      for (int e = tid; e < nrows * nv; e += 256) {  // S (tsub + 2 halo) contiguous columns of x, de-interleaved
        const int r = e / nv, v = e - r * nv, u = u0 + 4 * v;
        f32x4 x4 = {0.f, 0.f, 0.f, 0.f};
        if (u >= 0 && u < len && ci0 + r < a.Cin) x4 = *reinterpret_cast<const f32x4*>(xb + (size_t)r * a.ldx + u);
#pragma unroll
        for (int qq = 0; qq < 4; ++qq) {
          const int c = 4 * v + qq, pos = c / a.S, p = c - pos * a.S;
          const float xv = x4[qq];
          as[(p * nrows + r) * lda + pos] = (u + qq < len) ? (xv > 0.f ? xv : xv * a.slope) : 0.f;  // (u < 0: loaded as zero)
        }
      }
      __syncthreads();
      if (live) {
        const int nst = ((olen - ts0 < a.tsub ? olen - ts0 : a.tsub) + 1) >> 1;
        const int s0 = wt * spw, s1 = s0 + spw < nst ? s0 + spw : nst;
        const float* ap = ds + l31 * ldd + h;  // A: gy[co = l31][ts0 + 2 s + h]
        for (int s = s0; s < s1; ++s) {
          const float av = ap[2 * s];
#pragma unroll
          for (int g = 0; g < NG; ++g) acc[g] = __builtin_amdgcn_mfma_f32_32x32x2f32(av, as[boff[g] + 2 * s], acc[g], 0, 0, 0);
        }
      }
    }
  }
  if (!live) return;
  const int ci = ci0 + wci * 32 + l31;
  if (ci >= a.Cin) return;
  float* pbase = a.part + (size_t)(blockIdx.z * a.WT + wt) * a.Cout * a.Cin * a.K;
#pragma unroll
  for (int g = 0; g < NG; ++g) {
#pragma unroll
    for (int r = 0; r < 16; ++r) {
      const int co = co0 + (r & 3) + 8 * (r >> 2) + 4 * h;
      if (co < a.Cout) pbase[((size_t)co * a.Cin + ci) * a.K + g] = acc[g][r];
    }
  }
}

// ---- the data gradient --------------------------------------------------------------------------------------------------
struct DgradSArgs {
  const float* gy;     // [B][Cout][ldo]
  const float* x;      // [B][Cin][ldx], before the activation
  const float* apack;  // [Cin / 32][K][cop8][64 lanes][4]: lane (i, hh), element e = w[co = 8 c8 + 2 e + hh][ci = 32 blk + i][kk]
  const int32_t* lengths;
  float* gx;           // [B][Cin][ldx]
  int B, Cout, Cin, K, Lmax, ldo, ldx;
  int WM, WN;          // waves: WM blocks of 32 rows (ci) x WN blocks of 32 columns (t: S input positions each)
  int cop8;            // Cout rounded up to 32, / 8
  float slope;
  int kk0[CT_MAX_S], nt[CT_MAX_S];  // output phase p takes the taps kk0[p] + j S, j < nt[p]
  CtTaps tp;
};

template <int S>
__global__ void __launch_bounds__(256, 2) convsgrad_dgrad_kernel(DgradSArgs a) {
  extern __shared__ float cs_lds[];  // the gy window [32][ldw], column c = output position t0 - halo + c
  const int halo = a.tp.halo;
  const int TN = 32 * a.WN, W = TN + 2 * halo, ldw = W + 1;
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int l31 = lane & 31, h = lane >> 5;
  const int wm = wave % a.WM, wn = wave / a.WM;
  const int b = blockIdx.z, t0 = blockIdx.x * TN;
  const int blk = blockIdx.y * a.WM + wm;  // this wave's block of 32 input channels
  int len = a.lengths ? a.lengths[b] : a.Lmax;
  len = len < 0 ? 0 : (len > a.Lmax ? a.Lmax : len);
  const int olen = (len + S - 1) / S;
  const bool live = blk * 32 < a.Cin && t0 + wn * 32 < olen;  // wave-uniform
  cg_f32x16 acc[S];
#pragma unroll
  for (int p = 0; p < S; ++p)
#pragma unroll
    for (int e = 0; e < 16; ++e) acc[p][e] = 0.f;
  if (t0 < olen) {  // uniform over the workgroup
    const int nv = W / 4;
    const f32x4* ap = reinterpret_cast<const f32x4*>(a.apack) + (size_t)blk * a.K * a.cop8 * 64 + lane;
    const int col = wn * 32 + l31 + halo;
    for (int co0 = 0; co0 < a.Cout; co0 += 32) {
      __syncthreads();
      const float* gyb = a.gy + ((size_t)b * a.Cout + co0) * a.ldo;
      for (int e = tid; e < 32 * nv; e += 256) {
        const int r = e / nv, v = e - r * nv, t = t0 - halo + 4 * v;  // t % 4 == 0
        f32x4 g4 = {0.f, 0.f, 0.f, 0.f};
        if (t >= 0 && t < olen && co0 + r < a.Cout) g4 = *reinterpret_cast<const f32x4*>(gyb + (size_t)r * a.ldo + t);
#pragma unroll
        for (int qq = 0; qq < 4; ++qq) cs_lds[r * ldw + 4 * v + qq] = (t + qq < olen) ? g4[qq] : 0.f;  // (t < 0: loaded as zero)
      }
      __syncthreads();
      if (live) {
        const f32x4* apc = ap + (size_t)(co0 / 8) * 64;
#pragma unroll
        for (int p = 0; p < S; ++p) {
          for (int j = 0; j < a.nt[p]; ++j) {
            const int kk = a.kk0[p] + j * S;
            const f32x4* apk = apc + (size_t)kk * a.cop8 * 64;
            f32x4 af[4];
#pragma unroll
            for (int c = 0; c < 4; ++c) af[c] = apk[(size_t)c * 64];
            // B: gy[co = co0 + 8 c + 2 e + h][t - dl]
            const float* bp = cs_lds + h * ldw + col - a.tp.dl[kk];
#pragma unroll
            for (int c = 0; c < 4; ++c)
#pragma unroll
              for (int e = 0; e < 4; ++e)
                acc[p] = __builtin_amdgcn_mfma_f32_32x32x2f32(af[c][e], bp[(c * 8 + 2 * e) * ldw], acc[p], 0, 0, 0);
          }
        }
      }
    }
  }
  if (blk * 32 >= a.Cin) return;
  const int t = t0 + wn * 32 + l31;
#pragma unroll
  for (int p = 0; p < S; ++p) {
    const int u = S * t + p;
    if (u >= a.ldx) continue;
#pragma unroll
    for (int r = 0; r < 16; ++r) {
      const int ci = blk * 32 + (r & 3) + 8 * (r >> 2) + 4 * h;
      if (ci >= a.Cin) continue;
      const size_t i = ((size_t)b * a.Cin + ci) * a.ldx + u;
      float v = 0.f;  // zero from lengths[b] to the end of the row
      if (u < len) v = a.x[i] > 0.f ? acc[p][r] : acc[p][r] * a.slope;
      a.gx[i] = v;
    }
  }
}

// ---- packing on the device ----------------------------------------------------------------------------------------------
struct CsPackArgs {
  const float* w;     // master weights [Cout][Cin][K]
  const float* bias;  // [Cout] or nullptr
  float* fpack;       // FwdSArgs::apack
  float* bpack;       // DgradSArgs::apack
  float* bias_out;    // [Cout]
  int Cin, Cout, K, nblk_co, nblk_ci, cip8, cop8;
};

// blockIdx.y == 0: the forward's A fragments (and the bias, zeros without one); 1: the data gradient's
__global__ void __launch_bounds__(256) convsgrad_pack_kernel(CsPackArgs a) {
  const size_t idx = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  const bool fwd = blockIdx.y == 0;
  if (fwd && idx < (size_t)a.Cout) a.bias_out[idx] = a.bias ? a.bias[idx] : 0.f;
  const int c8n = fwd ? a.cip8 : a.cop8;
  const size_t total = (size_t)(fwd ? a.nblk_co : a.nblk_ci) * a.K * c8n * 256;
  if (idx >= total) return;
  const int e = idx & 3, lane = (idx >> 2) & 63;
  size_t r = idx >> 8;
  const int c8 = (int)(r % c8n);
  r /= c8n;
  const int kk = (int)(r % a.K), blk = (int)(r / a.K);
  const int row = blk * 32 + (lane & 31), red = c8 * 8 + 2 * e + (lane >> 5);  // the tile's row, the reduction's channel
  const int co = fwd ? row : red, ci = fwd ? red : row;
  (fwd ? a.fpack : a.bpack)[idx] = (co < a.Cout && ci < a.Cin) ? a.w[((size_t)co * a.Cin + ci) * a.K + kk] : 0.f;
}

// conv_grad.hip's plan for the same reduction, cut in chunks of OUTPUT positions; a tap's B operand is its own plane, so taps
// never share an MFMA
static CgPlan cs_plan(int Cin, int Cout, int K, int S, int B, int Lmax) {
  CgPlan p = cg_plan(Cin, Cout, K, B, (Lmax + S - 1) / S);
  p.CIB = 32; p.TS = 1; p.NG = K;
  return p;
}

static size_t cs_wgrad_lds(int S, int WCI, int tsub, int halo) {
  return ((size_t)32 * (tsub + 1) + (size_t)S * 32 * WCI * (tsub + 2 * halo + 1)) * sizeof(float);
}

template <int NG>
static int cs_launch_wgrad(const WgradSArgs& a, const CgPlan& p, hipStream_t st) {
  static DeviceOnce attr_once;  // per device (common.h)
  DISSC_HIP_CHECK(attr_once.max_lds(reinterpret_cast<const void*>(&convsgrad_wgrad_kernel<NG>), (int)CS_WG_LDS1));
  hipLaunchKernelGGL((convsgrad_wgrad_kernel<NG>), dim3(p.coT, p.ciS, p.P), dim3(256), cs_wgrad_lds(a.S, a.WCI, a.tsub, a.tp.halo),
                     st, a);
  return DISSC_OK;
}

template <int S>
static void cs_launch_dgrad(const DgradSArgs& a, hipStream_t st) {
  const int TN = 32 * a.WN;
  const int nt = ((a.ldx + S - 1) / S + TN - 1) / TN;  // every column of gx up to ldx is written
  hipLaunchKernelGGL((convsgrad_dgrad_kernel<S>), dim3(nt, (a.Cin + 32 * a.WM - 1) / (32 * a.WM), a.B), dim3(256),
                     (size_t)32 * (TN + 2 * a.tp.halo + 1) * sizeof(float), st, a);
}

// ---- the period fold ----------------------------------------------------------------------------------------------------
// x0[b p + w][h] = ypad_b[h p + w], h < ceil(n_b / p); ypad_b: utterance b reflect-padded at its own end, ypad[n + i] = y[n - 2 - i]
__global__ void __launch_bounds__(256) period_fold_fwd_kernel(const float* __restrict__ wav, const int32_t* __restrict__ lengths,
                                                              int period, int T, int ldw, int ldh, float* __restrict__ x0) {
  const int b = blockIdx.z, w = blockIdx.y, hh = blockIdx.x * blockDim.x + threadIdx.x;
  int n = lengths ? lengths[b] : T;
  n = n < 0 ? 0 : (n > T ? T : n);
  if (hh >= (n + period - 1) / period) return;
  int i = hh * period + w;
  if (i >= n) i = 2 * n - 2 - i;
  i = i < 0 ? 0 : i;  // (a length torch's reflect pad refuses: the Python side raises before any launch)
  x0[((size_t)b * period + w) * ldh + hh] = wav[(size_t)b * ldw + i];
}

// gwav[b][i] = gx0 at i's own place + gx0 at the padded place that mirrors i (i' = 2 n - 2 - i in [n, H p)); zero from n to ldw
__global__ void __launch_bounds__(256) period_fold_bwd_kernel(const float* __restrict__ gx0, const int32_t* __restrict__ lengths,
                                                              int period, int T, int ldw, int ldh, float* __restrict__ gwav) {
  const int b = blockIdx.y, i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= ldw) return;
  int n = lengths ? lengths[b] : T;
  n = n < 0 ? 0 : (n > T ? T : n);
  float g = 0.f;
  if (i < n) {
    const float* gb = gx0 + (size_t)b * period * ldh;
    g = gb[(size_t)(i % period) * ldh + i / period];
    const int m = 2 * n - 2 - i, top = (n + period - 1) / period * period;
    if (m >= n && m < top) g += gb[(size_t)(m % period) * ldh + m / period];
  }
  gwav[(size_t)b * ldw + i] = g;
}

}  // namespace dissc

using namespace dissc;

struct dissc_convsgrad : CgLayer {
  int s = 2;
  float* fpack = nullptr;  // the forward's A fragments
  float* bpack = nullptr;  // the data gradient's
  float* bias = nullptr;   // [Cout]
  ~dissc_convsgrad() {
    if (fpack) (void)hipFree(fpack);
    if (bpack) (void)hipFree(bpack);
    if (bias) (void)hipFree(bias);
  }
};

static size_t cs_npack(int rows, int red, int k) { return (size_t)((rows + 31) / 32) * k * ((red + 31) / 32 * 4) * 256; }

extern "C" {

int dissc_convsgrad_create(int Cin, int Cout, int k, int stride, dissc_convsgrad_t* out) {
  if (out) *out = nullptr;
  if (int rc = cg_check_create("dissc_convsgrad_create", out, Cin, Cout)) return rc;
  if (k < 3 || k > CG_MAX_K || k % 2 != 1) {
    set_error("dissc_convsgrad_create: kernel size %d (odd, 3 .. %d)", k, CG_MAX_K);
    return DISSC_EINVAL;
  }
  if (stride < 2 || stride > std::min(k, CT_MAX_S)) {
    set_error("dissc_convsgrad_create: stride %d with kernel size %d (2 <= stride <= min(k, %d))", stride, k, CT_MAX_S);
    return DISSC_EINVAL;
  }
  dissc_convsgrad* h = new dissc_convsgrad();
  h->opt = g_defaults;  // frozen here
  h->Cin = Cin; h->Cout = Cout; h->k = k; h->s = stride;
  *out = h;
  return DISSC_OK;
}

void dissc_convsgrad_destroy(dissc_convsgrad_t h) { delete h; }

int dissc_convsgrad_set_weights(dissc_convsgrad_t h, const float* w_dev, const float* bias_dev, void* stream) {
  if (!h || !w_dev) {
    set_error("dissc_convsgrad_set_weights: bad argument");
    return DISSC_EINVAL;
  }
  OptScope opt_scope(&h->opt);
  hipStream_t st = (hipStream_t)stream;
  const size_t nf = cs_npack(h->Cout, h->Cin, h->k), nb = cs_npack(h->Cin, h->Cout, h->k);
  if (!h->ready) {
    float *f = nullptr, *bk = nullptr, *bi = nullptr;  // handed to the handle only when all three are allocated
    if (hipMalloc((void**)&f, nf * sizeof(float)) != hipSuccess || hipMalloc((void**)&bk, nb * sizeof(float)) != hipSuccess ||
        hipMalloc((void**)&bi, (size_t)h->Cout * sizeof(float)) != hipSuccess) {
      if (f) (void)hipFree(f);
      if (bk) (void)hipFree(bk);
      set_error("dissc_convsgrad_set_weights: cannot allocate %zu bytes", (nf + nb + h->Cout) * sizeof(float));
      return DISSC_ENOMEM;
    }
    h->fpack = f; h->bpack = bk; h->bias = bi;
    h->ready = true;
  }
  CsPackArgs a;
  a.w = w_dev; a.bias = bias_dev; a.fpack = h->fpack; a.bpack = h->bpack; a.bias_out = h->bias;
  a.Cin = h->Cin; a.Cout = h->Cout; a.K = h->k;
  a.nblk_co = (h->Cout + 31) / 32; a.nblk_ci = (h->Cin + 31) / 32;
  a.cip8 = (h->Cin + 31) / 32 * 4; a.cop8 = (h->Cout + 31) / 32 * 4;
  const size_t most = std::max(std::max(nf, nb), (size_t)h->Cout);
  hipLaunchKernelGGL(convsgrad_pack_kernel, dim3((unsigned)((most + 255) / 256), 2), dim3(256), 0, st, a);
  DISSC_HIP_CHECK(hipGetLastError());
  return DISSC_OK;
}

long long dissc_convsgrad_packed(dissc_convsgrad_t h, int which, float* dst_dev, void* stream) {
  if (!h || which < 0 || which > 1) {
    set_error("dissc_convsgrad_packed: bad argument");
    return DISSC_EINVAL;
  }
  const size_t n = which ? cs_npack(h->Cin, h->Cout, h->k) : cs_npack(h->Cout, h->Cin, h->k);
  if (!dst_dev) return (long long)n;
  if (!h->ready) {
    set_error("dissc_convsgrad_packed: dissc_convsgrad_set_weights first");
    return DISSC_EINVAL;
  }
  DISSC_HIP_CHECK(hipMemcpyAsync(dst_dev, which ? h->bpack : h->fpack, n * sizeof(float), hipMemcpyDeviceToDevice, (hipStream_t)stream));
  return (long long)n;
}

// Lmax: input positions; a row of y / gy holds ceil(Lmax / stride)
int dissc_convsgrad_forward(dissc_convsgrad_t h, const float* x, float* y, const int32_t* lengths, int B, int ldx, int ldo,
                            int Lmax, float in_slope, void* stream) {
  int rc = cg_check_call(h, "dissc_convsgrad_forward", B, Lmax, 1, ldx, ldo, h ? h->s : 1);
  if (rc) return rc;
  if (!x || !y || ((uintptr_t)x & 15)) {
    set_error("dissc_convsgrad_forward: bad argument (x must be a 16-byte aligned device pointer)");
    return DISSC_EINVAL;
  }
  OptScope opt_scope(&h->opt);
  FwdSArgs a;
  a.x = x; a.apack = h->fpack; a.bias = h->bias; a.lengths = lengths; a.y = y;
  a.B = B; a.Cout = h->Cout; a.Cin = h->Cin; a.K = h->k; a.S = h->s; a.Lmax = Lmax; a.ldo = ldo; a.ldx = ldx;
  a.WM = h->Cout > 64 ? 4 : (h->Cout > 32 ? 2 : 1);
  a.WN = 4 / a.WM;
  a.cip8 = (h->Cin + 31) / 32 * 4;
  a.slope = in_slope;
  a.tp = ct_taps(h->k, h->s, (h->k - 1) / 2);
  const size_t row = (size_t)h->s * (32 * a.WN + 2 * a.tp.halo + 1) * sizeof(float);
  a.CK = h->Cin > 16 ? 32 : (h->Cin > 8 ? 16 : 8);  // a narrow layer (Cin = 1: the waveform) stages and multiplies 8 channels
  while (a.CK > 8 && a.CK * row > CS_FW_LDS) a.CK /= 2;
  const int TN = 32 * a.WN, olmax = (Lmax + h->s - 1) / h->s;
  hipLaunchKernelGGL(convsgrad_fwd_kernel, dim3((olmax + TN - 1) / TN, (h->Cout + 32 * a.WM - 1) / (32 * a.WM), B), dim3(256),
                     a.CK * row, (hipStream_t)stream, a);
  DISSC_HIP_CHECK(hipGetLastError());
  return DISSC_OK;
}

int dissc_convsgrad_partials(dissc_convsgrad_t h, int B, int Lmax, int* P, int* chunk) {
  if (int rc = cg_check_call(h, "dissc_convsgrad_partials", B, Lmax)) return rc;
  const CgPlan p = cs_plan(h->Cin, h->Cout, h->k, h->s, B, Lmax);
  if (P) *P = p.P;
  if (chunk) *chunk = p.cpp;
  return DISSC_OK;
}

size_t dissc_convsgrad_workspace_bytes(dissc_convsgrad_t h, int B, int Lmax) {
  if (!h || B <= 0 || Lmax <= 0) return 0;
  return cg_workspace(cs_plan(h->Cin, h->Cout, h->k, h->s, B, Lmax), B, h->Cout).bytes;
}

int dissc_convsgrad_backward(dissc_convsgrad_t h, const float* x, const float* gy, const int32_t* lengths, int B, int ldx,
                             int ldo, int Lmax, float in_slope, float* gx, float* gw, float* gb, void* workspace,
                             size_t workspace_bytes, void* stream) {
  const char* who = "dissc_convsgrad_backward";
  int rc = cg_check_call(h, who, B, Lmax, 1, ldx, ldo, h ? h->s : 1);
  if (rc) return rc;
  const CgPlan p = cs_plan(h->Cin, h->Cout, h->k, h->s, B, Lmax);
  float* part;
  double* bpart;
  if ((rc = cg_backward_begin(who, p, B, h->Cout, x, gy, gx, gw || gb, workspace, workspace_bytes, &part, &bpart))) return rc;
  OptScope opt_scope(&h->opt);
  hipStream_t st = (hipStream_t)stream;
  const CtTaps tp = ct_taps(h->k, h->s, (h->k - 1) / 2);
  if (gw) {
    WgradSArgs a;
    a.gy = gy; a.x = x; a.lengths = lengths; a.part = part;
    a.B = B; a.Cout = h->Cout; a.Cin = h->Cin; a.K = h->k; a.S = h->s; a.Lmax = Lmax; a.ldo = ldo; a.ldx = ldx;
    a.tsub = CG_T;
    while (a.tsub > CG_T / 4 && cs_wgrad_lds(h->s, p.WCI, a.tsub, tp.halo) > CS_WG_LDS) a.tsub /= 2;
    if (cs_wgrad_lds(h->s, p.WCI, a.tsub, tp.halo) > CS_WG_LDS1) {
      set_error("dissc_convsgrad_backward: the weight gradient's window does not fit (stride %d)", h->s);
      return DISSC_EINVAL;
    }
    a.slope = in_slope;
    a.WCI = p.WCI; a.WT = p.WT; a.nch = p.nch; a.cpp = p.cpp;
    a.tp = tp;
    if ((rc = cg_dispatch_ng(p.NG, who, "taps", [&](auto ng) { return cs_launch_wgrad<decltype(ng)::value>(a, p, st); }))) return rc;
    cg_launch_reduce(part, p.P * p.WT, p.gw, gw, st);
  }
  if (gb) cg_launch_bias(gy, lengths, 1, B, h->Cout, (Lmax + h->s - 1) / h->s, ldo, bpart, gb, st, h->s);
  if (gx) {
    DgradSArgs a;
    a.gy = gy; a.x = x; a.apack = h->bpack; a.lengths = lengths; a.gx = gx;
    a.B = B; a.Cout = h->Cout; a.Cin = h->Cin; a.K = h->k; a.Lmax = Lmax; a.ldo = ldo; a.ldx = ldx;
    a.WM = h->Cin > 64 ? 4 : (h->Cin > 32 ? 2 : 1);
    a.WN = 4 / a.WM;
    a.cop8 = (h->Cout + 31) / 32 * 4;
    a.slope = in_slope;
    a.tp = tp;
    for (int ph = 0; ph < CT_MAX_S; ++ph) a.kk0[ph] = a.nt[ph] = 0;
    for (int kk = h->k - 1; kk >= 0; --kk) {
      a.kk0[tp.p[kk]] = kk;
      ++a.nt[tp.p[kk]];
    }
    switch (h->s) {
#define CS_CASE(n) case n: cs_launch_dgrad<n>(a, st); break;
      CS_CASE(2) CS_CASE(3) CS_CASE(4) CS_CASE(5) CS_CASE(6) CS_CASE(7) CS_CASE(8)
#undef CS_CASE
    }
  }
  DISSC_HIP_CHECK(hipGetLastError());
  return DISSC_OK;
}

int dissc_period_fold_fwd(const float* wav, const int32_t* lengths, int B, int T, int period, int ldw, int ldh, float* x0,
                          void* stream) {
  if (!wav || !x0 || B <= 0 || B > 65535 || T <= 0 || period < 1 || period > 65535 || ldw < T || ldh < (T + period - 1) / period) {
    set_error("dissc_period_fold_fwd: bad argument (B = %d, T = %d, period = %d, ldw = %d, ldh = %d)", B, T, period, ldw, ldh);
    return DISSC_EINVAL;
  }
  const int H = (T + period - 1) / period;
  hipLaunchKernelGGL(period_fold_fwd_kernel, dim3((H + 255) / 256, period, B), dim3(256), 0, (hipStream_t)stream, wav, lengths,
                     period, T, ldw, ldh, x0);
  DISSC_HIP_CHECK(hipGetLastError());
  return DISSC_OK;
}

int dissc_period_fold_bwd(const float* gx0, const int32_t* lengths, int B, int T, int period, int ldw, int ldh, float* gwav,
                          void* stream) {
  if (!gx0 || !gwav || B <= 0 || B > 65535 || T <= 0 || period < 1 || period > 65535 || ldw < T || ldh < (T + period - 1) / period) {
    set_error("dissc_period_fold_bwd: bad argument (B = %d, T = %d, period = %d, ldw = %d, ldh = %d)", B, T, period, ldw, ldh);
    return DISSC_EINVAL;
  }
  hipLaunchKernelGGL(period_fold_bwd_kernel, dim3((ldw + 255) / 256, B), dim3(256), 0, (hipStream_t)stream, gx0, lengths, period,
                     T, ldw, ldh, gwav);
  DISSC_HIP_CHECK(hipGetLastError());
  return DISSC_OK;
}

}  // extern "C"
