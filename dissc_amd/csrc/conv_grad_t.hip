// A differentiable, ragged ConvTranspose1d layer for training the vocoder's generator on the MI355X: the five upsamplers
// ups[i] of the generator (512 -> 256 k 11 s 5, 256 -> 128 k 8 s 4, 128 -> 64 k 8 s 4, 64 -> 32 k 4 s 2, 32 -> 16 k 4 s 2), the
// layers conv_grad.hip's stride-1 Conv1d leaves out.
//
//   y[b,co,u] = bias[co] + sum_{ci,t,kk : s t + kk - pad = u} w[ci,co,kk] lrelu(x, in_slope)[b,ci,t],   pad = (k - s) / 2
//
// x [B][Cin][ldx] with lengths[b] valid INPUT positions, y [B][Cout][ldo] with s lengths[b] valid output positions; what lies
// beyond is read as zero and never written.  Everything is phrased on the s phase planes of the long side:
// plane_p[co][q] = gy[co][s q + p].  Tap kk touches ONE plane: kk - pad = s dl + p with 0 <= p < s, so that gy[s t + kk - pad]
// = plane_p[t + dl].
//   * Forward: convT_groups' phase-group launches of the direct conv kernels, as dissc_conv_transpose1d, but the packings are
//     built ON THE DEVICE from the master weights [Cin][Cout][k] (convtgrad_pack_kernel: one launch for every group, both
//     fragment orders, the bias replicated per phase row, and the data gradient's A fragments).
//   * Weight gradient: gw[ci][co][kk] = sum_b sum_{q < len_b} plane_p[co][q] lrelu(x)[ci][q - dl] -- conv_grad.hip's kernel
//     with a (plane, shift) per tap where that one has an offset per tap.  A chunk is 64 input positions = 64 s contiguous
//     columns of gy, read once with float4 loads and de-interleaved into the s planes in LDS; all k taps accumulate in one pass
//     on v_mfma_f32_32x32x2_f32 (as many MFMAs as the direct form: there are no zero taps).  The plan, the fixed-order sum over
//     the partials and the bias gradient are conv_grad.hip's (conv_grad.h), and so is the host side a layer handle shares with
//     the stride-1 one: the base CgLayer, the argument checks, the workspace layout and its carve, the dispatch over the taps.
//   * Data gradient: gx[ci][t] = lrelu'(x[ci][t]) sum_{co,kk} w[ci][co][kk] plane_p(kk)[co][t + dl(kk)], an implicit GEMM with
//     rows ci, columns t and the reduction over (co, kk) on the same MFMA.  The gy window of a column tile is staged
//     de-interleaved, so a B fragment is 32 consecutive floats of one plane; the derivative of the leaky ReLU (torch's rule at
//     x = 0: the slope) and the zeros from lengths[b] to the end of the row are the epilogue.
//     Where an utterance has fewer than 8 tiles of 128 rows (ups.0 at 28 columns) a workgroup takes 64 rows and two waves share
//     each tile's reduction, added in a fixed order: chosen from the layer and the row stride ldx, never from B or lengths, so an
//     utterance's gx bits do not depend on its batch (they do depend on the row stride it is stored with).
// LDS banks (ds_read_b32 / ds_write_b32: 32 banks, conflicts within a 32-lane half only).  Every fragment read is either 32
// consecutive floats or 32 rows of odd stride: conflict-free.  The de-interleaving writes of a float4 lane are s apart in
// column: conflict-free for s = 1 and 4, two-way for s = 2 and 8 and for some lane pairs of an odd s; they are 1 / k (weight
// gradient) or 1 / (Cin / 32 rows x k taps) (data gradient) of the LDS traffic.
#include <string.h>

#include <algorithm>

#include "conv_grad.h"

namespace dissc {

constexpr size_t CT_WG_LDS = 80 * 1024;  // weight gradient: two workgroups per CU, as conv_grad.hip
constexpr size_t CT_DG_LDS = 40 * 1024;  // data gradient: the staged slab of gy

// ---- the weight gradient ------------------------------------------------------------------------------------------------
struct WgradTArgs {
  const float* gy;   // [B][Cout][ldo]
  const float* x;    // [B][Cin][ldx], before the activation
  const int32_t* lengths;
  float* part;       // [P * WT][Cin][Cout][K]
  int B, Cout, Cin, K, S, Lmax, ldo, ldx;  // Lmax: input positions
  int tsub;          // positions staged at a time: CG_T, or CG_T / 2 where s planes of a whole chunk do not fit
  float slope;
  int WCI, WT, nch, cpp;
  CtTaps tp;
};

template <int NG>
__global__ void __launch_bounds__(256, 2) convtgrad_wgrad_kernel(WgradTArgs a) {
  extern __shared__ float ct_lds[];
  const int halo = a.tp.halo;
  const int ldd = a.tsub + 1, lda = a.tsub + 2 * halo + 1;  // odd row strides: a fragment read (32 rows x 1 column) is conflict-free
  float* ds = ct_lds;                      // planes of gy [S][32][ldd], column c = position ts0 + c
  float* as = ct_lds + a.S * 32 * ldd;     // lrelu(x) [32 WCI][lda], column c = position ts0 - halo + c
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int l31 = lane & 31, h = lane >> 5;
  const int wci = wave % a.WCI, wt = wave / a.WCI;
  const int co0 = blockIdx.x * 32, ci0 = blockIdx.y * 32 * a.WCI;
  const bool live = ci0 + wci * 32 < a.Cin;  // wave-uniform
  cg_f32x16 acc[NG];
  int aoff[NG], boff[NG];
#pragma unroll
  for (int g = 0; g < NG; ++g) {
#pragma unroll
    for (int e = 0; e < 16; ++e) acc[g][e] = 0.f;
    // rows of the tile are input channels, as in the master weights [Cin][Cout][k]: a lane's stores are k floats apart
    aoff[g] = (wci * 32 + l31) * lda + halo - a.tp.dl[g] + h;    // A: lrelu(x)[ci = l31][q - dl], q = ts0 + 2 s + h
    boff[g] = (a.tp.p[g] * 32 + l31) * ldd + h;                  // B: plane_p[co = l31][q]
  }
  const int nrows = 32 * a.WCI, aw4 = (a.tsub + 2 * halo) / 4;  // <= 20 float4 per row
  const int nv = a.S * a.tsub / 4;                               // float4 per row of the gy slab
  const int spw = (a.tsub / 2) / a.WT;                           // MFMA k-steps per time slice
  const long long npair = (long long)a.B * a.nch;
  const long long q0 = (long long)blockIdx.z * a.cpp, q1 = q0 + a.cpp < npair ? q0 + a.cpp : npair;
  for (long long q = q0; q < q1; ++q) {
    const int b = (int)(q / a.nch), t0 = (int)(q - (long long)b * a.nch) * CG_T;
    int len = a.lengths ? a.lengths[b] : a.Lmax;
    len = len < 0 ? 0 : (len > a.Lmax ? a.Lmax : len);
    const float* gyb = a.gy + ((size_t)b * a.Cout + co0) * a.ldo;
    const float* xb = a.x + ((size_t)b * a.Cin + ci0) * a.ldx;
    for (int ts0 = t0; ts0 < t0 + CG_T && ts0 < len; ts0 += a.tsub) {  // uniform over the workgroup
      __syncthreads();
      const int ulen = a.S * len;
      for (int e = tid; e < 32 * nv; e += 256) {  // S tsub contiguous columns of 32 rows of gy, de-interleaved
        const int r = e / nv, v = e - r * nv, u = a.S * ts0 + 4 * v;
        f32x4 g4 = {0.f, 0.f, 0.f, 0.f};
        if (u < ulen && co0 + r < a.Cout) g4 = *reinterpret_cast<const f32x4*>(gyb + (size_t)r * a.ldo + u);
#pragma unroll
        for (int qq = 0; qq < 4; ++qq) {
          const int c = 4 * v + qq, pos = c / a.S, p = c - pos * a.S;
          ds[(p * 32 + r) * ldd + pos] = (u + qq < ulen) ? g4[qq] : 0.f;
        }
      }
      {
        const int v = tid & 31, t = ts0 - halo + 4 * v;
        if (v < aw4)
          for (int r = tid >> 5; r < nrows; r += 8) {
            f32x4 x4 = {0.f, 0.f, 0.f, 0.f};
            if (t >= 0 && t < len && ci0 + r < a.Cin) x4 = *reinterpret_cast<const f32x4*>(xb + (size_t)r * a.ldx + t);
#pragma unroll
            for (int qq = 0; qq < 4; ++qq) {
              const float xv = x4[qq];
              as[r * lda + 4 * v + qq] = (t + qq < len) ? (xv > 0.f ? xv : xv * a.slope) : 0.f;  // (t < 0: loaded as zero)
            }
          }
      }
      __syncthreads();
      if (live) {
        const int nst = ((len - ts0 < a.tsub ? len - ts0 : a.tsub) + 1) >> 1;
        const int s0 = wt * spw, s1 = s0 + spw < nst ? s0 + spw : nst;
        for (int s = s0; s < s1; ++s) {
#pragma unroll
          for (int g = 0; g < NG; ++g)
            acc[g] = __builtin_amdgcn_mfma_f32_32x32x2f32(as[aoff[g] + 2 * s], ds[boff[g] + 2 * s], acc[g], 0, 0, 0);
        }
      }
    }
  }
  if (!live) return;
  const int co = co0 + l31;
  if (co >= a.Cout) return;
  float* pbase = a.part + (size_t)(blockIdx.z * a.WT + wt) * a.Cout * a.Cin * a.K;
#pragma unroll
  for (int g = 0; g < NG; ++g) {
#pragma unroll
    for (int r = 0; r < 16; ++r) {
      const int ci = ci0 + wci * 32 + (r & 3) + 8 * (r >> 2) + 4 * h;
      if (ci < a.Cin) pbase[((size_t)ci * a.Cout + co) * a.K + g] = acc[g][r];
    }
  }
}

// ---- the data gradient --------------------------------------------------------------------------------------------------
struct DgradTArgs {
  const float* gy;     // [B][Cout][ldo]
  const float* x;      // [B][Cin][ldx], before the activation
  const float* apack;  // [Cin / 32][K][cop8][64 lanes][4]: lane (i, hh), element e = w[ci = 32 blk + i][co = 8 c8 + 2 e + hh][kk]
  const int32_t* lengths;
  float* gx;           // [B][Cin][ldx]
  int B, Cout, Cin, K, S, Lmax, ldo, ldx;
  int WM, WN, KS;      // waves: WM blocks of 32 rows (ci) x WN blocks of 32 columns (t) x KS shares of a staged slab's channels
  int CK;              // output channels staged at a time (8, 16 or 32)
  int cop8;            // Cout rounded up to 32, / 8
  float slope;
  CtTaps tp;
};

__global__ void __launch_bounds__(256, 2) convtgrad_dgrad_kernel(DgradTArgs a) {
  extern __shared__ float ct_lds[];  // planes of the gy window [CK][S][ldw], column c = position t0 - halo + c
  const int halo = a.tp.halo;
  const int TN = 32 * a.WN, W = TN + 2 * halo, ldw = W + 1;
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int l31 = lane & 31, h = lane >> 5;
  const int wm = wave % a.WM, wn = (wave / a.WM) % a.WN, ks = wave / (a.WM * a.WN);
  const int n8 = (a.CK / 8) / a.KS, c80 = ks * n8;  // this wave's eights of a slab's channels: [c80, c80 + n8), n8 <= 4
  const int b = blockIdx.z, t0 = blockIdx.x * TN;
  const int blk = blockIdx.y * a.WM + wm;  // this wave's block of 32 input channels
  int len = a.lengths ? a.lengths[b] : a.Lmax;
  len = len < 0 ? 0 : (len > a.Lmax ? a.Lmax : len);
  const bool live = blk * 32 < a.Cin && t0 + wn * 32 < len;  // wave-uniform
  cg_f32x16 acc;
#pragma unroll
  for (int e = 0; e < 16; ++e) acc[e] = 0.f;
  if (t0 < len) {  // uniform over the workgroup
    const int nv = a.S * W / 4, u0 = a.S * (t0 - halo), ulen = a.S * len;  // u0 % 4 == 0: t0 % 32 == 0, halo % 4 == 0
    const f32x4* ap = reinterpret_cast<const f32x4*>(a.apack) + (size_t)blk * a.K * a.cop8 * 64 + lane;
    const int col = wn * 32 + l31 + halo;
    for (int co0 = 0; co0 < a.Cout; co0 += a.CK) {
      __syncthreads();
      const float* gyb = a.gy + ((size_t)b * a.Cout + co0) * a.ldo;
      for (int e = tid; e < a.CK * nv; e += 256) {
        const int r = e / nv, v = e - r * nv, u = u0 + 4 * v;
        f32x4 g4 = {0.f, 0.f, 0.f, 0.f};
        if (u >= 0 && u < ulen && co0 + r < a.Cout) g4 = *reinterpret_cast<const f32x4*>(gyb + (size_t)r * a.ldo + u);
#pragma unroll
        for (int qq = 0; qq < 4; ++qq) {
          const int c = 4 * v + qq, pos = c / a.S, p = c - pos * a.S;
          ct_lds[(r * a.S + p) * ldw + pos] = (u + qq < ulen) ? g4[qq] : 0.f;  // (u < 0: loaded as zero)
        }
      }
      __syncthreads();
      if (live) {
        const f32x4* apc = ap + (size_t)(co0 / 8 + c80) * 64;
        f32x4 cur[4], nxt[4];  // the A fragments of tap kk, those of kk + 1 in flight behind its MFMAs
#pragma unroll
        for (int c = 0; c < 4; ++c) {
          cur[c] = nxt[c] = f32x4{0.f, 0.f, 0.f, 0.f};
          if (c < n8) cur[c] = apc[(size_t)c * 64];
        }
        for (int kk = 0; kk < a.K; ++kk) {
          if (kk + 1 < a.K) {
            const f32x4* apn = apc + (size_t)(kk + 1) * a.cop8 * 64;
#pragma unroll
            for (int c = 0; c < 4; ++c)
              if (c < n8) nxt[c] = apn[(size_t)c * 64];
          }
          // B: plane_p[co = 8 (c80 + c) + 2 e + h][t + dl]
          const float* bp = ct_lds + ((c80 * 8 + h) * a.S + a.tp.p[kk]) * ldw + col + a.tp.dl[kk];
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
    if (a.KS > 1) {  // the shares of a tile's reduction, added in the order of ks (KS = 2 only)
      __syncthreads();
      float* red = ct_lds + (wm * a.WN + wn) * 16 * 64;
      if (live && ks == 1)
#pragma unroll
        for (int r = 0; r < 16; ++r) red[r * 64 + lane] = acc[r];
      __syncthreads();
      if (live && ks == 0)
#pragma unroll
        for (int r = 0; r < 16; ++r) acc[r] += red[r * 64 + lane];
    }
  }
  if (ks != 0) return;
  if (blk * 32 >= a.Cin) return;
  const int t = t0 + wn * 32 + l31;
  if (t >= a.ldx) return;
#pragma unroll
  for (int r = 0; r < 16; ++r) {
    const int ci = blk * 32 + (r & 3) + 8 * (r >> 2) + 4 * h;
    if (ci >= a.Cin) continue;
    const size_t i = ((size_t)b * a.Cin + ci) * a.ldx + t;
    float v = 0.f;  // zero from lengths[b] to the end of the row
    if (t < len) v = a.x[i] > 0.f ? acc[r] : acc[r] * a.slope;
    a.gx[i] = v;
  }
}

// ---- packing on the device ----------------------------------------------------------------------------------------------
struct CtPackGroup {
  float* wpack;  // the A-fragment order of conv_mfma32_kernel (m32) or of conv_mfma_kernel, as convgrad_repack_kernel writes it
  float* bias;   // [Mpad]
  int np, p0, dlo, ntap, nsub, nchunk, m32, Mpad;
};
struct CtPackArgs {
  const float* w;     // master weights [Cin][Cout][K]
  const float* bias;  // [Cout] or nullptr
  float* apack;       // DgradTArgs::apack
  int Cin, Cout, K, S, ngroups, nblk, cop8;
  CtPackGroup g[CT_MAX_S];
};

// blockIdx.y < ngroups: phase group y as a DevConv of Cout np rows (row = co np + pi) over the input taps dlo .. dlo + ntap - 1,
// tap j of phase p0 + pi being kk = p0 + pi + pad - S (dlo + j), zero where kk falls outside [0, K) (convT_phase_weights), and
// its bias; blockIdx.y == ngroups: the data gradient's A fragments.
__global__ void __launch_bounds__(256) convtgrad_pack_kernel(CtPackArgs a) {
  const size_t idx = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  if ((int)blockIdx.y == a.ngroups) {
    const size_t total = (size_t)a.nblk * a.K * a.cop8 * 256;
    if (idx >= total) return;
    const int e = idx & 3, lane = (idx >> 2) & 63;
    size_t r = idx >> 8;
    const int c8 = (int)(r % a.cop8);
    r /= a.cop8;
    const int kk = (int)(r % a.K), blk = (int)(r / a.K);
    const int ci = blk * 32 + (lane & 31), co = c8 * 8 + 2 * e + (lane >> 5);
    a.apack[idx] = (ci < a.Cin && co < a.Cout) ? a.w[((size_t)ci * a.Cout + co) * a.K + kk] : 0.f;
    return;
  }
  const CtPackGroup& g = a.g[blockIdx.y];
  const size_t total = (size_t)g.nsub * g.nchunk * g.ntap * (g.m32 ? 512 : 256);
  if (idx < (size_t)g.Mpad) g.bias[idx] = (a.bias && (int)idx < a.Cout * g.np) ? a.bias[idx / g.np] : 0.f;
  if (idx >= total) return;
  const int e = idx & 3, lane = (idx >> 2) & 63;
  int row, col, j;
  if (g.m32) {
    const int hf = (idx >> 8) & 1;
    size_t r = idx >> 9;
    j = (int)(r % g.ntap);
    r /= g.ntap;
    const int c = (int)(r % g.nchunk), ms = (int)(r / g.nchunk);
    row = ms * 32 + (lane & 31);
    col = c * KC + 2 * (4 * hf + e) + (lane >> 5);
  } else {
    size_t r = idx >> 8;
    j = (int)(r % g.ntap);
    r /= g.ntap;
    const int c = (int)(r % g.nchunk), ms = (int)(r / g.nchunk);
    row = ms * 16 + (lane & 15);
    col = c * KC + e * 4 + (lane >> 4);
  }
  float v = 0.f;
  if (row < a.Cout * g.np && col < a.Cin) {
    const int co = row / g.np, pi = row - co * g.np;
    const int kk = g.p0 + pi + (a.K - a.S) / 2 - a.S * (g.dlo + j);
    if (kk >= 0 && kk < a.K) v = a.w[((size_t)col * a.Cout + co) * a.K + kk];
  }
  g.wpack[idx] = v;
}

// conv_grad.hip's plan for the same reduction; a tap's A operand is its own plane, so taps never share an MFMA
static CgPlan ct_plan(int Cin, int Cout, int K, int B, int Lmax) {
  CgPlan p = cg_plan(Cin, Cout, K, B, Lmax);
  p.CIB = 32; p.TS = 1; p.NG = K;
  return p;
}

static size_t ct_wgrad_lds(int S, int WCI, int tsub, int halo) {
  return ((size_t)S * 32 * (tsub + 1) + (size_t)32 * WCI * (tsub + 2 * halo + 1)) * sizeof(float);
}

template <int NG>
static int ct_launch_wgrad(const WgradTArgs& a, const CgPlan& p, hipStream_t st) {
  static DeviceOnce attr_once;  // per device (common.h)
  DISSC_HIP_CHECK(attr_once.max_lds(reinterpret_cast<const void*>(&convtgrad_wgrad_kernel<NG>), (int)CT_WG_LDS));
  hipLaunchKernelGGL((convtgrad_wgrad_kernel<NG>), dim3(p.coT, p.ciS, p.P), dim3(256), ct_wgrad_lds(a.S, a.WCI, a.tsub, a.tp.halo),
                     st, a);
  return DISSC_OK;
}

}  // namespace dissc

using namespace dissc;

struct dissc_convtgrad : CgLayer {
  int s = 1;
  std::vector<ConvTGroup> plan;
  std::vector<DevConv> fwd;  // one per phase group
  float* apack = nullptr;    // the data gradient's A fragments
  ~dissc_convtgrad() {
    for (auto& dc : fwd) free_conv(dc);
    if (apack) (void)hipFree(apack);
  }
};

extern "C" {

int dissc_convtgrad_create(int Cin, int Cout, int k, int stride, dissc_convtgrad_t* out) {
  if (out) *out = nullptr;
  if (int rc = cg_check_create("dissc_convtgrad_create", out, Cin, Cout)) return rc;
  if (stride < 1 || stride > CT_MAX_S) {
    set_error("dissc_convtgrad_create: stride %d (1 .. %d)", stride, CT_MAX_S);
    return DISSC_EINVAL;
  }
  if (k < stride || k > CG_MAX_K || (k - stride) % 2 != 0) {
    set_error("dissc_convtgrad_create: kernel size %d with stride %d (stride <= k <= %d, k - stride even)", k, stride, CG_MAX_K);
    return DISSC_EINVAL;
  }
  dissc_convtgrad* h = new dissc_convtgrad();
  h->opt = g_defaults;  // frozen here
  h->Cin = Cin; h->Cout = Cout; h->k = k; h->s = stride;
  convT_groups(Cout, k, stride, h->plan);
  *out = h;
  return DISSC_OK;
}

void dissc_convtgrad_destroy(dissc_convtgrad_t h) { delete h; }

int dissc_convtgrad_set_weights(dissc_convtgrad_t h, const float* w_dev, const float* bias_dev, void* stream) {
  if (!h || !w_dev) {
    set_error("dissc_convtgrad_set_weights: bad argument");
    return DISSC_EINVAL;
  }
  OptScope opt_scope(&h->opt);
  hipStream_t st = (hipStream_t)stream;
  const int nblk = (h->Cin + 31) / 32, cop8 = (h->Cout + 31) / 32 * 4;
  const size_t napack = (size_t)nblk * h->k * cop8 * 256;
  if (!h->ready) {
    std::vector<DevConv> fwd;  // handed to the handle only when every group and the fragments are allocated
    float* apack = nullptr;
    int rc = DISSC_OK;
    for (const ConvTGroup& g : h->plan) {
      fwd.emplace_back();
      DevConv& dc = fwd.back();
      if ((rc = cg_alloc_conv("dissc_convtgrad_set_weights", h->Cout * g.np, h->Cin, g.ntap, 1, -g.dlo, dc))) break;
      dc.up = h->s; dc.up_np = g.np; dc.up_p0 = g.p0;
    }
    if (!rc && hipMalloc((void**)&apack, napack * sizeof(float)) != hipSuccess) {
      set_error("dissc_convtgrad_set_weights: cannot allocate %zu bytes", napack * sizeof(float));
      rc = DISSC_ENOMEM;
    }
    if (rc) {
      for (auto& dc : fwd) free_conv(dc);
      return rc;
    }
    h->fwd.swap(fwd);
    h->apack = apack;
    h->ready = true;
  }
  CtPackArgs a;
  a.w = w_dev; a.bias = bias_dev; a.apack = h->apack;
  a.Cin = h->Cin; a.Cout = h->Cout; a.K = h->k; a.S = h->s; a.ngroups = (int)h->plan.size(); a.nblk = nblk; a.cop8 = cop8;
  size_t most = napack;
  for (int i = 0; i < a.ngroups; ++i) {
    const DevConv& dc = h->fwd[i];
    CtPackGroup& g = a.g[i];
    g.wpack = dc.wpack; g.bias = dc.bias;
    g.np = h->plan[i].np; g.p0 = h->plan[i].p0; g.dlo = h->plan[i].dlo; g.ntap = h->plan[i].ntap;
    g.m32 = dc.m32; g.Mpad = dc.Mpad; g.nsub = dc.Mpad / (dc.m32 ? 32 : 16); g.nchunk = dc.nchunk;
    most = std::max(most, std::max((size_t)g.nsub * g.nchunk * g.ntap * (g.m32 ? 512 : 256), (size_t)g.Mpad));
  }
  hipLaunchKernelGGL(convtgrad_pack_kernel, dim3((unsigned)((most + 255) / 256), a.ngroups + 1), dim3(256), 0, st, a);
  DISSC_HIP_CHECK(hipGetLastError());
  return DISSC_OK;
}

// Lmax: input positions; a row of y / gy holds stride * Lmax
int dissc_convtgrad_forward(dissc_convtgrad_t h, const float* x, float* y, const int32_t* lengths, int B, int ldx, int ldo,
                            int Lmax, float in_slope, void* stream) {
  int rc = cg_check_call(h, "dissc_convtgrad_forward", B, Lmax, h ? h->s : 1, ldx, ldo);
  if (rc) return rc;
  if (!x || !y) {
    set_error("dissc_convtgrad_forward: bad argument");
    return DISSC_EINVAL;
  }
  OptScope opt_scope(&h->opt);
  for (const DevConv& dc : h->fwd)
    if ((rc = run_conv(dc, x, y, batch_of(lengths, 1, B, Lmax), EpiSpec(), h->Cin, ldx, ldo, in_slope, (hipStream_t)stream)))
      return rc;
  return DISSC_OK;
}

int dissc_convtgrad_partials(dissc_convtgrad_t h, int B, int Lmax, int* P, int* chunk) {
  if (int rc = cg_check_call(h, "dissc_convtgrad_partials", B, Lmax)) return rc;
  const CgPlan p = ct_plan(h->Cin, h->Cout, h->k, B, Lmax);
  if (P) *P = p.P;
  if (chunk) *chunk = p.cpp;
  return DISSC_OK;
}

size_t dissc_convtgrad_workspace_bytes(dissc_convtgrad_t h, int B, int Lmax) {
  if (!h || B <= 0 || Lmax <= 0) return 0;
  return cg_workspace(ct_plan(h->Cin, h->Cout, h->k, B, Lmax), B, h->Cout).bytes;
}

int dissc_convtgrad_backward(dissc_convtgrad_t h, const float* x, const float* gy, const int32_t* lengths, int B, int ldx,
                             int ldo, int Lmax, float in_slope, float* gx, float* gw, float* gb, void* workspace,
                             size_t workspace_bytes, void* stream) {
  const char* who = "dissc_convtgrad_backward";
  int rc = cg_check_call(h, who, B, Lmax, h ? h->s : 1, ldx, ldo);
  if (rc) return rc;
  const CgPlan p = ct_plan(h->Cin, h->Cout, h->k, B, Lmax);
  float* part;
  double* bpart;
  if ((rc = cg_backward_begin(who, p, B, h->Cout, x, gy, gx, gw || gb, workspace, workspace_bytes, &part, &bpart))) return rc;
  OptScope opt_scope(&h->opt);
  hipStream_t st = (hipStream_t)stream;
  const CtTaps tp = ct_taps(h->k, h->s, (h->k - h->s) / 2);
  if (gw) {
    WgradTArgs a;
    a.gy = gy; a.x = x; a.lengths = lengths; a.part = part;
    a.B = B; a.Cout = h->Cout; a.Cin = h->Cin; a.K = h->k; a.S = h->s; a.Lmax = Lmax; a.ldo = ldo; a.ldx = ldx;
    a.tsub = ct_wgrad_lds(h->s, p.WCI, CG_T, tp.halo) <= CT_WG_LDS ? CG_T : CG_T / 2;
    a.slope = in_slope;
    a.WCI = p.WCI; a.WT = p.WT; a.nch = p.nch; a.cpp = p.cpp;
    a.tp = tp;
    if (ct_wgrad_lds(h->s, p.WCI, a.tsub, tp.halo) > CT_WG_LDS) {
      set_error("dissc_convtgrad_backward: the weight gradient's window does not fit (stride %d)", h->s);
      return DISSC_EINVAL;
    }
    if ((rc = cg_dispatch_ng(p.NG, who, "taps", [&](auto ng) { return ct_launch_wgrad<decltype(ng)::value>(a, p, st); }))) return rc;
    cg_launch_reduce(part, p.P * p.WT, p.gw, gw, st);
  }
  if (gb) cg_launch_bias(gy, lengths, h->s, B, h->Cout, h->s * Lmax, ldo, bpart, gb, st);
  if (gx) {
    DgradTArgs a;
    a.gy = gy; a.x = x; a.apack = h->apack; a.lengths = lengths; a.gx = gx;
    a.B = B; a.Cout = h->Cout; a.Cin = h->Cin; a.K = h->k; a.S = h->s; a.Lmax = Lmax; a.ldo = ldo; a.ldx = ldx;
    // ups.0 / ups.1 run at 28 / 140 columns per utterance in training: wide layers take 32-column tiles, 128 rows a workgroup
    a.WM = h->Cin > 64 ? 4 : (h->Cin > 32 ? 2 : 1);
    a.WN = 4 / a.WM;
    a.KS = 1;
    a.cop8 = (h->Cout + 31) / 32 * 4;
    a.slope = in_slope;
    a.tp = tp;
    const size_t row = (size_t)h->s * (32 * a.WN + 2 * tp.halo + 1) * sizeof(float);
    a.CK = 32;
    while (a.CK > 8 && a.CK * row > CT_DG_LDS) a.CK /= 2;
    size_t lds = a.CK * row;
    // fewer than 8 tiles of 128 rows an utterance (ups.0: 4) leave CUs idle at the trainer's batch: 64 rows a workgroup, two waves
    // on each half of a slab's channels.  A function of the layer and the row stride ldx, never of B or lengths: an utterance's gx
    // bits do not depend on its batch (they do depend on the row stride it is stored with).
    if (a.WM == 4 && a.CK >= 16 && ((ldx + 31) / 32) * ((h->Cin + 127) / 128) < 8) {
      a.WM = 2;
      a.KS = 2;
      // the shares meet in LDS, one 16 x 64 accumulator per (wm, wn): more than the slab of a small stride (s = 1: 4-6 KB)
      lds = std::max(lds, (size_t)a.WM * a.WN * 16 * 64 * sizeof(float));
    }
    hipLaunchKernelGGL(convtgrad_dgrad_kernel, dim3((ldx + 32 * a.WN - 1) / (32 * a.WN), (h->Cin + 32 * a.WM - 1) / (32 * a.WM), B),
                       dim3(256), lds, st, a);
  }
  DISSC_HIP_CHECK(hipGetLastError());
  return DISSC_OK;
}

}  // extern "C"
