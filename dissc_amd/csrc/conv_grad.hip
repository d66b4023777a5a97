// A differentiable, ragged, stride-1 "same" Conv1d layer for training the vocoder's generator on the MI355X: the
// stride-1 dilated convs are 92 of the generator's 97 conv layers (conv_pre, the 90 ResBlock convs, conv_post).
//
//   y[b,:,t] = bias + sum_j w[:,:,j] . lrelu(x, in_slope)[b,:,t + j d - pad]  (+ add[b,:,t]),   pad = (k - 1) d / 2
//
// with dissc_conv1d's conventions (positions >= lengths[b] read as zero, never written).  Forward and backward-data run on the
// existing direct conv kernels (conv_mfma32_kernel, or the 16-row conv_mfma_kernel below 32 rows); backward-data is the same
// conv with the transposed, tap-flipped weights, as in train.hip.  Both packings are rebuilt ON THE DEVICE from the master
// weights [Cout][Cin][k] (convgrad_repack_kernel), so no weight makes a host round trip in a step.
//
// The weight gradient is the new kernel.  gw[co][ci][j] = sum_b sum_{t < len_b} gy[b][co][t] lrelu(x)[b][ci][t + off_j]
// is a [Cout x T] x [T x (k Cin)] GEMM whose reduction axis is (utterance, time) -- up to 32 x 8 960 = 286 720 long.
// v_mfma_f32_32x32x2_f32: A = 32 output channels x 2 positions, B = 32 "columns" x the same 2 positions, one accumulator
// per tap group, all fed from one LDS window of lrelu(x) (the activation is applied on load, as the forward does).
//   * The reduction is cut into chunks of CG_T = 64 positions; the (utterance, chunk) pairs, in the order b-major, are
//     dealt in consecutive runs of `cpp` pairs to P workgroups per output tile.  Each writes its own partial; a second
//     kernel sums the partials in a fixed order.  No atomics; P depends on the shape only (cg_plan), never on lengths.
//   * Narrow layers.  With Cin <= 16 the 32 B columns hold TS = 32 / CIB taps of CIB = 16 (8, 4, ..) channels each, so a
//     C = 16, k = 11 layer issues 6 MFMAs per step instead of 11; with Cin <= 64 the four waves that would sit on absent
//     channel blocks split the chunk's positions instead (WT = 2 or 4 time slices, each its own partial).
//   * Tap offsets are off_j = off0 + j dstep with |off_j| <= 32: nothing ties them to (k - 1) d / 2.  A ConvTranspose1d's
//     weight gradient (a stride-1 correlation of x with the phase planes of gy) is conv_grad_t.hip's kernel: this one with a
//     (plane, shift) per tap; it shares the plan, the reduction and the bias kernels below through conv_grad.h.
// A handle of dissc_convgrad_create_prec(prec = 1) runs each direction that has an instance in split-bf16 arithmetic instead:
// forward and backward-data on conv_bf3_kernel, the weight gradient on conv_grad_bf3.hip's kernel, both packings written by its
// repack kernel; every other direction, and every prec = 0 handle, runs exactly what is described above.
// The host side the two layers have in common is defined here too (conv_grad.h: CgLayer, the argument checks, the workspace
// layout with the preamble that carves it, cg_alloc_conv).
#include <string.h>

#include <algorithm>

#include "conv_grad.h"

namespace dissc {

constexpr int CG_HALO = 32;                 // largest |tap offset|, rounded up to 4 (MAX_TAP_SPAN / 2 = 30)
constexpr int CG_LDD = CG_T + 1;            // odd row strides: a fragment read (32 rows x 1 column) is conflict-free
constexpr int CG_HALO_WIDE = 36;            // ... of the spans in (MAX_TAP_SPAN, RB_TAP_SPAN]: instances of their own, so that the
                                            // LDS layout of every span <= MAX_TAP_SPAN stays what it was
constexpr int cg_lda(int halo) { return CG_T + 2 * halo + 1; }
constexpr size_t CG_PART_BUDGET = (size_t)56 << 20;  // bytes of partials (the workspace stays under 64 MB)
constexpr int CG_TARGET_WG = 512;           // two workgroups per CU

CgPlan cg_plan(int Cin, int Cout, int K, int B, int Lmax) {
  CgPlan p;
  p.WCI = Cin > 64 ? 4 : (Cin > 32 ? 2 : 1);
  p.WT = 4 / p.WCI;
  p.CIB = 32;
  while (p.CIB > 1 && p.CIB / 2 >= Cin) p.CIB /= 2;
  p.TS = 32 / p.CIB;
  p.NG = (K + p.TS - 1) / p.TS;
  p.coT = (Cout + 31) / 32;
  p.ciS = (Cin + 32 * p.WCI - 1) / (32 * p.WCI);
  p.nch = (Lmax + CG_T - 1) / CG_T;
  p.gw = (size_t)Cout * Cin * K;
  const long long N = (long long)B * p.nch;
  long long P = (CG_TARGET_WG + (long long)p.coT * p.ciS - 1) / ((long long)p.coT * p.ciS);
  const long long cap = (long long)(CG_PART_BUDGET / (p.gw * sizeof(float))) / p.WT;
  P = std::min(P, std::max(cap, 1LL));
  P = std::max(1LL, std::min(P, N));
  p.cpp = (int)((N + P - 1) / P);
  p.P = (int)((N + p.cpp - 1) / p.cpp);  // no empty partial
  return p;
}

template <int NG, int HALO = CG_HALO>
__global__ void __launch_bounds__(256, 2) convgrad_wgrad_kernel(WgradArgs a) {
  constexpr int CG_LDA = cg_lda(HALO);
  extern __shared__ float cg_lds[];
  float* ds = cg_lds;                 // gy  [32][CG_LDD]
  float* as = cg_lds + 32 * CG_LDD;   // lrelu(x) [32 WCI][CG_LDA], column c = position t0 - halo + c
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int l31 = lane & 31, h = lane >> 5;
  const int wci = wave % a.WCI, wt = wave / a.WCI;
  const int co0 = blockIdx.x * 32, ci0 = blockIdx.y * 32 * a.WCI;
  const int cil = l31 & (a.CIB - 1), tsub = l31 / a.CIB;  // this lane's B column: channel within the block, tap within the group
  const bool live = ci0 + wci * 32 < a.Cin;               // wave-uniform
  cg_f32x16 acc[NG];
  int boff[NG];
#pragma unroll
  for (int g = 0; g < NG; ++g) {
#pragma unroll
    for (int e = 0; e < 16; ++e) acc[g][e] = 0.f;
    const int tap = g * a.TS + tsub;
    const int tc = tap < a.K ? tap : a.K - 1;  // a column beyond the last tap reads a valid address; it is never stored
    boff[g] = (wci * 32 + cil) * CG_LDA + a.halo + a.off0 + tc * a.dstep + h;
  }
  const int nrows = 32 * a.WCI, aw4 = (CG_T + 2 * a.halo) / 4;
  const int spw = (CG_T / 2) / a.WT;  // MFMA k-steps per time slice
  const long long npair = (long long)a.B * a.nch;
  const long long q0 = (long long)blockIdx.z * a.cpp, q1 = q0 + a.cpp < npair ? q0 + a.cpp : npair;
  for (long long q = q0; q < q1; ++q) {
    const int b = (int)(q / a.nch), t0 = (int)(q - (long long)b * a.nch) * CG_T;
    int len = a.lengths ? a.lengths[b] : a.Lmax;
    len = len < 0 ? 0 : (len > a.Lmax ? a.Lmax : len);
    if (t0 >= len) continue;  // uniform over the workgroup
    __syncthreads();
    const float* gyb = a.gy + ((size_t)b * a.Cout + co0) * a.ldo;
    const float* xb = a.x + ((size_t)b * a.Cin + ci0) * a.ldx;
#pragma unroll
    for (int i = 0; i < 2; ++i) {  // gy tile: 32 rows x 16 float4
      const int e = tid + i * 256, r = e >> 4, v = e & 15, t = t0 + 4 * v;
      f32x4 g4 = {0.f, 0.f, 0.f, 0.f};
      if (t < len && co0 + r < a.Cout) g4 = *reinterpret_cast<const f32x4*>(gyb + (size_t)r * a.ldo + t);
#pragma unroll
      for (int qq = 0; qq < 4; ++qq) ds[r * CG_LDD + 4 * v + qq] = (t + qq < len) ? g4[qq] : 0.f;
    }
    {
      // (a wide halo's rows are up to 34 float4 long: two passes of the 32 lanes that share a row)
      for (int v = tid & 31; v < aw4; v += (HALO > CG_HALO ? 32 : aw4)) {
        const int t = t0 - a.halo + 4 * v;
        for (int r = tid >> 5; r < nrows; r += 8) {
          f32x4 x4 = {0.f, 0.f, 0.f, 0.f};
          if (t >= 0 && t < len && ci0 + r < a.Cin) x4 = *reinterpret_cast<const f32x4*>(xb + (size_t)r * a.ldx + t);
#pragma unroll
          for (int qq = 0; qq < 4; ++qq) {
            const float xv = x4[qq];
            as[r * CG_LDA + 4 * v + qq] = (t + qq < len) ? (xv > 0.f ? xv : xv * a.slope) : 0.f;  // (t < 0: loaded as zero)
          }
        }
      }
    }
    __syncthreads();
    if (live) {
      const int nst = ((len - t0 < CG_T ? len - t0 : CG_T) + 1) >> 1;
      const int s0 = wt * spw, s1 = s0 + spw < nst ? s0 + spw : nst;
      const float* ap = ds + l31 * CG_LDD + h;  // A: gy[co = l31][t0 + 2 s + h]
      for (int s = s0; s < s1; ++s) {
        const float av = ap[2 * s];
#pragma unroll
        for (int g = 0; g < NG; ++g) acc[g] = __builtin_amdgcn_mfma_f32_32x32x2f32(av, as[boff[g] + 2 * s], acc[g], 0, 0, 0);
      }
    }
  }
  if (!live) return;
  const int ci = ci0 + wci * 32 + cil;
  if (ci >= a.Cin) return;
  float* pbase = a.part + (size_t)(blockIdx.z * a.WT + wt) * a.Cout * a.Cin * a.K;
#pragma unroll
  for (int g = 0; g < NG; ++g) {
    const int tap = g * a.TS + tsub;
    if (tap >= a.K) continue;
#pragma unroll
    for (int r = 0; r < 16; ++r) {
      const int co = co0 + (r & 3) + 8 * (r >> 2) + 4 * h;
      if (co < a.Cout) pbase[((size_t)co * a.Cin + ci) * a.K + tap] = acc[g][r];
    }
  }
}

// out[i] = sum over the NP partials in a fixed order: sixteen strided chains per element (chain s takes partials s, s + 16,
// ..., eight loads in flight, added in that order), then a fixed pairwise tree over the chains.  A narrow layer has ~2 000
// partials of a few hundred elements: with one chain per element the kernel was one long dependent walk through memory.
__global__ void __launch_bounds__(256) convgrad_reduce_kernel(const float* __restrict__ part, int NP, size_t n,
                                                              float* __restrict__ out) {
  __shared__ float red[16][17];
  const int e = threadIdx.x & 15, s = threadIdx.x >> 4;
  const size_t i = (size_t)blockIdx.x * 16 + e;
  float sum = 0.f;
  if (i < n) {
    int p = s;
    for (; p + 16 * 7 < NP; p += 16 * 8) {
      float v[8];
#pragma unroll
      for (int q = 0; q < 8; ++q) v[q] = part[(size_t)(p + 16 * q) * n + i];
#pragma unroll
      for (int q = 0; q < 8; ++q) sum += v[q];
    }
    for (; p < NP; p += 16) sum += part[(size_t)p * n + i];
  }
  red[s][e] = sum;
  __syncthreads();
  if (s == 0 && i < n) {
    float t[16];
#pragma unroll
    for (int q = 0; q < 16; ++q) t[q] = red[q][e];
#pragma unroll
    for (int w = 1; w < 16; w *= 2)
#pragma unroll
      for (int q = 0; q < 16; q += 2 * w) t[q] += t[q + w];
    out[i] = t[0];
  }
}

__device__ __forceinline__ double cg_block_sum_d(double v, double* red) {
  const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) v += __shfl_xor(v, off);
  __syncthreads();
  if (lane == 0) red[wv] = v;
  __syncthreads();
  return (red[0] + red[1]) + (red[2] + red[3]);
}

// bpart[b][co] = sum_{t < len_b} gy[b][co][t], len_b = ceil(lengths[b] * len_mul / len_div) (a ConvTranspose1d's rows are stride
// times its lengths, a strided Conv1d's ceil(lengths / stride))
__global__ void __launch_bounds__(256) convgrad_bias_part_kernel(const float* __restrict__ gy, const int32_t* __restrict__ lengths,
                                                                 int len_mul, int len_div, int Cout, int Lmax, int ldo,
                                                                 double* __restrict__ bpart) {
  __shared__ double red[4];
  const int co = blockIdx.x, b = blockIdx.y;
  int len = lengths ? (lengths[b] * len_mul + len_div - 1) / len_div : Lmax;
  len = len < 0 ? 0 : (len > Lmax ? Lmax : len);
  const float* row = gy + ((size_t)b * Cout + co) * ldo;
  double s = 0.0;
  for (int t = threadIdx.x; t < len; t += 256) s += row[t];
  s = cg_block_sum_d(s, red);
  if (threadIdx.x == 0) bpart[(size_t)b * Cout + co] = s;
}

__global__ void convgrad_bias_reduce_kernel(const double* __restrict__ bpart, int B, int Cout, float* __restrict__ gb) {
  const int co = blockIdx.x * blockDim.x + threadIdx.x;
  if (co >= Cout) return;
  double s = 0.0;
  for (int b = 0; b < B; ++b) s += bpart[(size_t)b * Cout + co];
  gb[co] = (float)s;
}

// gx = (x > 0 ? 1 : slope) * gx inside an utterance (torch's rule at x = 0), zero from lengths[b] to the end of the row
__global__ void convgrad_mask_kernel(const float* __restrict__ x, const int32_t* __restrict__ lengths, int C, int Lmax, int ld,
                                     float slope, float* __restrict__ gx) {
  const int b = blockIdx.z, c = blockIdx.y;
  const int t = 4 * (blockIdx.x * blockDim.x + threadIdx.x);
  if (t >= ld) return;
  int len = lengths ? lengths[b] : Lmax;
  len = len < 0 ? 0 : (len > Lmax ? Lmax : len);
  const size_t i = ((size_t)b * C + c) * ld + t;
  f32x4 g = {0.f, 0.f, 0.f, 0.f};
  if (t < len) {
    g = *reinterpret_cast<const f32x4*>(gx + i);
    const f32x4 xv = *reinterpret_cast<const f32x4*>(x + i);
#pragma unroll
    for (int q = 0; q < 4; ++q) g[q] = (t + q < len) ? (xv[q] > 0.f ? g[q] : g[q] * slope) : 0.f;
  }
  *reinterpret_cast<f32x4*>(gx + i) = g;
}

// master weights [Cout][Cin][K] -> the A-fragment order of conv_mfma32_kernel (pack_conv_weights32, m32 = 1) or of the 16-row
// conv_mfma_kernel (pack_conv_weights, m32 = 0); transposed = the backward-data conv: rows = input channels, columns = output
// channels, taps flipped.  train_repack32_kernel with the 16-row order added.
__global__ void convgrad_repack_kernel(const float* __restrict__ w, int Cout, int Cin, int K, int nsub, int nchunk,
                                       int transposed, int m32, float* __restrict__ packed) {
  const size_t idx = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  const size_t total = (size_t)nsub * nchunk * K * (m32 ? 512 : 256);
  if (idx >= total) return;
  const int e = idx & 3, lane = (idx >> 2) & 63;
  int row, col, j;
  if (m32) {
    const int hf = (idx >> 8) & 1;
    size_t r = idx >> 9;
    j = (int)(r % K);
    r /= K;
    const int c = (int)(r % nchunk), ms = (int)(r / nchunk);
    row = ms * 32 + (lane & 31);
    col = c * KC + 2 * (4 * hf + e) + (lane >> 5);
  } else {
    size_t r = idx >> 8;
    j = (int)(r % K);
    r /= K;
    const int c = (int)(r % nchunk), ms = (int)(r / nchunk);
    row = ms * 16 + (lane & 15);
    col = c * KC + e * 4 + (lane >> 4);
  }
  float v = 0.f;
  if (!transposed) {
    if (row < Cout && col < Cin) v = w[((size_t)row * Cin + col) * K + j];
  } else {
    if (row < Cin && col < Cout) v = w[((size_t)col * Cin + row) * K + (K - 1 - j)];
  }
  packed[idx] = v;
}

template <int NG, int HALO = CG_HALO>
static int cg_launch_wgrad(const WgradArgs& a, const CgPlan& p, hipStream_t st) {
  const size_t lds = ((size_t)32 * CG_LDD + (size_t)32 * p.WCI * cg_lda(HALO)) * sizeof(float);
  static_assert(((size_t)32 * CG_LDD + (size_t)32 * 4 * cg_lda(HALO)) * sizeof(float) <= 80 * 1024, "two workgroups per CU");
  static DeviceOnce attr_once;  // per device (common.h)
  DISSC_HIP_CHECK(attr_once.max_lds(reinterpret_cast<const void*>(&convgrad_wgrad_kernel<NG, HALO>), 80 * 1024));
  hipLaunchKernelGGL((convgrad_wgrad_kernel<NG, HALO>), dim3(p.coT, p.ciS, p.P), dim3(256), lds, st, a);
  return DISSC_OK;
}

void cg_launch_reduce(const float* part, int NP, size_t n, float* out, hipStream_t st) {
  hipLaunchKernelGGL(convgrad_reduce_kernel, dim3((unsigned)((n + 15) / 16)), dim3(256), 0, st, part, NP, n, out);
}

void cg_launch_bias(const float* gy, const int32_t* lengths, int len_mul, int B, int Cout, int Lmax, int ldo, double* bpart,
                    float* gb, hipStream_t st, int len_div) {
  hipLaunchKernelGGL(convgrad_bias_part_kernel, dim3(Cout, B), dim3(256), 0, st, gy, lengths, len_mul, len_div, Cout, Lmax, ldo,
                     bpart);
  hipLaunchKernelGGL(convgrad_bias_reduce_kernel, dim3((Cout + 63) / 64), dim3(64), 0, st, bpart, B, Cout, gb);
}

int cg_check_create(const char* who, const void* out, int Cin, int Cout) {
  if (!out) {
    set_error("%s: bad argument", who);
    return DISSC_EINVAL;
  }
  if (Cin < 1 || Cout < 1 || Cin > 65535 || Cout > 65535) {
    set_error("%s: %d -> %d channels (both must be in 1 .. 65535)", who, Cin, Cout);
    return DISSC_EINVAL;
  }
  return DISSC_OK;
}

int cg_check_call(const CgLayer* h, const char* who, int B, int Lmax, int len_mul, int ldx, int ldo, int len_div) {
  if (!h || B <= 0 || Lmax <= 0 || B > 65535) {
    set_error("%s: bad argument (handle %p, B = %d, Lmax = %d)", who, (void*)h, B, Lmax);
    return DISSC_EINVAL;
  }
  if (len_mul <= 0) return DISSC_OK;  // a host-only query: no rows
  const long long need = ((long long)len_mul * Lmax + len_div - 1) / len_div;  // a row of y / gy
  if (ldx < Lmax || (long long)ldo < need || (ldx & 3) || (ldo & 3)) {
    if (len_div > 1)
      set_error("%s: row strides %d / %d must be multiples of 4 and >= Lmax = %d / ceil(Lmax / %d) = %d", who, ldx, ldo, Lmax,
                len_div, (int)need);
    else
      set_error("%s: row strides %d / %d must be multiples of 4 and >= Lmax = %d / %d x Lmax = %d", who, ldx, ldo, Lmax, len_mul,
                len_mul * Lmax);
    return DISSC_EINVAL;
  }
  if (!h->ready) {  // "dissc_conv[t|s]grad_" of the entry's own name
    set_error("%s: %.*sset_weights first", who, (int)(strrchr(who, '_') + 1 - who), who);
    return DISSC_EINVAL;
  }
  return DISSC_OK;
}

CgWorkspace cg_workspace(const CgPlan& p, int B, int Cout) {
  CgWorkspace w;
  w.bpart = cg_rup((size_t)p.P * p.WT * p.gw * sizeof(float), 256);
  w.bytes = w.bpart + cg_rup((size_t)B * Cout * sizeof(double), 256) + 256;
  return w;
}

int cg_backward_begin(const char* who, const CgPlan& p, int B, int Cout, const float* x, const float* gy, const float* gx,
                      bool wants_wb, void* workspace, size_t workspace_bytes, float** part, double** bpart) {
  if (!x || !gy || ((uintptr_t)x & 15) || ((uintptr_t)gy & 15) || ((uintptr_t)gx & 15)) {
    set_error("%s: x, gy and gx must be 16-byte aligned device pointers", who);
    return DISSC_EINVAL;
  }
  const CgWorkspace w = cg_workspace(p, B, Cout);
  if (wants_wb && (!workspace || workspace_bytes < w.bytes)) {
    set_error("%s: workspace %zu < %zu bytes", who, workspace_bytes, w.bytes);
    return DISSC_ENOMEM;
  }
  *part = (float*)cg_rup((size_t)workspace, 256);
  *bpart = (double*)((char*)*part + w.bpart);
  return DISSC_OK;
}

int cg_alloc_conv(const char* who, int rows, int cols, int taps, int dil, int pad_left, DevConv& dc, int prec) {
  std::vector<float> zeros((size_t)rows * cols * taps, 0.f);
  PrecScope prec_scope(prec);  // 1: the split-bf16 packing where conv_geometry gives the layer one
  if (int rc = make_conv(zeros.data(), nullptr, rows, cols, taps, dil, dc, 1, 1, pad_left)) return rc;
  if (dc.prec > prec || dc.wino || dc.wpack2) {
    set_error("%s: unexpected conv packing", who);
    return DISSC_EINVAL;
  }
  return DISSC_OK;
}

}  // namespace dissc

using namespace dissc;

struct dissc_convgrad : CgLayer {
  int dil = 1;
  int prec = 0;  // 1: split-bf16 in every direction that has an instance (dissc_convgrad_create_prec)
  DevConv fwd, bwd;
  ~dissc_convgrad() {
    free_conv(fwd);
    free_conv(bwd);
  }
};

extern "C" {

static int convgrad_create(const char* who, int max_span, int Cin, int Cout, int k, int dilation, dissc_convgrad_t* out) {
  if (out) *out = nullptr;
  if (int rc = cg_check_create(who, out, Cin, Cout)) return rc;
  if (k < 1 || k % 2 != 1 || k > CG_MAX_K) {
    set_error("%s: kernel size %d (odd, at most %d)", who, k, CG_MAX_K);
    return DISSC_EINVAL;
  }
  if (dilation < 1 || (long long)(k - 1) * dilation > max_span) {
    set_error("%s: (k - 1) x dilation = %d x %d exceeds the tap span %d", who, k - 1, dilation, max_span);
    return DISSC_EINVAL;
  }
  dissc_convgrad* h = new dissc_convgrad();
  h->opt = g_defaults;  // frozen here
  h->Cin = Cin; h->Cout = Cout; h->k = k; h->dil = dilation;
  *out = h;
  return DISSC_OK;
}

int dissc_convgrad_create(int Cin, int Cout, int k, int dilation, dissc_convgrad_t* out) {
  return convgrad_create("dissc_convgrad_create", MAX_TAP_SPAN, Cin, Cout, k, dilation, out);
}

// the same handle with the tap span of a ResBlock2 conv (k = 7, d = 12) admitted: what nn.conv1d creates
int dissc_convgrad_create_wide(int Cin, int Cout, int k, int dilation, dissc_convgrad_t* out) {
  static_assert(RB_TAP_SPAN / 2 <= CG_HALO_WIDE && CG_HALO_WIDE % 4 == 0, "the wide halo covers every admitted tap offset");
  return convgrad_create("dissc_convgrad_create_wide", RB_TAP_SPAN, Cin, Cout, k, dilation, out);
}

int dissc_convgrad_create_prec(int Cin, int Cout, int k, int dilation, int prec, dissc_convgrad_t* out) {
  if (prec != 0 && prec != 1) {
    if (out) *out = nullptr;
    set_error("dissc_convgrad_create_prec: prec %d (0 = fp32, 1 = split-bf16)", prec);
    return DISSC_EINVAL;
  }
  if (int rc = convgrad_create("dissc_convgrad_create_prec", RB_TAP_SPAN, Cin, Cout, k, dilation, out)) return rc;
  (*out)->prec = prec;
  return DISSC_OK;
}

// forward and data gradient: conv_geometry under the handle's precision, the function make_conv packs by and run_conv launches
// by; weight gradient: the test dissc_convgrad_backward dispatches on
int dissc_convgrad_precision_info(dissc_convgrad_t h, int32_t split[3]) {
  if (!h || !split) {
    set_error("dissc_convgrad_precision_info: bad argument");
    return DISSC_EINVAL;
  }
  OptScope opt_scope(&h->opt);
  PrecScope prec_scope(h->prec);
  DevConv f, b;
  conv_geometry(f, h->Cout, h->Cin, h->k, h->dil, 1, 1, -1);
  conv_geometry(b, h->Cin, h->Cout, h->k, h->dil, 1, 1, -1);
  split[0] = f.prec == 1;
  split[1] = b.prec == 1;
  split[2] = cg_wgrad_bf3_takes(h->prec, h->Cin, h->Cout, h->k, h->dil);
  return DISSC_OK;
}

void dissc_convgrad_destroy(dissc_convgrad_t h) { delete h; }

int dissc_convgrad_set_weights(dissc_convgrad_t h, const float* w_dev, const float* bias_dev, void* stream) {
  if (!h || !w_dev) {
    set_error("dissc_convgrad_set_weights: bad argument");
    return DISSC_EINVAL;
  }
  OptScope opt_scope(&h->opt);
  hipStream_t st = (hipStream_t)stream;
  int rc;
  if (!h->ready) {
    if ((rc = cg_alloc_conv("dissc_convgrad_set_weights", h->Cout, h->Cin, h->k, h->dil, -1, h->fwd, h->prec))) return rc;
    if ((rc = cg_alloc_conv("dissc_convgrad_set_weights", h->Cin, h->Cout, h->k, h->dil, -1, h->bwd, h->prec))) return rc;
    h->ready = true;
  }
  for (int tr = 0; tr < 2; ++tr) {
    DevConv& dc = tr ? h->bwd : h->fwd;
    if (dc.prec == 1) {  // split-bf16 fragments (hi | lo), rounded on the device
      cg_launch_repack_bf3(w_dev, h->Cout, h->Cin, h->k, dc.Mpad / 32, dc.nchunk, tr, dc.wpack, st);
      continue;
    }
    const int nsub = dc.Mpad / (dc.m32 ? 32 : 16);
    const size_t n = (size_t)nsub * dc.nchunk * h->k * (dc.m32 ? 512 : 256);
    hipLaunchKernelGGL(convgrad_repack_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, st, w_dev, h->Cout, h->Cin,
                       h->k, nsub, dc.nchunk, tr, dc.m32, dc.wpack);
  }
  if (bias_dev)
    DISSC_HIP_CHECK(hipMemcpyAsync(h->fwd.bias, bias_dev, h->Cout * sizeof(float), hipMemcpyDeviceToDevice, st));
  else
    DISSC_HIP_CHECK(hipMemsetAsync(h->fwd.bias, 0, h->Cout * sizeof(float), st));
  DISSC_HIP_CHECK(hipGetLastError());
  return DISSC_OK;
}

int dissc_convgrad_forward(dissc_convgrad_t h, const float* x, const float* add, float* y, const int32_t* lengths, int B,
                           int ldx, int ldo, int Lmax, float in_slope, void* stream) {
  if (int rc = cg_check_call(h, "dissc_convgrad_forward", B, Lmax, 1, ldx, ldo)) return rc;
  if (!x || !y) {
    set_error("dissc_convgrad_forward: bad argument");
    return DISSC_EINVAL;
  }
  OptScope opt_scope(&h->opt);
  return run_conv(h->fwd, x, y, batch_of(lengths, 1, B, Lmax), epi_of(add ? EPI_RES : EPI_STORE, add), h->Cin, ldx, ldo, in_slope,
                  (hipStream_t)stream);
}

int dissc_convgrad_partials(dissc_convgrad_t h, int B, int Lmax, int* P, int* chunk) {
  if (int rc = cg_check_call(h, "dissc_convgrad_partials", B, Lmax)) return rc;
  const CgPlan p = cg_plan(h->Cin, h->Cout, h->k, B, Lmax);
  if (P) *P = p.P;
  if (chunk) *chunk = p.cpp;
  return DISSC_OK;
}

size_t dissc_convgrad_workspace_bytes(dissc_convgrad_t h, int B, int Lmax) {
  if (!h || B <= 0 || Lmax <= 0) return 0;
  return cg_workspace(cg_plan(h->Cin, h->Cout, h->k, B, Lmax), B, h->Cout).bytes;
}

int dissc_convgrad_backward(dissc_convgrad_t h, const float* x, const float* gy, const int32_t* lengths, int B, int ldx,
                            int ldo, int Lmax, float in_slope, float* gx, float* gw, float* gb, void* workspace,
                            size_t workspace_bytes, void* stream) {
  const char* who = "dissc_convgrad_backward";
  int rc = cg_check_call(h, who, B, Lmax, 1, ldx, ldo);
  if (rc) return rc;
  const CgPlan p = cg_plan(h->Cin, h->Cout, h->k, B, Lmax);
  float* part;
  double* bpart;
  if ((rc = cg_backward_begin(who, p, B, h->Cout, x, gy, gx, gw || gb, workspace, workspace_bytes, &part, &bpart))) return rc;
  OptScope opt_scope(&h->opt);
  hipStream_t st = (hipStream_t)stream;
  if (gw) {
    WgradArgs a;
    a.gy = gy; a.x = x; a.lengths = lengths; a.part = part;
    a.B = B; a.Cout = h->Cout; a.Cin = h->Cin; a.K = h->k; a.Lmax = Lmax; a.ldo = ldo; a.ldx = ldx;
    a.off0 = -((h->k - 1) * h->dil) / 2; a.dstep = h->dil;
    a.halo = (((h->k - 1) * h->dil) / 2 + 3) & ~3;
    a.slope = in_slope;
    a.WCI = p.WCI; a.WT = p.WT; a.CIB = p.CIB; a.TS = p.TS; a.nch = p.nch; a.cpp = p.cpp;
    if (cg_wgrad_bf3_takes(h->prec, h->Cin, h->Cout, h->k, h->dil)) {
      if ((rc = cg_launch_wgrad_bf3(a, p, st))) return rc;
    } else if ((rc = cg_dispatch_ng(p.NG, who, "tap groups", [&](auto ng) {
           return a.halo > CG_HALO ? cg_launch_wgrad<decltype(ng)::value, CG_HALO_WIDE>(a, p, st)
                                   : cg_launch_wgrad<decltype(ng)::value>(a, p, st);
         })))
      return rc;
    cg_launch_reduce(part, p.P * p.WT, p.gw, gw, st);
  }
  if (gb) cg_launch_bias(gy, lengths, 1, B, h->Cout, Lmax, ldo, bpart, gb, st);
  if (gx) {
    // the same conv with W^T, taps flipped: channels swapped, gy read as zero beyond lengths
    if ((rc = run_conv(h->bwd, gy, gx, batch_of(lengths, 1, B, Lmax), EpiSpec(), h->Cout, ldo, ldx, 1.0f, st))) return rc;
    hipLaunchKernelGGL(convgrad_mask_kernel, dim3((ldx / 4 + 127) / 128, h->Cin, B), dim3(128), 0, st, x, lengths, h->Cin, Lmax,
                       ldx, in_slope, gx);
  }
  DISSC_HIP_CHECK(hipGetLastError());
  return DISSC_OK;
}

}  // extern "C"
