// The GAN losses of the vocoder's training step (reference sr/models.py:352-383: feature_loss, discriminator_loss, generator_loss)
// on the PAIRED, ragged, pre-activation maps nn.MultiPeriodDiscriminator produces: a map is [2 R][C][ld], rows 0 .. R - 1 the real
// half, rows R .. 2 R - 1 the generated half, row r and row R + r of length len[r] <= ld.  One forward and one backward entry serve a
// whole list of maps (up to GL_MAX_MAPS; the period side has 30): the per-map records travel by value in the kernels' arguments, as
// wnorm_bwd_kernel's slice does, so nothing is uploaded per step although every pointer changes every step.
//
// Pure streaming: every valid element is read once (forward) or read once and its gradient written once (backward); positions at
// or beyond a row's length are never read for their value.  No atomics, every sum in a fixed order: bit-reproducible from call to
// call, and a map's values and gradients do not depend on the list it is in.  Sums are taken in double (the kernels wait on memory).
#include <limits.h>
#include <math.h>

#include "common.h"

namespace dissc {

constexpr int GL_MAX_MAPS = DISSC_GANLOSS_MAX_MAPS;
constexpr int GL_NT = 256;             // threads of a workgroup
constexpr int GL_UPT = 4;              // float4 units per thread and half: 4 x 2 loads of 16 bytes in flight per thread
constexpr int GL_WG_UNITS = GL_NT * GL_UPT;  // a workgroup's span: 1024 units = 4096 columns of the flattened [R C][ld] half
constexpr int GL_MAX_UNITS = 1 << 30;  // float4 units of one half: unit indices and the 32-bit divisions below stay in range

struct GlMap {      // 48 bytes
  const float* x;   // [2 R][C][ld]
  float* gx;        // backward: the gradient, same layout (null: the map is skipped)
  const int32_t* len;  // [R], on the device
  int R, C, ld4;    // ld4 = ld / 4
  int wg0;          // the map's first workgroup in the launch
  int op;
  float slope;
};

struct GlTable {  // by value: 64 x 48 bytes + 2 ints, inside the 4 KB of kernel arguments
  GlMap m[GL_MAX_MAPS];
  int n, total_wg;
};

// the map a workgroup works for: the last one whose first workgroup is at or before it (wave-uniform: scalar code)
__device__ __forceinline__ int gl_find(const GlTable& t, int wg) {
  int lo = 0, hi = t.n - 1;
  while (lo < hi) {
    const int mid = (lo + hi + 1) >> 1;
    if (t.m[mid].wg0 <= wg) lo = mid; else hi = mid - 1;
  }
  return lo;
}

__device__ __forceinline__ int gl_len(const int32_t* len, int r, int ld) {
  const int n = len[r];
  return n < 0 ? 0 : (n > ld ? ld : n);
}

// where unit u of a map is: its first column t in row `row` of the real half, and that row's length
struct GlAt { size_t off; int t, len; };
__device__ __forceinline__ GlAt gl_at(const GlMap& d, unsigned u) {
  const unsigned row = u / (unsigned)d.ld4, c4 = u - row * (unsigned)d.ld4, r = row / (unsigned)d.C;
  GlAt a;
  a.off = (size_t)u * 4;
  a.t = (int)c4 * 4;
  a.len = gl_len(d.len, (int)r, d.ld4 * 4);
  return a;
}

__device__ __forceinline__ double gl_lrelu(float x, double slope) { return x > 0.f ? (double)x : (double)x * slope; }

// Stage 1: one partial (two doubles) per workgroup.  Thread order: its units u0 + tid, u0 + 256 + tid, ... in order, the four
// elements of a unit in order; then a fixed butterfly over the wave and ((w0 + w1) + (w2 + w3)) over the workgroup.
__global__ void __launch_bounds__(GL_NT) ganloss_fwd_kernel(const GlTable t, double* __restrict__ part) {
  __shared__ double red[8];
  const int wg = blockIdx.x, tid = threadIdx.x;
  const GlMap& d = t.m[gl_find(t, wg)];
  const unsigned U = (unsigned)d.R * (unsigned)d.C * (unsigned)d.ld4;
  const size_t half = (size_t)U * 4;
  const unsigned u0 = (unsigned)(wg - d.wg0) * GL_WG_UNITS + tid;
  const int op = d.op;
  const double slope = (double)d.slope;
  double s0 = 0.0, s1 = 0.0;
  // all of the thread's loads first (eight of 16 bytes in flight), then the sums in unit order
  f32x4 xr[GL_UPT], xg[GL_UPT];
  int rem[GL_UPT];  // valid elements of the unit, 0: not loaded at all
#pragma unroll
  for (int i = 0; i < GL_UPT; ++i) {
    const unsigned u = u0 + i * GL_NT;
    rem[i] = 0;
    xr[i] = xg[i] = f32x4{0.f, 0.f, 0.f, 0.f};
    if (u < U) {
      const GlAt a = gl_at(d, u);
      if (a.t < a.len) {
        rem[i] = a.len - a.t;
        xg[i] = *reinterpret_cast<const f32x4*>(d.x + half + a.off);
        if (op != DISSC_GANLOSS_GEN) xr[i] = *reinterpret_cast<const f32x4*>(d.x + a.off);
      }
    }
  }
#pragma unroll
  for (int i = 0; i < GL_UPT; ++i) {
#pragma unroll
    for (int e = 0; e < 4; ++e) {
      if (e >= rem[i]) break;  // a selection, not a product: a NaN beyond the length adds nothing
      if (op == DISSC_GANLOSS_FM) {
        s0 += fabs(gl_lrelu(xr[i][e], slope) - gl_lrelu(xg[i][e], slope));
      } else if (op == DISSC_GANLOSS_DISC) {
        const double a1 = 1.0 - (double)xr[i][e], g = (double)xg[i][e];
        s0 = fma(a1, a1, s0);
        s1 = fma(g, g, s1);
      } else {
        const double a1 = 1.0 - (double)xg[i][e];
        s0 = fma(a1, a1, s0);
      }
    }
  }
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) {
    s0 += __shfl_xor(s0, off);
    s1 += __shfl_xor(s1, off);
  }
  if ((tid & 63) == 0) {
    red[tid >> 6] = s0;
    red[4 + (tid >> 6)] = s1;
  }
  __syncthreads();
  if (tid == 0) {
    part[2 * (size_t)wg] = (red[0] + red[1]) + (red[2] + red[3]);
    part[2 * (size_t)wg + 1] = (red[4] + red[5]) + (red[6] + red[7]);
  }
}

// sum of a map's row lengths, by one wave: every lane gets it (integers: any order gives the same)
__device__ __forceinline__ long long gl_len_sum(const GlMap& d, int lane) {
  long long s = 0;
  for (int r = lane; r < d.R; r += 64) s += gl_len(d.len, r, d.ld4 * 4);
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) s += __shfl_xor(s, off);
  return s;
}

__device__ __forceinline__ double gl_factor(int op) { return op == DISSC_GANLOSS_FM ? 2.0 : 1.0; }

// Stage 2, one workgroup of 16 waves: wave w takes the maps w, w + 16, ...; lane l sums the map's partials l, l + 64, ... in index
// order, then the fixed butterfly.  vals[m] and vals[n + m] are the map's one or two values, out[0] their sum over the maps in
// index order, from the doubles.  N = C sum len = 0: value 0.
constexpr int GL_NT2 = 1024;
__global__ void __launch_bounds__(GL_NT2) ganloss_fwd2_kernel(const GlTable t, const double* __restrict__ part,
                                                              float* __restrict__ out) {
  __shared__ double val[GL_MAX_MAPS];
  const int tid = threadIdx.x, lane = tid & 63, wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  for (int m = wave; m < t.n; m += GL_NT2 / 64) {
    const GlMap& d = t.m[m];
    const int nwg = (m + 1 < t.n ? t.m[m + 1].wg0 : t.total_wg) - d.wg0;
    const double* p = part + 2 * (size_t)d.wg0;
    double s0 = 0.0, s1 = 0.0;
    for (int i = lane; i < nwg; i += 64) {
      s0 += p[2 * i];
      s1 += p[2 * i + 1];
    }
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) {
      s0 += __shfl_xor(s0, off);
      s1 += __shfl_xor(s1, off);
    }
    const double N = (double)d.C * (double)gl_len_sum(d, lane);
    const double v0 = N > 0.0 ? s0 * gl_factor(d.op) / N : 0.0, v1 = N > 0.0 ? s1 / N : 0.0;
    if (lane == 0) {
      out[1 + m] = (float)v0;
      out[1 + t.n + m] = (float)v1;
      val[m] = v0 + v1;
    }
  }
  __syncthreads();
  if (tid == 0) {
    double s = 0.0;
    for (int m = 0; m < t.n; ++m) s += val[m];
    out[0] = (float)s;
  }
}

// The gradient with respect to the pre-activation maps, both halves, zero at and beyond every length (the whole row is written).
// up0 / up1: the cotangents of the map's two values, g_total + g_vals[m] and g_total + g_vals[n + m]; one rounding per element.
__global__ void __launch_bounds__(GL_NT) ganloss_bwd_kernel(const GlTable t, const float* __restrict__ g_total,
                                                            const float* __restrict__ g_vals) {
  const int wg = blockIdx.x, tid = threadIdx.x;
  const int m = gl_find(t, wg);
  const GlMap& d = t.m[m];
  if (!d.gx) return;
  const unsigned U = (unsigned)d.R * (unsigned)d.C * (unsigned)d.ld4;
  const size_t half = (size_t)U * 4;
  const unsigned u0 = (unsigned)(wg - d.wg0) * GL_WG_UNITS + tid;
  const int op = d.op;
  const double slope = (double)d.slope;
  const double N = (double)d.C * (double)gl_len_sum(d, tid & 63);
  const double gt = g_total ? (double)g_total[0] : 0.0;
  const double k = N > 0.0 ? gl_factor(op) / N : 0.0;
  const double up0 = (gt + (g_vals ? (double)g_vals[m] : 0.0)) * k, up1 = (gt + (g_vals ? (double)g_vals[t.n + m] : 0.0)) * k;
#pragma unroll
  for (int i = 0; i < GL_UPT; ++i) {
    const unsigned u = u0 + i * GL_NT;
    if (u >= U) break;
    const GlAt a = gl_at(d, u);
    f32x4 gr = {0.f, 0.f, 0.f, 0.f}, gg = {0.f, 0.f, 0.f, 0.f};
    if (a.t < a.len) {
      const f32x4 xg = *reinterpret_cast<const f32x4*>(d.x + half + a.off);
      f32x4 xr = {0.f, 0.f, 0.f, 0.f};
      if (op != DISSC_GANLOSS_GEN) xr = *reinterpret_cast<const f32x4*>(d.x + a.off);
#pragma unroll
      for (int e = 0; e < 4; ++e) {
        if (a.t + e >= a.len) break;
        if (op == DISSC_GANLOSS_FM) {  // sign(0) = 0 as torch's abs has it; the leaky ReLU's derivative at 0 is the slope
          const double df = gl_lrelu(xr[e], slope) - gl_lrelu(xg[e], slope);
          const double sg = df > 0.0 ? up0 : (df < 0.0 ? -up0 : 0.0);
          gr[e] = (float)(xr[e] > 0.f ? sg : sg * slope);
          gg[e] = (float)(xg[e] > 0.f ? -sg : -sg * slope);
        } else if (op == DISSC_GANLOSS_DISC) {
          gr[e] = (float)(-2.0 * up0 * (1.0 - (double)xr[e]));
          gg[e] = (float)(2.0 * up1 * (double)xg[e]);
        } else {
          gg[e] = (float)(-2.0 * up0 * (1.0 - (double)xg[e]));
        }
      }
    }
    *reinterpret_cast<f32x4*>(d.gx + a.off) = gr;
    *reinterpret_cast<f32x4*>(d.gx + half + a.off) = gg;
  }
}

}  // namespace dissc

using namespace dissc;

// the refusals every entry shares and the launch table; -> 0, or DISSC_EINVAL with the message set
static int gl_table(const char* who, int n, const int* R, const int* C, const int* ld, GlTable* t) {
  if (n < 1 || n > GL_MAX_MAPS || !R || !C || !ld) {
    set_error("%s: %d maps (1 .. %d), or no R / C / ld arrays", who, n, GL_MAX_MAPS);
    return DISSC_EINVAL;
  }
  long long wg = 0;
  for (int i = 0; i < n; ++i) {
    if (R[i] < 1 || C[i] < 1 || ld[i] < 4 || (ld[i] & 3)) {
      set_error("%s: map %d is R %d, C %d, ld %d: R and C at least 1, ld a positive multiple of 4", who, i, R[i], C[i], ld[i]);
      return DISSC_EINVAL;
    }
    const long long units = (long long)R[i] * C[i] * (ld[i] / 4);
    if ((long long)R[i] * C[i] > INT_MAX || units > GL_MAX_UNITS) {
      set_error("%s: map %d has more than 2^30 float4s per half", who, i);
      return DISSC_EINVAL;
    }
    if (t) {
      t->m[i].R = R[i];
      t->m[i].C = C[i];
      t->m[i].ld4 = ld[i] / 4;
      t->m[i].wg0 = (int)wg;
    }
    wg += (units + GL_WG_UNITS - 1) / GL_WG_UNITS;
    if (wg > INT_MAX / 2) {
      set_error("%s: more workgroups than one launch takes (at map %d)", who, i);
      return DISSC_EINVAL;
    }
  }
  if (t) {
    t->n = n;
    t->total_wg = (int)wg;
    for (int i = n; i < GL_MAX_MAPS; ++i) t->m[i] = GlMap{nullptr, nullptr, nullptr, 0, 0, 0, INT_MAX, 0, 1.f};
  }
  return DISSC_OK;
}

static size_t gl_workspace(int total_wg) { return ((size_t)total_wg * 2 * sizeof(double) + 255) & ~(size_t)255; }

static int gl_fill(const char* who, GlTable* t, const float* const* maps, const int32_t* const* lengths, const int* ops,
                   const float* slopes) {
  if (!maps || !lengths || !ops || !slopes) {
    set_error("%s: null maps / lengths / ops / slopes array", who);
    return DISSC_EINVAL;
  }
  for (int i = 0; i < t->n; ++i) {
    if (!maps[i] || ((uintptr_t)maps[i] & 15) || !lengths[i]) {
      set_error("%s: map %d: null or not 16-byte aligned, or no lengths", who, i);
      return DISSC_EINVAL;
    }
    if (ops[i] < DISSC_GANLOSS_FM || ops[i] > DISSC_GANLOSS_GEN || !isfinite(slopes[i])) {
      set_error("%s: map %d: op %d outside 0 .. 2 (FM, DISC, GEN) or a slope that is not finite", who, i, ops[i]);
      return DISSC_EINVAL;
    }
    t->m[i].x = maps[i];
    t->m[i].gx = nullptr;
    t->m[i].len = lengths[i];
    t->m[i].op = ops[i];
    t->m[i].slope = slopes[i];
  }
  return DISSC_OK;
}

extern "C" {

size_t dissc_ganloss_workspace_bytes(int n, const int* R, const int* C, const int* ld) {
  GlTable t;
  if (gl_table("dissc_ganloss_workspace_bytes", n, R, C, ld, &t)) return 0;
  return gl_workspace(t.total_wg);
}

int dissc_ganloss_forward(int n, const float* const* maps, const int32_t* const* lengths, const int* R, const int* C,
                          const int* ld, const int* ops, const float* slopes, float* out, void* workspace, size_t workspace_bytes,
                          void* stream) {
  const char* who = "dissc_ganloss_forward";
  GlTable t;
  if (int rc = gl_table(who, n, R, C, ld, &t)) return rc;
  if (int rc = gl_fill(who, &t, maps, lengths, ops, slopes)) return rc;
  if (!out || !workspace || ((uintptr_t)workspace & 7) || workspace_bytes < gl_workspace(t.total_wg)) {
    set_error("%s: no out, or a workspace that is null, not 8-byte aligned or below %zu bytes", who, gl_workspace(t.total_wg));
    return DISSC_EINVAL;
  }
  hipLaunchKernelGGL(ganloss_fwd_kernel, dim3(t.total_wg), dim3(GL_NT), 0, (hipStream_t)stream, t, (double*)workspace);
  hipLaunchKernelGGL(ganloss_fwd2_kernel, dim3(1), dim3(GL_NT2), 0, (hipStream_t)stream, t, (const double*)workspace, out);
  DISSC_HIP_CHECK(hipGetLastError());
  return DISSC_OK;
}

int dissc_ganloss_backward(int n, const float* const* maps, const int32_t* const* lengths, const int* R, const int* C,
                           const int* ld, const int* ops, const float* slopes, const float* g_total, const float* g_vals,
                           float* const* gmaps, void* stream) {
  const char* who = "dissc_ganloss_backward";
  GlTable t;
  if (int rc = gl_table(who, n, R, C, ld, &t)) return rc;
  if (int rc = gl_fill(who, &t, maps, lengths, ops, slopes)) return rc;
  if (!gmaps || (!g_total && !g_vals)) {
    set_error("%s: no gmaps array, or neither g_total nor g_vals", who);
    return DISSC_EINVAL;
  }
  for (int i = 0; i < n; ++i) {
    if ((uintptr_t)gmaps[i] & 15) {
      set_error("%s: the gradient of map %d is not 16-byte aligned", who, i);
      return DISSC_EINVAL;
    }
    t.m[i].gx = gmaps[i];
  }
  hipLaunchKernelGGL(ganloss_bwd_kernel, dim3(t.total_wg), dim3(GL_NT), 0, (hipStream_t)stream, t, g_total, g_vals);
  DISSC_HIP_CHECK(hipGetLastError());
  return DISSC_OK;
}

}  // extern "C"
