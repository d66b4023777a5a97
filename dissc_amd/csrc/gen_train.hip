// What the generator's training step needs around the two MFMA gradient layers (conv_grad.hip, conv_grad_t.hip): weight norm of
// every layer in one launch per direction, the embeddings' forward on device tables and their dense gradient, the MRF mean,
// the tanh tail.  All bandwidth bound; no atomics, every sum in a fixed order: bit-reproducible from call to call.
#include <limits.h>

#include <algorithm>

#include "common.h"

namespace dissc {

// ---- weight norm: w = g v / ||v|| per row (index of dim 0), reference sr/models.py wraps all 97 convs in weight_norm(dim=0) ----
constexpr int WN_WAVE_COLS = 512;  // rows of up to this many columns: one wave each (two float4 sweeps); longer: one workgroup
constexpr int WN_SLICE = 128;      // tensors per launch: their gradient pointers travel by value in the kernel's arguments
constexpr long long WN_MAX_ROWS = 1ll << 22, WN_MAX_FLOATS = 1ll << 40;

struct WnRow {
  long long off;   // the row's first float in the flat layout
  long long toff;  // the same inside its own tensor (where the layer's own gw starts the row)
  int cols, slot;  // slot: tensor index inside its slice
  int grow, pad;   // index in the flat per-row layout (g, gg, 1 / ||v||)
};

struct WnSlice {  // by value, 3 KB
  const float* gw[WN_SLICE];
  const float* gb[WN_SLICE];
  int boff[WN_SLICE], nb[WN_SLICE];  // where the tensor's bias gradient goes in the flat one, and how long it is
};

// A row starts anywhere (its tensor starts 16-byte aligned, the row at r * cols floats into it): up to 3 scalar elements up to
// the next 16-byte boundary, float4s, up to 3 scalar elements.  The split depends on (cols, off mod 4) alone.
struct WnSpan { int head, nbody, tail; };
__device__ __forceinline__ WnSpan wn_span(long long off, int cols) {
  WnSpan s;
  s.head = min(cols, (4 - (int)(off & 3)) & 3);
  s.nbody = (cols - s.head) >> 2;
  s.tail = cols - s.head - 4 * s.nbody;
  return s;
}

// The row's sums  aa = sum a[j]^2  and (TWO)  ab = sum a[j] b[j]  in DOUBLE (the products of two floats are then exact, and the
// kernel stays bandwidth bound): every thread one chain over its own elements (head, its float4s in order, tail), then a fixed
// butterfly over the wave and, for a workgroup, ((w0 + w1) + (w2 + w3)) over the four waves.  Every thread gets the sums.
template <int NT, bool TWO>
__device__ __forceinline__ void wn_sums(const float* __restrict__ a, const float* __restrict__ b, const WnSpan sp, int tid,
                                        double* red, double& aa, double& ab) {
  double saa = 0.0, sab = 0.0;
  const f32x4* a4 = reinterpret_cast<const f32x4*>(a + sp.head);
  const f32x4* b4 = reinterpret_cast<const f32x4*>(b + sp.head);
  if (tid < sp.head) {
    saa = (double)a[tid] * a[tid];
    if (TWO) sab = (double)a[tid] * b[tid];
  }
  for (int c = tid; c < sp.nbody; c += NT) {
    const f32x4 x = a4[c];
#pragma unroll
    for (int e = 0; e < 4; ++e) saa = fma((double)x[e], (double)x[e], saa);
    if (TWO) {
      const f32x4 y = b4[c];
#pragma unroll
      for (int e = 0; e < 4; ++e) sab = fma((double)x[e], (double)y[e], sab);
    }
  }
  if (tid < sp.tail) {
    const int j = sp.head + 4 * sp.nbody + tid;
    saa = fma((double)a[j], (double)a[j], saa);
    if (TWO) sab = fma((double)a[j], (double)b[j], sab);
  }
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) {
    saa += __shfl_xor(saa, off);
    if (TWO) sab += __shfl_xor(sab, off);
  }
  if (NT > 64) {
    if ((tid & 63) == 0) {
      red[tid >> 6] = saa;
      red[4 + (tid >> 6)] = sab;
    }
    __syncthreads();
    saa = (red[0] + red[1]) + (red[2] + red[3]);
    sab = (red[4] + red[5]) + (red[6] + red[7]);
  }
  aa = saa;
  ab = sab;
}

template <int NT>
__device__ __forceinline__ void wn_fwd_row(const WnRow r, const float* __restrict__ v, const float* __restrict__ g,
                                           float* __restrict__ w, float* __restrict__ inv_norm, int tid, double* red) {
  const WnSpan sp = wn_span(r.off, r.cols);
  const float* vr = v + r.off;
  float* wr = w + r.off;
  double ss, unused;
  wn_sums<NT, false>(vr, vr, sp, tid, red, ss, unused);
  const double norm = sqrt(ss);
  const double sc = (double)g[r.grow] / norm;  // w = v (g / ||v||), one rounding per element
  if (tid == 0) inv_norm[r.grow] = (float)(1.0 / norm);
  if (tid < sp.head) wr[tid] = (float)(vr[tid] * sc);
  const f32x4* v4 = reinterpret_cast<const f32x4*>(vr + sp.head);
  f32x4* w4 = reinterpret_cast<f32x4*>(wr + sp.head);
  for (int c = tid; c < sp.nbody; c += NT) {
    const f32x4 x = v4[c];
    f32x4 o;
#pragma unroll
    for (int e = 0; e < 4; ++e) o[e] = (float)(x[e] * sc);
    w4[c] = o;
  }
  if (tid < sp.tail) {
    const int j = sp.head + 4 * sp.nbody + tid;
    wr[j] = (float)(vr[j] * sc);
  }
}

// grid: ceil(n_wave / 4) workgroups of four one-wave rows, n_block one-workgroup rows, then ceil(nbias / 256) that copy the
// flat bias next to the weights
__global__ void __launch_bounds__(256) wnorm_fwd_kernel(const WnRow* __restrict__ tab, int n_wave, int n_block,
                                                        const float* __restrict__ v, const float* __restrict__ g,
                                                        float* __restrict__ w, float* __restrict__ inv_norm,
                                                        const float* __restrict__ bias, float* __restrict__ bias_out, int nbias) {
  __shared__ double red[8];
  const int nwb = (n_wave + 3) >> 2, bid = blockIdx.x, tid = threadIdx.x;
  if (bid < nwb) {
    const int r = bid * 4 + (tid >> 6);
    if (r < n_wave) wn_fwd_row<64>(tab[r], v, g, w, inv_norm, tid & 63, red);
  } else if (bid < nwb + n_block) {
    wn_fwd_row<256>(tab[n_wave + bid - nwb], v, g, w, inv_norm, tid, red);
  } else {
    const int i = (bid - nwb - n_block) * 256 + tid;
    if (i < nbias) bias_out[i] = bias[i];
  }
}

// gg = (v . gw) / ||v||,  gv = (g / ||v||) (gw - v (v . gw) / ||v||^2); a null gw: exact zeros.  ||v||^2 is summed again, in
// double and in the pass that reads v for the dot product anyway: the difference gw - v (v . gw) / ||v||^2 cancels (entirely,
// for a row of one column), and a norm rounded to fp32 in between would leave its rounding error there.
template <int NT>
__device__ __forceinline__ void wn_bwd_row(const WnRow r, const float* __restrict__ v, const float* __restrict__ g,
                                           const float* __restrict__ gw, float* __restrict__ gv, float* __restrict__ gg, int tid,
                                           double* red) {
  const WnSpan sp = wn_span(r.off, r.cols);
  const float* vr = v + r.off;
  float* gr = gv + r.off;
  const int j_tail = sp.head + 4 * sp.nbody + tid;
  f32x4* g4 = reinterpret_cast<f32x4*>(gr + sp.head);
  if (!gw) {
    if (tid == 0) gg[r.grow] = 0.f;
    if (tid < sp.head) gr[tid] = 0.f;
    for (int c = tid; c < sp.nbody; c += NT) g4[c] = f32x4{0.f, 0.f, 0.f, 0.f};
    if (tid < sp.tail) gr[j_tail] = 0.f;
    return;
  }
  const float* wr = gw + r.toff;  // r.toff = r.off mod 4: the same split
  double ss, dot;
  wn_sums<NT, true>(vr, wr, sp, tid, red, ss, dot);
  const double inv = 1.0 / sqrt(ss);
  const double gs = (double)g[r.grow] * inv, k = dot * inv * inv;
  if (tid == 0) gg[r.grow] = (float)(dot * inv);
  if (tid < sp.head) gr[tid] = (float)(gs * fma(-(double)vr[tid], k, (double)wr[tid]));
  const f32x4* v4 = reinterpret_cast<const f32x4*>(vr + sp.head);
  const f32x4* w4 = reinterpret_cast<const f32x4*>(wr + sp.head);
  for (int c = tid; c < sp.nbody; c += NT) {
    const f32x4 x = v4[c], y = w4[c];
    f32x4 o;
#pragma unroll
    for (int e = 0; e < 4; ++e) o[e] = (float)(gs * fma(-(double)x[e], k, (double)y[e]));
    g4[c] = o;
  }
  if (tid < sp.tail) gr[j_tail] = (float)(gs * fma(-(double)vr[j_tail], k, (double)wr[j_tail]));
}

// grid: as the forward's, then one workgroup per tensor of the slice that gathers its bias gradient (null: zeros)
__global__ void __launch_bounds__(256) wnorm_bwd_kernel(const WnRow* __restrict__ tab, int n_wave, int n_block,
                                                        const float* __restrict__ v, const float* __restrict__ g,
                                                        float* __restrict__ gv, float* __restrict__ gg,
                                                        float* __restrict__ gb_flat, const WnSlice sl) {
  __shared__ double red[8];
  const int nwb = (n_wave + 3) >> 2, bid = blockIdx.x, tid = threadIdx.x;
  if (bid < nwb) {
    const int r = bid * 4 + (tid >> 6);
    if (r < n_wave) {
      const WnRow row = tab[r];
      wn_bwd_row<64>(row, v, g, sl.gw[row.slot], gv, gg, tid & 63, red);
    }
  } else if (bid < nwb + n_block) {
    const WnRow row = tab[n_wave + bid - nwb];
    wn_bwd_row<256>(row, v, g, sl.gw[row.slot], gv, gg, tid, red);
  } else {
    const int s = bid - nwb - n_block;
    const float* src = sl.gb[s];
    float* dst = gb_flat + sl.boff[s];
    for (int i = tid; i < sl.nb[s]; i += 256) dst[i] = src ? src[i] : 0.f;
  }
}

// ---- embeddings' gradient: dense, one workgroup per table row, dictionary rows first ----
// A dictionary row: wave w scans the positions [w Q, (w + 1) Q) of the B T list, Q = ceil(B T / 4), in order (64 ids per load, the
// matches by ballot), lane l keeps the sums of channels l, l + 64, ...; then ((w0 + w1) + (w2 + w3)).  A speaker row: wave w takes the
// channels c = w (mod 4); per channel the lanes sum t = l, l + 64, ... of every matching utterance in order, then a fixed butterfly.
// Both orders are functions of (B, T) alone: a position at or beyond lengths[b], or of another id, adds nothing.
constexpr int EMB_MAX_E = 256;
__global__ void __launch_bounds__(256) embed_concat_bwd_kernel(const float* __restrict__ gx, const int64_t* __restrict__ code,
                                                               const int64_t* __restrict__ spkr,
                                                               const int32_t* __restrict__ lengths, int B, int T, int E, int has_f0,
                                                               int n_codes, int n_spk, int C, int ldx, float* __restrict__ g_dict,
                                                               float* __restrict__ g_spkr) {
  __shared__ float red[4][EMB_MAX_E];
  const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63;
  if ((int)blockIdx.x < n_codes) {
    const int id = blockIdx.x;
    float acc[EMB_MAX_E / 64] = {0.f, 0.f, 0.f, 0.f};
    const int N = B * T, Q = (N + 3) >> 2;
    const int p1 = min(N, (wave + 1) * Q);
    for (int p0 = wave * Q; p0 < p1; p0 += 64) {  // 64 positions' ids at once; the matches are then taken in ascending order
      const int p = p0 + lane;
      bool hit = false;
      if (p < p1) {
        const int b = p / T, t = p - b * T;
        long long c = code[p];
        c = c < 0 ? 0 : (c >= n_codes ? n_codes - 1 : c);  // as the forward clamps
        hit = t < (lengths ? lengths[b] : T) && c == id;
      }
      unsigned long long hits = __ballot(hit);
      while (hits) {
        const int q = p0 + __ffsll((long long)hits) - 1;
        hits &= hits - 1;
        const int b = q / T, t = q - b * T;
        const float* src = gx + (size_t)b * C * ldx + t;
#pragma unroll
        for (int i = 0; i < EMB_MAX_E / 64; ++i)
          if (lane + 64 * i < E) acc[i] += src[(size_t)(lane + 64 * i) * ldx];
      }
    }
#pragma unroll
    for (int i = 0; i < EMB_MAX_E / 64; ++i) red[wave][lane + 64 * i] = acc[i];
    __syncthreads();
    for (int c = tid; c < E; c += 256) g_dict[(size_t)id * E + c] = (red[0][c] + red[1][c]) + (red[2][c] + red[3][c]);
    return;
  }
  const int id = blockIdx.x - n_codes;
  const int c0 = E + (has_f0 ? 1 : 0);
  for (int c = wave; c < E; c += 4) {
    float s = 0.f;
    for (int b0 = 0; b0 < B; b0 += 64) {  // 64 utterances' speakers at once; the matches in ascending order
      bool hit = false;
      if (b0 + lane < B) {
        long long sp = spkr[b0 + lane];
        sp = sp < 0 ? 0 : (sp >= n_spk ? n_spk - 1 : sp);
        hit = sp == id;
      }
      unsigned long long hits = __ballot(hit);
      while (hits) {
        const int b = b0 + __ffsll((long long)hits) - 1;
        hits &= hits - 1;
        const int len = min(lengths ? lengths[b] : T, T);
        const float* src = gx + ((size_t)b * C + c0 + c) * ldx;
        for (int t = lane; t < len; t += 64) s += src[t];
      }
    }
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) s += __shfl_xor(s, off);
    if (lane == 0) g_spkr[(size_t)id * E + c] = s;
  }
}

// ---- ragged element-wise kernels on [B][C][ld] rows, four positions per thread; grid (ceil(ld / 1024), C, B) ----
struct MrfPtrs { const float* p[DISSC_MAX_RK]; };

__device__ __forceinline__ int row_len(const int32_t* lengths, int b, int L) {
  const int n = lengths ? lengths[b] : L;
  return n < 0 ? 0 : (n > L ? L : n);
}

// y = ((r0 + r1) + r2) / nk, the reference's order and a true division (ragged_epi.h's epi_mrf); nothing written beyond lengths
__global__ void __launch_bounds__(256) mrf_mean_fwd_kernel(const MrfPtrs r, int nk, float* __restrict__ y,
                                                           const int32_t* __restrict__ lengths, int C, int ld, int L) {
  const int b = blockIdx.z, t = 4 * (blockIdx.x * 256 + threadIdx.x);
  const int len = row_len(lengths, b, L);
  if (t >= len) return;
  const size_t at = ((size_t)b * C + blockIdx.y) * ld + t;
  f32x4 a = *reinterpret_cast<const f32x4*>(r.p[0] + at);
  for (int j = 1; j < nk; ++j) {
    const f32x4 x = *reinterpret_cast<const f32x4*>(r.p[j] + at);
    a[0] += x[0]; a[1] += x[1]; a[2] += x[2]; a[3] += x[3];
  }
  const float d = (float)nk;
#pragma unroll
  for (int e = 0; e < 4; ++e) a[e] = __fdiv_rn(a[e], d);
  if (t + 4 <= len) {
    *reinterpret_cast<f32x4*>(y + at) = a;
  } else {
    for (int e = 0; t + e < len; ++e) y[at + e] = a[e];
  }
}

// gx = g / nk inside lengths, zero from there to ld: written once, every branch reads the same tensor
__global__ void __launch_bounds__(256) mrf_mean_bwd_kernel(const float* __restrict__ g, int nk, float* __restrict__ gx,
                                                           const int32_t* __restrict__ lengths, int C, int ld, int L) {
  const int b = blockIdx.z, t = 4 * (blockIdx.x * 256 + threadIdx.x);
  if (t >= ld) return;
  const int len = row_len(lengths, b, L);
  const size_t at = ((size_t)b * C + blockIdx.y) * ld + t;
  f32x4 a = {0.f, 0.f, 0.f, 0.f};
  if (t < len) {
    a = *reinterpret_cast<const f32x4*>(g + at);
    const float d = (float)nk;
#pragma unroll
    for (int e = 0; e < 4; ++e) a[e] = (t + e < len) ? __fdiv_rn(a[e], d) : 0.f;
  }
  *reinterpret_cast<f32x4*>(gx + at) = a;
}

// y = tanh(x) inside lengths (nothing written beyond); rows of x and y may have different strides (the wav has hop T columns)
__global__ void __launch_bounds__(256) tanh_fwd_kernel(const float* __restrict__ x, float* __restrict__ y,
                                                       const int32_t* __restrict__ lengths, int C, int ldx, int ldy, int L) {
  const int b = blockIdx.z, t = 4 * (blockIdx.x * 256 + threadIdx.x);
  const int len = row_len(lengths, b, L);
  const float* xr = x + ((size_t)b * C + blockIdx.y) * ldx;
  float* yr = y + ((size_t)b * C + blockIdx.y) * ldy;
  for (int e = 0; e < 4 && t + e < len; ++e) yr[t + e] = tanhf(xr[t + e]);
}

// gx = gy (1 - y^2) from the saved output inside lengths, zero from there to ldx
__global__ void __launch_bounds__(256) tanh_bwd_kernel(const float* __restrict__ y, const float* __restrict__ gy,
                                                       float* __restrict__ gx, const int32_t* __restrict__ lengths, int C, int ldx,
                                                       int ldy, int L) {
  const int b = blockIdx.z, t = 4 * (blockIdx.x * 256 + threadIdx.x);
  const int len = row_len(lengths, b, L);
  const float* yr = y + ((size_t)b * C + blockIdx.y) * ldy;
  const float* gr = gy + ((size_t)b * C + blockIdx.y) * ldy;
  float* xr = gx + ((size_t)b * C + blockIdx.y) * ldx;
  for (int e = 0; e < 4 && t + e < ldx; ++e) {
    float o = 0.f;
    if (t + e < len) {
      const float v = yr[t + e];
      o = gr[t + e] * fmaf(-v, v, 1.f);
    }
    xr[t + e] = o;
  }
}

}  // namespace dissc

using namespace dissc;

struct dissc_wnorm {
  int n = 0;
  std::vector<int> rows, cols;
  std::vector<long long> off, row_off;  // per tensor: first float in the flat layout, first row in the per-row layout
  long long total = 0, total_rows = 0;
  std::vector<WnRow> table;            // slice-major; inside a slice the one-wave rows first, then the one-workgroup rows
  std::vector<int> s_base, s_wave, s_block;  // per slice: first record, one-wave rows, one-workgroup rows
  WnRow* d_table = nullptr;
  int dev = -1;
};

static int wn_upload(dissc_wnorm* h) {
  int dev = 0;
  DISSC_HIP_CHECK(hipGetDevice(&dev));
  if (h->d_table) {
    if (dev != h->dev) {
      set_error("dissc_wnorm: the handle's row table is on device %d, the current device is %d (a handle serves one device)",
                h->dev, dev);
      return DISSC_EINVAL;
    }
    return DISSC_OK;
  }
  DISSC_HIP_CHECK(hipMalloc((void**)&h->d_table, h->table.size() * sizeof(WnRow)));
  DISSC_HIP_CHECK(hipMemcpy(h->d_table, h->table.data(), h->table.size() * sizeof(WnRow), hipMemcpyHostToDevice));
  h->dev = dev;
  return DISSC_OK;
}

static bool aligned16(const void* p) { return ((uintptr_t)p & 15) == 0; }

extern "C" {

int dissc_wnorm_wave_cols(void) { return WN_WAVE_COLS; }

int dissc_wnorm_create(int n, const int* rows, const int* cols, dissc_wnorm_t* out) {
  if (out) *out = nullptr;
  if (!out || !rows || !cols || n < 1) {
    set_error("dissc_wnorm_create: need n >= 1 tensors, their rows and cols, and a place for the handle");
    return DISSC_EINVAL;
  }
  long long total = 0, total_rows = 0;
  for (int i = 0; i < n; ++i) {
    if (rows[i] < 1 || cols[i] < 1) {
      set_error("dissc_wnorm_create: tensor %d is %d x %d; rows and cols must be at least 1", i, rows[i], cols[i]);
      return DISSC_EINVAL;
    }
    total_rows += rows[i];
    total = ((total + 3) & ~3ll) + (long long)rows[i] * cols[i];  // < 2^62 + 2^40: no overflow before the test below
    if (total_rows > WN_MAX_ROWS || total > WN_MAX_FLOATS) {
      set_error("dissc_wnorm_create: more than %lld rows or %lld floats in all (at tensor %d)", WN_MAX_ROWS, WN_MAX_FLOATS, i);
      return DISSC_EINVAL;
    }
  }
  dissc_wnorm* h = new dissc_wnorm();
  h->n = n;
  h->rows.assign(rows, rows + n);
  h->cols.assign(cols, cols + n);
  h->off.resize(n);
  h->row_off.resize(n);
  long long at = 0, rat = 0;
  for (int i = 0; i < n; ++i) {
    at = (at + 3) & ~3ll;
    h->off[i] = at;
    h->row_off[i] = rat;
    at += (long long)rows[i] * cols[i];
    rat += rows[i];
  }
  h->total = (at + 3) & ~3ll;
  h->total_rows = rat;
  h->table.reserve((size_t)rat);
  for (int s0 = 0; s0 < n; s0 += WN_SLICE) {
    const int s1 = std::min(n, s0 + WN_SLICE);
    h->s_base.push_back((int)h->table.size());
    for (int pass = 0; pass < 2; ++pass) {
      const size_t before = h->table.size();
      for (int i = s0; i < s1; ++i) {
        if ((cols[i] > WN_WAVE_COLS) != (pass == 1)) continue;
        for (int r = 0; r < rows[i]; ++r) {
          WnRow w;
          w.toff = (long long)r * cols[i];
          w.off = h->off[i] + w.toff;
          w.cols = cols[i];
          w.slot = i - s0;
          w.grow = (int)(h->row_off[i] + r);
          w.pad = 0;
          h->table.push_back(w);
        }
      }
      (pass == 0 ? h->s_wave : h->s_block).push_back((int)(h->table.size() - before));
    }
  }
  *out = h;
  return DISSC_OK;
}

void dissc_wnorm_destroy(dissc_wnorm_t h) {
  if (!h) return;
  if (h->d_table) (void)hipFree(h->d_table);
  delete h;
}

int dissc_wnorm_offsets(dissc_wnorm_t h, long long* off, long long* row_off, long long* total_floats, long long* total_rows) {
  if (!h) {
    set_error("dissc_wnorm_offsets: null handle");
    return DISSC_EINVAL;
  }
  for (int i = 0; i < h->n; ++i) {
    if (off) off[i] = h->off[i];
    if (row_off) row_off[i] = h->row_off[i];
  }
  if (total_floats) *total_floats = h->total;
  if (total_rows) *total_rows = h->total_rows;
  return DISSC_OK;
}

int dissc_wnorm_forward(dissc_wnorm_t h, const float* v_flat, const float* g_flat, float* w_flat, float* inv_norm,
                        const float* bias_flat, float* bias_out, int nbias, void* stream) {
  if (!h || !v_flat || !g_flat || !w_flat || !inv_norm || !aligned16(v_flat) || !aligned16(w_flat) || nbias < 0 ||
      (nbias > 0 && (!bias_flat || !bias_out))) {
    set_error("dissc_wnorm_forward: null handle or pointer, v_flat / w_flat not 16-byte aligned, or a bias count without its pointers");
    return DISSC_EINVAL;
  }
  if (int rc = wn_upload(h)) return rc;
  for (size_t s = 0; s < h->s_base.size(); ++s) {
    const int nb = s == 0 ? nbias : 0;
    const unsigned grid = (unsigned)((h->s_wave[s] + 3) / 4 + h->s_block[s] + (nb + 255) / 256);
    hipLaunchKernelGGL(wnorm_fwd_kernel, dim3(grid), dim3(256), 0, (hipStream_t)stream, h->d_table + h->s_base[s], h->s_wave[s],
                       h->s_block[s], v_flat, g_flat, w_flat, inv_norm, bias_flat, bias_out, nb);
  }
  DISSC_HIP_CHECK(hipGetLastError());
  return DISSC_OK;
}

int dissc_wnorm_backward(dissc_wnorm_t h, const float* v_flat, const float* g_flat, const float* const* gw_ptrs, float* gv_flat, float* gg_flat, const float* const* gb_ptrs,
                         const int* bias_n, float* gb_flat, void* stream) {
  if (!h || !v_flat || !g_flat || !gw_ptrs || !gv_flat || !gg_flat || !aligned16(v_flat) || !aligned16(gv_flat) ||
      (gb_ptrs && (!bias_n || !gb_flat))) {
    set_error("dissc_wnorm_backward: null handle or pointer, v_flat / gv_flat not 16-byte aligned, or gb_ptrs without bias_n and gb_flat");
    return DISSC_EINVAL;
  }
  long long btot = 0;
  for (int i = 0; i < h->n; ++i) {
    if (!aligned16(gw_ptrs[i])) {
      set_error("dissc_wnorm_backward: the gradient of tensor %d is not 16-byte aligned", i);
      return DISSC_EINVAL;
    }
    if (gb_ptrs) {
      if (bias_n[i] < 0 || (btot += bias_n[i] + 3ll) > INT_MAX) {
        set_error("dissc_wnorm_backward: bias_n[%d] = %d is negative or the biases' total leaves the int range", i, bias_n[i]);
        return DISSC_EINVAL;
      }
    }
  }
  if (int rc = wn_upload(h)) return rc;
  int boff = 0;
  for (size_t s = 0; s < h->s_base.size(); ++s) {
    const int t0 = (int)s * WN_SLICE, nt = std::min(h->n - t0, WN_SLICE);
    WnSlice sl;
    for (int i = 0; i < WN_SLICE; ++i) {
      sl.gw[i] = i < nt ? gw_ptrs[t0 + i] : nullptr;
      sl.gb[i] = (i < nt && gb_ptrs) ? gb_ptrs[t0 + i] : nullptr;
      sl.nb[i] = (i < nt && gb_ptrs) ? bias_n[t0 + i] : 0;
      boff = (boff + 3) & ~3;  // every bias 16-byte aligned in the flat layout, as the weights are
      sl.boff[i] = boff;
      boff += sl.nb[i];
    }
    const unsigned grid = (unsigned)((h->s_wave[s] + 3) / 4 + h->s_block[s] + (gb_ptrs ? nt : 0));
    hipLaunchKernelGGL(wnorm_bwd_kernel, dim3(grid), dim3(256), 0, (hipStream_t)stream, h->d_table + h->s_base[s], h->s_wave[s],
                       h->s_block[s], v_flat, g_flat, gv_flat, gg_flat, gb_flat, sl);
  }
  DISSC_HIP_CHECK(hipGetLastError());
  return DISSC_OK;
}

static int embed_args_bad(const char* who, const void* x, const int64_t* code, const float* f0, const int64_t* spkr, const void* dict_w,
                          const void* spkr_w, int B, int T, int E, int n_codes, int n_spk, int ldx, bool bwd) {
  (void)f0;
  if (!x || !code || !dict_w || (spkr && !spkr_w)) {
    set_error("%s: null pointer (the activations, the ids and the dictionary are needed; a speaker table with speaker ids)", who);
    return 1;
  }
  if (B < 1 || T < 1 || E < 1 || n_codes < 1 || (spkr && n_spk < 1) || ldx < T || (long long)B * T > INT_MAX) {
    set_error("%s: B %d, T %d, E %d, n_codes %d, n_spk %d, ldx %d: all must be at least 1, ldx >= T, B T within int", who, B, T, E,
              n_codes, n_spk, ldx);
    return 1;
  }
  if (B > 65535 || 2 * (long long)E + 1 > 65535) {
    set_error("%s: B %d or E %d beyond the grid's 65535", who, B, E);
    return 1;
  }
  if (bwd && E > EMB_MAX_E) {
    set_error("%s: embedding_dim %d: the gradient kernel keeps %d channel sums per wave at most", who, E, EMB_MAX_E);
    return 1;
  }
  return 0;
}

int dissc_embed_concat_fwd(const int64_t* code, const float* f0, const int64_t* spkr, const float* dict_w, const float* spkr_w,
                           const int32_t* lengths, int B, int T, int E, int n_codes, int n_spk, float* x, int ldx, void* stream) {
  if (embed_args_bad("dissc_embed_concat_fwd", x, code, f0, spkr, dict_w, spkr_w, B, T, E, n_codes, n_spk, ldx, false))
    return DISSC_EINVAL;
  ZeroSpans zs;
  zs.n = 0;
  launch_embed_concat(code, f0, spkr, dict_w, spkr_w, lengths, B, T, E, f0 ? 1 : 0, spkr ? 1 : 0, n_codes, n_spk, x, ldx, zs,
                      (hipStream_t)stream);
  DISSC_HIP_CHECK(hipGetLastError());
  return DISSC_OK;
}

int dissc_embed_concat_bwd(const float* gx, const int64_t* code, int has_f0, const int64_t* spkr, const int32_t* lengths, int B,
                           int T, int E, int n_codes, int n_spk, int ldx, float* g_dict, float* g_spkr, void* stream) {
  if (embed_args_bad("dissc_embed_concat_bwd", gx, code, nullptr, spkr, g_dict, g_spkr, B, T, E, n_codes, n_spk, ldx, true))
    return DISSC_EINVAL;
  const int C = E + (has_f0 ? 1 : 0) + (spkr ? E : 0);
  const long long grid = (long long)n_codes + (spkr ? n_spk : 0);
  if (grid > INT_MAX) {
    set_error("dissc_embed_concat_bwd: %lld table rows: more than one launch can take", grid);
    return DISSC_EINVAL;
  }
  hipLaunchKernelGGL(embed_concat_bwd_kernel, dim3((unsigned)grid), dim3(256), 0, (hipStream_t)stream, gx, code, spkr, lengths, B, T,
                     E, has_f0 ? 1 : 0, n_codes, n_spk, C, ldx, g_dict, g_spkr);
  DISSC_HIP_CHECK(hipGetLastError());
  return DISSC_OK;
}

static int rows_args_bad(const char* who, const void* a, const void* b, int B, int C, int ld, int Lmax, bool need4) {
  if (!a || !b || B < 1 || C < 1 || ld < 1 || Lmax < 0 || Lmax > ld || B > 65535 || C > 65535 || (need4 && (ld & 3)) ||
      (need4 && (!aligned16(a) || !aligned16(b)))) {
    set_error("%s: null pointer, B %d or C %d outside 1 .. 65535, Lmax %d outside 0 .. ld %d%s", who, B, C, Lmax, ld,
              need4 ? ", ld not a multiple of 4 or a pointer not 16-byte aligned" : "");
    return 1;
  }
  return 0;
}

int dissc_mrf_mean_fwd(const float* const* r, int nk, float* y, const int32_t* lengths, int B, int C, int ld, int Lmax, void* stream) {
  if (!r || nk < 1 || nk > DISSC_MAX_RK) {
    set_error("dissc_mrf_mean_fwd: nk %d outside 1 .. %d, or no branch pointers", nk, DISSC_MAX_RK);
    return DISSC_EINVAL;
  }
  MrfPtrs p;
  for (int j = 0; j < DISSC_MAX_RK; ++j) p.p[j] = j < nk ? r[j] : nullptr;
  for (int j = 0; j < nk; ++j)
    if (rows_args_bad("dissc_mrf_mean_fwd", r[j], y, B, C, ld, Lmax, true)) return DISSC_EINVAL;
  hipLaunchKernelGGL(mrf_mean_fwd_kernel, dim3((ld + 1023) / 1024, C, B), dim3(256), 0, (hipStream_t)stream, p, nk, y, lengths, C, ld,
                     Lmax);
  DISSC_HIP_CHECK(hipGetLastError());
  return DISSC_OK;
}

int dissc_mrf_mean_bwd(const float* g, int nk, float* gx, const int32_t* lengths, int B, int C, int ld, int Lmax, void* stream) {
  if (nk < 1 || nk > DISSC_MAX_RK) {
    set_error("dissc_mrf_mean_bwd: nk %d outside 1 .. %d", nk, DISSC_MAX_RK);
    return DISSC_EINVAL;
  }
  if (rows_args_bad("dissc_mrf_mean_bwd", g, gx, B, C, ld, Lmax, true)) return DISSC_EINVAL;
  hipLaunchKernelGGL(mrf_mean_bwd_kernel, dim3((ld + 1023) / 1024, C, B), dim3(256), 0, (hipStream_t)stream, g, nk, gx, lengths, C, ld,
                     Lmax);
  DISSC_HIP_CHECK(hipGetLastError());
  return DISSC_OK;
}

int dissc_tanh_fwd(const float* x, float* y, const int32_t* lengths, int B, int C, int ldx, int ldy, int Lmax, void* stream) {
  if (rows_args_bad("dissc_tanh_fwd", x, y, B, C, ldx, Lmax, false) || ldy < Lmax) {
    if (ldy < Lmax) set_error("dissc_tanh_fwd: ldy %d below Lmax %d", ldy, Lmax);
    return DISSC_EINVAL;
  }
  hipLaunchKernelGGL(tanh_fwd_kernel, dim3((Lmax + 1023) / 1024 + (Lmax == 0), C, B), dim3(256), 0, (hipStream_t)stream, x, y, lengths,
                     C, ldx, ldy, Lmax);
  DISSC_HIP_CHECK(hipGetLastError());
  return DISSC_OK;
}

int dissc_tanh_bwd(const float* y, const float* gy, float* gx, const int32_t* lengths, int B, int C, int ldx, int ldy, int Lmax,
                   void* stream) {
  if (!gy || rows_args_bad("dissc_tanh_bwd", y, gx, B, C, ldx, Lmax, false) || ldy < Lmax) {
    if (!gy || ldy < Lmax) set_error("dissc_tanh_bwd: no gy, or ldy %d below Lmax %d", ldy, Lmax);
    return DISSC_EINVAL;
  }
  hipLaunchKernelGGL(tanh_bwd_kernel, dim3((ldx + 1023) / 1024, C, B), dim3(256), 0, (hipStream_t)stream, y, gy, gx, lengths, C, ldx,
                     ldy, Lmax);
  DISSC_HIP_CHECK(hipGetLastError());
  return DISSC_OK;
}

}  // extern "C"
