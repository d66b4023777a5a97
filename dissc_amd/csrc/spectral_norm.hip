// Spectral norm of a whole list of weight matrices at once (torch.nn.utils.spectral_norm, reference sr/models.py:288: discriminator 0
// of the MultiScaleDiscriminator): one power iteration  v = normalize(W^T u), u = normalize(W v),  sigma = u . (W v),  w = W / sigma,
// and the gradient  gW = gw / sigma - (sum gw o W / sigma^2) u v^T  with u, v held constant.  Every stage is ONE launch over all
// tensors of the handle (a per-tensor record table on the device; a workgroup finds its tensor by its index); the stages are
// matrix-vector products and element-wise passes, all bandwidth bound.  No atomics, every sum in a fixed order, dots and norms in
// double with one rounding to float for u, v and sigma: bit-reproducible from call to call, and a tensor's results do not depend on
// the list it is in.
#include <limits.h>

#include <algorithm>

#include "common.h"

namespace dissc {

constexpr int SN_CHUNK_ROWS = 32;    // rows per partial chunk of W^T u: one workgroup sums these rows of its column span
constexpr int SN_SPAN_COLS = 1024;   // columns per workgroup span (W^T u, its column sums, v): 256 threads, four columns each
constexpr int SN_WAVE_COLS = 512;    // W v and the gradient: rows of up to this many columns take one wave each, longer ones a workgroup
constexpr int SN_FLAT_SPAN = 4096;   // elements per workgroup of the passes over a tensor as a flat array (W / sigma, sum gw o W)
constexpr int SN_MAX_TENSORS = 128;  // the gradient pointers travel by value in the kernel's arguments
constexpr long long SN_MAX_ROWS = 1ll << 22, SN_MAX_COLS = 1ll << 26, SN_MAX_FLOATS = 1ll << 32;
constexpr double SN_EPS = 1e-12;     // F.normalize(..., eps=1e-12): x / max(||x||, eps)

struct SnTensor {
  long long off;     // the tensor's first float in the flat layout of W, w and gW (a multiple of 4)
  long long poff;    // its first double among the W^T u partials [nchunk][cols]
  int rows, cols;
  int uoff, voff;    // its first element in the flat layouts of u (and W v) and of v (and W^T u); multiples of 4
  int nchunk, nspan; // row chunks, column spans
  int soff;          // its first double among the spans' sums of squares
  int vec;           // cols % 4 == 0: every row starts 16-byte aligned (off % 4 == 0), so rows are read as float4s
  int b_wtu, b_col, b_row, b_flat;  // the tensor's first workgroup in the W^T u grid (nchunk nspan), the column grid (nspan), the
                                    // row grid (ceil(rows / 4) or rows) and the flat grid (ceil(rows cols / SN_FLAT_SPAN))
  int wave;          // 1: cols <= SN_WAVE_COLS, four one-wave rows per workgroup of the row grid; 0: one workgroup per row
  int pad;
};

struct SnPtrs {  // by value, 1 KB
  const float* p[SN_MAX_TENSORS];
};

// the last tensor whose first workgroup is at or below bid (every tensor has at least one workgroup in every grid: the firsts
// strictly increase, and tab[0]'s is 0)
template <int SnTensor::*FIRST>
__device__ __forceinline__ int sn_find(const SnTensor* __restrict__ tab, int n, int bid) {
  int lo = 0, hi = n - 1;
  while (lo < hi) {
    const int mid = (lo + hi + 1) >> 1;
    if (tab[mid].*FIRST <= bid) lo = mid; else hi = mid - 1;
  }
  return lo;
}

__device__ __forceinline__ double sn_wave_sum(double x) {  // a fixed butterfly: every lane gets the sum
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) x += __shfl_xor(x, off);
  return x;
}

// the sum over a 256-thread workgroup, for every thread: the butterfly, then ((w0 + w1) + (w2 + w3)).  Called by all threads; the
// first barrier lets the readers of an earlier call finish with red[4].
__device__ __forceinline__ double sn_block_sum(double x, double* red, int tid) {
  x = sn_wave_sum(x);
  __syncthreads();
  if ((tid & 63) == 0) red[tid >> 6] = x;
  __syncthreads();
  return (red[0] + red[1]) + (red[2] + red[3]);
}

// ---- stage 1: partials of W^T u.  Workgroup (chunk, span) of a tensor: part[chunk][c] = sum over the chunk's rows, in order, of
// W[r][c] u[r] for the span's columns; consecutive threads take consecutive columns (float4s), so the rows are read and the partials
// written coalesced. ----
__global__ void __launch_bounds__(256) snorm_wtu_kernel(const SnTensor* __restrict__ tab, int n, const float* __restrict__ W,
                                                        const float* __restrict__ u, double* __restrict__ part) {
  const SnTensor t = tab[sn_find<&SnTensor::b_wtu>(tab, n, blockIdx.x)];
  const int local = blockIdx.x - t.b_wtu, chunk = local / t.nspan, span = local - chunk * t.nspan, tid = threadIdx.x;
  const int r0 = chunk * SN_CHUNK_ROWS, r1 = min(t.rows, r0 + SN_CHUNK_ROWS);  // chunk < nchunk = ceil(rows / 32): r0 < rows
  const float* Wt = W + t.off;
  const float* ut = u + t.uoff;
  double* pt = part + t.poff + (long long)chunk * t.cols;
  if (t.vec) {
    // c % 4 == 0 and cols % 4 == 0: c < cols implies c + 3 < cols, and off + r cols + c is a multiple of 4: an aligned float4
    // inside row r
    const int c = span * SN_SPAN_COLS + 4 * tid;
    if (c < t.cols) {
      double a0 = 0.0, a1 = 0.0, a2 = 0.0, a3 = 0.0;
#pragma unroll 8
      for (int r = r0; r < r1; ++r) {
        const f32x4 x = *reinterpret_cast<const f32x4*>(Wt + (long long)r * t.cols + c);
        const double ur = (double)ut[r];
        a0 = fma((double)x[0], ur, a0);
        a1 = fma((double)x[1], ur, a1);
        a2 = fma((double)x[2], ur, a2);
        a3 = fma((double)x[3], ur, a3);
      }
      pt[c] = a0, pt[c + 1] = a1, pt[c + 2] = a2, pt[c + 3] = a3;
    }
  } else {
    // scalar loads: column span 1024 + tid + 256 e, guarded by c < cols; r < rows
    double a[4] = {0.0, 0.0, 0.0, 0.0};
    const int c0 = span * SN_SPAN_COLS + tid;
#pragma unroll 4
    for (int r = r0; r < r1; ++r) {
      const float* wr = Wt + (long long)r * t.cols;
      const double ur = (double)ut[r];
#pragma unroll
      for (int e = 0; e < 4; ++e)
        if (c0 + 256 * e < t.cols) a[e] = fma((double)wr[c0 + 256 * e], ur, a[e]);
    }
#pragma unroll
    for (int e = 0; e < 4; ++e)
      if (c0 + 256 * e < t.cols) pt[c0 + 256 * e] = a[e];
  }
}

// ---- stage 2: t = W^T u, the chunks' partials summed in index order per column, and the span's sum of squares ----
__global__ void __launch_bounds__(256) snorm_colsum_kernel(const SnTensor* __restrict__ tab, int n, const double* __restrict__ part,
                                                           double* __restrict__ tsum, double* __restrict__ spansq) {
  __shared__ double red[4];
  const SnTensor t = tab[sn_find<&SnTensor::b_col>(tab, n, blockIdx.x)];
  const int span = blockIdx.x - t.b_col, tid = threadIdx.x;
  const double* pt = part + t.poff;
  double q = 0.0;
#pragma unroll
  for (int e = 0; e < 4; ++e) {
    const int c = span * SN_SPAN_COLS + tid + 256 * e;
    if (c < t.cols) {  // part[k][c], k < nchunk: inside the tensor's nchunk cols partials
      double s = 0.0;
#pragma unroll 8
      for (int k = 0; k < t.nchunk; ++k) s += pt[(long long)k * t.cols + c];  // the loads run ahead, the adds stay in index order
      tsum[t.voff + c] = s;
      q = fma(s, s, q);
    }
  }
  q = sn_block_sum(q, red, tid);
  if (tid == 0) spansq[t.soff + span] = q;
}

// ---- stage 3: v = t / max(||t||, eps); ||t||^2 = the spans' sums in index order (every workgroup of the tensor adds the same
// numbers in the same order) ----
__global__ void __launch_bounds__(256) snorm_vnorm_kernel(const SnTensor* __restrict__ tab, int n, const double* __restrict__ tsum,
                                                          const double* __restrict__ spansq, float* __restrict__ v_out) {
  const SnTensor t = tab[sn_find<&SnTensor::b_col>(tab, n, blockIdx.x)];
  const int span = blockIdx.x - t.b_col, tid = threadIdx.x;
  double ss = 0.0;
  for (int k = 0; k < t.nspan; ++k) ss += spansq[t.soff + k];
  const double d = fmax(sqrt(ss), SN_EPS);
#pragma unroll
  for (int e = 0; e < 4; ++e) {
    const int c = span * SN_SPAN_COLS + tid + 256 * e;
    if (c < t.cols) v_out[t.voff + c] = (float)(tsum[t.voff + c] / d);
  }
}

// one thread's share of  sum a[c] b[c]  over a row of `cols` columns: float4s where vec (a and b 16-byte aligned, cols % 4 == 0:
// c4 < cols / 4 keeps 4 c4 + 3 < cols), else scalars c < cols
template <int NT>
__device__ __forceinline__ double sn_dot_share(const float* __restrict__ a, const float* __restrict__ b, int cols, int vec, int tid) {
  double s = 0.0;
  if (vec) {
    const f32x4* a4 = reinterpret_cast<const f32x4*>(a);
    const f32x4* b4 = reinterpret_cast<const f32x4*>(b);
    for (int c4 = tid; c4 < (cols >> 2); c4 += NT) {
      const f32x4 x = a4[c4], y = b4[c4];
#pragma unroll
      for (int e = 0; e < 4; ++e) s = fma((double)x[e], (double)y[e], s);
    }
  } else {
    for (int c = tid; c < cols; c += NT) s = fma((double)a[c], (double)b[c], s);
  }
  return s;
}

// ---- stage 4: s = W v, one dot per row: a wave per row (four rows per workgroup) or a workgroup per row ----
__global__ void __launch_bounds__(256) snorm_rowdot_kernel(const SnTensor* __restrict__ tab, int n, const float* __restrict__ W,
                                                           const float* __restrict__ v, double* __restrict__ srow) {
  __shared__ double red[4];
  const SnTensor t = tab[sn_find<&SnTensor::b_row>(tab, n, blockIdx.x)];
  const int local = blockIdx.x - t.b_row, tid = threadIdx.x;
  const float* vt = v + t.voff;  // voff % 4 == 0: 16-byte aligned
  if (t.wave) {
    const int r = local * 4 + (tid >> 6);
    if (r < t.rows) {  // a whole wave at a time
      const double s = sn_wave_sum(sn_dot_share<64>(W + t.off + (long long)r * t.cols, vt, t.cols, t.vec, tid & 63));
      if ((tid & 63) == 0) srow[t.uoff + r] = s;
    }
  } else {  // local < rows by the grid
    const double s = sn_block_sum(sn_dot_share<256>(W + t.off + (long long)local * t.cols, vt, t.cols, t.vec, tid), red, tid);
    if (tid == 0) srow[t.uoff + local] = s;
  }
}

// ---- stage 5, one workgroup per tensor: u = s / max(||s||, eps) (iterate) or u_in; sigma = u . s with the float u; the state's u
// and sigma, and without an iteration its v, a copy of v_in ----
__global__ void __launch_bounds__(256) snorm_usigma_kernel(const SnTensor* __restrict__ tab, const double* __restrict__ srow,
                                                           const float* __restrict__ u_in, const float* __restrict__ v_in, int iterate,
                                                           float* __restrict__ st_u, float* __restrict__ st_v, float* __restrict__ st_sigma) {
  __shared__ double red[4];
  const SnTensor t = tab[blockIdx.x];
  const int tid = threadIdx.x;
  const double* s = srow + t.uoff;
  double d = 1.0;
  if (iterate) {
    double q = 0.0;
    for (int r = tid; r < t.rows; r += 256) q = fma(s[r], s[r], q);
    d = fmax(sqrt(sn_block_sum(q, red, tid)), SN_EPS);
  }
  double sg = 0.0;
  for (int r = tid; r < t.rows; r += 256) {
    const float uf = iterate ? (float)(s[r] / d) : u_in[t.uoff + r];
    st_u[t.uoff + r] = uf;
    sg = fma((double)uf, s[r], sg);
  }
  sg = sn_block_sum(sg, red, tid);
  if (tid == 0) st_sigma[blockIdx.x] = (float)sg;
  if (!iterate)
    for (int c = tid; c < t.cols; c += 256) st_v[t.voff + c] = v_in[t.voff + c];
}

// ---- stage 6: w = W / sigma, the tensor as a flat array of rows cols floats.  off % 4 == 0 makes the TENSOR 16-byte aligned
// whatever its cols: float4 i4 < floor(numel / 4) lies inside it, the last numel % 4 elements go one by one (the tensor's last
// workgroup).  A true division, as torch's weight / sigma. ----
__global__ void __launch_bounds__(256) snorm_scale_kernel(const SnTensor* __restrict__ tab, int n, const float* __restrict__ W,
                                                          const float* __restrict__ st_sigma, float* __restrict__ w_out) {
  const int ti = sn_find<&SnTensor::b_flat>(tab, n, blockIdx.x);
  const SnTensor t = tab[ti];
  const int blk = blockIdx.x - t.b_flat, tid = threadIdx.x;
  const long long numel = (long long)t.rows * t.cols, n4 = numel >> 2;
  const float sg = st_sigma[ti];
  const f32x4* x4 = reinterpret_cast<const f32x4*>(W + t.off);
  f32x4* o4 = reinterpret_cast<f32x4*>(w_out + t.off);
#pragma unroll
  for (int j = 0; j < 4; ++j) {
    const long long i4 = (long long)blk * (SN_FLAT_SPAN / 4) + tid + 256 * j;
    if (i4 < n4) {
      const f32x4 x = x4[i4];
      f32x4 o;
#pragma unroll
      for (int e = 0; e < 4; ++e) o[e] = x[e] / sg;
      o4[i4] = o;
    }
  }
  if ((long long)(blk + 1) * SN_FLAT_SPAN >= numel && tid < (int)(numel & 3)) {  // the last workgroup: 4 n4 + tid < numel
    const long long i = 4 * n4 + tid;
    w_out[t.off + i] = W[t.off + i] / sg;
  }
}

// ---- backward 1: the flat grid's partial sums of gw o W (a null gw: zero, nothing read) ----
__global__ void __launch_bounds__(256) snorm_gdot_kernel(const SnTensor* __restrict__ tab, int n, const float* __restrict__ W,
                                                         const SnPtrs gw, double* __restrict__ bpart) {
  __shared__ double red[4];
  const int ti = sn_find<&SnTensor::b_flat>(tab, n, blockIdx.x);
  const SnTensor t = tab[ti];
  const int blk = blockIdx.x - t.b_flat, tid = threadIdx.x;
  const float* g = gw.p[ti];
  double s = 0.0;
  if (g) {  // uniform over the workgroup; the same bounds as snorm_scale_kernel's (g: rows cols floats, 16-byte aligned)
    const long long numel = (long long)t.rows * t.cols, n4 = numel >> 2;
    const f32x4* x4 = reinterpret_cast<const f32x4*>(W + t.off);
    const f32x4* g4 = reinterpret_cast<const f32x4*>(g);
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      const long long i4 = (long long)blk * (SN_FLAT_SPAN / 4) + tid + 256 * j;
      if (i4 < n4) {
        const f32x4 x = x4[i4], y = g4[i4];
#pragma unroll
        for (int e = 0; e < 4; ++e) s = fma((double)x[e], (double)y[e], s);
      }
    }
    if ((long long)(blk + 1) * SN_FLAT_SPAN >= numel && tid < (int)(numel & 3)) {
      const long long i = 4 * n4 + tid;
      s = fma((double)W[t.off + i], (double)g[i], s);
    }
  }
  s = sn_block_sum(s, red, tid);
  if (tid == 0) bpart[blockIdx.x] = s;
}

// ---- backward 2, one workgroup per tensor: coef = (sum gw o W) / sigma^2, the partials in a fixed order ----
__global__ void __launch_bounds__(256) snorm_coef_kernel(const SnTensor* __restrict__ tab, int n, int nflat,
                                                         const double* __restrict__ bpart, const float* __restrict__ st_sigma,
                                                         double* __restrict__ coef) {
  __shared__ double red[4];
  const int ti = blockIdx.x, tid = threadIdx.x;
  const int b0 = tab[ti].b_flat, b1 = ti + 1 < n ? tab[ti + 1].b_flat : nflat;
  double s = 0.0;
  for (int b = b0 + tid; b < b1; b += 256) s += bpart[b];
  s = sn_block_sum(s, red, tid);
  const double sg = (double)st_sigma[ti];
  if (tid == 0) coef[ti] = s / (sg * sg);
}

// one row of  gW = gw / sigma - coef u[r] v[c]  (a null gw: exact zeros); the row grid and the loads of snorm_rowdot_kernel: float4s
// where vec (gw, like W, has its rows 16-byte aligned then), else scalars
template <int NT>
__device__ __forceinline__ void sn_bwd_row(const float* __restrict__ g, const float* __restrict__ v, float* __restrict__ o, int cols,
                                           int vec, double inv, double ku, int tid) {
  if (vec) {
    const f32x4* v4 = reinterpret_cast<const f32x4*>(v);
    const f32x4* g4 = reinterpret_cast<const f32x4*>(g);
    f32x4* o4 = reinterpret_cast<f32x4*>(o);
    for (int c4 = tid; c4 < (cols >> 2); c4 += NT) {
      f32x4 r = {0.f, 0.f, 0.f, 0.f};
      if (g) {
        const f32x4 x = g4[c4], y = v4[c4];
#pragma unroll
        for (int e = 0; e < 4; ++e) r[e] = (float)fma(-ku, (double)y[e], (double)x[e] * inv);
      }
      o4[c4] = r;
    }
  } else {
    for (int c = tid; c < cols; c += NT) o[c] = g ? (float)fma(-ku, (double)v[c], (double)g[c] * inv) : 0.f;
  }
}

// ---- backward 3: the gradient, over the row grid ----
__global__ void __launch_bounds__(256) snorm_bwd_kernel(const SnTensor* __restrict__ tab, int n, const SnPtrs gw,
                                                        const float* __restrict__ st_u, const float* __restrict__ st_v,
                                                        const float* __restrict__ st_sigma, const double* __restrict__ coef,
                                                        float* __restrict__ gW) {
  const int ti = sn_find<&SnTensor::b_row>(tab, n, blockIdx.x);
  const SnTensor t = tab[ti];
  const int local = blockIdx.x - t.b_row, tid = threadIdx.x;
  const int r = t.wave ? local * 4 + (tid >> 6) : local;
  if (r >= t.rows) return;
  const float* g = gw.p[ti];
  const double inv = 1.0 / (double)st_sigma[ti], ku = coef[ti] * (double)st_u[t.uoff + r];
  const long long ro = (long long)r * t.cols;
  if (t.wave)
    sn_bwd_row<64>(g ? g + ro : nullptr, st_v + t.voff, gW + t.off + ro, t.cols, t.vec, inv, ku, tid & 63);
  else
    sn_bwd_row<256>(g ? g + ro : nullptr, st_v + t.voff, gW + t.off + ro, t.cols, t.vec, inv, ku, tid);
}

}  // namespace dissc

using namespace dissc;

struct dissc_snorm {
  int n = 0;
  std::vector<SnTensor> table;
  long long total = 0, utotal = 0, vtotal = 0, ptotal = 0;  // floats of W / of u / of v, doubles of the W^T u partials
  int stotal = 0;                                           // column spans in all
  int g_wtu = 0, g_col = 0, g_row = 0, g_flat = 0;          // the four grids
  SnTensor* d_table = nullptr;
  double* d_ws = nullptr;  // [partials | t = W^T u | the spans' sums of squares | s = W v | the flat grid's partials | coef]
  int dev = -1;
  long long state_floats() const { return utotal + vtotal + ((n + 3) & ~3); }
  long long ws_doubles() const { return ptotal + vtotal + stotal + utotal + g_flat + n; }
};

static int sn_upload(dissc_snorm* h) {
  int dev = 0;
  DISSC_HIP_CHECK(hipGetDevice(&dev));
  if (h->d_table) {
    if (dev != h->dev) {
      set_error("dissc_snorm: the handle's table and workspace are on device %d, the current device is %d (a handle serves one device)",
                h->dev, dev);
      return DISSC_EINVAL;
    }
    return DISSC_OK;
  }
  SnTensor* tab = nullptr;
  double* ws = nullptr;
  DISSC_HIP_CHECK(hipMalloc((void**)&tab, h->table.size() * sizeof(SnTensor)));
  if (hipMalloc((void**)&ws, (size_t)h->ws_doubles() * sizeof(double)) != hipSuccess) {
    (void)hipFree(tab);
    set_error("dissc_snorm: no device memory for the workspace of %lld doubles", h->ws_doubles());
    return DISSC_EHIP;
  }
  if (hipMemcpy(tab, h->table.data(), h->table.size() * sizeof(SnTensor), hipMemcpyHostToDevice) != hipSuccess) {
    (void)hipFree(tab);
    (void)hipFree(ws);
    set_error("dissc_snorm: the upload of the tensor table failed");
    return DISSC_EHIP;
  }
  h->d_table = tab;
  h->d_ws = ws;
  h->dev = dev;
  return DISSC_OK;
}

static bool sn_aligned16(const void* p) { return ((uintptr_t)p & 15) == 0; }

extern "C" {

int dissc_snorm_chunk_rows(void) { return SN_CHUNK_ROWS; }
int dissc_snorm_span_cols(void) { return SN_SPAN_COLS; }
int dissc_snorm_wave_cols(void) { return SN_WAVE_COLS; }
int dissc_snorm_flat_span(void) { return SN_FLAT_SPAN; }

int dissc_snorm_create(int n, const int* rows, const int* cols, dissc_snorm_t* out) {
  if (out) *out = nullptr;
  if (!out || !rows || !cols || n < 1 || n > SN_MAX_TENSORS) {
    set_error("dissc_snorm_create: need 1 .. %d tensors (n = %d), their rows and cols, and a place for the handle", SN_MAX_TENSORS, n);
    return DISSC_EINVAL;
  }
  long long total = 0, trows = 0, tcols = 0;
  for (int i = 0; i < n; ++i) {
    if (rows[i] < 1 || cols[i] < 1) {
      set_error("dissc_snorm_create: tensor %d is %d x %d; rows and cols must be at least 1", i, rows[i], cols[i]);
      return DISSC_EINVAL;
    }
    trows += rows[i];
    tcols += cols[i];
    total += (long long)rows[i] * cols[i];  // < 2^62 + 2^32: no overflow before the test below
    if (trows > SN_MAX_ROWS || tcols > SN_MAX_COLS || total > SN_MAX_FLOATS) {
      set_error("dissc_snorm_create: more than %lld rows, %lld columns or %lld floats in all (at tensor %d)", SN_MAX_ROWS, SN_MAX_COLS,
                SN_MAX_FLOATS, i);
      return DISSC_EINVAL;
    }
  }
  dissc_snorm* h = new dissc_snorm();
  h->n = n;
  h->table.resize(n);
  // the limits keep every count below in range: at most 2^32 / 2^12 + n flat workgroups, 2^22 row workgroups,
  // sum (rows / 32 + 1) (cols / 1024 + 1) <= 2^17 + 2^17 + 2^16 + n W^T u workgroups, 2^27 + 2^26 partial doubles
  for (int i = 0; i < n; ++i) {
    SnTensor& t = h->table[i];
    t.off = h->total;
    t.poff = h->ptotal;
    t.rows = rows[i];
    t.cols = cols[i];
    t.uoff = (int)h->utotal;
    t.voff = (int)h->vtotal;
    t.nchunk = (rows[i] + SN_CHUNK_ROWS - 1) / SN_CHUNK_ROWS;
    t.nspan = (cols[i] + SN_SPAN_COLS - 1) / SN_SPAN_COLS;
    t.soff = h->stotal;
    t.vec = cols[i] % 4 == 0;
    t.wave = cols[i] <= SN_WAVE_COLS;
    t.b_wtu = h->g_wtu;
    t.b_col = h->g_col;
    t.b_row = h->g_row;
    t.b_flat = h->g_flat;
    t.pad = 0;
    const long long numel = (long long)rows[i] * cols[i];
    h->total = (h->total + numel + 3) & ~3ll;
    h->utotal = (h->utotal + rows[i] + 3) & ~3ll;
    h->vtotal = (h->vtotal + cols[i] + 3) & ~3ll;
    h->ptotal += (long long)t.nchunk * cols[i];
    h->stotal += t.nspan;
    h->g_wtu += t.nchunk * t.nspan;
    h->g_col += t.nspan;
    h->g_row += t.wave ? (rows[i] + 3) / 4 : rows[i];
    h->g_flat += (int)((numel + SN_FLAT_SPAN - 1) / SN_FLAT_SPAN);
  }
  *out = h;
  return DISSC_OK;
}

void dissc_snorm_destroy(dissc_snorm_t h) {
  if (!h) return;
  if (h->d_table) (void)hipFree(h->d_table);
  if (h->d_ws) (void)hipFree(h->d_ws);
  delete h;
}

int dissc_snorm_offsets(dissc_snorm_t h, long long* off, long long* u_off, long long* v_off, long long* total_floats,
                        long long* total_u, long long* total_v, long long* state_floats) {
  if (!h) {
    set_error("dissc_snorm_offsets: null handle");
    return DISSC_EINVAL;
  }
  for (int i = 0; i < h->n; ++i) {
    if (off) off[i] = h->table[i].off;
    if (u_off) u_off[i] = h->table[i].uoff;
    if (v_off) v_off[i] = h->table[i].voff;
  }
  if (total_floats) *total_floats = h->total;
  if (total_u) *total_u = h->utotal;
  if (total_v) *total_v = h->vtotal;
  if (state_floats) *state_floats = h->state_floats();
  return DISSC_OK;
}

int dissc_snorm_forward(dissc_snorm_t h, const float* w_orig, const float* u_in, const float* v_in, int iterate, float* w_out,
                        float* state_out, void* stream) {
  if (!h || !w_orig || !u_in || !v_in || !w_out || !state_out) {
    set_error("dissc_snorm_forward: null handle or pointer");
    return DISSC_EINVAL;
  }
  if (!sn_aligned16(w_orig) || !sn_aligned16(u_in) || !sn_aligned16(v_in) || !sn_aligned16(w_out) || !sn_aligned16(state_out)) {
    set_error("dissc_snorm_forward: w_orig, u_in, v_in, w_out and state_out must be 16-byte aligned");
    return DISSC_EINVAL;
  }
  if (iterate != 0 && iterate != 1) {
    set_error("dissc_snorm_forward: iterate = %d is neither 0 nor 1", iterate);
    return DISSC_EINVAL;
  }
  if (w_out == w_orig || state_out == u_in || state_out == v_in) {
    set_error("dissc_snorm_forward: w_out / state_out must not be an input (the inputs are never written)");
    return DISSC_EINVAL;
  }
  if (int rc = sn_upload(h)) return rc;
  hipStream_t st = (hipStream_t)stream;
  const SnTensor* tab = h->d_table;
  double* part = h->d_ws;
  double* tsum = part + h->ptotal;
  double* spansq = tsum + h->vtotal;
  double* srow = spansq + h->stotal;
  float* st_u = state_out;
  float* st_v = state_out + h->utotal;
  float* st_sigma = st_v + h->vtotal;
  if (iterate) {
    hipLaunchKernelGGL(snorm_wtu_kernel, dim3(h->g_wtu), dim3(256), 0, st, tab, h->n, w_orig, u_in, part);
    hipLaunchKernelGGL(snorm_colsum_kernel, dim3(h->g_col), dim3(256), 0, st, tab, h->n, part, tsum, spansq);
    hipLaunchKernelGGL(snorm_vnorm_kernel, dim3(h->g_col), dim3(256), 0, st, tab, h->n, tsum, spansq, st_v);
  }
  hipLaunchKernelGGL(snorm_rowdot_kernel, dim3(h->g_row), dim3(256), 0, st, tab, h->n, w_orig, iterate ? st_v : v_in, srow);
  hipLaunchKernelGGL(snorm_usigma_kernel, dim3(h->n), dim3(256), 0, st, tab, srow, u_in, v_in, iterate, st_u, st_v, st_sigma);
  hipLaunchKernelGGL(snorm_scale_kernel, dim3(h->g_flat), dim3(256), 0, st, tab, h->n, w_orig, st_sigma, w_out);
  DISSC_HIP_CHECK(hipGetLastError());
  return DISSC_OK;
}

int dissc_snorm_backward(dissc_snorm_t h, const float* w_orig, const float* state, const float* const* gw_ptrs, float* gw_orig,
                         void* stream) {
  if (!h || !w_orig || !state || !gw_ptrs || !gw_orig) {
    set_error("dissc_snorm_backward: null handle or pointer");
    return DISSC_EINVAL;
  }
  if (!sn_aligned16(w_orig) || !sn_aligned16(state) || !sn_aligned16(gw_orig)) {
    set_error("dissc_snorm_backward: w_orig, state and gw_orig must be 16-byte aligned");
    return DISSC_EINVAL;
  }
  SnPtrs gw;
  for (int i = 0; i < SN_MAX_TENSORS; ++i) {
    gw.p[i] = i < h->n ? gw_ptrs[i] : nullptr;
    if (!sn_aligned16(gw.p[i])) {
      set_error("dissc_snorm_backward: the gradient of tensor %d is not 16-byte aligned", i);
      return DISSC_EINVAL;
    }
  }
  if (int rc = sn_upload(h)) return rc;
  hipStream_t st = (hipStream_t)stream;
  const SnTensor* tab = h->d_table;
  double* bpart = h->d_ws + h->ptotal + h->vtotal + h->stotal + h->utotal;
  double* coef = bpart + h->g_flat;
  const float* st_u = state;
  const float* st_v = state + h->utotal;
  const float* st_sigma = st_v + h->vtotal;
  hipLaunchKernelGGL(snorm_gdot_kernel, dim3(h->g_flat), dim3(256), 0, st, tab, h->n, w_orig, gw, bpart);
  hipLaunchKernelGGL(snorm_coef_kernel, dim3(h->n), dim3(256), 0, st, tab, h->n, h->g_flat, bpart, st_sigma, coef);
  hipLaunchKernelGGL(snorm_bwd_kernel, dim3(h->g_row), dim3(256), 0, st, tab, h->n, gw, st_u, st_v, st_sigma, coef, gw_orig);
  DISSC_HIP_CHECK(hipGetLastError());
  return DISSC_OK;
}

}  // extern "C"
