// Prosody metrics on device-side F0 tracks: what reference eval.py computes per file with numpy / scipy once it has the
// two YAAPT tracks -- scipy.stats.wasserstein_distance of the zero-extended tracks (eval.py:96-102) and aligned_ffe with
// utils.interp's nearest-neighbour resampling (eval.py:50-57, utils.py:39-45).  Restated in tests/eval_ref.py.
// The tracks stay where the tracker left them (f32 [R, ld]); only one double per pair / interval goes back to the host.
// All arithmetic below is IEEE double on the float32 values widened to double, without contraction into FMAs: the FFE is
// compared bit for bit with numpy, and 4 432 of the (cur_len, target_len) pairs below 120 put a grid point exactly on a
// midpoint of the other grid.
#include "common.h"

#pragma clang fp contract(off)

namespace dissc {

constexpr int EMD_NT = 256;
constexpr int FFE_NT = 256;
constexpr int FFE_LANES = 16;  // a quarter-wave per interval (intervals are 1 .. ~400 frames)

// 64-lane butterfly, then the 4 wave sums through LDS: the same order on every run and for every grid
__device__ __forceinline__ double emd_block_sum(double v, double* red) {
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) v += __shfl_xor(v, off);
  const int wave = threadIdx.x >> 6;
  __syncthreads();
  if ((threadIdx.x & 63) == 0) red[wave] = v;
  __syncthreads();
  return (red[0] + red[1]) + (red[2] + red[3]);
}

// One workgroup per pair.  Both samples are staged in LDS with their zero extension, sorted there as plain float keys,
// and the merged order is walked by merge path: thread t owns the merged positions [t * chunk, (t + 1) * chunk), finds
// its start (i, j) by a binary search on the diagonal i + j = t * chunk, and from there the counts of the two cdfs are
// just i and j.  A term is |i / la - j / lb| * (next - cur) after taking `cur`; between equal values the gap is 0, so
// the order inside a run of ties (40 % of a track is exact zeros) cannot change the sum.
__global__ void __launch_bounds__(EMD_NT) track_emd_kernel(const float* __restrict__ tracks, int n_rows, int ld,
                                                           const int32_t* __restrict__ pairs, int max_pair_frames,
                                                           double* __restrict__ out) {
  extern __shared__ float emd_keys[];
  __shared__ double red[4];
  const int32_t* e = pairs + 6 * (size_t)blockIdx.x;
  const int ra = e[0], na = e[1], la = e[2], rb = e[3], nb = e[4], lb = e[5];
  const bool ok = ra >= 0 && ra < n_rows && rb >= 0 && rb < n_rows && na >= 0 && nb >= 0 && la >= 1 && lb >= 1 &&
                  na <= la && nb <= lb && na <= ld && nb <= ld && (long long)la + lb <= (long long)max_pair_frames;
  if (!ok) {  // uniform over the workgroup
    if (threadIdx.x == 0) out[blockIdx.x] = __builtin_nan("");
    return;
  }
  float* a = emd_keys;
  float* b = emd_keys + la;
  const float* ta = tracks + (size_t)ra * ld;
  const float* tb = tracks + (size_t)rb * ld;
  for (int i = threadIdx.x; i < la; i += EMD_NT) a[i] = i < na ? ta[i] : 0.0f;
  for (int i = threadIdx.x; i < lb; i += EMD_NT) b[i] = i < nb ? tb[i] : 0.0f;
  __syncthreads();

  // bitonic network with every comparator ascending (first step of a merge pairs i with i ^ (2k - 1), the others with
  // i ^ j): positions >= n behave as +inf that never moves, so a comparator that reaches beyond n is skipped and any n
  // sorts without padding.  Both samples go through the same passes.
  const int nmax = la > lb ? la : lb;
  for (int k = 1; k < nmax; k <<= 1) {
    for (int j = k; j > 0; j >>= 1) {
      const int mask = j == k ? 2 * k - 1 : j;
      // comparators of sample a to enumerate: the valid ones (hi < n) are the first n / 2 of an i ^ j step, but of the
      // mirrored step they are the LAST of the trailing partial block, so that step enumerates every low index
      const int ca = j == k ? la : (la + 1) / 2, cb = j == k ? lb : (lb + 1) / 2;
      for (int c = threadIdx.x; c < ca + cb; c += EMD_NT) {
        const bool second = c >= ca;
        float* s = second ? b : a;
        const int n = second ? lb : la;
        const int q = second ? c - ca : c;
        const int lo = ((q & ~(j - 1)) << 1) | (q & (j - 1));  // q-th index with bit j clear
        const int hi = lo ^ mask;
        if (hi < n) {
          const float x = s[lo], y = s[hi];
          if (y < x) {
            s[lo] = y;
            s[hi] = x;
          }
        }
      }
      __syncthreads();
    }
  }

  const int total = la + lb;
  const int chunk = (total + EMD_NT - 1) / EMD_NT;
  const int k0 = min(threadIdx.x * chunk, total - 1), k1 = min(k0 + chunk, total - 1);  // terms k0 .. k1 - 1 of total - 1
  double sum = 0.0;
  if (k0 < k1) {
    int lo = max(0, k0 - lb), hi = min(k0, la);
    while (lo < hi) {  // merge path: a first on ties
      const int mid = (lo + hi) >> 1;
      if (a[mid] <= b[k0 - 1 - mid]) lo = mid + 1; else hi = mid;
    }
    int i = lo, j = k0 - lo;
    for (int k = k0; k < k1; ++k) {
      const bool take_a = j >= lb || (i < la && a[i] <= b[j]);
      const float cur = take_a ? a[i] : b[j];
      i += take_a ? 1 : 0;
      j += take_a ? 0 : 1;
      const float next = j >= lb ? a[i] : (i >= la ? b[j] : fminf(a[i], b[j]));
      sum += fabs((double)i / (double)la - (double)j / (double)lb) * ((double)next - (double)cur);
    }
  }
  sum = emd_block_sum(sum, red);
  if (threadIdx.x == 0) out[blockIdx.x] = sum;
}

// linspace(0, 1, n)[j] as numpy builds it: j * (1 / (n - 1)), the last point exactly 1
__device__ __forceinline__ double grid_point(int j, int n, double step) { return j == n - 1 ? 1.0 : (double)j * step; }

// index of the generated frame that interp1d(kind='nearest') on linspace(0, 1, cur) gives for point t of
// linspace(0, 1, tgt): clip(searchsorted(mid, x_new, side='left'), 0, cur - 1), mid[i] = x[i] / 2 + x[i + 1] / 2
__device__ __forceinline__ int nearest_index(int t, int tgt, int cur, double step_t, double step_c) {
  const double xn = tgt == 1 ? 0.0 : grid_point(t, tgt, step_t);
  int lo = 0, hi = cur - 1;  // number of midpoints < xn
  while (lo < hi) {
    const int m = (lo + hi) >> 1;
    const double mid = grid_point(m, cur, step_c) / 2.0 + grid_point(m + 1, cur, step_c) / 2.0;
    if (mid < xn) lo = m + 1; else hi = m;
  }
  return lo;
}

__global__ void __launch_bounds__(FFE_NT) track_ffe_kernel(const float* __restrict__ tracks, int n_rows, int ld,
                                                           const int32_t* __restrict__ iv, int n_intervals,
                                                           double* __restrict__ ffe, int32_t* __restrict__ status) {
  const int s = (blockIdx.x * FFE_NT + threadIdx.x) / FFE_LANES;
  const int lane = threadIdx.x & (FFE_LANES - 1);
  int count = 0, tgt = 0, st = 0;
  bool live = false;
  if (s < n_intervals) {
    const int32_t* e = iv + 6 * (size_t)s;
    const int rr = e[0], lr = e[1], hr = e[2], rs = e[3], ls = e[4], hs = e[5];
    const bool ok = rr >= 0 && rr < n_rows && rs >= 0 && rs < n_rows && lr >= 0 && lr <= hr && hr <= ld && ls >= 0 &&
                    ls <= hs && hs <= ld;
    tgt = ok ? hr - lr : 0;
    const int cur = ok ? hs - ls : 0;
    st = !ok ? DISSC_FFE_BAD_ENTRY : (cur == 0 && tgt > 0 ? DISSC_FFE_EMPTY_SYN : 0);
    live = true;
    if (st == 0 && tgt > 0) {
      const float* ref = tracks + (size_t)rr * ld + lr;
      const float* syn = tracks + (size_t)rs * ld + ls;
      const double step_t = tgt > 1 ? 1.0 / (double)(tgt - 1) : 0.0;
      const double step_c = cur > 1 ? 1.0 / (double)(cur - 1) : 0.0;
      for (int t = lane; t < tgt; t += FFE_LANES) {
        double v;
        if (cur == 1) v = (double)tgt * (double)syn[0];  // utils.interp: `target_len * vals` on an ndarray is a product
        else if (cur == tgt) v = (double)syn[t];
        else v = (double)syn[nearest_index(t, tgt, cur, step_t, step_c)];
        const double r = ((double)ref[t] + 0.0001) / (v + 0.0001) - 1.0;
        count += fabs(r) > 0.2 ? 1 : 0;
      }
    }
  }
#pragma unroll
  for (int off = FFE_LANES / 2; off > 0; off >>= 1) count += __shfl_xor(count, off, FFE_LANES);
  if (live && lane == 0) {
    ffe[s] = (st == 0 && tgt > 0) ? (double)count / (double)tgt : __builtin_nan("");
    status[s] = st;
  }
}

}  // namespace dissc

extern "C" size_t dissc_track_emd_workspace_bytes(int, int) { return 0; }
extern "C" size_t dissc_track_ffe_workspace_bytes(int) { return 0; }

extern "C" int dissc_track_emd(const float* tracks, int n_rows, int ld, const int32_t* pairs, int n_pairs,
                               int max_pair_frames, double* emd_out, void* /*workspace*/, size_t /*workspace_bytes*/,
                               void* stream) {
  using namespace dissc;
  if (n_pairs < 0 || n_rows < 0 || ld < 0 || max_pair_frames < 0 ||
      (n_pairs > 0 && (!tracks || !pairs || !emd_out || n_rows == 0))) {
    set_error("dissc_track_emd: bad argument");
    return DISSC_EINVAL;
  }
  if (max_pair_frames > DISSC_EMD_MAX_PAIR_FRAMES) {
    set_error("dissc_track_emd: a pair of %d frames does not fit the LDS of a workgroup (at most %d for both tracks together)",
              max_pair_frames, DISSC_EMD_MAX_PAIR_FRAMES);
    return DISSC_EINVAL;
  }
  if (n_pairs == 0) return DISSC_OK;
  static DeviceOnce attr_once;
  DISSC_HIP_CHECK(attr_once.max_lds(reinterpret_cast<const void*>(&track_emd_kernel),
                                    DISSC_EMD_MAX_PAIR_FRAMES * (int)sizeof(float)));
  const size_t lds = (size_t)(max_pair_frames > 0 ? max_pair_frames : 1) * sizeof(float);
  hipLaunchKernelGGL(track_emd_kernel, dim3(n_pairs), dim3(EMD_NT), lds, (hipStream_t)stream, tracks, n_rows, ld, pairs,
                     max_pair_frames, emd_out);
  DISSC_HIP_CHECK(hipGetLastError());
  return DISSC_OK;
}

extern "C" int dissc_track_ffe(const float* tracks, int n_rows, int ld, const int32_t* intervals, int n_intervals,
                               double* ffe_out, int32_t* status_out, void* /*workspace*/, size_t /*workspace_bytes*/,
                               void* stream) {
  using namespace dissc;
  if (n_intervals < 0 || n_rows < 0 || ld < 0 ||
      (n_intervals > 0 && (!tracks || !intervals || !ffe_out || !status_out || n_rows == 0))) {
    set_error("dissc_track_ffe: bad argument");
    return DISSC_EINVAL;
  }
  if (n_intervals == 0) return DISSC_OK;
  const int per_block = FFE_NT / FFE_LANES;
  hipLaunchKernelGGL(track_ffe_kernel, dim3((n_intervals + per_block - 1) / per_block), dim3(FFE_NT), 0,
                     (hipStream_t)stream, tracks, n_rows, ld, intervals, n_intervals, ffe_out, status_out);
  DISSC_HIP_CHECK(hipGetLastError());
  return DISSC_OK;
}
