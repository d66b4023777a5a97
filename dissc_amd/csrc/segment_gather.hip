// The vocoder trainer's batch as ONE gather launch from a corpus packed on the device: CodeDataset.__getitem__ with eval_mode
// False (reference sr/dataset.py:240-267, _sample_interval 199-219).  An utterance of T frames is n = T hop samples after the
// trim; shorter than the segment it is doubled until it is long enough, and doubling is periodic: sample i of the crop is sample
// (start_step hop + i) mod n, frame j is frame (start_step + j) mod T.  The B (utterance, start_step) pairs are validated on the
// host against the host copy of the frame offsets and travel by value in the kernel's arguments; the kernel reads the offsets of
// its utterance from the device copy.  Copies only: bit-exact, every output element written by one thread.
#include "common.h"

namespace dissc {

constexpr int SEG_MAX_BATCH = 256;
constexpr int SEG_THREADS = 256;

struct SegTable {  // by value, 2 KB
  int utt[SEG_MAX_BATCH];
  int start[SEG_MAX_BATCH];
};

// row b's elements in one index space: [0, segment) y, [segment, segment + F) code, [segment + F, segment + 2 F) f0, then spkr
__global__ void __launch_bounds__(SEG_THREADS) segment_gather_kernel(const SegTable tab, const long long* __restrict__ frame_off,
                                                                     const float* __restrict__ audio, const int32_t* __restrict__ codes,
                                                                     const float* __restrict__ f0s, const int32_t* __restrict__ spkrs,
                                                                     int hop, int segment, int F, float* __restrict__ y,
                                                                     int64_t* __restrict__ code, float* __restrict__ f0,
                                                                     int64_t* __restrict__ spkr) {
  const int b = blockIdx.y;
  const int u = tab.utt[b];                                // 0 <= u < U, checked on the host
  const unsigned start = (unsigned)tab.start[b];           // 0 <= start <= T 2^j - F, checked on the host
  const size_t f_first = (size_t)frame_off[u];
  const unsigned T = (unsigned)(frame_off[u + 1] - frame_off[u]);  // 1 <= T, T hop < 2^31 (dissc_segment_create)
  const unsigned e = blockIdx.x * SEG_THREADS + threadIdx.x;       // < 2^31 by the grid (segment + 2 F + 1 < 2^31)
  if (e < (unsigned)segment) {
    // start hop + e < T 2^j hop < 2^31 (j = 0: T hop itself; j > 0: T 2^(j-1) hop < segment < 2^30); the source index is below T hop
    const unsigned src = (start * (unsigned)hop + e) % (T * (unsigned)hop);
    y[(size_t)b * segment + e] = audio[f_first * hop + src];
  } else if (e < (unsigned)(segment + F)) {
    const unsigned j = e - segment;
    code[(size_t)b * F + j] = (int64_t)codes[f_first + (start + j) % T];
  } else if (e < (unsigned)(segment + 2 * F)) {
    const unsigned j = e - segment - F;
    f0[(size_t)b * F + j] = f0s[f_first + (start + j) % T];
  } else if (e == (unsigned)(segment + 2 * F)) {
    spkr[b] = (int64_t)spkrs[u];
  }
}

}  // namespace dissc

using namespace dissc;

struct dissc_segment {
  int U = 0, hop = 0, dev = -1;
  std::vector<long long> off;  // U + 1 frame offsets, the host copy every table is checked against
  long long* d_off = nullptr;
  float* d_audio = nullptr;
  int32_t* d_codes = nullptr;
  float* d_f0 = nullptr;
  int32_t* d_spkr = nullptr;
};

extern "C" {

int dissc_segment_max_batch(void) { return SEG_MAX_BATCH; }

void dissc_segment_destroy(dissc_segment_t h) {
  if (!h) return;
  if (h->d_off) (void)hipFree(h->d_off);
  if (h->d_audio) (void)hipFree(h->d_audio);
  if (h->d_codes) (void)hipFree(h->d_codes);
  if (h->d_f0) (void)hipFree(h->d_f0);
  if (h->d_spkr) (void)hipFree(h->d_spkr);
  delete h;
}

int dissc_segment_create(int U, const long long* frames, int hop, const float* audio, const int32_t* codes, const float* f0,
                         const int32_t* spkr, dissc_segment_t* out) {
  if (out) *out = nullptr;
  if (!out || !frames || !audio || !codes || !f0 || !spkr || U < 1 || hop < 1) {
    set_error("dissc_segment_create: need at least one utterance (U = %d), hop >= 1 (%d), the five host arrays and a place for the handle",
              U, hop);
    return DISSC_EINVAL;
  }
  dissc_segment* h = new dissc_segment();
  h->U = U;
  h->hop = hop;
  h->off.assign((size_t)U + 1, 0);
  for (int u = 0; u < U; ++u) {
    if (frames[u] < 1 || frames[u] * hop >= (1ll << 31)) {
      set_error("dissc_segment_create: utterance %d has %lld frames; need at least 1 and fewer than 2^31 samples", u, frames[u]);
      delete h;
      return DISSC_EINVAL;
    }
    h->off[u + 1] = h->off[u] + frames[u];
  }
  const size_t nf = (size_t)h->off[U];
  bool ok = hipGetDevice(&h->dev) == hipSuccess;
  ok = ok && hipMalloc((void**)&h->d_off, ((size_t)U + 1) * sizeof(long long)) == hipSuccess;
  ok = ok && hipMalloc((void**)&h->d_audio, nf * hop * sizeof(float)) == hipSuccess;
  ok = ok && hipMalloc((void**)&h->d_codes, nf * sizeof(int32_t)) == hipSuccess;
  ok = ok && hipMalloc((void**)&h->d_f0, nf * sizeof(float)) == hipSuccess;
  ok = ok && hipMalloc((void**)&h->d_spkr, (size_t)U * sizeof(int32_t)) == hipSuccess;
  ok = ok && hipMemcpy(h->d_off, h->off.data(), ((size_t)U + 1) * sizeof(long long), hipMemcpyHostToDevice) == hipSuccess;
  ok = ok && hipMemcpy(h->d_audio, audio, nf * hop * sizeof(float), hipMemcpyHostToDevice) == hipSuccess;
  ok = ok && hipMemcpy(h->d_codes, codes, nf * sizeof(int32_t), hipMemcpyHostToDevice) == hipSuccess;
  ok = ok && hipMemcpy(h->d_f0, f0, nf * sizeof(float), hipMemcpyHostToDevice) == hipSuccess;
  ok = ok && hipMemcpy(h->d_spkr, spkr, (size_t)U * sizeof(int32_t), hipMemcpyHostToDevice) == hipSuccess;
  if (!ok) {
    (void)hipGetLastError();
    set_error("dissc_segment_create: no device memory for, or a failed upload of, a corpus of %zu frames of %d samples", nf, hop);
    dissc_segment_destroy(h);
    return DISSC_EHIP;
  }
  *out = h;
  return DISSC_OK;
}

// the last legal start_step of utterance u at this segment: T 2^j - F, 2^j the doublings that reach the segment
static long long seg_interval_end(const dissc_segment* h, int u, int segment) {
  const long long T = h->off[u + 1] - h->off[u];
  long long n = T * h->hop;
  while (n < segment) n *= 2;
  return n / h->hop - segment / h->hop;
}

int dissc_segment_interval_end(dissc_segment_t h, int utterance, int segment, long long* out) {
  if (!h || !out || utterance < 0 || utterance >= h->U || segment < h->hop || segment % h->hop != 0 || segment >= (1 << 30)) {
    set_error("dissc_segment_interval_end: null handle or result, utterance %d outside the corpus, or a segment of %d samples that "
              "is no positive multiple of the hop below 2^30", utterance, segment);
    return DISSC_EINVAL;
  }
  *out = seg_interval_end(h, utterance, segment);
  return DISSC_OK;
}

int dissc_segment_gather(dissc_segment_t h, const int32_t* table, int B, int segment, float* y, int64_t* code, float* f0,
                         int64_t* spkr, void* stream) {
  if (B < 1 || B > SEG_MAX_BATCH) {
    set_error("dissc_segment_gather: B = %d; one launch takes 1 .. %d rows", B, SEG_MAX_BATCH);
    return DISSC_EINVAL;
  }
  if (!h || !table || !y || !code || !f0 || !spkr) {
    set_error("dissc_segment_gather: null handle or pointer");
    return DISSC_EINVAL;
  }
  if (segment < h->hop || segment % h->hop != 0 || segment >= (1 << 30)) {
    set_error("dissc_segment_gather: segment %d must be a positive multiple of code_hop_size %d below 2^30", segment, h->hop);
    return DISSC_EINVAL;
  }
  int dev = 0;
  DISSC_HIP_CHECK(hipGetDevice(&dev));
  if (dev != h->dev) {
    set_error("dissc_segment_gather: the corpus is on device %d, the current device is %d", h->dev, dev);
    return DISSC_EINVAL;
  }
  SegTable tab;
  for (int b = 0; b < SEG_MAX_BATCH; ++b) {
    const int u = b < B ? table[2 * b] : 0, s = b < B ? table[2 * b + 1] : 0;
    if (u < 0 || u >= h->U) {
      set_error("dissc_segment_gather: row %d: utterance %d is outside the corpus of %d", b, u, h->U);
      return DISSC_EINVAL;
    }
    const long long end = seg_interval_end(h, u, segment);
    if (b < B && (s < 0 || s > end)) {
      set_error("dissc_segment_gather: row %d: start_step %d of utterance %d is outside [0, %lld]", b, s, u, end);
      return DISSC_EINVAL;
    }
    tab.utt[b] = u;
    tab.start[b] = s;
  }
  const int F = segment / h->hop;
  const unsigned per_row = (unsigned)segment + 2u * (unsigned)F + 1u;
  hipLaunchKernelGGL(segment_gather_kernel, dim3((per_row + SEG_THREADS - 1) / SEG_THREADS, B), dim3(SEG_THREADS), 0,
                     (hipStream_t)stream, tab, h->d_off, h->d_audio, h->d_codes, h->d_f0, h->d_spkr, h->hop, segment, F, y, code,
                     f0, spkr);
  DISSC_HIP_CHECK(hipGetLastError());
  return DISSC_OK;
}

}  // extern "C"
