// Log-mel spectrogram and the L1 distance between two of them: the vocoder's validation figure (`validation/mel_spec_error`,
// reference sr/train.py:231-269, on the mel_spectrogram of sr/dataset.py:46-69).  Restated in tests/mel_ref.py.
//
// What is computed, per utterance of n samples: the signal is extended by (n_fft - hop) / 2 samples on either side by
// mirroring about its first / last sample; frame f covers extended samples [hop f, hop f + n_fft) for f < n / hop; a frame is
// weighted by a periodic Hann window of `win` samples sitting in the middle of the n_fft, transformed by the one-sided DFT,
// mag = sqrt(re^2 + im^2 + 1e-9), mel = basis . mag with the Slaney filterbank below, out = log(max(mel, 1e-5)).
//
// How: the STFT is a GEMM on v_mfma_f32_32x32x2_f32.  A = the windowed cosine / sine rows (double on the host, rounded once),
// B = the frames, read IMPLICITLY from the tile's samples in LDS: element (k, f) is x[hop f + k], no im2col buffer.  One
// workgroup of four waves per (utterance, tile of MEL_TF = 64 frames); the waves deal the blocks of 32 DFT bins among
// themselves, each wave runs both 32-frame halves of the tile against every A fragment it loads (0.125 KB of A per MFMA).
// Cosine and sine products of a bin block land in accumulators of the same layout, so the magnitude is element-wise in
// registers -- and a 32x32 accumulator is at once 16 B operands of the mel GEMM (register r of lane l holds bin
// (r & 3) + 8 (r >> 2) + 4 (l >> 5) of frame l & 31: the k order the mel basis is packed in), so the magnitudes never leave
// the registers.  The four waves' partial mels are summed through LDS in a fixed order, wave 0 takes the log and stores, or
// (mel_l1) keeps the first signal's log-mel in registers, runs the second signal through the same tile and adds up
// |a - b|: one fp32 subtraction per cell, every addition after it in double and in a fixed order (lane, tile, utterance).
// No atomics: the sums are bit-reproducible and an utterance does not see its neighbours in the batch.
//
// DFT bins whose mel column is all zero below the first / above the last used bin are not computed (DC and Nyquist for the
// shipped 0 .. sr / 2 configs: 511 bins = 16 blocks with one zero row), k chunks where the window is zero are skipped.
// The steps of a tile are in mel_tile.h, shared with the gradient (mel_grad.hip), which recomputes the forward with them.
#include <math.h>

#include <algorithm>

#include "mel_tile.h"

namespace dissc {

template <int NMT, int NSIG, bool VEC>
__global__ void __launch_bounds__(MEL_NT) mel_kernel(const MelArgs p) {
  extern __shared__ float smem[];
  int b, tile, F;
  if (!ragged_tile<MEL_TF>(blockIdx.x, p.B, [&](int i) { return mel_nframes(p, i); }, b, tile, F)) return;
  const int tid = threadIdx.x, lane = tid & 63, wave = __builtin_amdgcn_readfirstlane(tid >> 6), l31 = lane & 31, h = lane >> 5;
  const int n = mel_len(p, b);
  const __amdgpu_buffer_rsrc_t rs_dft = wave_rsrc(p.dft, p.dft_bytes), rs_mel = wave_rsrc(p.melw, p.melw_bytes);

  float keep[2][NMT][16];  // wave 0: log-mel of the first signal (mel_l1)
  double lane_sum = 0.0;

#pragma unroll 1
  for (int sg = 0; sg < NSIG; ++sg) {
    if (sg) __syncthreads();  // wave 0 has read the last partial sums out of the LDS
    mel_stage(p, smem, p.sig[sg] + (size_t)b * p.ld[sg], n, tile, tid);
    __syncthreads();

    f32x16 macc[2][NMT];
#pragma unroll
    for (int t = 0; t < 2; ++t)
#pragma unroll
      for (int mt = 0; mt < NMT; ++mt)
#pragma unroll
        for (int r = 0; r < 16; ++r) macc[t][mt][r] = 0.f;

#pragma unroll 1
    for (int blk = wave; blk < p.nblk; blk += 4) {
      f32x16 ac[2], as[2];
      mel_stft_block<VEC>(p, smem, rs_dft, blk, lane, ac, as);
      // magnitudes in place, then straight into the mel GEMM as its B operand
#pragma unroll
      for (int t = 0; t < 2; ++t)
#pragma unroll
        for (int r = 0; r < 16; ++r) ac[t][r] = mel_mag(ac[t][r], as[t][r]);
      mel_gemm_block<NMT>(rs_mel, blk, lane, ac, macc);
    }

    mel_sum_waves<NMT>(smem, wave, lane, macc);  // through the LDS the samples no longer need
    if (wave == 0) {
#pragma unroll
      for (int t = 0; t < 2; ++t) {
        const int frame = tile * MEL_TF + t * 32 + l31;
#pragma unroll
        for (int mt = 0; mt < NMT; ++mt)
#pragma unroll
          for (int r = 0; r < 16; ++r) {
            float v = mel_total<NMT>(smem, lane, macc, t, mt, r);
            const int row = mt * 32 + (r & 3) + 8 * (r >> 2) + 4 * h;
            const bool live = row < p.num_mels && frame < F;
            if (NSIG == 1) {
              if (!p.linear) v = v > 1e-5f ? logf(v) : p.log_floor;
              if (live) p.out[((size_t)b * p.num_mels + row) * p.ldF + frame] = v;
            } else {
              v = v > 1e-5f ? logf(v) : p.log_floor;
              if (sg == 0) {
                keep[t][mt][r] = v;
              } else {
                const float d = fabsf(keep[t][mt][r] - v);
                if (live) lane_sum += (double)d;
              }
            }
          }
      }
    }
  }
  if (NSIG == 2 && wave == 0) {
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) lane_sum += __shfl_xor(lane_sum, off);
    if (lane == 0) p.tile_sums[blockIdx.x] = lane_sum;
  }
}

// the tiles of an utterance follow each other in the enumeration: add them up in that order
__global__ void mel_l1_reduce_kernel(const MelArgs p, double* __restrict__ out) {
  const int b = blockIdx.x * blockDim.x + threadIdx.x;
  if (b >= p.B) return;
  int first = 0;
  for (int i = 0; i < b; ++i) first += (mel_nframes(p, i) + MEL_TF - 1) / MEL_TF;
  const int nt = (mel_nframes(p, b) + MEL_TF - 1) / MEL_TF;
  double s = 0.0;
  for (int t = 0; t < nt; ++t) s += p.tile_sums[first + t];
  out[b] = mel_len(p, b) > p.pad ? s : __builtin_nan("");
}

// ---- host: Slaney mel scale and filterbank (librosa.filters.mel with its defaults, restated) -----------------------------------
static double hz_to_mel(double f) {
  const double f_sp = 200.0 / 3.0, min_log_hz = 1000.0, logstep = log(6.4) / 27.0;
  return f >= min_log_hz ? min_log_hz / f_sp + log(f / min_log_hz) / logstep : f / f_sp;
}
static double mel_to_hz(double m) {
  const double f_sp = 200.0 / 3.0, min_log_hz = 1000.0, logstep = log(6.4) / 27.0, min_log_mel = min_log_hz / f_sp;
  return m >= min_log_mel ? min_log_hz * exp(logstep * (m - min_log_mel)) : f_sp * m;
}

static bool mel_filterbank(int sr, int n_fft, int num_mels, double fmin, double fmax, double* out) {
  if (sr <= 0 || n_fft < 2 || (n_fft & 1) || num_mels < 1 || !out) return false;
  if (fmax <= 0) fmax = 0.5 * sr;
  if (fmin < 0 || fmin >= fmax) return false;
  const int nb = n_fft / 2 + 1;
  std::vector<double> edge(num_mels + 2);
  const double m_lo = hz_to_mel(fmin), m_hi = hz_to_mel(fmax);
  for (int i = 0; i < num_mels + 2; ++i) edge[i] = mel_to_hz(m_lo + (m_hi - m_lo) * (double)i / (double)(num_mels + 1));
  for (int m = 0; m < num_mels; ++m) {
    const double norm = 2.0 / (edge[m + 2] - edge[m]);  // Slaney: every triangle has unit area
    for (int k = 0; k < nb; ++k) {
      const double f = (double)k * (double)sr / (double)n_fft;
      const double up = (f - edge[m]) / (edge[m + 1] - edge[m]), down = (edge[m + 2] - f) / (edge[m + 2] - edge[m + 1]);
      out[(size_t)m * nb + k] = std::max(0.0, std::min(up, down)) * norm;
    }
  }
  return true;
}

}  // namespace dissc

using namespace dissc;

extern "C" {

int dissc_mel_filterbank(int sr, int n_fft, int num_mels, double fmin, double fmax, double* out) {
  if (!mel_filterbank(sr, n_fft, num_mels, fmin, fmax, out)) {
    set_error("dissc_mel_filterbank: bad argument (sr %d, n_fft %d, num_mels %d, fmin %g, fmax %g)", sr, n_fft, num_mels, fmin, fmax);
    return DISSC_EINVAL;
  }
  return DISSC_OK;
}

int dissc_mel_create(int sr, int n_fft, int num_mels, int hop, int win, double fmin, double fmax, dissc_mel_t* out) {
  if (!out) {
    set_error("dissc_mel_create: bad argument");
    return DISSC_EINVAL;
  }
  *out = nullptr;
  const auto bad = [&](const char* why) {
    set_error("dissc_mel_create: %s (sr %d, n_fft %d, num_mels %d, hop %d, win %d, fmin %g, fmax %g)", why, sr, n_fft, num_mels,
              hop, win, fmin, fmax);
    return DISSC_EINVAL;
  };
  if (sr <= 0) return bad("sampling rate must be positive");
  if (n_fft < 64 || n_fft > 2048 || n_fft % 64) return bad("n_fft must be a multiple of 64 up to 2048");
  if (win < 1 || win > n_fft) return bad("win must be in 1 .. n_fft");
  if (hop < 1 || hop > n_fft || ((n_fft - hop) & 1)) return bad("hop must be in 1 .. n_fft with n_fft - hop even");
  if (hop < 4) return bad("hop must be at least 4");
  if (num_mels < 1 || num_mels > 128) return bad("num_mels must be in 1 .. 128");
  if (fmax <= 0) fmax = 0.5 * sr;
  if (fmin < 0 || fmin >= fmax || fmax > 0.5 * sr) return bad("need 0 <= fmin < fmax <= sr / 2");

  const int nb = n_fft / 2 + 1;
  std::vector<double> fb((size_t)num_mels * nb);
  mel_filterbank(sr, n_fft, num_mels, fmin, fmax, fb.data());
  int b_lo = nb, b_hi = -1;
  for (int m = 0; m < num_mels; ++m)
    for (int k = 0; k < nb; ++k)
      if (fb[(size_t)m * nb + k] != 0.0) {
        b_lo = std::min(b_lo, k);
        b_hi = std::max(b_hi, k);
      }
  if (b_hi < 0) return bad("the filterbank is empty");

  dissc_mel* h = new dissc_mel();
  h->sr = sr; h->n_fft = n_fft; h->num_mels = num_mels; h->hop = hop; h->win = win; h->pad = (n_fft - hop) / 2;
  h->b_lo = b_lo;
  h->nblk = (b_hi - b_lo + 1 + 31) / 32;
  h->nmt = (num_mels + 31) / 32;
  h->nchunk = n_fft / 8;
  const int w_lo = (n_fft - win) / 2;  // the window's first sample inside the frame
  h->j_lo = w_lo / 8;
  h->j_hi = (w_lo + win + 7) / 8;
  // LDS row stride: 16-byte aligned rows, consecutive frames (hop apart) 4 (mod 8) floats apart so that the 16 lanes of a
  // ds_read_b128 pass cover all banks; a hop that is no multiple of 4 is read one float at a time from rows an odd stride apart
  h->rs = hop % 4 ? hop + 1 : ((hop / 4) % 2 ? hop : hop + 4);
  h->rows = MEL_TF - 1 + (n_fft + hop - 1) / hop;
  h->lds_bytes = std::max((size_t)h->rows * h->rs, (size_t)2 * 2 * h->nmt * 16 * 64) * sizeof(float);
  if (h->lds_bytes > (size_t)MEL_MAX_LDS) {
    const size_t need = h->lds_bytes;
    delete h;
    set_error("dissc_mel_create: a tile of %d frames needs %zu bytes of LDS, a workgroup has %d (n_fft %d, hop %d)", MEL_TF, need,
              MEL_MAX_LDS, n_fft, hop);
    return DISSC_EINVAL;
  }

  // windowed DFT rows in double, rounded once; phases reduced exactly
  std::vector<double> wnd(n_fft, 0.0);
  for (int i = 0; i < win; ++i) wnd[w_lo + i] = 0.5 - 0.5 * cos(2.0 * M_PI * (double)i / (double)win);
  const double tw = 2.0 * M_PI / n_fft;
  h->dft_host.assign((size_t)h->nblk * h->nchunk * 2 * 256, 0.f);
  for (int blk = 0; blk < h->nblk; ++blk)
    for (int l = 0; l < 64; ++l) {
      const int bin = b_lo + blk * 32 + (l & 31);
      if (bin > b_hi) continue;
      for (int j = 0; j < h->nchunk; ++j)
        for (int e = 0; e < 4; ++e) {
          const int k = 8 * j + 4 * (l >> 5) + e;
          const double ph = tw * (double)(((long long)bin * k) % n_fft);
          const size_t at = (((size_t)blk * h->nchunk + j) * 2 * 64 + l) * 4 + e;
          h->dft_host[at] = (float)(wnd[k] * cos(ph));
          h->dft_host[at + 256] = (float)(wnd[k] * sin(ph));
        }
    }
  h->melw_host.assign((size_t)h->nblk * h->nmt * 4 * 256, 0.f);
  for (int blk = 0; blk < h->nblk; ++blk)
    for (int mt = 0; mt < h->nmt; ++mt)
      for (int q = 0; q < 4; ++q)
        for (int l = 0; l < 64; ++l)
          for (int e = 0; e < 4; ++e) {
            const int m = mt * 32 + (l & 31), bin = b_lo + blk * 32 + 8 * q + 4 * (l >> 5) + e;
            if (m < num_mels && bin <= b_hi)
              h->melw_host[((((size_t)blk * h->nmt + mt) * 4 + q) * 64 + l) * 4 + e] = (float)fb[(size_t)m * nb + bin];
          }
  // the gradient's operands (mel_grad.hip): the same rows packed transposed.  Synthesis: slab of 32 frame samples x bin block,
  // [block][slab][cos | sin][q][lane][4]: lane l, e -> sample 32 slab + (l & 31), bin 8 q + 4 (l >> 5) + e of the block -- the
  // order in which an accumulator of the analysis holds its bins.  Mel: [block][q][lane][4]: bin l & 31, mel 8 q + 4 (l >> 5) + e.
  h->s_lo = w_lo / 32;
  h->s_hi = (w_lo + win + 31) / 32;
  h->srs = hop | 1;  // odd: the 32 frames of an accumulator register fall into 32 banks
  h->grad_lds_bytes = ((size_t)h->rows * h->rs + std::max((size_t)h->rows * h->srs, (size_t)2 * 2 * h->nmt * 16 * 64)) * sizeof(float);
  const int nslab = n_fft / 32;
  h->dftT_host.assign((size_t)h->nblk * nslab * 2 * 4 * 256, 0.f);
  for (int blk = 0; blk < h->nblk; ++blk)
    for (int sl = 0; sl < nslab; ++sl)
      for (int q = 0; q < 4; ++q)
        for (int l = 0; l < 64; ++l)
          for (int e = 0; e < 4; ++e) {
            const int bin = b_lo + blk * 32 + 8 * q + 4 * (l >> 5) + e, k = 32 * sl + (l & 31);
            if (bin > b_hi) continue;
            const double ph = tw * (double)(((long long)bin * k) % n_fft);
            const size_t at = (((((size_t)blk * nslab + sl) * 2) * 4 + q) * 64 + l) * 4 + e;
            h->dftT_host[at] = (float)(wnd[k] * cos(ph));
            h->dftT_host[at + 1024] = (float)(wnd[k] * sin(ph));
          }
  h->melT_host.assign((size_t)h->nblk * h->nmt * 4 * 256, 0.f);
  for (int blk = 0; blk < h->nblk; ++blk)
    for (int q = 0; q < h->nmt * 4; ++q)
      for (int l = 0; l < 64; ++l)
        for (int e = 0; e < 4; ++e) {
          const int m = 8 * q + 4 * (l >> 5) + e, bin = b_lo + blk * 32 + (l & 31);
          if (m < num_mels && bin <= b_hi)
            h->melT_host[(((size_t)blk * h->nmt * 4 + q) * 64 + l) * 4 + e] = (float)fb[(size_t)m * nb + bin];
        }
  *out = h;
  return DISSC_OK;
}

void dissc_mel_destroy(dissc_mel_t h) {
  if (!h) return;
  if (h->dft) (void)hipFree(h->dft);
  if (h->melw) (void)hipFree(h->melw);
  if (h->dftT) (void)hipFree(h->dftT);
  if (h->melT) (void)hipFree(h->melT);
  delete h;
}

int dissc_mel_frames(dissc_mel_t h, int n_samples) { return h && n_samples > 0 ? n_samples / h->hop : 0; }

size_t dissc_mel_workspace_bytes(dissc_mel_t h, int B, int Nmax) {
  if (!h || B < 1 || Nmax < 1) return 0;
  return (size_t)std::max(mel_max_tiles(h, B, Nmax), 1) * sizeof(double);
}

}  // extern "C"

// the packed bases go to the device with the handle's first launch (creating a handle needs no GPU); a handle serves one device
int dissc::mel_upload(dissc_mel* h) {
  std::lock_guard<std::mutex> g(h->mu);
  int dev = 0;
  DISSC_HIP_CHECK(hipGetDevice(&dev));
  if (h->device == dev) return DISSC_OK;
  if (h->device >= 0) {
    set_error("dissc_mel: the handle lives on device %d, the call came on device %d", h->device, dev);
    return DISSC_EINVAL;
  }
  int rc;
  if ((rc = upload(h->dft_host, &h->dft))) return rc;
  if ((rc = upload(h->melw_host, &h->melw))) return rc;
  std::vector<float>().swap(h->dft_host);
  std::vector<float>().swap(h->melw_host);
  h->device = dev;
  return DISSC_OK;
}

void dissc::mel_fill(const dissc_mel* h, MelArgs& p) {
  p.dft = h->dft; p.melw = h->melw;
  p.dft_bytes = (unsigned)((size_t)h->nblk * h->nchunk * 2048);
  p.melw_bytes = (unsigned)((size_t)h->nblk * h->nmt * 4096);
  p.n_fft = h->n_fft; p.hop = h->hop; p.pad = h->pad; p.rs = h->rs; p.rows = h->rows; p.nblk = h->nblk; p.nchunk = h->nchunk;
  p.j_lo = h->j_lo; p.j_hi = h->j_hi; p.num_mels = h->num_mels;
  p.log_floor = (float)log((double)1e-5f);
}

template <int NSIG>
static int mel_launch(dissc_mel* h, const MelArgs& p, int ntiles, hipStream_t stream) {
  static DeviceOnce once[8];
  const bool vec = h->hop % 4 == 0;
  const dim3 grid(ntiles), block(MEL_NT);
#define DISSC_MEL_CASE(NMT_, VEC_)                                                                               \
  {                                                                                                              \
    DISSC_HIP_CHECK(once[(NMT_ - 1) * 2 + VEC_].max_lds(reinterpret_cast<const void*>(&mel_kernel<NMT_, NSIG, VEC_>), MEL_MAX_LDS)); \
    hipLaunchKernelGGL((mel_kernel<NMT_, NSIG, VEC_>), grid, block, h->lds_bytes, stream, p);                    \
  }
  switch (h->nmt * 2 + (vec ? 1 : 0)) {
    case 2: DISSC_MEL_CASE(1, false) break;
    case 3: DISSC_MEL_CASE(1, true) break;
    case 4: DISSC_MEL_CASE(2, false) break;
    case 5: DISSC_MEL_CASE(2, true) break;
    case 6: DISSC_MEL_CASE(3, false) break;
    case 7: DISSC_MEL_CASE(3, true) break;
    case 8: DISSC_MEL_CASE(4, false) break;
    default: DISSC_MEL_CASE(4, true) break;
  }
#undef DISSC_MEL_CASE
  DISSC_HIP_CHECK(hipGetLastError());
  return DISSC_OK;
}

extern "C" {

int dissc_mel_forward(dissc_mel_t h, const float* wav, int ld, const int32_t* n_samples_dev, int B, float* mel_out, int ldF,
                      int flags, void* /*workspace*/, size_t /*workspace_bytes*/, void* stream) {
  if (!h || !wav || !n_samples_dev || !mel_out || B < 1 || ld < 1 || ldF < ld / h->hop || (flags & ~DISSC_MEL_LINEAR)) {
    set_error("dissc_mel_forward: bad argument");
    return DISSC_EINVAL;
  }
  const int ntiles = mel_max_tiles(h, B, ld);
  if (ntiles == 0) return DISSC_OK;
  int rc;
  if ((rc = mel_upload(h))) return rc;
  MelArgs p = {};
  mel_fill(h, p);
  p.sig[0] = wav; p.ld[0] = ld; p.n_cap = ld;
  p.n_samples = n_samples_dev; p.B = B; p.out = mel_out; p.ldF = ldF; p.linear = (flags & DISSC_MEL_LINEAR) ? 1 : 0;
  return mel_launch<1>(h, p, ntiles, (hipStream_t)stream);
}

int dissc_mel_l1(dissc_mel_t h, const float* a, int lda, const float* b, int ldb, const int32_t* n_samples_dev, int B,
                 double* sum_out, void* workspace, size_t workspace_bytes, void* stream) {
  if (!h || !a || !b || !n_samples_dev || !sum_out || B < 1 || lda < 1 || ldb < 1) {
    set_error("dissc_mel_l1: bad argument");
    return DISSC_EINVAL;
  }
  const int ld = std::min(lda, ldb);  // n_samples is cut to the shorter row
  const int ntiles = mel_max_tiles(h, B, ld);
  if (!workspace || workspace_bytes < dissc_mel_workspace_bytes(h, B, ld)) {
    set_error("dissc_mel_l1: workspace too small (%zu bytes, need %zu)", workspace_bytes, dissc_mel_workspace_bytes(h, B, ld));
    return DISSC_ENOMEM;
  }
  int rc;
  if ((rc = mel_upload(h))) return rc;
  MelArgs p = {};
  mel_fill(h, p);
  p.sig[0] = a; p.sig[1] = b; p.ld[0] = lda; p.ld[1] = ldb; p.n_cap = ld;
  p.n_samples = n_samples_dev; p.B = B; p.tile_sums = static_cast<double*>(workspace);
  if (ntiles > 0 && (rc = mel_launch<2>(h, p, ntiles, (hipStream_t)stream))) return rc;
  hipLaunchKernelGGL(mel_l1_reduce_kernel, dim3((B + 63) / 64), dim3(64), 0, (hipStream_t)stream, p, sum_out);
  DISSC_HIP_CHECK(hipGetLastError());
  return DISSC_OK;
}

}  // extern "C"
