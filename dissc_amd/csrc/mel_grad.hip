// Gradient of the log-mel spectrogram of mel.hip with respect to the samples, and the fused training form of its L1
// distance (the generator's mel loss, reference sr/train.py:154-176): one vector-Jacobian product, two entry points.
//
// Per workgroup = (utterance, tile of MEL_TF frames), the forward's enumeration:
//   1. the cotangent of the LINEAR mel, G [mel][frame], goes to the tile's slot of the workspace: the caller's cotangent
//      (linear mode), or that times (mel > 1e-5f ? 1 / mel : 0) with the mel recomputed by the forward's own tile functions
//      (mel_tile.h: same float ops, same order, so the clamp is the forward's), or (l1_grad) scale * sign(lb - la) times the
//      same factor, with both log-mels recomputed and |la - lb| summed exactly as mel_l1 sums it (same bits);
//   2. every wave recomputes re / im of its bin blocks (accumulators of 32 bins x 32 frames), g_mag = basis^T G on the matrix
//      cores (A = the filterbank packed transposed, B = G), g_re = g_mag re / mag and g_im = g_mag im / mag in place;
//   3. those accumulators are at once the B operands (k = bins) of the synthesis GEMM against the windowed cosine / sine rows
//      packed transposed: 32 frame samples (a slab) x 32 frames per accumulator, added into an overlap-add strip of
//      (MEL_TF - 1) hop + n_fft floats in the LDS.  Slabs outside the window and bin blocks outside the filterbank are
//      skipped as in the forward.  Adds into the strip are plain read-modify-writes in a fixed order: in one step the four
//      waves (four bin blocks) work on four consecutive slabs, which touch disjoint strip cells when hop is a multiple of 32
//      and at least 128; for any other hop they take turns.  A barrier ends every step.
//   4. the strip goes to the workspace; mel_grad_fold_kernel gathers, per sample, the strips that cover it (tiles overlap by
//      n_fft - hop) and the two mirror images, in a fixed order, and writes zero beyond the utterance.
// No atomics; nothing depends on the batch or on timing: bit-reproducible.
#include <math.h>

#include <algorithm>

#include "mel_tile.h"

namespace dissc {

static_assert(DISSC_MEL_GRAD_TILE_FRAMES == MEL_TF, "the gradient's tile is the forward's: mel_tile.h and the L1 sums' bits rest on it");

struct MelGradArgs {
  MelArgs m;  // sig[0]: the signal (backward) or the target (l1_grad); sig[1]: the generated signal of l1_grad
  const float* dftT;  // [block][slab][cos | sin][q][lane][4]
  const float* melT;  // [block][q][lane][4]
  unsigned dftT_bytes, melT_bytes;
  int s_lo, s_hi, srs, nslab, fast, strip_len;
  const float* g_mel;  // [B][num_mels][ldG] (backward)
  int ldG;
  const double* scale;  // [B] (l1_grad)
  float* gtile;   // [tile][NMT * 32][MEL_TF]
  float* strips;  // [tile][strip_len]
  float* grad;    // [B][ldg]
  int ldg, ld_out;
};

// cotangent of the log-mel -> cotangent of the mel; the comparison is the forward's clamp
__device__ __forceinline__ float mel_log_cot(float cot, float v) { return cot * (v > 1e-5f ? 1.0f / v : 0.f); }

template <int NMT, bool L1, bool VEC>
__global__ void __launch_bounds__(MEL_NT) mel_grad_kernel(const MelGradArgs p) {
  extern __shared__ float smem[];
  int b, tile, F;
  if (!ragged_tile<MEL_TF>(blockIdx.x, p.m.B, [&](int i) { return mel_nframes(p.m, i); }, b, tile, F)) return;
  const int tid = threadIdx.x, lane = tid & 63, wave = __builtin_amdgcn_readfirstlane(tid >> 6), l31 = lane & 31, h = lane >> 5;
  const int n = mel_len(p.m, b);
  const int hop = p.m.hop, SRS = p.srs;
  float* strip = smem + p.m.rows * p.m.rs;  // first the scratch of the waves' partial mels
  float* gt = p.gtile + (size_t)blockIdx.x * (NMT * 32 * MEL_TF);
  const __amdgpu_buffer_rsrc_t rs_dft = wave_rsrc(p.m.dft, p.m.dft_bytes), rs_mel = wave_rsrc(p.m.melw, p.m.melw_bytes);
  const __amdgpu_buffer_rsrc_t rs_dftT = wave_rsrc(p.dftT, p.dftT_bytes), rs_melT = wave_rsrc(p.melT, p.melT_bytes);
  const bool recompute = L1 || !p.m.linear;

  // ---- 1. G
  float keep[2][NMT][16];  // wave 0: log-mel of the target (l1_grad)
  double lane_sum = 0.0;
  const float scale = L1 ? (float)p.scale[b] : 0.f;
#pragma unroll 1
  for (int sg = 0; sg < (L1 ? 2 : 1); ++sg) {
    if (sg) __syncthreads();
    mel_stage(p.m, smem, p.m.sig[sg] + (size_t)b * p.m.ld[sg], n, tile, tid);
    __syncthreads();
    if (!recompute) break;

    f32x16 macc[2][NMT];
#pragma unroll
    for (int t = 0; t < 2; ++t)
#pragma unroll
      for (int mt = 0; mt < NMT; ++mt)
#pragma unroll
        for (int r = 0; r < 16; ++r) macc[t][mt][r] = 0.f;
#pragma unroll 1
    for (int blk = wave; blk < p.m.nblk; blk += 4) {
      f32x16 ac[2], as[2];
      mel_stft_block<VEC>(p.m, smem, rs_dft, blk, lane, ac, as);
#pragma unroll
      for (int t = 0; t < 2; ++t)
#pragma unroll
        for (int r = 0; r < 16; ++r) ac[t][r] = mel_mag(ac[t][r], as[t][r]);
      mel_gemm_block<NMT>(rs_mel, blk, lane, ac, macc);
    }
    mel_sum_waves<NMT>(strip, wave, lane, macc);
    if (wave == 0) {
#pragma unroll
      for (int t = 0; t < 2; ++t) {
        const int frame = tile * MEL_TF + t * 32 + l31;
#pragma unroll
        for (int mt = 0; mt < NMT; ++mt)
#pragma unroll
          for (int r = 0; r < 16; ++r) {
            const float v = mel_total<NMT>(strip, lane, macc, t, mt, r);
            const int row = mt * 32 + (r & 3) + 8 * (r >> 2) + 4 * h;
            const bool live = row < p.m.num_mels && frame < F;
            float* dst = gt + row * MEL_TF + t * 32 + l31;
            if (!L1) {
              const float cot = live ? p.g_mel[((size_t)b * p.m.num_mels + row) * p.ldG + frame] : 0.f;
              *dst = mel_log_cot(cot, v);
            } else {
              const float lg = v > 1e-5f ? logf(v) : p.m.log_floor;
              if (sg == 0) {
                keep[t][mt][r] = lg;
              } else {
                const float df = keep[t][mt][r] - lg;
                const float d = fabsf(df);
                if (live) lane_sum += (double)d;
                const float sgn = df > 0.f ? -1.f : (df < 0.f ? 1.f : 0.f);  // sign(lb - la), sign(0) = 0
                *dst = mel_log_cot(live ? sgn * scale : 0.f, v);
              }
            }
          }
      }
    }
  }
  if (L1 && wave == 0) {
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) lane_sum += __shfl_xor(lane_sum, off);
    if (lane == 0) p.m.tile_sums[blockIdx.x] = lane_sum;
  }
  if (!recompute) {  // linear mode: the cotangent as it came
    for (int i = tid; i < NMT * 32 * MEL_TF; i += MEL_NT) {
      const int row = i / MEL_TF, frame = tile * MEL_TF + (i - row * MEL_TF);
      gt[i] = (row < p.m.num_mels && frame < F) ? p.g_mel[((size_t)b * p.m.num_mels + row) * p.ldG + frame] : 0.f;
    }
  }
  __syncthreads();  // wave 0 has read the partial mels out of the strip's LDS
  for (int i = tid; i < p.m.rows * SRS; i += MEL_NT) strip[i] = 0.f;
  __threadfence_block();  // G: written by some lanes, read by all
  __syncthreads();

  // ---- 2. and 3.
#pragma unroll 1
  for (int blk0 = 0; blk0 < p.m.nblk; blk0 += 4) {
    const int blk = blk0 + wave;
    const bool active = blk < p.m.nblk;
    f32x16 gre[2], gim[2];
    if (active) {
      mel_stft_block<VEC>(p.m, smem, rs_dft, blk, lane, gre, gim);
      f32x16 gm[2];
#pragma unroll
      for (int t = 0; t < 2; ++t)
#pragma unroll
        for (int r = 0; r < 16; ++r) gm[t][r] = 0.f;
#pragma unroll 2
      for (int q = 0; q < NMT * 4; ++q) {
        const f32x4 w = rsrc_load16(rs_melT, lane * 16, (unsigned)(blk * NMT * 4 + q) * 1024u);
#pragma unroll
        for (int e = 0; e < 4; ++e) {
          const float* g = gt + (8 * q + 4 * h + e) * MEL_TF + l31;
          gm[0] = __builtin_amdgcn_mfma_f32_32x32x2f32(w[e], g[0], gm[0], 0, 0, 0);
          gm[1] = __builtin_amdgcn_mfma_f32_32x32x2f32(w[e], g[32], gm[1], 0, 0, 0);
        }
      }
#pragma unroll
      for (int t = 0; t < 2; ++t)
#pragma unroll
        for (int r = 0; r < 16; ++r) {
          const float s = gm[t][r] / mel_mag(gre[t][r], gim[t][r]);  // mag >= sqrt(1e-9)
          gre[t][r] *= s;
          gim[t][r] *= s;
        }
    }
#pragma unroll 1
    for (int step = p.s_lo - (p.fast ? 3 : 0); step < p.s_hi; ++step) {
      const int slab = p.fast ? step + wave : step;
      const bool on = active && slab >= p.s_lo && slab < p.s_hi;
      f32x16 d[2];
      if (on) {
#pragma unroll
        for (int t = 0; t < 2; ++t)
#pragma unroll
          for (int r = 0; r < 16; ++r) d[t][r] = 0.f;
        const unsigned off = (unsigned)(blk * p.nslab + slab) * 8192u;
#pragma unroll
        for (int q = 0; q < 4; ++q) {
          const f32x4 wc = rsrc_load16(rs_dftT, lane * 16, off + (unsigned)q * 1024u);
          const f32x4 ws = rsrc_load16(rs_dftT, lane * 16, off + 4096u + (unsigned)q * 1024u);
#pragma unroll
          for (int e = 0; e < 4; ++e) {
            d[0] = __builtin_amdgcn_mfma_f32_32x32x2f32(wc[e], gre[0][4 * q + e], d[0], 0, 0, 0);
            d[1] = __builtin_amdgcn_mfma_f32_32x32x2f32(wc[e], gre[1][4 * q + e], d[1], 0, 0, 0);
            d[0] = __builtin_amdgcn_mfma_f32_32x32x2f32(ws[e], gim[0][4 * q + e], d[0], 0, 0, 0);
            d[1] = __builtin_amdgcn_mfma_f32_32x32x2f32(ws[e], gim[1][4 * q + e], d[1], 0, 0, 0);
          }
        }
      }
      // register r of lane l: frame sample 32 slab + (r & 3) + 8 (r >> 2) + 4 (l >> 5) of frame l & 31 -> strip cell hop f + sample,
      // kept as row (cell / hop) of stride SRS.  hop >= 8: the 64 lanes of a register touch 64 different cells.
      const auto add = [&]() {
        const int q0 = 32 * slab + 4 * h, row0 = q0 / hop, c0 = q0 - row0 * hop;
#pragma unroll
        for (int r = 0; r < 16; ++r) {
          int c = c0 + (r & 3) + 8 * (r >> 2), row = row0 + l31;
          while (c >= hop) {
            c -= hop;
            ++row;
          }
          strip[row * SRS + c] += d[0][r];
          strip[(row + 32) * SRS + c] += d[1][r];
        }
      };
      if (p.fast) {
        if (on) add();
        __syncthreads();
      } else {
#pragma unroll 1
        for (int w = 0; w < 4; ++w) {
          if (on && wave == w) add();
          __syncthreads();
        }
      }
    }
  }

  // ---- 4. the tile's strip, rows undone
  const int Ft = F - tile * MEL_TF < MEL_TF ? F - tile * MEL_TF : MEL_TF;
  float* out = p.strips + (size_t)blockIdx.x * p.strip_len;
  for (int i = tid; i < (Ft - 1) * hop + p.m.n_fft; i += MEL_NT) {
    const int r = i / hop;
    out[i] = strip[r * SRS + (i - r * hop)];
  }
}

// One thread per sample: the cells of the mirrored signal that are images of the sample (itself, its image about the
// first sample, its image about the last), each summed over the tiles whose strips cover it, in that order.
__global__ void mel_grad_fold_kernel(const MelGradArgs p) {
  const int b = blockIdx.y, s = blockIdx.x * blockDim.x + threadIdx.x;
  if (s >= p.ld_out) return;
  const int n = mel_len(p.m, b), F = mel_nframes(p.m, b);
  float g = 0.f;
  if (s < n && F > 0) {
    int first = 0;
    for (int i = 0; i < b; ++i) first += (mel_nframes(p.m, i) + MEL_TF - 1) / MEL_TF;
    const int nt = (F + MEL_TF - 1) / MEL_TF, hop = p.m.hop, pad = p.m.pad, TH = MEL_TF * hop, SL = p.strip_len;
    const int ext = (F - 1) * hop + p.m.n_fft;  // cells the frames cover
    const auto cell = [&](int c) {
      float acc = 0.f;
      if (c < 0 || c >= ext) return acc;
      const int t_hi = c / TH < nt - 1 ? c / TH : nt - 1;
      for (int t = c >= SL ? (c - SL) / TH + 1 : 0; t <= t_hi; ++t) {
        const int Ft = F - t * MEL_TF < MEL_TF ? F - t * MEL_TF : MEL_TF, off = c - t * TH;
        if (off < (Ft - 1) * hop + p.m.n_fft) acc += p.strips[(size_t)(first + t) * SL + off];
      }
      return acc;
    };
    g = cell(s + pad);
    if (s >= 1 && s <= pad) g += cell(pad - s);
    if (s <= n - 2 && s >= n - 1 - pad) g += cell(pad + 2 * (n - 1) - s);
  }
  p.grad[(size_t)b * p.ldg + s] = g;
}

}  // namespace dissc

using namespace dissc;

static size_t align256(size_t v) { return (v + 255) / 256 * 256; }

// the gradient's bases go to the device with the handle's first backward launch
static int mel_grad_upload(dissc_mel* h) {
  int rc;
  if ((rc = mel_upload(h))) return rc;
  std::lock_guard<std::mutex> g(h->mu);
  if (h->dftT) return DISSC_OK;
  if ((rc = upload(h->melT_host, &h->melT))) return rc;
  if ((rc = upload(h->dftT_host, &h->dftT))) return rc;
  std::vector<float>().swap(h->dftT_host);
  std::vector<float>().swap(h->melT_host);
  return DISSC_OK;
}

template <bool L1>
static int mel_grad_launch(dissc_mel* h, const MelGradArgs& p, int ntiles, hipStream_t stream) {
  static DeviceOnce once[8];
  const bool vec = h->hop % 4 == 0;
  const dim3 grid(ntiles), block(MEL_NT);
#define DISSC_MEL_CASE(NMT_, VEC_)                                                                                        \
  {                                                                                                                       \
    DISSC_HIP_CHECK(once[(NMT_ - 1) * 2 + VEC_].max_lds(reinterpret_cast<const void*>(&mel_grad_kernel<NMT_, L1, VEC_>), MEL_MAX_LDS)); \
    hipLaunchKernelGGL((mel_grad_kernel<NMT_, L1, VEC_>), grid, block, h->grad_lds_bytes, stream, p);                     \
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

// what both entry points share: checks, the workspace's three parts, the tile kernel, the fold
template <bool L1>
static int mel_grad_run(const char* who, dissc_mel* h, MelGradArgs& p, int B, int ld, float* grad, int ldg, int ld_out, void* workspace,
                        size_t workspace_bytes, double* sum_out, hipStream_t stream) {
  if (h->hop < 8 || h->grad_lds_bytes > (size_t)MEL_MAX_LDS) {
    set_error("%s: the gradient needs hop >= 8 and %zu bytes of LDS for a tile of %d frames, a workgroup has %d (n_fft %d, hop %d)", who,
              h->grad_lds_bytes, MEL_TF, MEL_MAX_LDS, h->n_fft, h->hop);
    return DISSC_EINVAL;
  }
  if (ldg < ld_out) {
    set_error("%s: ldg %d is shorter than the signal's row of %d", who, ldg, ld_out);
    return DISSC_EINVAL;
  }
  const size_t need = dissc_mel_grad_workspace_bytes(h, B, ld);
  if (!workspace || workspace_bytes < need) {
    set_error("%s: workspace too small (%zu bytes, need %zu)", who, workspace_bytes, need);
    return DISSC_ENOMEM;
  }
  if (misaligned16(workspace)) {
    set_error("%s: the workspace must be 16-byte aligned", who);
    return DISSC_EINVAL;
  }
  int rc;
  if ((rc = mel_grad_upload(h))) return rc;
  const int ntiles = mel_max_tiles(h, B, ld);
  mel_fill(h, p.m);
  p.m.n_cap = ld; p.m.B = B;
  p.dftT = h->dftT; p.melT = h->melT;
  p.nslab = h->n_fft / 32;
  p.dftT_bytes = (unsigned)((size_t)h->nblk * p.nslab * 8192);
  p.melT_bytes = (unsigned)((size_t)h->nblk * h->nmt * 4096);
  p.s_lo = h->s_lo; p.s_hi = h->s_hi; p.srs = h->srs;
  p.fast = (h->hop % 32 == 0 && h->hop >= 128) ? 1 : 0;
  p.strip_len = (MEL_TF - 1) * h->hop + h->n_fft;
  char* ws = static_cast<char*>(workspace);
  p.m.tile_sums = reinterpret_cast<double*>(ws);
  ws += align256((size_t)std::max(ntiles, 1) * sizeof(double));
  p.gtile = reinterpret_cast<float*>(ws);
  ws += align256((size_t)ntiles * h->nmt * 32 * MEL_TF * sizeof(float));
  p.strips = reinterpret_cast<float*>(ws);
  p.grad = grad; p.ldg = ldg; p.ld_out = ld_out;
  if (ntiles > 0 && (rc = mel_grad_launch<L1>(h, p, ntiles, stream))) return rc;
  hipLaunchKernelGGL(mel_grad_fold_kernel, dim3((ld_out + 255) / 256, B), dim3(256), 0, stream, p);
  if (L1) hipLaunchKernelGGL(mel_l1_reduce_kernel, dim3((B + 63) / 64), dim3(64), 0, stream, p.m, sum_out);
  DISSC_HIP_CHECK(hipGetLastError());
  return DISSC_OK;
}

extern "C" {

size_t dissc_mel_grad_workspace_bytes(dissc_mel_t h, int B, int Nmax) {
  if (!h || B < 1 || Nmax < 1) return 0;
  const size_t ntiles = (size_t)mel_max_tiles(h, B, Nmax);
  return align256(std::max(ntiles, (size_t)1) * sizeof(double)) + align256(ntiles * h->nmt * 32 * MEL_TF * sizeof(float)) +
         align256(ntiles * ((size_t)(MEL_TF - 1) * h->hop + h->n_fft) * sizeof(float));
}

int dissc_mel_backward(dissc_mel_t h, const float* wav, int ld, const int32_t* n_samples_dev, int B, const float* g_mel, int ldF,
                       int flags, float* grad_wav, int ldg, void* workspace, size_t workspace_bytes, void* stream) {
  if (!h || !wav || !n_samples_dev || !g_mel || !grad_wav || B < 1 || ld < 1 || ldF < ld / h->hop || (flags & ~DISSC_MEL_LINEAR)) {
    set_error("dissc_mel_backward: bad argument");
    return DISSC_EINVAL;
  }
  MelGradArgs p = {};
  p.m.sig[0] = wav; p.m.ld[0] = ld;
  p.m.n_samples = n_samples_dev; p.m.linear = (flags & DISSC_MEL_LINEAR) ? 1 : 0;
  p.g_mel = g_mel; p.ldG = ldF;
  return mel_grad_run<false>("dissc_mel_backward", h, p, B, ld, grad_wav, ldg, ld, workspace, workspace_bytes, nullptr,
                             (hipStream_t)stream);
}

int dissc_mel_l1_grad(dissc_mel_t h, const float* a, int lda, const float* b, int ldb, const int32_t* n_samples_dev, int B,
                      const double* scale_dev, double* sum_out, float* grad_b, int ldg, void* workspace, size_t workspace_bytes,
                      void* stream) {
  if (!h || !a || !b || !n_samples_dev || !scale_dev || !sum_out || !grad_b || B < 1 || lda < 1 || ldb < 1) {
    set_error("dissc_mel_l1_grad: bad argument");
    return DISSC_EINVAL;
  }
  MelGradArgs p = {};
  p.m.sig[0] = a; p.m.sig[1] = b; p.m.ld[0] = lda; p.m.ld[1] = ldb;
  p.m.n_samples = n_samples_dev;
  p.scale = scale_dev;
  return mel_grad_run<true>("dissc_mel_l1_grad", h, p, B, std::min(lda, ldb), grad_b, ldg, ldb, workspace, workspace_bytes, sum_out,
                            (hipStream_t)stream);
}

}  // extern "C"
