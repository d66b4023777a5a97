// What the mel kernels of mel.hip (forward, fused L1) and mel_grad.hip (their gradient) share: the argument struct, the
// handle, and the steps of one tile of MEL_TF frames -- staging the mirrored samples, the STFT of a block of 32 bins, the mel
// GEMM on its magnitudes, the ordered sum of the four waves' partial mels.  The gradient recomputes the forward with these
// very functions: its clamp decisions and its L1 sums are the forward's bit for bit because they are the same float
// operations in the same order.
#pragma once
#include <math.h>

#include <mutex>
#include <vector>

#include "common.h"
#include "ragged_epi.h"

typedef float f32x16 __attribute__((ext_vector_type(16)));

namespace dissc {

constexpr int MEL_TF = DISSC_MEL_TILE_FRAMES;  // frames per workgroup: two 32-column MFMA tiles per wave
constexpr int MEL_NT = 256;
constexpr int MEL_MAX_LDS = 160 * 1024;
static_assert(MEL_TF == 64, "a wave runs exactly two 32-frame MFMA tiles");

struct MelArgs {
  const float* sig[2];  // [B][ld[s]] each; sig[1] only for mel_l1
  int ld[2];
  int n_cap;                 // an utterance is cut to this many samples (the shorter row)
  const int32_t* n_samples;  // [B]
  int B;
  const float* dft;   // [block][chunk][cos | sin][lane][4]: lane l, e -> row (l & 31) of the block, k = 8 chunk + 4 (l >> 5) + e
  const float* melw;  // [block][mel tile][q][lane][4]: lane l, e -> mel row (l & 31) of the tile, bin 8 q + 4 (l >> 5) + e
  unsigned dft_bytes, melw_bytes;
  int n_fft, hop, pad, rs, rows, nblk, nchunk, j_lo, j_hi, num_mels;
  float* out;  // [B][num_mels][ldF] (mel_forward)
  int ldF, linear;
  float log_floor;     // log(1e-5f), rounded once on the host
  double* tile_sums;   // one per enumerated workgroup (mel_l1)
};

#ifdef __HIPCC__
__device__ __forceinline__ int mel_len(const MelArgs& p, int i) {
  const int n = p.n_samples[i];
  return n < p.n_cap ? n : p.n_cap;
}
// frames of utterance i; none when it is too short to mirror
__device__ __forceinline__ int mel_nframes(const MelArgs& p, int i) {
  const int n = mel_len(p, i);
  return n > p.pad ? n / p.hop : 0;
}

// the tile's samples, mirrored about the utterance's own ends; row r of the LDS holds samples [hop r, hop (r + 1))
__device__ __forceinline__ void mel_stage(const MelArgs& p, float* smem, const float* x, int n, int tile, int tid) {
  const int hop = p.hop, RS = p.rs;
  const int s0 = tile * MEL_TF * hop - p.pad, total = p.rows * hop;
  for (int i = tid; i < total; i += MEL_NT) {
    int s = s0 + i;
    s = s < 0 ? -s : s;
    s = s >= n ? 2 * (n - 1) - s : s;
    const int r = i / hop;
    smem[r * RS + (i - r * hop)] = (s >= 0 && s < n) ? x[s] : 0.f;  // beyond the mirror: frames that are not stored
  }
}

// re (ac) and im (as) of the 32 bins of block blk for both 32-frame halves of the tile
template <bool VEC>
__device__ __forceinline__ void mel_stft_block(const MelArgs& p, const float* smem, __amdgpu_buffer_rsrc_t rs_dft, int blk, int lane,
                                               f32x16 (&ac)[2], f32x16 (&as)[2]) {
  const int hop = p.hop, RS = p.rs, l31 = lane & 31, h = lane >> 5;
#pragma unroll
  for (int t = 0; t < 2; ++t)
#pragma unroll
    for (int r = 0; r < 16; ++r) ac[t][r] = as[t][r] = 0.f;
  // the lane's four consecutive k of chunk j start at k0 = 8 j + 4 h: LDS row k0 / hop further down, column k0 % hop
  int k0 = 8 * p.j_lo + 4 * h;
  int col = k0 % hop;
  int base = (l31 + k0 / hop) * RS;
  unsigned aoff = (unsigned)(blk * p.nchunk + p.j_lo) * 2048u;
  for (int j = p.j_lo; j < p.j_hi; ++j) {
    const f32x4 wc = rsrc_load16(rs_dft, lane * 16, aoff);
    const f32x4 ws = rsrc_load16(rs_dft, lane * 16, aoff + 1024u);
    f32x4 x0, x1;
    if (VEC) {  // hop % 4 == 0: the four k sit in one row, 16-byte aligned
      x0 = *reinterpret_cast<const f32x4*>(smem + base + col);
      x1 = *reinterpret_cast<const f32x4*>(smem + base + 32 * RS + col);
    } else {
#pragma unroll
      for (int e = 0; e < 4; ++e) {
        const int c = col + e, at = base + (c >= hop ? c - hop + RS : c);  // hop >= 4: at most one row further
        x0[e] = smem[at];
        x1[e] = smem[at + 32 * RS];
      }
    }
#pragma unroll
    for (int e = 0; e < 4; ++e) {
      ac[0] = __builtin_amdgcn_mfma_f32_32x32x2f32(wc[e], x0[e], ac[0], 0, 0, 0);
      as[0] = __builtin_amdgcn_mfma_f32_32x32x2f32(ws[e], x0[e], as[0], 0, 0, 0);
      ac[1] = __builtin_amdgcn_mfma_f32_32x32x2f32(wc[e], x1[e], ac[1], 0, 0, 0);
      as[1] = __builtin_amdgcn_mfma_f32_32x32x2f32(ws[e], x1[e], as[1], 0, 0, 0);
    }
    aoff += 2048u;
    col += 8;
    while (col >= hop) {
      col -= hop;
      base += RS;
    }
  }
}

__device__ __forceinline__ float mel_mag(float re, float im) { return sqrtf(re * re + im * im + 1e-9f); }

// the block's magnitudes (in ac) straight into the mel GEMM as its B operand
template <int NMT>
__device__ __forceinline__ void mel_gemm_block(__amdgpu_buffer_rsrc_t rs_mel, int blk, int lane, const f32x16 (&ac)[2],
                                               f32x16 (&macc)[2][NMT]) {
  const unsigned moff = (unsigned)blk * (unsigned)(NMT * 4096);
#pragma unroll
  for (int mt = 0; mt < NMT; ++mt)
#pragma unroll
    for (int q = 0; q < 4; ++q) {
      const f32x4 w = rsrc_load16(rs_mel, lane * 16, moff + (unsigned)((mt * 4 + q) * 1024));
#pragma unroll
      for (int e = 0; e < 4; ++e) {
        macc[0][mt] = __builtin_amdgcn_mfma_f32_32x32x2f32(w[e], ac[0][4 * q + e], macc[0][mt], 0, 0, 0);
        macc[1][mt] = __builtin_amdgcn_mfma_f32_32x32x2f32(w[e], ac[1][4 * q + e], macc[1][mt], 0, 0, 0);
      }
    }
}

// the four waves' partial mels: (w0 + w2) + (w1 + w3), through 2 * mel_sum_floats<NMT>() floats of LDS that nothing else
// needs meanwhile.  Afterwards wave 0 reads the total of an element with mel_total().
template <int NMT>
constexpr int mel_sum_floats() { return 2 * NMT * 16 * 64; }

template <int NMT>
__device__ __forceinline__ void mel_sum_waves(float* scratch, int wave, int lane, f32x16 (&macc)[2][NMT]) {
  constexpr int PER_WAVE = mel_sum_floats<NMT>();
  __syncthreads();
  if (wave >= 2) {
    float* dst = scratch + (wave - 2) * PER_WAVE + lane;
#pragma unroll
    for (int t = 0; t < 2; ++t)
#pragma unroll
      for (int mt = 0; mt < NMT; ++mt)
#pragma unroll
        for (int r = 0; r < 16; ++r) dst[((t * NMT + mt) * 16 + r) * 64] = macc[t][mt][r];
  }
  __syncthreads();
  if (wave < 2) {
    const float* src = scratch + wave * PER_WAVE + lane;
#pragma unroll
    for (int t = 0; t < 2; ++t)
#pragma unroll
      for (int mt = 0; mt < NMT; ++mt)
#pragma unroll
        for (int r = 0; r < 16; ++r) macc[t][mt][r] += src[((t * NMT + mt) * 16 + r) * 64];
  }
  __syncthreads();
  if (wave == 1) {
    float* dst = scratch + lane;
#pragma unroll
    for (int t = 0; t < 2; ++t)
#pragma unroll
      for (int mt = 0; mt < NMT; ++mt)
#pragma unroll
        for (int r = 0; r < 16; ++r) dst[((t * NMT + mt) * 16 + r) * 64] = macc[t][mt][r];
  }
  __syncthreads();
}

// wave 0, after mel_sum_waves: the mel of row mt * 32 + (r & 3) + 8 (r >> 2) + 4 (lane >> 5), frame t * 32 + (lane & 31) of the tile
template <int NMT>
__device__ __forceinline__ float mel_total(const float* scratch, int lane, const f32x16 (&macc)[2][NMT], int t, int mt, int r) {
  return macc[t][mt][r] + scratch[lane + ((t * NMT + mt) * 16 + r) * 64];
}
#endif

}  // namespace dissc

struct dissc_mel {
  int sr, n_fft, num_mels, hop, win, pad;
  int b_lo, nblk, nmt, nchunk, j_lo, j_hi, rs, rows;
  size_t lds_bytes;
  std::vector<float> dft_host, melw_host;  // packed, uploaded by the first launch
  std::mutex mu;
  int device = -1;
  float* dft = nullptr;
  float* melw = nullptr;
  // the gradient's (mel_grad.hip): the same two bases packed transposed, uploaded by the first backward launch
  int s_lo, s_hi, srs;  // 32-sample slabs of the frame the window touches; LDS row stride of the overlap-add strip
  size_t grad_lds_bytes;
  std::vector<float> dftT_host, melT_host;
  float* dftT = nullptr;
  float* melT = nullptr;
};

namespace dissc {
int mel_upload(dissc_mel* h);  // mel.hip
__global__ void mel_l1_reduce_kernel(const MelArgs p, double* __restrict__ out);
void mel_fill(const dissc_mel* h, MelArgs& p);
inline int mel_max_tiles(const dissc_mel* h, int B, int Nmax) { return B * ((Nmax / h->hop + MEL_TF - 1) / MEL_TF); }
}  // namespace dissc
