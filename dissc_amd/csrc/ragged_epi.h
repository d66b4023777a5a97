// Pieces every conv / residual-pair kernel shares, written once: the ragged tile walk, the residual / MRF epilogue
// arithmetic and a few small helpers.  The bit-level guarantees (a ragged utterance is independent of its neighbours, fused
// pairs equal separate launches, small-grid tiers equal large ones, the MRF sums in the reference's order) rest on every
// kernel enumerating the same tiles and doing the same float ops in the same order, i.e. on calling these.
#pragma once
#include "common.h"

namespace dissc {

__device__ __forceinline__ float lrelu(float v, float slope) { return v > 0.f ? v : v * slope; }

constexpr int round32_16(int n) { return (n - 16 + 31) / 32 * 32 + 16; }  // smallest v >= n with v % 32 == 16

// host: the 16-byte vector accesses need 16-byte aligned rows
inline bool misaligned16(const void* q) { return (reinterpret_cast<uintptr_t>(q) & 15) != 0; }

// ---- ragged tile walk ---------------------------------------------------------------------------------------------------
// Workgroup `lin` of a ragged batch when only the tiles that EXIST are enumerated: utterance 0's ceil(len_0 / TW) tiles, then
// utterance 1's, ...  The workgroups beyond the last real tile all sit at the END of the dispatch order and return at once.
// (Enumerating (tile, utterance) pairs and returning from the tiles beyond an utterance's end leaves the empty workgroups
// between the real ones: 7-9 % on ragged batches for conv_wino_kernel, +0.65 ms per ragged forward for the pair stages.)
// Every wave finds its pair by a prefix sum of the tile counts over its lanes.  len_of(i): utterance i's length in the
// units TW counts.  false: no such tile; otherwise b (utterance), tile (index within it) and len, all wave-uniform.
template <int TW, class LenOf>
__device__ __forceinline__ bool ragged_tile(int lin, int nb, LenOf len_of, int& b, int& tile, int& len) {
  const int lane = threadIdx.x & 63;
  int base = 0, fb = -1, ft = 0, fl = 0;
  for (int b0 = 0; b0 < nb; b0 += 64) {
    const int l = b0 + lane < nb ? len_of(b0 + lane) : 0;
    const int nt = (l + TW - 1) / TW;
    int incl = nt;
#pragma unroll
    for (int o = 1; o < 64; o <<= 1) {
      const int v = __shfl_up(incl, o, 64);
      if (lane >= o) incl += v;
    }
    const int total = __shfl(incl, 63, 64);
    if (lin < base + total) {
      const unsigned long long m = __ballot(base + incl > lin);
      const int lb = __ffsll((long long)m) - 1;
      fb = b0 + lb;
      fl = __shfl(l, lb, 64);
      ft = lin - base - __shfl(incl - nt, lb, 64);
      break;
    }
    base += total;
  }
  // uniform by construction; say so after the loop (its exit depends on __shfl results, which look divergent to the
  // compiler, and with them every address derived from the tile: 64-bit per-lane address math instead of scalar bases)
  b = __builtin_amdgcn_readfirstlane(fb);
  tile = __builtin_amdgcn_readfirstlane(ft);
  len = __builtin_amdgcn_readfirstlane(fl);
  return b >= 0;
}

// Which tile is this workgroup's in conv_mfma32_kernel, lin128_kernel and conv2s128_kernel: b (utterance), bx (time tile of
// BN columns), by (group, M tile).  false: nothing to do.
template <int BN>
__device__ __forceinline__ bool conv_tile_of(const ConvArgs& a, int& b, int& bx, int& by) {
  b = blockIdx.z, bx = blockIdx.x, by = blockIdx.y;
  int ntile = gridDim.x, nb = gridDim.z;
  if (a.xcd) {
    // XCD order (1-D grid): the hardware deals workgroup ids round-robin over the 8 XCDs, each with its own 4 MB L2.
    // The ids are cut into SWEEPS over all time tiles, one per group of xcd_mg M tiles (weight slabs that fit the L2
    // together); inside a sweep the xcd_mg M tiles of one time tile -- which read the same input window -- take
    // consecutive slots of ONE XCD.  So a window crosses the fabric once per sweep (not once per M tile) and a weight
    // slab once per XCD (not once per utterance).
    const int mt = a.mt_per_group * a.groups, mg = a.xcd_mg;
    const int sweep = blockIdx.x / a.xcd_span, r = blockIdx.x - sweep * a.xcd_span;
    const int s = r >> 3, sq = s / mg;
    const int tt = (r & 7) + 8 * sq;
    by = sweep * mg + (s - sq * mg);
    ntile = a.xcd_ntile;
    nb = a.xcd_nb;
    if (tt >= ntile * nb || by >= mt) return false;
    b = tt / ntile;
    bx = tt - b * ntile;
  }
  if (a.ragged_enum) {
    // Ragged batch: only the (time tile, utterance) pairs that exist are enumerated (ragged_tile).  Not for
    // EPI_STORE_ACT, whose tiles beyond an utterance's end still have zero tails to write.
    int olen;
    const auto olen_of = [&](int i) {
      return a.lengths_out ? a.lengths_out[i]
                           : (a.olen_default >= 0 ? a.olen_default : (a.lengths ? a.lengths[i] * a.len_mul : a.len_default));
    };
    return ragged_tile<BN>(b * ntile + bx, nb, olen_of, b, bx, olen);
  }
  return true;
}

// ---- residual / MRF epilogue --------------------------------------------------------------------------------------------
// v = conv + bias (and whatever else the kernel applies first); each mode then stores, in this op order (the MRF sum is the
// reference's xs += resblock_j(x) ... x = xs / num_kernels):
//   EPI_STORE    out = v
//   EPI_RES      out = v + res
//   EPI_MRF_SET  acc = v + res
//   EPI_MRF_ADD  acc = acc + (v + res)
//   EPI_MRF_DIV  acc = (acc + (v + res)) / mrf_div
// on one element (T = float) or one float4 (T = f32x4).  res() and acc_old() fetch the residual and the accumulator's old
// value; they are called only in the modes that read them, where the mode reads them -- a kernel that fetched them early
// (before an exchange barrier) passes functions that return what it fetched.
__device__ __forceinline__ bool epi_rmw(int epi) { return epi == EPI_MRF_ADD || epi == EPI_MRF_DIV; }

__device__ __forceinline__ float epi_plus(float v, float r) { return v + r; }
__device__ __forceinline__ f32x4 epi_plus(f32x4 v, const f32x4& r) {
  v[0] += r[0]; v[1] += r[1]; v[2] += r[2]; v[3] += r[3];
  return v;
}

// the MRF half (EPI_MRF_ADD / EPI_MRF_DIV): x = conv + bias + residual -> the accumulator's new value
__device__ __forceinline__ float epi_mrf(int epi, float x, float ac, float mrf_div) {
  x = ac + x;
  if (epi == EPI_MRF_DIV) x = __fdiv_rn(x, mrf_div);
  return x;
}
__device__ __forceinline__ f32x4 epi_mrf(int epi, f32x4 x, const f32x4& ac, float mrf_div) {
  x[0] = ac[0] + x[0]; x[1] = ac[1] + x[1]; x[2] = ac[2] + x[2]; x[3] = ac[3] + x[3];
  if (epi == EPI_MRF_DIV) {
    x[0] = __fdiv_rn(x[0], mrf_div); x[1] = __fdiv_rn(x[1], mrf_div);
    x[2] = __fdiv_rn(x[2], mrf_div); x[3] = __fdiv_rn(x[3], mrf_div);
  }
  return x;
}

// every mode but EPI_STORE: x = conv + bias + residual
template <class T, class AccOld>
__device__ __forceinline__ void epi_store_res(int epi, T* out, T* acc, T x, AccOld acc_old, float mrf_div) {
  if (epi == EPI_RES) {
    *out = x;
  } else if (epi == EPI_MRF_SET) {
    *acc = x;
  } else {
    *acc = epi_mrf(epi, x, acc_old(), mrf_div);
  }
}

template <class T, class Res, class AccOld>
__device__ __forceinline__ void epi_store(int epi, T* out, T* acc, T v, Res res, AccOld acc_old, float mrf_div) {
  if (epi == EPI_STORE) {
    *out = v;
  } else {
    epi_store_res(epi, out, acc, epi_plus(v, res()), acc_old, mrf_div);
  }
}

__device__ __forceinline__ f32x4* quad_at(float* p) { return reinterpret_cast<f32x4*>(p); }
__device__ __forceinline__ f32x4 load_quad(const float* p) { return *reinterpret_cast<const f32x4*>(p); }

// elements idx .. idx+3 of a row, res and acc read here
__device__ __forceinline__ void epi_store4(int epi, float* out, float* acc, const float* res, size_t idx, f32x4 v, float mrf_div) {
  epi_store(epi, quad_at(out + idx), quad_at(acc + idx), v, [&] { return load_quad(res + idx); },
            [&] { return load_quad(acc + idx); }, mrf_div);
}

// element idx alone (a ragged tail), res and acc read here
__device__ __forceinline__ void epi_store1(int epi, float* out, float* acc, const float* res, size_t idx, float v, float mrf_div) {
  epi_store(epi, out + idx, acc + idx, v, [&] { return res[idx]; }, [&] { return acc[idx]; }, mrf_div);
}

}  // namespace dissc
