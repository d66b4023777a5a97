// Shared by respair_f23.hip (C = 32) and respair16_f23.hip (C = 16): the register-only Toom-Cook residual pairs, F(2,3) on four
// points and F(3,4) on six.
#pragma once
#include "common.h"
#include "ragged_epi.h"

namespace dissc {

struct PairFArgs {
  const float* x;
  float* out;
  float* acc;
  const float* w1;  // [chunk 2][sub-filter 4][point 4][half 2][64 lanes][4 k-steps]
  const float* w2;
  const float* b1;
  const float* b2;
  const int32_t* lengths;
  int len_default, len_mul;
  int ld;
  long long bstride;
  float slope, mrf_div;
  int epi;
  int dbg;  // diagnostics ("kernel_dbg" option): knock-outs -- bit 0 the tap loops, 1 the T epilogue, 2 the output epilogue,
            // 3 (six-point kernel) the weight stream: every step loads the first step's 6 KB
};

// (b, len, first output column) of workgroup (blockIdx.x: tile, blockIdx.y: utterance), as respair.hip's pair_tile
template <int WOUT>
__device__ __forceinline__ bool f23_tile(const PairFArgs& a, int B, int& b, int& len, int& o0) {
  if (a.lengths == nullptr) {
    b = blockIdx.y;
    len = a.len_default;
    o0 = blockIdx.x * WOUT;
    return o0 < len;
  }
  int tile;
  if (!ragged_tile<WOUT>(blockIdx.y * gridDim.x + blockIdx.x, B, [&](int i) { return a.lengths[i] * a.len_mul; }, b, tile, len))
    return false;
  o0 = tile * WOUT;
  return true;
}

// F(2,3) weight transform at the points 0, 1, -1, inf (host, double)
static const double kF23G[4][3] = {{1.0, 0.0, 0.0}, {0.5, 0.5, 0.5}, {0.5, -0.5, 0.5}, {0.0, 0.0, 1.0}};

// F(3,4) weight transform at the points 0, 1, -1, 2, -2, inf (host, double)
static const double kTc6G[6][4] = {{1.0 / 4, 0.0, 0.0, 0.0},
                                   {-1.0 / 6, -1.0 / 6, -1.0 / 6, -1.0 / 6},
                                   {-1.0 / 6, 1.0 / 6, -1.0 / 6, 1.0 / 6},
                                   {1.0 / 24, 2.0 / 24, 4.0 / 24, 8.0 / 24},
                                   {1.0 / 24, -2.0 / 24, 4.0 / 24, -8.0 / 24},
                                   {0.0, 0.0, 0.0, 1.0}};

// respair16_f23.hip
int pack_pair16_f23(const float* w, float** dev, int KS);
int launch_pair16_f23(const PairFArgs& a, int KS, int dil, int B, int Lmax, hipStream_t stream);

}  // namespace dissc
