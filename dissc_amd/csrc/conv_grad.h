// What the two differentiable conv layers share (conv_grad.hip: the stride-1 Conv1d; conv_grad_t.hip: ConvTranspose1d): the
// partial plan of the weight gradient, the fixed-order sum over its partials and the bias gradient.  Defined in conv_grad.hip.
#pragma once
#include "common.h"

namespace dissc {

constexpr int CG_T = DISSC_CONVGRAD_CHUNK;  // positions per chunk
constexpr int CG_MAX_K = 11;
typedef float cg_f32x16 __attribute__((ext_vector_type(16)));

struct CgPlan {
  int WCI, WT;    // waves of a workgroup: WCI blocks of 32 input channels x WT time slices of a chunk
  int CIB, TS;    // B columns: TS taps x CIB channels (CIB = 32: one tap)
  int NG;         // tap groups = accumulators per wave
  int coT, ciS;   // output tiles, input super-blocks (grid x, y)
  int nch;        // chunks per utterance
  int P, cpp;     // partials per output tile (grid z), (utterance, chunk) pairs per partial
  size_t gw;      // floats of one gradient
};
// a function of the shape only, never of lengths; Lmax in the units the chunks are cut in
CgPlan cg_plan(int Cin, int Cout, int K, int B, int Lmax);

inline size_t cg_rup(size_t x, size_t m) { return (x + m - 1) / m * m; }

// out[i] = sum over the NP partials part[p][i], i < n, in a fixed order
void cg_launch_reduce(const float* part, int NP, size_t n, float* out, hipStream_t st);
// gb[co] = sum_b sum_{t < min(lengths[b] * len_mul, Lmax)} gy[b][co][t], in double; bpart: B * Cout doubles of workspace
void cg_launch_bias(const float* gy, const int32_t* lengths, int len_mul, int B, int Cout, int Lmax, int ldo, double* bpart,
                    float* gb, hipStream_t st);

}  // namespace dissc
