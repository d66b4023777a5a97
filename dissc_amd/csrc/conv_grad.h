// What the three differentiable conv layers share (conv_grad.hip: the stride-1 Conv1d; conv_grad_t.hip: ConvTranspose1d;
// conv_grad_s.hip: the strided Conv1d): the partial plan of the weight gradient, the fixed-order sum over its partials, the bias
// gradient, the (plane, shift) table of a strided layer's taps, and the host side of a layer handle (base, argument checks, the
// backward's workspace layout, the tap-group dispatch).  Defined in conv_grad.hip.
#pragma once
#include <algorithm>
#include <cstdlib>
#include <type_traits>

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

// The two strided layers are phrased on the s phase planes of their long side, plane_p[c][q] = long[c][s q + p]: tap kk reads
// long[s t + kk - pad] = plane_p[t + dl] with kk - pad = s dl + p, 0 <= p < s (ConvTranspose1d: pad = (k - s) / 2, the long side
// is y / gy; strided Conv1d: pad = (k - 1) / 2, the long side is x).
constexpr int CT_MAX_S = 8;
struct CtTaps {
  int p[CG_MAX_K], dl[CG_MAX_K];  // tap kk reads plane p[kk] at t + dl[kk]
  int halo;                       // >= every |dl|, multiple of 4
};
inline CtTaps ct_taps(int k, int s, int pad) {
  CtTaps t;
  int m = 0;
  for (int kk = 0; kk < CG_MAX_K; ++kk) {
    const int o = (kk < k ? kk : k - 1) - pad;
    t.p[kk] = ((o % s) + s) % s;
    t.dl[kk] = (o - t.p[kk]) / s;  // exact
    m = std::max(m, std::abs(t.dl[kk]));
  }
  t.halo = (m + 3) & ~3;
  return t;
}

// one launch of the stride-1 weight gradient (conv_grad.hip's fp32 kernel, conv_grad_bf3.hip's split-bf16 one)
struct WgradArgs {
  const float* gy;   // [B][Cout][ldo]
  const float* x;    // [B][Cin][ldx], before the activation
  const int32_t* lengths;
  float* part;       // [P * WT][Cout][Cin][K]
  int B, Cout, Cin, K, Lmax, ldo, ldx;
  int off0, dstep;   // tap j reads x[t + off0 + j * dstep]
  int halo;          // LDS window = [t0 - halo, t0 + CG_T + halo), halo % 4 == 0, >= every |tap offset|
  float slope;
  int WCI, WT, CIB, TS, nch, cpp;
};

// The split-bf16 weight gradient (conv_grad_bf3.hip).  cg_wgrad_bf3_takes: whether a handle of precision `prec` runs its weight
// gradient there -- what dissc_convgrad_backward dispatches on and dissc_convgrad_precision_info reports.  The launch takes the
// fp32 kernel's arguments and plan (same chunks, same partials, same partial layout) and rounds a.halo up itself.
bool cg_wgrad_bf3_takes(int prec, int Cin, int Cout, int K, int dil);
int cg_launch_wgrad_bf3(const WgradArgs& a, const CgPlan& p, hipStream_t st);
// master weights [Cout][Cin][K] -> conv_bf3_kernel's A fragments (pack_conv_weights_bf3's order) of a layer of nsub 32-row
// tiles; transposed: the data gradient's conv (rows = input channels, taps flipped)
void cg_launch_repack_bf3(const float* w, int Cout, int Cin, int K, int nsub, int nchunk, int transposed, float* packed,
                          hipStream_t st);

// out[i] = sum over the NP partials part[p][i], i < n, in a fixed order
void cg_launch_reduce(const float* part, int NP, size_t n, float* out, hipStream_t st);
// gb[co] = sum_b sum_{t < min(ceil(lengths[b] * len_mul / len_div), Lmax)} gy[b][co][t], in double; bpart: B * Cout doubles of
// workspace.  Lmax: positions of gy
void cg_launch_bias(const float* gy, const int32_t* lengths, int len_mul, int B, int Cout, int Lmax, int ldo, double* bpart,
                    float* gb, hipStream_t st, int len_div = 1);

// ---- the host side of a layer handle; `who` is the C entry that was called: every message starts with it ----
struct CgLayer {  // the base of dissc_convgrad, dissc_convtgrad and dissc_convsgrad
  Options opt;  // this handle's snapshot of the tuning options (common.h)
  int Cin = 0, Cout = 0, k = 0;
  bool ready = false;  // device buffers allocated (the first set_weights)
};

// create: the out pointer and the channel range; kernel size, dilation and stride rules are each layer's own
int cg_check_create(const char* who, const void* out, int Cin, int Cout);
// a call on a handle: the arguments; then, with len_mul > 0 (1, or the stride: a row of y / gy holds len_mul * Lmax; with
// len_div = the stride of a strided Conv1d: ceil(Lmax / len_div)), the row strides and "set_weights first"
int cg_check_call(const CgLayer* h, const char* who, int B, int Lmax, int len_mul = 0, int ldx = 0, int ldo = 0, int len_div = 1);

// the backward's workspace behind its 256-byte aligned base: partials at 0, the bias gradient's doubles at `bpart`; `bytes` is
// what *_workspace_bytes promises
struct CgWorkspace {
  size_t bpart, bytes;
};
CgWorkspace cg_workspace(const CgPlan& p, int B, int Cout);
// the backward's preamble: x, gy and gx 16-byte aligned, the workspace as large as promised where gw or gb is wanted; carves it
int cg_backward_begin(const char* who, const CgPlan& p, int B, int Cout, const float* x, const float* gy, const float* gx,
                      bool wants_wb, void* workspace, size_t workspace_bytes, float** part, double** bpart);

// launch(std::integral_constant<int, NG>) for NG in 1 .. CG_MAX_K; `unit` names what NG counts in the refusal of any other
template <class F>
int cg_dispatch_ng(int NG, const char* who, const char* unit, F&& launch) {
  static_assert(CG_MAX_K == 11, "one case per tap-group count up to CG_MAX_K");
  switch (NG) {
#define CG_CASE(n) case n: return launch(std::integral_constant<int, n>());
    CG_CASE(1) CG_CASE(2) CG_CASE(3) CG_CASE(4) CG_CASE(5) CG_CASE(6) CG_CASE(7) CG_CASE(8) CG_CASE(9) CG_CASE(10) CG_CASE(11)
#undef CG_CASE
  }
  set_error("%s: %d %s", who, NG, unit);
  return DISSC_EINVAL;
}

// set_weights' allocation of one direct conv: the zeros uploaded are the packing's padding (weights never leave the device); a
// packing the device-side repack does not write is refused (prec = 1: conv_bf3_kernel's split-bf16 fragments are admitted)
int cg_alloc_conv(const char* who, int rows, int cols, int taps, int dil, int pad_left, DevConv& dc, int prec = 0);

}  // namespace dissc
