// The split-bf16 ("bf16x3") half of the differentiable stride-1 Conv1d (conv_grad.hip; dissc_convgrad_create_prec, prec = 1):
// the weight gradient on the bf16 matrix cores, and the device-side packing of conv_bf3_kernel's weight fragments.  The forward
// and the data gradient of such a handle are conv_bf3_kernel launches (conv_bf3.hip); plan, partials, reduction and the bias
// gradient are the fp32 layer's (conv_grad.h).
//
//   gw[co][ci][j] = sum_b sum_{t < len_b} gy[b][co][t] lrelu(x)[b][ci][t + off_j]
//
// on v_mfma_f32_32x32x16_bf16: rows = 32 output channels, columns = 32 input channels, the MFMA's k axis = 16 time positions,
// one accumulator per tap.  Every fp32 operand v is split once, when it is staged, into hi = bf16(v), lo = bf16(v - hi), and
// every product is the three MFMAs hi*hi, hi*lo, lo*hi, in that order, accumulated in fp32.
//   * Chunks of CG_T = 64 positions, dealt to P partials by cg_plan, as the fp32 kernel: the same WgradArgs, the same partial
//     layout [P * WT][Cout][Cin][K], summed by convgrad_reduce_kernel.  Cin >= 32 only (cg_wgrad_bf3_takes): one tap per
//     accumulator, no tap packing.
//   * A = gy tiles at aligned times: an LDS image [co][t] of bf16, hi and lo planes, rows of 144 bytes (16 consecutive rows
//     start 36 banks apart: a ds_read_b128 of one fragment is conflict-free).  Read once per 16-position step, outside the
//     tap loop.
//   * B = lrelu(x) at t + off_j, off_j arbitrary.  The window is stored TIME-MAJOR, [32-channel block][hi | lo][t][32 ci] bf16 with
//     64-byte rows, so a tap is a whole-row offset and a fragment (8 consecutive times of one channel per lane) is two
//     ds_read_b64_tr_b16.  A 32-lane half reads 4 consecutive rows x 64 bytes = 256 contiguous bytes: all 64 banks once, at
//     any row offset.  Every lane's address is 8-byte aligned.  The transposed read needs EXEC all ones: every branch around
//     it is uniform over the workgroup, and a wave whose channel block lies beyond Cin, like a step beyond the utterance's
//     end, reads rows staged as zeros (pad, don't mask) and is not stored.
//   * Staging: a thread loads f32x4 along time for 4 adjacent channels, applies the ragged zeroing and the leaky ReLU, splits,
//     and writes four 8-byte stores per plane (the transpose, once per chunk).  Lanes of one store instruction that differ in
//     the time quad write different times of their quads (quad q's instruction i holds time (i + q) & 3), so the 32 lanes of a
//     half cover 256 distinct bytes instead of one 64-byte row four times.
//   * The next pair's global loads are issued into registers before the current pair's MFMAs where the registers allow it
//     (up to WB_PF_MAX_NG accumulators; 72 staging registers beside 16 per tap); with more taps a unit is loaded and stored
//     at once, with no overlap, as the fp32 kernel stages.
#include "conv_grad.h"

namespace dissc {

typedef __bf16 wb_bf16x8 __attribute__((ext_vector_type(8)));
typedef short wb_s16x4 __attribute__((ext_vector_type(4)));
typedef short wb_s16x8 __attribute__((ext_vector_type(8)));
typedef unsigned int wb_u32x2 __attribute__((ext_vector_type(2)));

constexpr int WB_GY_LD = 2 * CG_T + 16;     // bytes of a gy row
constexpr int WB_GY_PLANE = 32 * WB_GY_LD;  // bytes of one plane of the gy image
constexpr int WB_X0 = 2 * WB_GY_PLANE;      // the x image starts here (a multiple of 256)
constexpr int WB_ROW = 64;                  // bytes of a row of the x image: 32 channels
constexpr int WB_MAX_HALO = 32;             // (MAX_TAP_SPAN / 2, rounded up to 8)
constexpr int WB_XU = 4;                    // x units of a thread: 4 WCI x 2 (CG_T + 2 WB_MAX_HALO) / 256
constexpr int WB_PF_MAX_NG = 4;             // prefetch behind the MFMAs up to this many accumulators
static_assert(WB_X0 % 256 == 0, "x rows keep their bank phase");
static_assert(WB_X0 + 4 * 2 * (CG_T + 2 * WB_MAX_HALO) * WB_ROW <= 80 * 1024, "two workgroups per CU");

// four values -> their hi halves and their lo halves, each packed into 8 bytes
__device__ __forceinline__ void wb_split4(const float (&v)[4], wb_u32x2& hi, wb_u32x2& lo) {
  unsigned short hb[4], lb[4];
#pragma unroll
  for (int c = 0; c < 4; ++c) {
    const __bf16 hv = (__bf16)v[c];
    hb[c] = __builtin_bit_cast(unsigned short, hv);
    lb[c] = __builtin_bit_cast(unsigned short, (__bf16)(v[c] - (float)hv));
  }
  hi = wb_u32x2{(unsigned)hb[0] | ((unsigned)hb[1] << 16), (unsigned)hb[2] | ((unsigned)hb[3] << 16)};
  lo = wb_u32x2{(unsigned)lb[0] | ((unsigned)lb[1] << 16), (unsigned)lb[2] | ((unsigned)lb[3] << 16)};
}

__device__ __forceinline__ wb_bf16x8 wb_read_tr(const unsigned char* p) {  // rows p, p + 4 rows: 8 times of this lane's channel
  typedef wb_s16x4 __attribute__((address_space(3))) * lds_ptr;
  const wb_s16x4 r0 = __builtin_amdgcn_ds_read_tr16_b64_v4i16((lds_ptr)(p));
  const wb_s16x4 r1 = __builtin_amdgcn_ds_read_tr16_b64_v4i16((lds_ptr)(p + 4 * WB_ROW));
  return __builtin_bit_cast(wb_bf16x8, __builtin_shufflevector(r0, r1, 0, 1, 2, 3, 4, 5, 6, 7));
}

template <int NG, bool PF>
__global__ void __launch_bounds__(256, 2) convgrad_wgrad_bf3_kernel(WgradArgs a) {
  extern __shared__ __attribute__((aligned(16))) unsigned char wb_lds[];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int l31 = lane & 31, h = lane >> 5;
  const int wsh = a.WCI == 4 ? 2 : (a.WCI == 2 ? 1 : 0);
  const int wci = wave & (a.WCI - 1), wt = wave >> wsh;
  const int co0 = blockIdx.x * 32, ci0 = blockIdx.y * 32 * a.WCI;
  const int W = CG_T + 2 * a.halo;    // rows of the x image (a.halo % 8 == 0: W % 16 == 0)
  const int plane = W * WB_ROW;       // bytes of one plane of one channel block
  const int nunit = a.WCI * 2 * W;    // (W / 4 time quads) x (8 WCI channel quads)
  const long long npair = (long long)a.B * a.nch;
  const long long q0 = (long long)blockIdx.z * a.cpp, q1 = q0 + a.cpp < npair ? q0 + a.cpp : npair;

  cg_f32x16 acc[NG];
#pragma unroll
  for (int g = 0; g < NG; ++g)
#pragma unroll
    for (int e = 0; e < 16; ++e) acc[g][e] = 0.f;

  // the first pair at or after q that has positions (the rest of an utterance past its length is skipped at once), or q1
  auto seek = [&](long long q, int& b, int& t0, int& len) -> long long {
    while (q < q1) {
      b = (int)(q / a.nch);
      t0 = (int)(q - (long long)b * a.nch) * CG_T;
      len = a.lengths ? a.lengths[b] : a.Lmax;
      len = len < 0 ? 0 : (len > a.Lmax ? a.Lmax : len);
      if (t0 < len) return q;
      q = (long long)(b + 1) * a.nch;
    }
    return q1;
  };

  // staging, a unit at a time: gy unit i = one quad of a row (2 per thread), x unit i = one time quad of 4 adjacent channels
  auto load_gy = [&](int i, int b, int t0, int len, f32x4& g4) {
    const int e = tid + i * 256, r = e >> 4, t = t0 + 4 * (e & 15);
    g4 = f32x4{0.f, 0.f, 0.f, 0.f};
    if (t < len && co0 + r < a.Cout) g4 = *reinterpret_cast<const f32x4*>(a.gy + ((size_t)b * a.Cout + co0 + r) * a.ldo + t);
  };
  auto load_x = [&](int i, int b, int t0, int len, f32x4 (&x4)[4]) {
    const int u = tid + i * 256;
    const int cq = (u >> 2) & 7, rest = u >> 5, blk = rest & (a.WCI - 1), tq = 4 * (rest >> wsh) + (u & 3);
    const int t = t0 - a.halo + 4 * tq;
#pragma unroll
    for (int c = 0; c < 4; ++c) {
      const int ci = ci0 + blk * 32 + 4 * cq + c;
      x4[c] = f32x4{0.f, 0.f, 0.f, 0.f};
      if (u < nunit && t >= 0 && t < len && ci < a.Cin) x4[c] = *reinterpret_cast<const f32x4*>(a.x + ((size_t)b * a.Cin + ci) * a.ldx + t);
    }
  };
  auto store_gy = [&](int i, int t0, int len, const f32x4& g4) {
    const int e = tid + i * 256, r = e >> 4, v = e & 15, t = t0 + 4 * v;
    float g[4];
#pragma unroll
    for (int qq = 0; qq < 4; ++qq) g[qq] = (t + qq < len) ? g4[qq] : 0.f;
    wb_u32x2 hi, lo;
    wb_split4(g, hi, lo);
    unsigned char* p = wb_lds + r * WB_GY_LD + v * 8;
    *reinterpret_cast<wb_u32x2*>(p) = hi;
    *reinterpret_cast<wb_u32x2*>(p + WB_GY_PLANE) = lo;
  };
  auto store_x = [&](int i, int t0, int len, const f32x4 (&x4)[4]) {
    const int u = tid + i * 256;
    if (u >= nunit) return;
    const int rot = u & 3, cq = (u >> 2) & 7, rest = u >> 5, blk = rest & (a.WCI - 1), tq = 4 * (rest >> wsh) + rot;
    const int t = t0 - a.halo + 4 * tq;
    wb_u32x2 ph[4], pl[4];  // [time of the quad]: 4 channels, hi and lo
#pragma unroll
    for (int tt = 0; tt < 4; ++tt) {
      float v[4];
#pragma unroll
      for (int c = 0; c < 4; ++c) {
        const float xv = x4[c][tt];
        v[c] = (t + tt < len) ? (xv > 0.f ? xv : xv * a.slope) : 0.f;  // (t < 0, ci >= Cin: loaded as zero)
      }
      wb_split4(v, ph[tt], pl[tt]);
    }
    unsigned char* xb = wb_lds + WB_X0 + blk * 2 * plane + 4 * tq * WB_ROW + cq * 8;
#pragma unroll
    for (int j = 0; j < 4; ++j) {  // store j of quad tq holds time (j + tq) & 3: see the head of the file
      wb_u32x2 sh = ph[j], sl = pl[j];
#pragma unroll
      for (int r = 1; r < 4; ++r) {
        sh = rot == r ? ph[(j + r) & 3] : sh;
        sl = rot == r ? pl[(j + r) & 3] : sl;
      }
      unsigned char* p = xb + ((j + rot) & 3) * WB_ROW;
      *reinterpret_cast<wb_u32x2*>(p) = sh;
      *reinterpret_cast<wb_u32x2*>(p + plane) = sl;
    }
  };
  constexpr int NPF = PF ? WB_XU : 1;  // without the prefetch a unit is loaded and stored at once ...
  constexpr int WB_UNROLL = NG >= 10 ? 1 : WB_XU;  // ... and beside 160 accumulator registers or more, one unit after the other
  f32x4 gr[2], xr[NPF][4];
  auto stage_load = [&](int b, int t0, int len) {
#pragma unroll
    for (int i = 0; i < 2; ++i) load_gy(i, b, t0, len, gr[i]);
#pragma unroll
    for (int i = 0; i < NPF; ++i) load_x(i, b, t0, len, xr[i]);
  };
  auto stage_store = [&](int b, int t0, int len) {
    if (PF) {
#pragma unroll
      for (int i = 0; i < 2; ++i) store_gy(i, t0, len, gr[i]);
#pragma unroll
      for (int i = 0; i < NPF; ++i) store_x(i, t0, len, xr[i]);
    } else {
      stage_load(b, t0, len);  // gy and the first x unit
#pragma unroll
      for (int i = 0; i < 2; ++i) store_gy(i, t0, len, gr[i]);
#pragma unroll(WB_UNROLL)
      for (int i = 0; i * 256 < nunit; ++i) {
        if (i) load_x(i, b, t0, len, xr[0]);
        store_x(i, t0, len, xr[0]);
      }
    }
  };

  // A: gy[co = l31][t0 + 16 s + 8 h ..+7].  B: lane 16 grp + 4 q + p supplies row q, channels 16 (grp & 1) + 4 p ..+3 of the block
  // of 4 rows at time 8 (grp >> 1) (+ 4 for the second read), and receives channel (lane & 31), 8 times: the operand's own map.
  const unsigned char* ap = wb_lds + l31 * WB_GY_LD + h * 16;
  const int grp = lane >> 4, i16 = lane & 15;
  const unsigned char* bp = wb_lds + WB_X0 + wci * 2 * plane + (a.halo + a.off0 + 8 * (grp >> 1) + (i16 >> 2)) * WB_ROW +
                            (16 * (grp & 1) + 4 * (i16 & 3)) * 2;
  const int tapb = a.dstep * WB_ROW;
  const int spw = 4 >> (2 - wsh);  // 16-position steps per time slice: 4 / WT
  const int s0 = wt * spw;

  int b, t0, len;
  long long q = seek(q0, b, t0, len);
  if (PF && q < q1) stage_load(b, t0, len);
  while (q < q1) {  // uniform over the workgroup
    __syncthreads();
    stage_store(b, t0, len);
    __syncthreads();
    int bn = 0, t0n = 0, lenn = 0;
    const long long qn = seek(q + 1, bn, t0n, lenn);
    if (PF && qn < q1) {
      stage_load(bn, t0n, lenn);
      __builtin_amdgcn_sched_barrier(0);  // the loads stay ahead of the MFMAs
    }
    for (int si = 0; si < spw; ++si) {  // (a trip count the compiler sees as uniform: EXEC stays whole)
      const int s = s0 + si;
      const wb_bf16x8 ah = *reinterpret_cast<const wb_bf16x8*>(ap + s * 32);
      const wb_bf16x8 al = *reinterpret_cast<const wb_bf16x8*>(ap + s * 32 + WB_GY_PLANE);
      int so = s * 16 * WB_ROW;
      asm volatile("" : "+v"(so));  // opaque: the per-tap addresses are formed in the step, not kept across steps (2 registers a tap)
      const unsigned char* bs = bp + so;
      // the next tap's fragments are read behind this tap's MFMAs, one tap ahead and no further: left alone, the scheduler
      // hoists every tap's reads to the top of the step, 16 registers a tap
      // (a running address: one register, not one per tap and plane)
      wb_bf16x8 bh = wb_read_tr(bs), bl = wb_read_tr(bs + plane);
#pragma unroll
      for (int g = 0; g < NG; ++g) {
        wb_bf16x8 bhn = bh, bln = bl;
        if (g + 1 < NG) {
          bs += tapb;
          bhn = wb_read_tr(bs);
          bln = wb_read_tr(bs + plane);
        }
        __builtin_amdgcn_sched_barrier(0);
        acc[g] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(ah, bh, acc[g], 0, 0, 0);
        acc[g] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(ah, bl, acc[g], 0, 0, 0);
        acc[g] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(al, bh, acc[g], 0, 0, 0);
        __builtin_amdgcn_sched_barrier(0);
        bh = bhn; bl = bln;
      }
    }
    q = qn; b = bn; t0 = t0n; len = lenn;
  }

  const int ci = ci0 + wci * 32 + l31;
  if (ci >= a.Cin) return;
  float* pbase = a.part + (size_t)(blockIdx.z * a.WT + wt) * a.Cout * a.Cin * a.K;
#pragma unroll
  for (int g = 0; g < NG; ++g) {
#pragma unroll
    for (int r = 0; r < 16; ++r) {
      const int co = co0 + (r & 3) + 8 * (r >> 2) + 4 * h;
      if (co < a.Cout) pbase[((size_t)co * a.Cin + ci) * a.K + g] = acc[g][r];
    }
  }
}

// master weights [Cout][Cin][K] -> [32-row tile][chunk * K + tap][hi | lo][lane] x 8 bf16, lane l, element e ->
// W[32 ms + (l & 31)][KC chunk + 8 (l >> 5) + e][tap]: pack_conv_weights_bf3's order, its rounding (f32_to_bf16_rne; weights are
// finite) done in integers.  transposed = the data gradient's conv: rows = input channels, columns = output channels, taps flipped.
__device__ __forceinline__ unsigned wb_rne(float f) {
  unsigned u = __builtin_bit_cast(unsigned, f);
  u += 0x7fffu + ((u >> 16) & 1u);
  return u >> 16;
}

__global__ void __launch_bounds__(256) convgrad_repack_bf3_kernel(const float* __restrict__ w, int Cout, int Cin, int K, int nsub,
                                                                  int nchunk, int transposed, unsigned short* __restrict__ packed) {
  const size_t idx = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  const size_t total = (size_t)nsub * nchunk * K * 512;
  if (idx >= total) return;
  const int e = idx & 7, lane = (idx >> 3) & 63;
  size_t r = idx >> 9;  // step of a tile
  const int j = (int)(r % K);
  const int c = (int)((r / K) % nchunk), ms = (int)(r / K / nchunk);
  const int row = ms * 32 + (lane & 31), col = c * KC + 8 * (lane >> 5) + e;
  float v = 0.f;
  if (!transposed) {
    if (row < Cout && col < Cin) v = w[((size_t)row * Cin + col) * K + j];
  } else {
    if (row < Cin && col < Cout) v = w[((size_t)col * Cin + row) * K + (K - 1 - j)];
  }
  const unsigned hi = wb_rne(v);
  const unsigned lo = wb_rne(v - __builtin_bit_cast(float, hi << 16));
  const size_t slot = (r * 2) * 64 + lane;
  packed[slot * 8 + e] = (unsigned short)hi;
  packed[(slot + 64) * 8 + e] = (unsigned short)lo;
}

bool cg_wgrad_bf3_takes(int prec, int Cin, int Cout, int K, int dil) {
  return prec == 1 && Cin >= 32 && Cout >= 32 && (K - 1) * dil <= MAX_TAP_SPAN;
}

template <int NG>
static int wb_launch(const WgradArgs& a, const CgPlan& p, hipStream_t st) {
  constexpr bool PF = NG <= WB_PF_MAX_NG;
  const size_t lds = (size_t)WB_X0 + (size_t)p.WCI * 2 * (CG_T + 2 * a.halo) * WB_ROW;
  static DeviceOnce attr_once;  // per device (common.h)
  DISSC_HIP_CHECK(attr_once.max_lds(reinterpret_cast<const void*>(&convgrad_wgrad_bf3_kernel<NG, PF>), 80 * 1024));
  hipLaunchKernelGGL((convgrad_wgrad_bf3_kernel<NG, PF>), dim3(p.coT, p.ciS, p.P), dim3(256), lds, st, a);
  return DISSC_OK;
}

int cg_launch_wgrad_bf3(const WgradArgs& a0, const CgPlan& p, hipStream_t st) {
  const char* who = "dissc_convgrad_backward";
  WgradArgs a = a0;
  a.halo = (a0.halo + 7) & ~7;  // whole groups of four time quads
  if (p.TS != 1 || p.NG != a.K || a.halo > WB_MAX_HALO || p.WCI * 2 * (CG_T + 2 * a.halo) > 256 * WB_XU) {
    set_error("%s: no split-bf16 weight gradient for %d -> %d channels, %d taps, halo %d", who, a.Cin, a.Cout, a.K, a0.halo);
    return DISSC_EINVAL;
  }
  return cg_dispatch_ng(p.NG, who, "taps", [&](auto ng) { return wb_launch<decltype(ng)::value>(a, p, st); });
}

void cg_launch_repack_bf3(const float* w, int Cout, int Cin, int K, int nsub, int nchunk, int transposed, float* packed,
                          hipStream_t st) {
  const size_t n = (size_t)nsub * nchunk * K * 512;
  hipLaunchKernelGGL(convgrad_repack_bf3_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, st, w, Cout, Cin, K, nsub, nchunk,
                     transposed, reinterpret_cast<unsigned short*>(packed));
}

}  // namespace dissc
