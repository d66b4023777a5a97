// enc_bf3_kernel: the HuBERT encoder's matrix-pipe-bound layers in split-bf16 ("bf16x3") arithmetic, for handles created with
// enc_precision = 1 (dissc_hubert_create_ex).  fp32 handles never come here.
//
// Two shapes, one kernel:
//   STRIDE 1: 1x1 convs, i.e. the linears (post_extract_proj, qkv, out_proj, fc1, fc2), epilogues bias / bias + GELU / bias + residual;
//   STRIDE 2: the VALID feature convs conv1..conv6 (k = 3 and k = 2), GELU epilogue.
// The arithmetic and the operand layout are conv_bf3_kernel's (conv_bf3.hip): weights split ONCE on the host into bf16 hi / lo
// planes in A-fragment order (pack_conv_weights_bf3), activations split ONCE per staged value when the prefetched registers are
// written to LDS, products lo*hi, hi*lo, hi*hi into one fp32 accumulator of v_mfma_f32_32x32x16_bf16.  Activations stay fp32
// [B][C][ld] in HBM; bias, GELU and residual are the fp32 epilogue of the other 32-row kernels (conv_epilogue32).
//
// What differs from conv_bf3_kernel:
//   * stride 2: even and odd input positions go to SEPARATE planes at the staging store -- [channel octet][hi|lo][parity][column]
//     x 8 bf16 -- so that tap j of output column l is plane parity j & 1, column l + (j >> 1): a B fragment (8 consecutive channels
//     of one input position) stays one conflict-free ds_read_b128 and the tap loop moves no data;
//   * staging is spread over the WHOLE workgroup: slot = (chunk, channel octet, output column), the slots dealt round the
//     threads (stride 2: the two input positions under that column, + one more column for the third tap), 8 coalesced loads and
//     8 * STRIDE splits per slot.  conv_bf3_kernel gives the whole window to its first 2 * XW / 4 threads; with one tap per chunk
//     there are only 24 MFMAs to hide a wave's staging behind, and vector-ALU work is paid in matrix-pipe time on this part;
//   * the weight fragments are fetched two steps ahead and the linears stage four chunks per barrier (see the kernel);
//   * the A fragments come through a wave-uniform buffer descriptor (wave_rsrc, common.h);
//   * tiles are enumerated by the shared ragged walk in XCD order (conv_tile_of), like the fp32 kernels these layers leave.
// Every output element sees the same MFMA sequence over (chunk, tap) whatever the tile shape or its place in the batch, so an
// utterance's result does not depend on the batch it runs in (the guarantee of the fp32 path).
#include "common.h"
#include "conv_epilogue32.h"

namespace dissc {

typedef __bf16 bf16x8 __attribute__((ext_vector_type(8)));

constexpr int enc_bf3_xw(int BN) { return BN + 4; }  // columns per LDS plane: BN (+ 1 for the third tap of a stride-2 conv)

// CPB: 16-channel chunks staged per barrier.  DEPTH: weight-fragment steps in registers (DEPTH - 1 of them in flight).
// One step (16 channels x one tap) is only 3 MI NI MFMAs of 32 cycles: a load issued one step ahead has not come back from the
// L2 when its MFMAs are due.  So the A fragments are fetched DEPTH - 1 steps ahead into statically indexed register slots (the
// step loop is unrolled by DEPTH: no register rotation, which would wait for the youngest load), and the linears, whose chunk
// is a single step, stage CPB = 4 chunks per barrier, so that the next group's activations have four steps to arrive.
template <int MI, int NI, int WM, int WN, int STRIDE, int CPB, int DEPTH>
__global__ void __launch_bounds__(64 * WM * WN, 2) enc_bf3_kernel(const ConvArgs a) {
  constexpr int NT = 64 * WM * WN;
  constexpr int BN = 32 * NI * WN;
  constexpr int XW = enc_bf3_xw(BN);
  constexpr int NCOL = BN + (STRIDE == 2 ? 1 : 0);   // staged columns (of STRIDE input positions each)
  constexpr int NSLOT = CPB * 2 * NCOL;              // (chunk, channel octet, column)
  constexpr int NS = (NSLOT + NT - 1) / NT;          // staging slots per thread
  constexpr int CHK = 4 * STRIDE * XW;               // one staged chunk, in 16-byte units
  constexpr int BUF = CPB * CHK;                     // one buffer
  extern __shared__ __attribute__((aligned(16))) float xs[];  // 2 x BUF x 16 B | epilogue patches

  int b, bx, by;
  if (!conv_tile_of<BN>(a, b, bx, by)) return;
  const int len = (a.lengths ? a.lengths[b] * a.len_mul : a.len_default);  // valid INPUT positions
  const int olen = a.lengths_out ? a.lengths_out[b] : (a.olen_default >= 0 ? a.olen_default : len);
  const int t0 = bx * BN;
  if (t0 >= olen) return;

  const int tid = threadIdx.x, lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int wm = wave / WN, wn = wave % WN;
  const int l31 = lane & 31, h = lane >> 5;
  const int KS = a.KS, nq = a.nchunk * KS;
  const int ngroup = (a.nchunk + CPB - 1) / CPB, spg = CPB * KS;  // staged groups, steps per group
  const int ms0 = by * (MI * WM) + wm * MI;  // 32-row subtile
  const float* xb = a.x + (size_t)b * a.x_bstride;
  bf16x8* const lds8 = reinterpret_cast<bf16x8*>(xs);
  const int tin0 = t0 * STRIDE;  // VALID convs: no padding

  // Staging slot s = tid + i * NT -> (chunk cc of the group, channel octet oc, column): input positions tin0 + STRIDE * column ..
  // + STRIDE - 1 of 8 channels.  Loads are unconditional and clamped into the row; the ragged tail and the channels beyond CIN
  // are zeroed at the LDS store.
  float sp[NS][8][STRIDE];
  auto stage_load = [&](int g) {
#pragma unroll
    for (int i = 0; i < NS; ++i) {
      const int s = tid + i * NT;
      if (s < NSLOT) {
        const int co = s / NCOL, col = s - co * NCOL;  // co = 2 * cc + oc
        int t = tin0 + STRIDE * col;
        t = t > a.ldx - STRIDE ? a.ldx - STRIDE : t;
#pragma unroll
        for (int e = 0; e < 8; ++e) {
          int ci = g * (CPB * KC) + 8 * co + e;
          ci = ci < a.CIN ? ci : a.CIN - 1;
          const float* p = xb + (size_t)ci * a.ldx + t;
          if constexpr (STRIDE == 2) {
            const float2 v = *reinterpret_cast<const float2*>(p);
            sp[i][e][0] = v.x;
            sp[i][e][1] = v.y;
          } else {
            sp[i][e][0] = *p;
          }
        }
      }
    }
  };
  auto stage_store = [&](int g) {
#pragma unroll
    for (int i = 0; i < NS; ++i) {
      const int s = tid + i * NT;
      if (s < NSLOT) {
        const int co = s / NCOL, col = s - co * NCOL;
        const int t = tin0 + STRIDE * col;
        bf16x8* pl = lds8 + (g & 1) * BUF + (2 * co) * STRIDE * XW + col;  // planes [cc][oc][hi|lo][parity]
#pragma unroll
        for (int par = 0; par < STRIDE; ++par) {
          const bool tok = (t + par) < len;
          bf16x8 vh, vl;
#pragma unroll
          for (int e = 0; e < 8; ++e) {
            const bool ok = tok && (g * (CPB * KC) + 8 * co + e) < a.CIN;
            const float x = ok ? sp[i][e][par] : 0.f;
            const __bf16 xh = (__bf16)x;
            vh[e] = xh;
            vl[e] = (__bf16)(x - (float)xh);
          }
          pl[par * XW] = vh;
          pl[(STRIDE + par) * XW] = vl;
        }
      }
    }
  };

  f32x16 acc[MI][NI];
#pragma unroll
  for (int mi = 0; mi < MI; ++mi)
#pragma unroll
    for (int ni = 0; ni < NI; ++ni)
#pragma unroll
      for (int e = 0; e < 16; ++e) acc[mi][ni][e] = 0.f;

  // A fragments of step q (= chunk * KS + tap): [ms32][q][hi|lo][lane] x 8 bf16 = 2 KB per (ms32, q); step q lives in slot q % DEPTH
  const __amdgpu_buffer_rsrc_t wr = wave_rsrc(a.wpack, (unsigned)((size_t)a.nsub_group * nq * 2048));
  unsigned wq[MI];
  f32x4 av[DEPTH][MI][2];
#pragma unroll
  for (int mi = 0; mi < MI; ++mi) wq[mi] = (unsigned)(ms0 + mi) * (unsigned)nq * 2048u;
  auto load_a = [&](f32x4 (&slot)[MI][2], int q) {
    q = q < nq ? q : nq - 1;
#pragma unroll
    for (int mi = 0; mi < MI; ++mi) {
      slot[mi][0] = rsrc_load16(wr, lane * 16, wq[mi] + (unsigned)q * 2048u);
      slot[mi][1] = rsrc_load16(wr, lane * 16, wq[mi] + (unsigned)q * 2048u + 1024u);
    }
  };
#pragma unroll
  for (int u = 0; u < DEPTH - 1; ++u) load_a(av[u], u);

  stage_load(0);
  stage_store(0);
  __syncthreads();

  const int boff8 = (2 * h) * STRIDE * XW + wn * (32 * NI) + l31;
  int g = 0, s = 0, cc = 0, j = 0;  // staged group; step, chunk and tap within it
  for (int q0 = 0; q0 < nq; q0 += DEPTH) {
#pragma unroll
    for (int u = 0; u < DEPTH; ++u) {
      const int q = q0 + u;
      if (q >= nq) break;
      load_a(av[(u + DEPTH - 1) % DEPTH], q + DEPTH - 1);  // into the slot the previous step has just read
      const bool more = g + 1 < ngroup;
      if (s == 0 && more) stage_load(g + 1);  // in flight behind this group's MFMAs
      __builtin_amdgcn_sched_barrier(0);      // keep the prefetches ahead of the MFMAs
      // tap j of output column l reads input position STRIDE * l + j: plane parity j % STRIDE, column l + j / STRIDE
      const bf16x8* bj = lds8 + (g & 1) * BUF + cc * CHK + boff8 + (STRIDE == 2 ? (j & 1) * XW + (j >> 1) : 0);
      // (column block outermost: two B fragments live at a time, each feeding the MI row blocks)
#pragma unroll
      for (int ni = 0; ni < NI; ++ni) {
        const bf16x8 bh = bj[ni * 32], bl = bj[ni * 32 + STRIDE * XW];
#pragma unroll
        for (int mi = 0; mi < MI; ++mi) {
          const bf16x8 ah = __builtin_bit_cast(bf16x8, av[u][mi][0]);
          const bf16x8 al = __builtin_bit_cast(bf16x8, av[u][mi][1]);
          acc[mi][ni] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(al, bh, acc[mi][ni], 0, 0, 0);
          acc[mi][ni] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(ah, bl, acc[mi][ni], 0, 0, 0);
          acc[mi][ni] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(ah, bh, acc[mi][ni], 0, 0, 0);
        }
      }
      __builtin_amdgcn_sched_barrier(0);
      if (++j == KS) {
        j = 0;
        ++cc;
      }
      if (++s == spg) {  // the group is done: the next one goes to the other buffer
        s = 0;
        cc = 0;
        if (more) stage_store(g + 1);
        __syncthreads();
        ++g;
      }
    }
  }
  __syncthreads();  // (a last group of fewer than CPB chunks ends without the barrier above)

  conv_epilogue32<MI, NI>(a, acc, xs, b, t0, olen, 0, ms0, wn);
}

// ---- host side ----------------------------------------------------------------------------------------------------------

// the layers this kernel takes: 1x1 convs and the stride-2 VALID convs with k = 2 / 3, ungrouped, >= 64 output rows (the weight
// packing pads the rows to pack_conv_weights_bf3's tile, which both tile shapes below divide)
bool enc_bf3_supported(int Cout, int Cin, int KS, int dil, int groups, int stride, int pad_left) {
  if (groups != 1 || dil != 1 || pad_left != 0 || Cout < 64 || Cin < 1) return false;
  return (stride == 1 && KS == 1) || (stride == 2 && (KS == 2 || KS == 3));
}

template <int MI, int NI, int WM, int WN, int STRIDE, int CPB>
static int launch_enc_bf3_t(ConvArgs a, int B, int Lmax_out, hipStream_t stream) {
  constexpr int BM = 32 * MI * WM, BN = 32 * NI * WN, NW = WM * WN;
  constexpr int CW = 32 * NI + 4;
  a.mt_per_group = (a.M + BM - 1) / BM;
  const int mt = a.mt_per_group;
  dim3 grid((Lmax_out + BN - 1) / BN, mt, B);
  a.ragged_enum = (opts().ragged_enum && (a.lengths || a.lengths_out) && B > 1) ? 1 : 0;
  // the enumeration of launch32_t (conv_mfma32.hip): "xcd_order" bit 0 the linears, bit 1 the stride-2 convs; as many weight
  // slabs per sweep as stay L2-resident next to the streamed windows (hi + lo planes: the bytes of the fp32 slab)
  a.xcd = ((opts().xcd_order & (STRIDE == 2 ? 2 : 1)) && mt >= 2) ? 1 : 0;
  if (a.xcd) {
    const double slab = (double)BM * a.CIN * a.KS * sizeof(float);
    int mg = (int)(3.2 * 1024 * 1024 / slab);
    if (mg < 2 || mg > mt) mg = mt;
    while (mt % mg) --mg;
    if (opts().xcd_mg > 0) mg = opts().xcd_mg < mt ? opts().xcd_mg : mt;
    const long long tt_pad = ((long long)grid.x * B + 7) / 8 * 8;
    if (tt_pad * mg * ((mt + mg - 1) / mg) > 0x7fffffffLL) {
      a.xcd = 0;
    } else {
      a.xcd_ntile = (int)grid.x;
      a.xcd_nb = B;
      a.xcd_mg = mg;
      a.xcd_span = (int)(tt_pad * mg);
      grid = dim3((unsigned)(tt_pad * mg * ((mt + mg - 1) / mg)), 1, 1);
    }
  }
  constexpr int DEPTH = 3;
  size_t lds = (size_t)2 * CPB * 4 * STRIDE * enc_bf3_xw(BN) * 16;
  if (lds < (size_t)NW * 8 * CW * sizeof(float)) lds = (size_t)NW * 8 * CW * sizeof(float);
  static DeviceOnce attr_once;  // per device (common.h)
  DISSC_HIP_CHECK(attr_once.max_lds(reinterpret_cast<const void*>(&enc_bf3_kernel<MI, NI, WM, WN, STRIDE, CPB, DEPTH>), 160 * 1024));
  hipLaunchKernelGGL((enc_bf3_kernel<MI, NI, WM, WN, STRIDE, CPB, DEPTH>), grid, dim3(64 * WM * WN), lds, stream, a);
  DISSC_HIP_CHECK(hipGetLastError());
  return DISSC_OK;
}

int launch_enc_bf3(const ConvArgs& a, int B, int Lmax_out, int stride, hipStream_t stream) {
  if (!enc_bf3_supported(a.M, a.CIN, a.KS, a.dil, a.groups, stride, a.pad_left) || a.up != 1 || a.slope != 1.0f || a.scale ||
      !(a.epi == EPI_STORE || a.epi == EPI_RES) || a.ldx < 4) {
    set_error("launch_enc_bf3: unsupported layer (rows %d, k %d, stride %d, groups %d, padding %d, epilogue %d)", a.M, a.KS, stride,
              a.groups, a.pad_left, a.epi);
    return DISSC_EINVAL;
  }
  // 256 x 128 tiles (128 accumulator registers per lane: the short bf16 MFMAs need 24 of them per weight fragment pair to
  // keep the weight stream inside the L2's rate).  Grids that leave CUs without their two workgroups step down -- 128 x 128
  // (the 768-row linears of a 32 x 10 s batch: 384 -> 768 workgroups, three or four per CU), then 64 x 128 (short or single
  // utterances; layers below 256 rows) -- same MFMA sequence per output element, bit-identical result (cf. launch_conv_bf3)
  const long long nwg = (long long)((Lmax_out + 127) / 128) * ((a.M + 255) / 256) * B;
  const int step = a.M < 256 ? 2 : (!opts().small_grid ? 0 : (nwg < 256LL * opts().small_grid ? 2 : (nwg < 512LL * opts().small_grid ? 1 : 0)));
  if (stride == 2) {
    if (step == 2) return launch_enc_bf3_t<1, 2, 2, 2, 2, 1>(a, B, Lmax_out, stream);
    return launch_enc_bf3_t<2, 4, 4, 1, 2, 1>(a, B, Lmax_out, stream);
  }
  if (step == 2) return launch_enc_bf3_t<1, 2, 2, 2, 1, 4>(a, B, Lmax_out, stream);
  if (step == 1) return launch_enc_bf3_t<1, 4, 4, 1, 1, 2>(a, B, Lmax_out, stream);
  return launch_enc_bf3_t<2, 4, 4, 1, 1, 4>(a, B, Lmax_out, stream);
}

}  // namespace dissc
