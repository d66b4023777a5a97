// Host-side helpers shared by the generator and the predictors: device copies of packed
// conv weights and the launch wrapper around conv_mfma_kernel.
#include <string.h>

#include "common.h"

namespace dissc {

// option "ragged_enum" (default 1): see conv_mfma32.hip
thread_local int g_conv_prec = 0;  // (per thread: handles may be built concurrently) what make_conv packs for; dissc_gen_create raises it to opts().precision for its own layers

int upload(const std::vector<float>& h, float** d) {
  DISSC_HIP_CHECK(hipMalloc((void**)d, h.size() * sizeof(float)));
  DISSC_HIP_CHECK(hipMemcpy(*d, h.data(), h.size() * sizeof(float), hipMemcpyHostToDevice));
  return DISSC_OK;
}

// Which kernel family a layer of Mg rows per group is packed for and launched on.
// 64-cycle MFMAs wherever a 32-row tile is not mostly padding; 48 rows per group (HuBERT's positional conv) are three
// 16-row tiles of the 16x16x4 kernel instead of two 32-row tiles of which a quarter is padding
int conv_m32_rule(int Mg, int groups) { return (opts().use_mfma32 && Mg >= 32 && !(Mg == 48 && groups > 1)) ? 1 : 0; }

// The launch geometry of a layer (everything of a DevConv that is not a device pointer or a packing's Mpad): what make_conv
// packs for and what dissc_conv_info answers from, without an upload.
void conv_geometry(DevConv& dc, int Cout, int Cin, int KS, int dil, int groups, int stride, int pad_left) {
  const int Mg = Cout / groups, Cg = Cin / groups;
  dc.m32 = conv_m32_rule(Mg, groups);
  // split-bf16 only where conv_mfma32.hip has an instance for it
  const bool lin_big = (KS == 1 && Mg >= 256 && (Cg + KC - 1) / KC >= 8);
  dc.prec = (g_conv_prec == 1 && dc.m32 && stride == 1 && groups == 1 && (KS - 1) * dil <= MAX_TAP_SPAN && !lin_big)
                ? 1 : 0;
  // the encoder's route (a split-bf16 HuBERT handle): its own kernel, also for the linears and stride-2 convs refused above
  if (g_conv_prec == 2 && dc.m32 && enc_bf3_supported(Cout, Cin, KS, dil, groups, stride, pad_left)) dc.prec = 2;
  dc.CIN = Cg; dc.M = Mg; dc.KS = KS; dc.dil = dil; dc.nchunk = (Cg + KC - 1) / KC; dc.up = 1;
  dc.groups = groups; dc.stride = stride; dc.pad_left = pad_left;
  dc.macs_per_t = (double)Cout * Cg * KS;
}

// w: [Cout][Cin/groups][KS] (PyTorch layout); Cout, Cin are the TOTAL channel counts.
int make_conv(const float* w, const float* bias, int Cout, int Cin, int KS, int dil, DevConv& dc,
              int groups, int stride, int pad_left) {
  std::vector<float> packed;
  int Mpad, nchunk;
  const int Mg = Cout / groups, Cg = Cin / groups;
  conv_geometry(dc, Cout, Cin, KS, dil, groups, stride, pad_left);
  if (dc.prec) pack_conv_weights_bf3(w, Cout, Cg, KS, packed, Mpad, nchunk);
  else if (dc.m32) pack_conv_weights32(w, Cout, Cg, KS, packed, Mpad, nchunk, groups);
  else pack_conv_weights(w, Cout, Cg, KS, packed, Mpad, nchunk, groups);
  std::vector<float> b((size_t)Mpad * groups, 0.f);
  if (bias)
    for (int g = 0; g < groups; ++g) memcpy(b.data() + (size_t)g * Mpad, bias + (size_t)g * Mg, Mg * sizeof(float));
  dc.nchunk = nchunk; dc.Mpad = Mpad;
  int rc = upload(packed, &dc.wpack);
  if (rc) return rc;
  if (dc.m32 && !dc.prec && dil == 1 && conv2s128_shape(Cout, Cin, KS, stride, groups) && opts().conv2s128) {
    std::vector<float> p2;  // the second packing costs 4 Cout Cin KS bytes (3 MB per HuBERT feature conv)
    pack_s2_weights128(w, Cout, Cin, p2);
    if ((rc = upload(p2, &dc.wpack2))) return rc;
  }
  return upload(b, &dc.bias);
}

// The phase groups of ConvTranspose1d(k, s, padding (k - s) / 2): one conv launch per group of output phases.
void convT_groups(int Cout, int k, int s, std::vector<ConvTGroup>& out) {
  const int pad = (k - s) / 2;
  out.clear();
  // input taps of phase p: delta in [dlo, dhi] with 0 <= p + pad - s*delta < k
  auto taps = [&](int p, int& dlo, int& dhi) {
    dlo = 1 << 30;
    dhi = -(1 << 30);
    for (int kk = (p + pad) % s; kk < k; kk += s) {
      const int delta = (p + pad - kk) / s;  // exact
      dlo = delta < dlo ? delta : dlo;
      dhi = delta > dhi ? delta : dhi;
    }
  };
  // Narrow layers (few output rows) are store/latency bound: one launch over the union of the
  // taps (some zero weights) beats several small ones; wide layers skip the zero taps instead.
  const bool single = Cout < 64;
  int p0 = 0;
  while (p0 < s) {
    int dlo, dhi;
    taps(p0, dlo, dhi);
    int np = 1;
    while (p0 + np < s) {
      int l2, h2;
      taps(p0 + np, l2, h2);
      if (single) {
        dlo = l2 < dlo ? l2 : dlo;
        dhi = h2 > dhi ? h2 : dhi;
      } else if (l2 != dlo || h2 != dhi) {
        break;
      }
      ++np;
    }
    out.push_back(ConvTGroup{p0, np, dlo, dhi - dlo + 1});
    p0 += np;
  }
}

int make_convT(const float* w, const float* bias, int Cin, int Cout, int k, int s,
               std::vector<DevConv>& groups) {
  groups.clear();
  std::vector<ConvTGroup> plan;
  convT_groups(Cout, k, s, plan);
  for (const ConvTGroup& g : plan) {
    const int p0 = g.p0, np = g.np, dlo = g.dlo, ntap = g.ntap;
    std::vector<float> wc;
    convT_phase_weights(w, Cin, Cout, k, s, p0, np, dlo, ntap, wc);
    std::vector<float> bc((size_t)Cout * np);
    for (int co = 0; co < Cout; ++co)
      for (int pi = 0; pi < np; ++pi) bc[co * np + pi] = bias ? bias[co] : 0.f;
    groups.emplace_back();
    DevConv& dc = groups.back();
    int rc = make_conv(wc.data(), bc.data(), Cout * np, Cin, ntap, 1, dc, 1, 1, -dlo);
    if (rc) return rc;
    dc.up = s;
    dc.up_np = np;
    dc.up_p0 = p0;
    dc.macs_per_t = groups.size() == 1 ? (double)Cin * Cout * k : 0.0;  // algorithmic MACs counted once
  }
  return DISSC_OK;
}

int set_affine(DevConv& dc, const float* scale, const float* shift, int n) {
  // same [groups][Mpad] indexing as the bias
  std::vector<float> sc((size_t)dc.Mpad * dc.groups, 1.f), sh((size_t)dc.Mpad * dc.groups, 0.f);
  for (int i = 0; i < n && i < dc.M * dc.groups; ++i) {
    const size_t k = (size_t)(i / dc.M) * dc.Mpad + (i % dc.M);
    sc[k] = scale ? scale[i] : 1.f;
    sh[k] = shift ? shift[i] : 0.f;
  }
  int rc = upload(sc, &dc.scale);
  if (rc) return rc;
  return upload(sh, &dc.shift);
}

void free_conv(DevConv& dc) {
  if (dc.wpack) (void)hipFree(dc.wpack);
  if (dc.wpack2) (void)hipFree(dc.wpack2);
  if (dc.bias) (void)hipFree(dc.bias);
  if (dc.scale) (void)hipFree(dc.scale);
  if (dc.shift) (void)hipFree(dc.shift);
  dc.wpack = dc.wpack2 = dc.bias = dc.scale = dc.shift = nullptr;
}

// Tile shape id of the 32-row kernel for one launch of the layer, -1 = the class default.  General path only: the special
// instances (split-bf16, strided, grouped, wide-tap and the big 1x1 layers) keep their tile.
int conv_launch_cfg32(const DevConv& dc, int B, int Lmax_out) {
  const int span = (dc.KS - 1) * dc.dil;
  const bool lin_big = (dc.KS == 1 && dc.M >= 256 && dc.nchunk >= 8);
  if (dc.m32 && !dc.prec && dc.stride == 1 && dc.groups == 1 && span <= MAX_TAP_SPAN && !lin_big)
    return conv32_pick_cfg(dc.M, B, Lmax_out);
  return -1;
}

// What one launch of the layer runs on: kernel family, tile shape id in force, BM x BN.  Host only.
int conv_launch_info(const DevConv& dc, int B, int Lmax_out, int* family, int* cfg, int* bm, int* bn) {
  const int span = (dc.KS - 1) * dc.dil;
  if (dc.prec || dc.stride != 1 || dc.groups != 1 || span > MAX_TAP_SPAN) {
    set_error("conv_launch_info: only the general stride-1 fp32 instances (span <= %d) are described", MAX_TAP_SPAN);
    return DISSC_EINVAL;
  }
  if (dc.m32) {
    const int c32 = conv_launch_cfg32(dc, B, Lmax_out);
    if (c32 < 0) {
      set_error("conv_launch_info: %d x %d 1x1 layer runs on a special instance with a fixed tile", dc.M, dc.CIN);
      return DISSC_EINVAL;
    }
    *family = 32; *cfg = conv32_launch_cfg(c32, dc.M); *bm = conv32_cfg_bm(*cfg); *bn = conv32_cfg_bn(*cfg);
  } else {
    *family = 16; *cfg = conv_cfg(dc.M);
    if (span == 0 && *cfg == 0 && dc.nchunk >= 8) {
      set_error("conv_launch_info: %d x %d 1x1 layer runs on a special instance with a fixed tile", dc.M, dc.CIN);
      return DISSC_EINVAL;
    }
    *bm = conv_cfg_bm(*cfg); *bn = conv_cfg_bn(*cfg);
  }
  return DISSC_OK;
}

int run_conv(const DevConv& dc, const float* x, float* out, const Batch& bt, const EpiSpec& ep, int C_x, int ldx, int ldo,
             float slope, hipStream_t stream, int dma_in) {
  if (dc.wino) {  // transform-domain layers: no activated store (EPI_STORE_ACT, out_slope), no LDS-DMA input
    if (ep.epi == EPI_STORE_ACT || dma_in || C_x != dc.CIN) {
      set_error("run_conv: transform-domain layer (C = %d, k = %d): no EPI_STORE_ACT, no dma_in, C_x must be C (%d)", dc.M, dc.KS, C_x);
      return DISSC_EINVAL;
    }
    return (dc.wino == 2 ? run_wino8 : run_wino)(dc, x, out, bt, ep, ldx, ldo, slope, stream);
  }
  ConvArgs a;
  a.out_slope = ep.out_slope; a.dma_in = dma_in;
  a.x = x; a.wpack = dc.wpack; a.wpack2 = dc.wpack2; a.bias = dc.bias; a.scale = dc.scale; a.shift = dc.shift; a.res = ep.res;
  a.out = out; a.acc = ep.acc;
  a.lengths = bt.lengths; a.len_default = bt.len_default; a.len_mul = bt.len_mul;
  a.lengths_out = bt.lengths_out; a.olen_default = bt.olen_default;
  a.CIN = dc.CIN; a.M = dc.M; a.KS = dc.KS; a.dil = dc.dil; a.nchunk = dc.nchunk;
  a.pad_left = dc.pad_left >= 0 ? dc.pad_left : ((dc.KS - 1) * dc.dil) / 2;
  a.xcd = 0; a.xcd_ntile = 0; a.xcd_nb = 0; a.xcd_mg = 0; a.xcd_span = 0;
  a.ragged_enum = 0;
  a.groups = dc.groups; a.nsub_group = dc.Mpad / (dc.m32 ? 32 : 16); a.act = dc.act; a.m32 = dc.m32; a.prec = dc.prec;
  a.cfg32 = conv_launch_cfg32(dc, bt.B, bt.Lmax);
  const bool wide = dc.stride == 1 && (dc.KS - 1) * dc.dil > MAX_TAP_SPAN;  // (every wide instance has the same time tile)
  a.XW = conv_xw(dc.M, dc.KS, dc.dil, dc.stride, dc.m32, wide ? WIDE_TILE_BN : a.cfg32 >= 0 ? conv32_cfg_bn(a.cfg32) : 0);
  a.ldx = ldx; a.ldo = ldo;
  a.x_bstride = (long long)C_x * ldx;
  a.o_bstride = (long long)(dc.M * dc.groups / dc.up_np) * ldo;
  a.slope = slope; a.mrf_div = ep.mrf_div; a.epi = ep.epi; a.up = dc.up; a.up_np = dc.up_np; a.up_p0 = dc.up_p0;
  return launch_conv(a, bt.B, bt.Lmax, dc.stride, stream);
}

}  // namespace dissc
