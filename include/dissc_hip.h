/*
 * dissc_hip.h -- C ABI of libdissc_hip.so, the MI355X (gfx950) implementation of
 * the DISSC inference hot path.
 *
 * The reference (gallilmaimon/DISSC) has no FFI layer: the hot path sits behind
 * four nn.Module call signatures.  Each entry point below
 * names the reference interface it replaces; the dissc_amd Python package re-creates those
 * Python signatures on top of this ABI through ctypes.
 *
 * Conventions
 *   - every data pointer passed to a *_forward / kernel entry point is a DEVICE
 *     pointer owned by the caller (PyTorch's allocator in practice); pointers
 *     passed to *_create are HOST pointers (weights are copied and re-packed
 *     once, the library owns the device copy);
 *   - no allocation and no synchronisation inside *_forward: work is enqueued
 *     on the given hipStream_t (passed as void*; NULL = the null stream);
 *   - return 0 on success, a negative DISSC_E* code on failure; nothing throws
 *     across the ABI; dissc_last_error() returns a thread-local message;
 *   - one handle per process/GPU, handles are independent; calls on ONE handle must be stream-ordered
 *     (a handle owns helper streams/events and the caller's workspace is its scratch); the only
 *     process-wide state is the tuning table behind dissc_set_option.
 */
#ifndef DISSC_HIP_H
#define DISSC_HIP_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define DISSC_OK 0
#define DISSC_EINVAL (-1)   /* bad argument / unsupported configuration */
#define DISSC_ENOMEM (-2)   /* workspace too small / device allocation failed */
#define DISSC_EHIP (-3)     /* a HIP runtime call failed */
#define DISSC_ENOTFOUND (-4) /* a required weight tensor is missing */
#define DISSC_ENOTSUP (-5)  /* an optional dependency is absent (RCCL for the dissc_comm_* / dissc_allgather_waves entries) */
#define DISSC_ECOMM (-6)    /* an RCCL call failed */

/* A named host tensor (fp32, contiguous, PyTorch layout). */
typedef struct {
  const char* name;   /* state_dict key after weight-norm folding, e.g. "ups.0.weight" */
  const float* data;  /* host pointer */
  int64_t shape[4];
  int32_t ndim;
} DisscTensor;

const char* dissc_last_error(void);
/* ABI version of this header: bumped when a signature changes or a section is added (5: dissc_convgrad_*;
 * 6: dissc_conv_info, and dissc_get_option reads the tile-shape keys; 7: dissc_wino8_info; 8: the split-bf16 diagnostics
 * dissc_conv1d_prec, dissc_conv_transpose1d_prec, dissc_resblock1d_bf3, dissc_bf3_info and mode 5 of dissc_respair1d;
 * 9: dissc_wino_info).  ADDED since, without a bump (no signature changed; a binding that needs one checks for the symbol):
 * dissc_gen_create_rb (the generator with ResBlock2 blocks), dissc_resblock2_1d, dissc_resblock2_info, dissc_convgrad_create_wide
 * (tap spans up to 72), dissc_convgrad_create_prec and dissc_convgrad_precision_info (the split-bf16 training layer). */
int dissc_abi_version(void);
/* Number of HIP devices visible / name of device `dev` (for diagnostics). */
int dissc_device_count(void);
int dissc_device_name(int dev, char* buf, size_t buflen);

/* ------------------------------------------------------------------------- *
 * HiFi-GAN unit/F0/speaker-conditioned generator.
 * Replaces: CodeGenerator.forward + Generator.forward + ResBlock1.forward,
 *           reference sr/models.py:179-225, :98-114, :34-41 (called from
 *           generate(), reference sr/inference.py:67-76).
 * ------------------------------------------------------------------------- */
#define DISSC_MAX_UPS 8
#define DISSC_MAX_RK 4

typedef struct {
  int32_t model_in_dim;             /* 257 = 128 code | 1 f0 | 128 spkr  (config "model_in_dim") */
  int32_t upsample_initial_channel; /* 512 */
  int32_t num_upsamples;            /* 5 */
  int32_t upsample_rates[DISSC_MAX_UPS];        /* 5,4,4,2,2 */
  int32_t upsample_kernel_sizes[DISSC_MAX_UPS]; /* 11,8,8,4,4 */
  int32_t num_kernels;              /* 3 */
  int32_t resblock_kernel_sizes[DISSC_MAX_RK];      /* 3,7,11 */
  int32_t resblock_dilations[DISSC_MAX_RK][3];      /* 1,3,5 each */
  int32_t num_embeddings;           /* 100 */
  int32_t embedding_dim;            /* 128 */
  int32_t num_speakers;             /* 200 rows in spkr.weight (reference sr/models.py:133) */
  int32_t has_f0;                   /* config "f0" */
  int32_t has_spkr;                 /* config "multispkr" */
} DisscGenConfig;

typedef struct dissc_gen* dissc_gen_t;

/* weights: folded (weight-norm removed) tensors named like the reference's
 * state_dict after remove_weight_norm(): "conv_pre.weight/.bias",
 * "ups.{i}.weight/.bias" ([Cin,Cout,k]), "resblocks.{n}.convs{1,2}.{m}.weight/.bias",
 * "conv_post.weight/.bias", "dict.weight", "spkr.weight". */
int dissc_gen_create(const DisscGenConfig* cfg, const DisscTensor* weights, size_t n_weights,
                     dissc_gen_t* out);
/* the same with the handle's arithmetic given explicitly instead of read from the process-wide "precision" option:
 * -1 = that option, 0 = exact fp32, 1 = split-bf16 (opt-in, see dissc_set_option) */
int dissc_gen_create_ex(const DisscGenConfig* cfg, const DisscTensor* weights, size_t n_weights, int precision,
                        dissc_gen_t* out);
/* the same with the residual block type of the config's "resblock" key (reference sr/models.py:80): 1 = ResBlock1, what the two
 * entries above build; 2 = ResBlock2 (HiFi-GAN V3): block n has TWO convs, "resblocks.{n}.convs.{m}.weight/.bias", m = 0, 1, and
 * computes  for m: x = x + conv_{d_m}(lrelu(x, 0.1))  with d_m = resblock_dilations[j][m] (the third entry is not read), then
 * the stage's MRF mean in the reference's order.  Each block runs as two direct conv launches, x_k through the chain's
 * buffers, the second carrying the MRF epilogue, on the chain's side stream; (k - 1) d_m <= 72.  precision 1: every conv follows
 * the per-layer rule of the other layers (split-bf16 where >= 32 rows and (k - 1) d_m <= 60 grant an instance, fp32 elsewhere). */
int dissc_gen_create_rb(const DisscGenConfig* cfg, const DisscTensor* weights, size_t n_weights, int precision, int resblock,
                        dissc_gen_t* out);
void dissc_gen_destroy(dissc_gen_t g);
/* samples produced per input frame (= prod(upsample_rates) = 320) */
int dissc_gen_hop(dissc_gen_t g);
size_t dissc_gen_workspace_bytes(dissc_gen_t g, int B, int Tmax);
/* FLOPs (2*MAC) of one forward for `frames` total valid frames (roofline accounting) */
double dissc_gen_flops(dissc_gen_t g, int64_t frames);
/* 2 * multiply-adds the matrix pipe EXECUTES for `frames` code frames: equal to dissc_gen_flops unless ResBlock convs
 * run in the Toom-Cook F(4,3) transform domain (csrc/conv_wino.hip; option "wino", default on for the C >= 64 stages),
 * which do 6 ceil(k / 3) / 4 products per output and channel pair instead of k. */
double dissc_gen_flops_executed(dissc_gen_t g, int64_t frames);
/*
 * code    i64 [B,Tmax]   unit ids in [0,num_embeddings)
 * f0      f32 [B,Tmax]   one value per frame (reference shape [B,1,T])
 * spkr    i64 [B]        speaker ids in [0,num_speakers)
 * lengths i32 [B]        valid frames per utterance (NULL = all Tmax).  Every
 *                        layer treats positions >= length as the zero padding the
 *                        reference's B=1 run would see, so a ragged batch is
 *                        sample-exact with per-utterance runs.
 * wav_out f32 [B,hop*Tmax]  samples >= hop*length[b] are written as 0.
 */
int dissc_gen_forward(dissc_gen_t g, const int64_t* code, const float* f0, const int64_t* spkr,
                      const int32_t* lengths, int B, int Tmax, float* wav_out, void* workspace,
                      size_t workspace_bytes, void* stream);
/* Stand-alone conv entry points (unit-testable building blocks of the above).
 * x f32 [B,Cin,ldx] -> y f32 [B,Cout,ldo]; "same" zero padding at both ends of
 * each utterance's valid length; in_slope = leaky-ReLU slope applied to the
 * input on load (1.0 = none).  w: HOST pointer [Cout,Cin,k] (re-packed per call:
 * test/debug path only). */
int dissc_conv1d(const float* x, const float* w_host, const float* bias_host, float* y,
                 const int32_t* lengths, int B, int Cin, int Cout, int k, int dilation, int ldx,
                 int ldo, int Lmax, float in_slope, void* stream);
/* ConvTranspose1d(Cin,Cout,k,stride,padding=(k-stride)/2); w HOST [Cin,Cout,k];
 * y [B,Cout,ldo] with length stride*len. */
int dissc_conv_transpose1d(const float* x, const float* w_host, const float* bias_host, float* y,
                           const int32_t* lengths, int B, int Cin, int Cout, int k, int stride,
                           int ldx, int ldo, int Lmax, float in_slope, void* stream);
/* The same two with the arithmetic given: prec 0 = exactly the entries above, 1 = the generator's split-bf16 mode ("precision" = 1:
 * conv_bf3_kernel, csrc/conv_bf3.hip).  prec = 1 is DISSC_EINVAL with a message, before anything is packed, where the layer (or a
 * phase group of the ConvTranspose) gets no split-bf16 instance -- fewer than 32 GEMM rows, taps spanning more than 60 columns,
 * the big 1x1 layers -- and where x is not 16-byte aligned or ldx no multiple of 4: it never runs fp32 instead. */
int dissc_conv1d_prec(const float* x, const float* w_host, const float* bias_host, float* y,
                      const int32_t* lengths, int B, int Cin, int Cout, int k, int dilation, int ldx,
                      int ldo, int Lmax, float in_slope, int prec, void* stream);
int dissc_conv_transpose1d_prec(const float* x, const float* w_host, const float* bias_host, float* y,
                                const int32_t* lengths, int B, int Cin, int Cout, int k, int stride,
                                int ldx, int ldo, int Lmax, float in_slope, int prec, void* stream);

/* Stride-2 VALID conv (HuBERT's feature convs; reference data/encode.py:21-22,32 via fairseq ConvFeatureExtractionModel):
 * x f32 [B,Cin,ldx] -> y f32 [B,Cout,ldo] with (len - k) / 2 + 1 outputs per utterance, no padding; w HOST [Cout,Cin,k];
 * act 1 = exact-erf GELU on the output.  form 0 = the direct implicit GEMM, 1 = the polyphase Toom-Cook form (k = 3 only:
 * F(7,2) on the even samples + a 1-tap GEMM on the odd ones, 15 instead of 21 products per 7 outputs; conv_s2tc.hip).
 * lengths_in: device int32 [B] or NULL (= Lmax_in everywhere).  Synchronous; test / gate entry, weights packed per call. */
int dissc_conv1d_s2(const float* x, const float* w_host, const float* bias_host, float* y, const int32_t* lengths_in, int B,
                    int Cin, int Cout, int k, int ldx, int ldo, int Lmax_in, int act, int form, void* stream);
/* dissc_conv1d_s2's direct form with the arithmetic as an argument: prec 0 = exact fp32, 1 = split-bf16 (enc_bf3.hip; k = 2 / 3,
 * Cout >= 64). */
int dissc_conv1d_s2_prec(const float* x, const float* w_host, const float* bias_host, float* y, const int32_t* lengths_in, int B,
                         int Cin, int Cout, int k, int ldx, int ldo, int Lmax_in, int act, int prec, void* stream);
/* Stand-alone linear as the encoder runs it (tests): x f32 [B,Cin,ld] -> y f32 [B,Cout,ld] on columns [0, lengths[b]) (NULL = Tmax),
 * y = W x + bias, exact-erf GELU if act 1, + res if res != NULL (layout of y).  w HOST [Cout,Cin]; prec as above.  Synchronous. */
int dissc_linear_prec(const float* x, const float* w_host, const float* bias_host, const float* res, float* y,
                      const int32_t* lengths, int B, int Cin, int Cout, int ld, int Tmax, int act, int prec, void* stream);
/* Diagnostics: average ms of `iters` launches of one C -> C, k = 3, stride 2 conv + GELU on B rows of L input samples. */
int dissc_conv_s2_bench(int B, int C, int L, int form, int iters, float* ms_out);

/* Tuning hook: the DEFAULTS of handles created LATER (also reachable through the environment variable
 * DISSC_OPTIONS="key=value,key=value" read by the Python binding).  Every handle -- generator, HuBERT, predictor, trainer --
 * takes a snapshot of all options when it is created and never reads the process-wide values again: forwards are
 * re-entrant per handle, two handles created under different options keep their own behaviour whatever is set in between
 * (tests/test_gpu_generator.py::test_options_are_frozen_into_the_handle).  The stand-alone entries without a handle
 * (dissc_conv1d, dissc_respair1d, the *_bench diagnostics) read the defaults at call time.
 * Options marked [experimental] select kernels whose gates failed; they are only in libraries built with
 * DISSC_EXPERIMENTAL=1 (dissc_get_option("experimental") == 1) and are refused or ignored otherwise.
 *   multistream (1)      generator: the ResBlocks of a stage run as concurrent chains on HIP streams (two side
 *                        streams per device, shared by all generator handles of the process; the longer chains at higher
 *                        stream priority, the phase groups of a ConvTranspose layer concurrently on the same streams)
 *   precision (0)        0 = exact fp32 MFMA everywhere (default, bench.py's headline); 1 = split-bf16 GENERATOR
 *                        ("bf16x3": hi*hi + hi*lo + lo*hi on the bf16 matrix cores, fp32 accumulate; conv_bf3.hip,
 *                        resblock_bf3.hip) -- ~2^-17 product error, waveform RMS ~4e-6 vs the reference (bar 1e-4),
 *                        ~2x the fp32 rate.  Predictors and HuBERT feed integer decisions: `precision` never touches them;
 *                        HuBERT has `enc_precision`.
 *   enc_precision (0)    read at dissc_hubert_create: 0 = exact fp32 MFMA (default); 1 = split-bf16 ENCODER: the feature convs
 *                        conv1..conv6 and every linear (post_extract_proj, qkv, out_proj, fc1, fc2) in the same hi*hi + hi*lo +
 *                        lo*hi arithmetic (enc_bf3.hip); conv0 + GroupNorm, the LayerNorms, attention, the positional conv and the
 *                        k-means step stay fp32.  Opt-in, never a default: the units it flips against float64 are counted and held
 *                        to the derived bound of the fp32 path (tests/test_gpu_hubert_split_bf16.py).
 *   mfma32 (1)           use the 32x32x2 MFMA kernel for layers with >= 32 output rows
 *   conv_cfg_bm{16,32,64,128,256} / conv32_cfg_bm{32,64,128,256}
 *                        tile-shape id per GEMM-M class (tables in conv_mfma.hip / conv_mfma32.hip)
 *   small_grid (1)       launches with fewer than value x 256 workgroups step down to smaller conv tiles (0 = never)
 *   lin128 (1)           HuBERT's linears on lin_gemm.hip's 256 x 128 tiles (0: conv_mfma32_kernel's 256 x 64 instances)
 *   conv2s128 (1)        HuBERT's stride-2, k = 3 feature convs on lin_gemm.hip's tiles (0: conv_mfma32_kernel; 2: 32 channels
 *                        per barrier)
 *   kernel_dbg (0)       diagnostics only: knock-outs inside the kernels (bit meanings in their sources); wrong results when set
 *   pair_max_c (32)      widest fp32 stage whose residual pairs (conv_d -> conv_1 -> +x) run as ONE launch each
 *                        (respair.hip; 0 = every conv its own launch; results are bit-identical either way)
 *   pair_f23 (3)         read at dissc_gen_create, a bit mask: 1 = the k = 11 residual pairs of the 32-channel stage, 2 = those of the
 *                        16-channel stage run as register-only Toom-Cook F(2,3) (respair_f23.hip / respair16_f23.hip: 8 products per
 *                        output instead of 11, no LDS exchange; forward 1.5 % faster; not bit-identical to the direct pairs, error no
 *                        larger); 4 / 8 = their k = 3 pairs too (2 products per output instead of 3: per launch -12 % at C = 32, 0 at
 *                        C = 16, nothing in the forward -- off); 0 = the direct pairs of respair.hip.  Bits 1 / 2 are the per-stage
 *                        switch of the register-only transform-domain pairs; pair_tc6 picks the form per (stage, k)
 *   pair_tc6 (3)         read at dissc_gen_create, a bit mask honoured only for a stage whose pair_f23 bit is set: 1 = the k = 7,
 *                        2 = the k = 11 residual pairs of the 32-channel stage run on six Toom-Cook points as F(3,4)
 *                        (respair32_tc6_kernel in respair_f23.hip: 4 / 6 products per output instead of the direct pair's 7 /
 *                        F(2,3)'s 8, still no LDS exchange; per launch -22...-27 % at k = 7 and -11...-16 % at k = 11, forward
 *                        2.3 % faster; rounding within 1.4 x the direct pair's on trained-like data); 4 / 8 = the same for
 *                        the 16-channel stage (no instance: ignored); 0 = F(2,3) for k = 11, the direct pair for k = 7
 *   pair_f23_c64 (1)     read at dissc_gen_create, honoured only while pair_f23 != 0: the k = 3 residual pairs of the 64-channel
 *                        stage run as ONE register-only F(2,3) launch each (respair64_f23_kernel in respair_f23.hip) instead of two
 *                        conv_wino launches; 0 = the two launches.  Not bit-identical to them; rounding no larger
 *   pair_tc6_c64 (1)     read at dissc_gen_create, a bit mask honoured only while pair_f23 != 0 (independent of pair_tc6 and
 *                        pair_f23_c64): 1 = the k = 7, 2 = the k = 11 residual pairs of the 64-channel stage run as ONE
 *                        register-only six-point F(3,4) launch each (respair64_tc6_kernel in respair_f23.hip) instead of two
 *                        transform-domain launches (k = 7: per launch -13...-22 %, forward 1.4 % faster; k = 11: slower at
 *                        d = 5 and in the forward, off); 0 = the two launches.  Not bit-identical to them; rounding within
 *                        1.6 x the direct launches' on trained-like data
 *   chain_f23 (3)        read at dissc_gen_create, a bit mask honoured only for fp32 handles while wino != 0, pair_f23 != 0 and the
 *                        stage is within pair_max_c:
 *                        1 = the k = 3, dilations (1, 3, 5) ResBlock of the 32-channel stage, 2 = that of the 16-channel stage
 *                        runs as ONE register-only F(2,3) launch (reschain32_f23_kernel in respair_f23.hip,
 *                        reschain16_f23_kernel in respair16_f23.hip: x_1, x_2 and the residuals stay on the CU, 2 C^2
 *                        products per output and conv instead of 3 C^2); 0 = three one-launch pairs.  Not bit-identical to
 *                        them.  A chain-level choice: dissc_pair_info does not see it
 *   rb2_fused (59)       read at dissc_gen_create_rb, a bit mask honoured only for fp32 handles: the ResBlock2 blocks of the 32-channel
 *                        stage with k = 3 / 5 / 7 (bits 1 / 2 / 4) and of the 16-channel stage (bits 8 / 16 / 32) run as ONE launch each
 *                        (csrc/resblock2.hip: x_1 in LDS; instances (k; d0, d1) = (3; 1, 2), (5; 2, 6), (7; 3, 12)) instead of two
 *                        direct conv launches; same bits either way.  Default: every shape but C = 32, k = 7, where the one launch measured
 *                        16 % slower (profiles/resblock2.md).  dissc_resblock2_info reports the form
 *   pair_dma (1)         read at dissc_gen_create: the two-launch direct residual pairs of the >= 32-channel stages hand their
 *                        intermediate over activated with zero tails, and the second conv stages its windows by LDS-DMA
 *   wino8 (1)            read at dissc_gen_create: 1 = the ResBlock convs selected by wino8_mask run on conv_wino8.hip's
 *                        8-wave workgroups (eight Toom-Cook points: F(6,3), 8 ceil(k / 3) / 6 products per output, or F(5,4) with
 *                        4-tap sub-filters, 8 ceil(k / 4) / 5 -- forward 4 % faster than with F(4,3) everywhere, per-layer rounding
 *                        1.4-1.7x the F(4,3) form's); 0 = the F(4,3) form everywhere; 2 = dissc_conv1d uses it too (tests).
 *                        wino8_mask (0450770550 octal): one bit per SHAPE, 9 cls + 3 ki + di with cls 0 / 1 / 2 for C = 64 / 128 / >= 256,
 *                        ki 0 / 1 / 2 for k = 3 / 7 / 11, di 0 / 1 / 2 for dilation 1 / 3 / 5 (three octal digits per class).
 *                        wino8_r4 (1): the shapes of wino8_r4_mask (0770770010, same layout) run as F(5,4); 2 = dissc_conv1d too; 0 =
 *                        never.  wino8_c64_wide (3): C = 64 instances -- 1 = 64 x 128 tiles, 0 = 64 x 64, 2 = 64 x 64
 *                        built for two workgroups per CU, 3 = 1 for k = 7 as F(6,3) and 2 for everything else (k = 11; k = 7 as F(5,4))
 *   wino8_sv (1)         conv_wino8.hip, the 128 x 64 tile of a k = 7 / 11 shape (C >= 128 on a full grid): the eight waves of a
 *                        workgroup share the input transform -- each forms all eight points of one channel into a double-buffered
 *                        V, one barrier per 8 channels -- instead of every wave forming its own point's tile from the same window
 *                        samples; bit-identical (0 = private tiles).  k = 7, dilation 5 as F(6,3) has no shared instance and keeps
 *                        private tiles.  dissc_wino8_form reports the form of a launch
 *   ragged_enum (1)      conv_mfma32_kernel on a ragged batch enumerates only the (time tile, utterance) pairs that exist (the
 *                        empty workgroups all sit at the end of the dispatch order); 0 = tile x utterance grid with early exits
 *   pair_wino (0)        [experimental] read at dissc_gen_create: 0 = off (default: the whole-forward gain is 0.2 %); 1 = the residual pairs this measured faster for (C = 32, k = 11, d = 1 / 3;
 *                        the first pair of the C = 64, k = 3 chain) run as ONE launch with both convs in the Toom-Cook
 *                        transform domain and the intermediate in LDS (respair_wino.hip); 2 = every shape with an instance
 *                        (C = 32: k = 7 / 11; C = 64: k = 3, first pair of a chain); 0 = none
 *   pairw_chv (2)        [experimental] respair_wino.hip: 2 = one 12-wave workgroup per CU, 1 = two 6-wave workgroups with half the tile
 *   graphs (0)           [experimental] generator forwards of B * Tmax <= graph_frames (2048) are captured once into a hipGraph
 *                        and replayed (off: slower than the plain three-stream launches on ROCm 7.2)
 *   wino (1)             read at dissc_gen_create: 1 = ResBlock convs with C >= 64 (at C = 64 those with k >= 3) run in the
 *                        Toom-Cook F(4,3) transform domain (conv_wino.hip), 0 = all direct,
 *                        2 = dissc_conv1d uses it too (tests)
 *   wino_sv (1)          conv_wino.hip, C >= 128: the 12 waves of a workgroup share the input transform (one barrier per
 *                        8 channels) instead of every wave forming its own tile; bit-identical, faster (0 = private tiles)
 *   enc_tc (0)           [experimental] read at dissc_hubert_create: 1 = the k = 3, stride-2 feature convs (conv1..conv4) run in polyphase
 *                        Toom-Cook form (conv_s2tc.hip: 15 / 7 instead of 3 MFMA products per output; opt-in: its gate failed --
 *                        6 % faster per launch, 2.35x the direct form's rounding error); 0 = direct implicit GEMM (default).
 *                        s2tc_xmode (0): 0 = row tiles pinned to XCDs, 1 = the row tiles of a time tile share an XCD
 *   hubert_split (1)     dissc_hubert_forward runs a batch of >= 16 utterances as 2-4 parts on streams of their own, which
 *                        fill the partly filled last workgroup rounds of each other's launches (0 never, 1 unless the
 *                        whole batch fills whole rounds by itself, N >= 2 always N parts); the units do not depend on it
 *   xcd_order (11)       XCD-aware workgroup order of the 32x32x2 implicit-GEMM launches with >= 2 M tiles (bit 0: 1x1 convs =
 *                        HuBERT's linears, bit 1: stride-2 convs = its feature extractor, bit 2: every other instance): a 1-D
 *                        grid whose ids are dealt in sweeps over groups of M tiles (weight slabs that fit one XCD's L2 together),
 *                        the M tiles of one input window on consecutive slots of one XCD.  Same tiles, same arithmetic, bit-
 *                        identical results; 21 % less fabric traffic on the encoder.  xcd_mg (0 = automatic): M tiles per sweep.
 *                        Bit 3: the fused attention's workgroups in XCD order (the query tiles of one (utterance, head) on one
 *                        XCD: its K / V rows cross the fabric once)
 * Unknown keys return DISSC_EINVAL. */
int dissc_set_option(const char* key, int value);
/* Read back any option's DEFAULT (so that a wrapper can set an option around the creation of one handle and restore it), the
 * conv_cfg_bm* / conv32_cfg_bm* tile-shape ids as set (before the clamps of the launch path: dissc_conv_info has those), plus
 * "experimental" (1: the library was built with DISSC_EXPERIMENTAL=1), "graph_hits", "graph_captures". */
int dissc_get_option(const char* key, int* value);

/* Diagnostics (not on the product path): average milliseconds of `iters` launches of
 * one Conv1d layer shape on synthetic device data; `epi` 0 plain, 1 +residual,
 * 2..4 MRF accumulate modes; `flags` = 0x8000 | cfg<<8 | bm_class<<16 overrides the
 * tile shape for this process (0 = keep). */
int dissc_conv_bench(int B, int Cin, int Cout, int k, int dilation, int L, int epi, int iters,
                     int flags, float* ms_out);

/* Diagnostics / tests (not on the product path): ONE residual pair of a ResBlock1,
 *   y = x + conv_1(lrelu(conv_d(lrelu(x))))          (reference sr/models.py:34-41; `epi` 1 = that, 2..4 = the MRF modes on `acc`)
 * on device data x / y / acc f32 [B,C,ld] with host weights [C,C,k] + biases [C], through a chosen implementation:
 * mode 0 = two direct conv launches, 1 = the fused direct pair (C = 16 / 32), 2 = two transform-domain launches
 * (conv_wino), 3 = the fused transform-domain pair (C = 16 with k = 11, C = 32 with k = 7 / 11, C = 64 with k = 3 / 7 / 11, in
 * the form dissc_pair_info reports under the current options), 4 = two transform-domain launches in the forms the generator's
 * plan gives the shape under the current options when it does not fuse the pair (F(4,3) on conv_wino, F(6,3) or F(5,4) on
 * conv_wino8, per conv), 5 = two direct launches packed for split-bf16 (conv_bf3_kernel, the epilogue on the second: how the
 * generator runs its 128- and 256-channel pairs under "precision" = 1; DISSC_EINVAL where the shape gets no such instance).
 * y must not alias x.  dissc_respair1d synchronises the stream; dissc_pair_bench times `iters` launches on synthetic data. */
int dissc_respair1d(const float* x, const float* w1_host, const float* b1_host, const float* w2_host, const float* b2_host,
                    float* y, float* acc, const int32_t* lengths, int B, int C, int k, int dilation, int ld, int Lmax,
                    float slope, int epi, float mrf_div, int mode, void* stream);
int dissc_pair_bench(int B, int C, int k, int dilation, int L, int epi, int iters, int mode, float* ms_out);
/* What mode 3 of the two would build for (C, k, dilation) under the current option defaults: `form_out` 1 = the register-only
 * F(2,3) pair, 2 = the register-only six-point pair, 0 = the F(4,3) pair kernel (DISSC_EXPERIMENTAL=1 builds); `tile_out` the
 * outputs one workgroup of that instance owns (0 for form 0).  DISSC_EINVAL where mode 3 has no instance.  Host only: no GPU
 * is touched. */
int dissc_pair_info(int C, int k, int dilation, int* form_out, int* tile_out);
/* ONE ResBlock2 (y1 = x + conv_d0(lrelu(x)), y2 = y1 + conv_d1(lrelu(y1)); reference sr/models.py:50-65) on device data x [B][C][ld]
 * with host weights [C][C][k] and biases [C], packed per call: epi 1 writes y2 to y, epi 2 / 3 / 4 (the MRF modes) update acc.
 * mode 0 = two direct conv launches, mode 1 = the one-launch kernel (csrc/resblock2.hip; C = 32 / 16 and (k; d0, d1) = (3; 1, 2),
 * (5; 2, 6), (7; 3, 12): DISSC_EINVAL for any other shape); the two are bit-identical.  Tests / diagnostics; synchronous. */
int dissc_resblock2_1d(const float* x, const float* w1_host, const float* b1_host, const float* w2_host, const float* b2_host, float* y,
                       float* acc, const int32_t* lengths, int B, int C, int k, int d0, int d1, int ld, int Lmax, float slope, int epi,
                       float mrf_div, int mode, void* stream);
/* per-launch time (ms, the average of `iters` runs after two warm-up runs) of one ResBlock2 in mode 0 / 1 on B synthetic utterances of L columns */
int dissc_resblock2_bench(int B, int C, int k, int d0, int d1, int L, int epi, int iters, int mode, float* ms_out);
/* HOST ONLY: the form a (C; k; d0, d1) ResBlock2 takes in an fp32 generator handle created under the current options -- 0 = two direct
 * conv launches, 1 = one launch (option rb2_fused) -- and the outputs one workgroup of the one-launch form owns (0 for form 0). */
int dissc_resblock2_info(int C, int k, int d0, int d1, int* form_out, int* tile_out);
/* The launches dissc_conv1d (up = 1: Cin -> Cout, k taps, `dilation`) or dissc_conv_transpose1d (up > 1: k taps, stride `up`,
 * dilation 1) makes on a batch of B utterances of at most Lmax_out columns per launch (for a ConvTranspose: INPUT columns), under
 * the current option defaults: one for a conv, one per group of output phases for a ConvTranspose.  Per launch: the kernel
 * family (16 = conv_mfma_kernel, 32 = conv_mfma32_kernel), the tile shape id in force after the overrides' clamps and the
 * small-grid step-down, its BM x BN, the GEMM rows (Cout, or Cout * np), and for a ConvTranspose the phases [p0, p0 + np) of
 * the group, its input taps `ntap` and the left padding of its conv (np = 1, p0 = 0, ntap = k and (k - 1) dilation / 2 for a conv).
 * The answer comes from the launch path's own planning functions.  Up to max_out entries are written, *n_out is the number of
 * launches.  DISSC_EINVAL for the layers that run on a special instance with a fixed tile (taps spanning more than 60 columns,
 * the big 1x1 layers).  Host only: no GPU is touched. */
typedef struct {
  int32_t family, cfg, bm, bn, rows;
  int32_t p0, np, ntap, pad_left;
} DisscConvLaunch;
int dissc_conv_info(int Cin, int Cout, int k, int dilation, int up, int B, int Lmax_out, DisscConvLaunch* out, int max_out,
                    int* n_out);

/* The conv_wino8_kernel instance and grid that a C -> C conv of k taps and `dilation` launches in its eight-point Toom-Cook form
 * -- R = 3: F(6,3), R = 4: F(5,4) -- on a batch of B utterances of at most Lmax columns, under the current option defaults
 * ("small_grid", "wino8_c64_wide"): the tile of (32 mi) rows x (32 ni) columns built for `wps` waves per SIMD, ns = ceil(k / r)
 * sub-filters, `unit` = (9 - r) dilation ns outputs per transform unit, `ot` outputs per tile (a multiple of unit), `cpr` input
 * channels staged per round, gx = ceil(Lmax / ot) time tiles of the longest utterance and gy = C / (32 mi) row tiles (a divisor of
 * 8).  The answer is the launch path's own plan, the widths those of the instance itself.  DISSC_EINVAL for a shape without an
 * instance.  Host only: no GPU is touched. */
typedef struct {
  int32_t mi, ni, wps, r, ns;
  int32_t unit, ot, cpr, gx, gy;
} DisscWino8Plan;
int dissc_wino8_info(int C, int k, int dilation, int R, int B, int Lmax, DisscWino8Plan* out);
/* Which form of that instance the same launch takes under the current option defaults ("wino8_sv"): *shared_out = 1 where the
 * eight waves of a workgroup share one input transform (the 128 x 64 tile, mi = 4, ni = 2, wps = 2, of a k = 7 / 11 shape), 0 where
 * every wave forms its own tile.  The answer is the launch path's own choice.  DISSC_EINVAL as dissc_wino8_info.  Host only: no GPU
 * is touched.  (Added without a new ABI number: nothing that existed changed.) */
int dissc_wino8_form(int C, int k, int dilation, int R, int B, int Lmax, int* shared_out);

/* The conv_wino_kernel instance and grid that a C -> C conv of k taps and `dilation` launches in its six-point Toom-Cook form
 * F(4,3) (what dissc_conv1d runs under "wino" = 2 with "wino8" below 2, both launches of mode 2 of dissc_respair1d, and the
 * generator's ConvForm::f43 layers) on a batch of B utterances of at most Lmax columns, under the current option defaults
 * ("small_grid", "wino_sv"): ns = ceil(k / 3) sub-filters, `cpr` input channels staged per barrier round, `rh` row halves (and
 * 3 - rh column halves) of wave tiles of (32 tw) rows x (32 tw) columns, `shv` 1 = the transform shared between the waves;
 * `unit` = 4 dilation ns outputs per tile unit, `ot` = unit * floor(32 tw / (dilation ns)) * (3 - rh) outputs per workgroup tile,
 * gx = ceil(Lmax / ot) time tiles of the longest utterance, gy = C / (32 tw rh) row tiles (a divisor of 8), `wgs` workgroups in
 * the grid, `lds_bytes` of dynamic LDS (at most 160 KB).  The answer is the launch path's own plan, the widths those of the
 * instance itself.  C = 64 / 128 / 256 / 512, k = 3 / 7 / 11, dilation 1 / 3 / 5; C = 32 is answered too: no layer takes it, it is
 * the diagnostic instance mode 2 of dissc_respair1d runs.  DISSC_EINVAL for any other shape, B < 1 or Lmax < 1.  Host only: no GPU
 * is touched. */
typedef struct {
  int32_t ns, dilation, cpr, rh, tw, shv;
  int32_t unit, ot, gx, gy, wgs, lds_bytes;
} DisscWinoPlan;
int dissc_wino_info(int C, int k, int dilation, int B, int Lmax, DisscWinoPlan* out);

/* Diagnostics / tests: residual pairs [m0, m1) of ONE ResBlock1 (three pairs x_k += conv_1(lrelu(conv_d(lrelu(x_k)))), d =
 * dil3[0..2]) in split-bf16 arithmetic on resblock_bf3_kernel (csrc/resblock_bf3.hip), as the generator launches it under
 * "precision" = 1: the whole block (m0 = 0, m1 = 3; C = 16 / 32) or one pair per launch chained through epi 0 (C = 64).
 * x f32 [B,C,ld] on the device; w6_host / b6_host: six HOST pointers [C,C,k] / [C] in execution order (c1_0, c2_0, c1_1, c2_1,
 * c1_2, c2_2); acc f32 [B,C,ld] on the device, updated on [0, len) only: epi 0 acc = x_k (a partial block), 2 acc = x_k, 3 acc += x_k,
 * 4 acc = (acc + x_k) / mrf_div.  DISSC_EINVAL with a message, nothing launched: C not 16 / 32 / 64, k not 3 / 7 / 11, a dilation
 * outside 1 .. 5, m0 >= m1 or outside [0, 3], another epi, B or Lmax <= 0, ld < 4 or no multiple of 4, x or acc not 16-byte
 * aligned, acc aliasing x.  Synchronises the stream. */
int dissc_resblock1d_bf3(const float* x, const float* const* w6_host, const float* const* b6_host, float* acc,
                         const int32_t* lengths, int B, int C, int k, const int32_t* dil3, int ld, int Lmax, float slope,
                         int epi, float mrf_div, int m0, int m1, void* stream);
/* Diagnostics / tests: ONE k = 3 ResBlock1 -- three residual pairs of dilations dil3 -- on device data with host weights, as
 * dissc_resblock1d_bf3 takes them; y (epi = 1, EPI_RES; must not alias x) or acc (the MRF modes 2 / 3 / 4) receives the block's
 * output.  mode 0 = three launches, every pair in the one-launch form the generator gives it without "chain_f23", x_1 / x_2
 * through scratch; mode 1 = the one-launch F(2,3) chain, DISSC_EINVAL (nothing written) where the shape has no instance
 * (instances: C = 16 / 32, k = 3, dilations (1, 3, 5)).  dissc_reschain1d synchronises the stream; dissc_chain_bench times `iters`
 * launches of a k = 3, dilations (1, 3, 5) block on synthetic data.  dissc_chain_info reports the chain kernel's geometry: the
 * outputs a workgroup owns, the span it computes in every pair, the halo per side ((span - wout) / 2), its LDS bytes and the
 * column tiles per wave.  Host only: no GPU is touched. */
int dissc_reschain1d(const float* x, const float* const* w6_host, const float* const* b6_host, float* y, float* acc,
                     const int32_t* lengths, int B, int C, int k, const int32_t* dil3, int ld, int Lmax, float slope, int epi,
                     float mrf_div, int mode, void* stream);
typedef struct {
  int wout, span, halo, lds_bytes, tiles_per_wave;
} DisscChainInfo;
int dissc_chain_info(int C, int k, const int32_t* dil3, DisscChainInfo* out);
int dissc_chain_bench(int B, int C, int L, int epi, int iters, int mode, float* ms_out);
/* What the generator's split-bf16 kernels would launch, answered by the planning functions the launches themselves call.
 * dil3 == NULL: the conv_bf3_kernel tile of a Cin -> Cout conv of k taps and `dilation` (for a phase group of a ConvTranspose:
 * its GEMM rows and taps as dissc_conv_info reports them, dilation 1) on B utterances of at most Lmax columns under the current
 * option defaults ("small_grid"): bm x bn, `tile` its index in the kernel's table (0 .. 3 by row class 32 / 64 / 128 / 256),
 * small_grid = 1 where a layer of >= 128 rows steps down to the 64 x 128 tile; DISSC_EINVAL where the layer gets no split-bf16
 * instance.  dil3 != NULL: the resblock_bf3_kernel window of pairs [m0, m1) of a block of C = Cout channels and k taps (Cin,
 * dilation, B, Lmax unused): `cols` window columns per workgroup, `pad` LDS padding columns on each side, `h4` halo columns on
 * each side, bn = cols - 2 h4 centre columns written.  Host only: no GPU is touched. */
typedef struct {
  int32_t bm, bn, small_grid, tile;
  int32_t cols, h4, pad;
} DisscBf3Info;
int dissc_bf3_info(int Cout, int Cin, int k, int dilation, int B, int Lmax, const int32_t* dil3, int m0, int m1,
                   DisscBf3Info* out);

/* ------------------------------------------------------------------------- *
 * Length / pitch predictors and infer.py's integer sample logic.
 * Replaces: LenPredictor.forward (reference model/len_predictor.py:35-52),
 *   PitchPredictor / PitchPredictorBase .infer_freq (model/pitch_predictor.py:72-104,
 *   145-176), dedup_seq (dataset/utils.py:14-16), len_carryover_correction
 *   (infer.py:158-172), torch.repeat_interleave (infer.py:32).
 * The reference runs B=1 per (utterance x target); these take a ragged batch
 * (lengths i32 [B], NULL = all Lmax) and are sample-exact with B=1 runs.
 * ------------------------------------------------------------------------- */
typedef struct dissc_pred* dissc_pred_t;
/* kind: 0 = LenPredictor, 1 = PitchPredictor ("new", positional encoding, BN on cnn2),
 * 2 = PitchPredictorBase.  weights: the state_dict tensors by name; every eval-mode
 * BatchNorm is passed pre-folded as "<conv>.bn_scale" / "<conv>.bn_shift"
 * (alpha = weight/sqrt(var+eps), beta = bias - mean*alpha). */
int dissc_pred_create(int kind, const DisscTensor* weights, size_t n_weights, dissc_pred_t* out);
void dissc_pred_destroy(dissc_pred_t p);
size_t dissc_pred_workspace_bytes(dissc_pred_t p, int B, int Lmax);
/* LenPredictor.norm_mean / norm_std (reference infer.py:72: len_norm_stats.pth) */
int dissc_len_set_norm(dissc_pred_t p, float mean, float std);
/* seq i64 [B,Lmax] dedup'd units, spk i64 [B] -> out f32 [B,ldo] frames per unit */
int dissc_len_forward(dissc_pred_t p, const int64_t* seq, const int64_t* spk, const int32_t* lengths,
                      int B, int Lmax, float* out, int ldo, void* workspace, size_t workspace_bytes,
                      void* stream);
/* seq i64 [B,Tmax] frame-rate units -> out f32 [B,ldo]: (class_logit > 0) * f0; norm != 0 keeps
 * the speaker-normalised value, else f0*id2std[spk] + id2mean[spk] (device arrays of n_stats
 * entries; ids are clamped into them -- the Python wrapper raises IndexError first, like
 * nn.Embedding does in the reference). */
int dissc_pitch_forward(dissc_pred_t p, const int64_t* seq, const int64_t* spk,
                        const int32_t* lengths, int B, int Tmax, int norm, const float* id2mean,
                        const float* id2std, int n_stats, float* out, int ldo, void* workspace,
                        size_t workspace_bytes, void* stream);
/* Per-speaker F0 statistics over VOICED (non-zero) frames, fp64 (replaces reference
 * data/data_utils.py:33-46 calculate_pitch_stats, the step between data/encode.py and infer.py).
 * f0 f64 [offsets[n_speakers]]: the frames grouped by speaker, speaker s = [offsets[s], offsets[s+1]);
 * -> mean, std (population, ddof = 0) f64 [n_speakers], count of voiced frames i64 [n_speakers].
 * A speaker without voiced frames yields NaN like numpy.  Deterministic (fixed reduction tree). */
int dissc_pitch_stats(const double* f0, const int64_t* offsets, int n_speakers, double* mean_out,
                      double* std_out, int64_t* count_out, void* stream);
/* run-length encode: units i64 [B,Tmax] -> vals i64 [B,Tmax], counts i32 [B,Tmax], n i32 [B] */
int dissc_dedup(const int64_t* units, const int32_t* lengths, int B, int Tmax, int64_t* vals,
                int32_t* counts, int32_t* n_out, void* stream);
/* error-diffusion rounding of predicted lengths: lens f32 [B,ld] (n[b] valid) ->
 * lens_int i32 [B,ld], totals i32 [B] = frames after expansion */
int dissc_len_carryover(const float* lens, const int32_t* n, int B, int ld, int32_t* lens_int,
                        int32_t* totals, void* stream);
/* repeat_interleave: vals i64 [B,ld_in], lens_int i32 [B,ld_in] -> out i64 [B,ld_out] */
int dissc_expand(const int64_t* vals, const int32_t* lens_int, const int32_t* n, int B, int ld_in,
                 int64_t* out, int ld_out, void* stream);

/* ------------------------------------------------------------------------- *
 * HuBERT-base unit encoder + k-means quantiser.
 * Replaces: textless SpeechEncoder.__call__ as used at reference data/encode.py:21-22,32
 *   = fairseq HubertModel.extract_features(source, mask=False, output_layer=n_layers)
 *   + KMeansQuantizer.predict.  Those libraries are un-vendored third parties (fairseq @
 *   dd106d95, textlesslib HEAD; reference README.md:31-34); the algorithm is restated in
 *   oracle/hubert_ref.py and pinned to HF transformers.HubertModel + sklearn KMeans.
 * weights: fairseq checkpoint names ("feature_extractor.conv_layers.{i}.0.weight",
 *   "feature_extractor.conv_layers.0.2.weight/bias", "layer_norm.*", "post_extract_proj.*",
 *   "encoder.pos_conv.0.weight" (weight-norm already folded, [768,48,128]) / ".bias",
 *   "encoder.layer_norm.*", "encoder.layers.{i}.self_attn.{q,k,v,out}_proj.*",
 *   ".self_attn_layer_norm.*", ".fc1.*", ".fc2.*", ".final_layer_norm.*").
 * centers: host f32 [n_centers,768] k-means centroids (NULL = dense features only).
 * ------------------------------------------------------------------------- */
typedef struct dissc_hubert* dissc_hubert_t;
int dissc_hubert_create(int n_layers, const DisscTensor* weights, size_t n_weights,
                        const float* centers, int n_centers, dissc_hubert_t* out);
/* the same with the handle's arithmetic given explicitly instead of read from the process-wide "enc_precision" option:
 * -1 = that option, 0 = exact fp32, 1 = split-bf16 (opt-in, see dissc_set_option); anything else DISSC_EINVAL */
int dissc_hubert_create_ex(int n_layers, const DisscTensor* weights, size_t n_weights, const float* centers, int n_centers,
                           int precision, dissc_hubert_t* out);
/* the handle's arithmetic: 0 = fp32, 1 = split-bf16 */
int dissc_hubert_precision(dissc_hubert_t m);
void dissc_hubert_destroy(dissc_hubert_t m);
/* frames produced for n_samples input samples: floor((n-400)/320)+1 for n >= 400 */
int dissc_hubert_frames(int n_samples);
size_t dissc_hubert_workspace_bytes(dissc_hubert_t m, int B, int Nmax);
/* wav f32 [B,Nmax] (16 kHz, un-normalised like hubert-base), n_samples i32 [B] (NULL = Nmax)
 * -> dense_out f32 [B,768,ldT] channels-first, ldT = frames(Nmax) rounded up to 4 (may be NULL)
 *    units_out i64 [B,frames(Nmax)] (may be NULL).  Each utterance is exact w.r.t. a B=1 run.
 * A model handle is SINGLE-STREAM: the part streams and fork/join events of the split forward belong to the handle, so
 * two forwards of one handle must not be in flight at once (create one handle per concurrent stream).  On error, `stream`
 * has already been made to wait for every part stream that received work: the workspace may be reused once it drains. */
int dissc_hubert_forward(dissc_hubert_t m, const float* wav, const int32_t* n_samples, int B, int Nmax,
                         float* dense_out, int64_t* units_out, void* workspace,
                         size_t workspace_bytes, void* stream);
/* The quantiser's predict() on its own -- the integer step of the path (reference data/encode.py:21-22: textless
 * KMeansQuantizer -> sklearn predict), the very launch dissc_hubert_forward makes on its own features:
 *   units[t] = the FIRST k minimising  cnorm[k] - 2 <dense[t], centers[k]>,
 * every dot product ONE fp32 fma chain acc = fmaf(x[d], c[d], acc) over d = 0..D-1 from 0, k scanned upwards with a strict '<'
 * from +inf (a NaN score never wins; a row of NaNs gets unit 0) -- specified to the bit, so that identical inputs give identical
 * indices on any implementation (oracle/host_ref.c: oracle_kmeans_assign_f32), exact ties included.
 * dense f32 [T,D] rows, centers f32 [K,D], cnorm f32 [K] (NULL = computed here as the chain fmaf(c[d], c[d], s); then the call
 * allocates and synchronises), units int64 [T]: device pointers. */
int dissc_kmeans_assign(const float* dense, const float* centers, const float* cnorm, int T, int K, int D, int64_t* units,
                        void* stream);

/* Diagnostics: sustained fp32 v_mfma_f32_16x16x4_f32 rate (TFLOP/s) of this GPU at its
 * real clocks -- the practical ceiling the conv kernels are compared with. */
int dissc_mfma_peak(int iters, float* tflops);
/* Diagnostics: y[i] = erf(x[i]) as the GELU epilogues evaluate it (branch-free, < 1 ulp; HuBERT's exact-erf GELU,
 * arch per HF:154-213,371-445 [3P]); x, y: device f32 [n]. */
int dissc_erf_check(const float* x, float* y, int n, void* stream);
/* Diagnostics: the encoder's fused self-attention (exact softmax, fp32; the launch dissc_hubert_forward makes) on its own.
 * qkv f32 [B][3D][ld] channels-first (rows Q | K | V; head h owns rows 64h .. 64h + 63 of each; Q already scaled by 1/8, as the
 * forward's qkv GEMM leaves it), lens i32 [B] frames per utterance (each <= Tmax <= ld, ld % 4 == 0), H = D / 64 heads
 * -> out f32 [B][D][ld]: columns t < lens[b] written, the rest untouched.  Device pointers; asynchronous on `stream`. */
int dissc_attention(const float* qkv, const int32_t* lens, int B, int Tmax, int D, int ld, float* out, void* stream);
/* Diagnostics: the encoder's LayerNorm over the channels of a channels-first tensor (fp32, moments of the row shifted by one
 * of its own values; the launch the forward makes 14 times): x f32 [B][C][ld] (C % 16 == 0, C <= 768), gamma / beta f32 [C],
 * lens i32 [B] (each <= ld) -> y f32 [B][C][ld]: columns t < lens[b] written, the rest untouched.  Device pointers;
 * asynchronous on `stream`. */
int dissc_layernorm_cf(const float* x, const float* gamma, const float* beta, const int32_t* lens, int B, int C, int ld, float eps,
                       float* y, void* stream);
/* Diagnostics: ms[0] a pure-MFMA kernel alone, ms[1] a pure-fp32-VALU kernel alone, ms[2] both
 * at once on two streams (do the two pipes overlap on this part?). */
int dissc_pipe_overlap(int mfma_iters, int valu_iters, float* ms);

/* ------------------------------------------------------------------------- *
 * Waveform post-processing.
 * Replaces: generate(), reference sr/inference.py:73-75 ((y*32768).astype(int16),
 * C truncation + wrap) and librosa.util.normalize at :206/:250 (x / max|x|).
 * wav f32 [B,ld] (in place), lengths in SAMPLES per utterance.
 * ------------------------------------------------------------------------- */
int dissc_wav_postprocess(float* wav, const int32_t* n_samples, int B, int ld, void* stream);

/* ------------------------------------------------------------------------- *
 * Waveform exchange buffer (the payload of the path's all-gather).
 * Replaces: the per-worker file writes of the reference's Pool(8) (sr/inference.py:205-207,
 * 249-251,288-292,351-354).  Every rank packs the waveforms it decoded into ONE flat f32 buffer of
 * the same size on every rank (ragged: rows back to back, nothing padded to the longest waveform):
 *   floats [0,4)            int32 bits: {rows used, 0, data floats used lo, hi}
 *   floats [4, 4+4*n_cap)   table, one entry per row: int32 {job id (-1 = unused), sample count,
 *                           offset lo, offset hi} -- offset in floats from the start of the data region,
 *                           a multiple of 4 (the exclusive prefix sum of the sample counts rounded up to 4)
 *   floats [4+4*n_cap, ..)  data region: row r at its offset, zero-filled up to the next multiple of 4
 * The header and table are written by the host (a few KB, one H2D copy); dissc_pack_rows moves the B
 * utterances of one generator batch (wav f32 [B, ld_wav], n_samples i32 [B], offsets i64 [B], all device;
 * n_max = the largest sample count of the batch, sizes the launch) into the data region, 16 B per lane.
 * data must be 16-byte aligned.
 * ------------------------------------------------------------------------- */
int dissc_pack_rows(const float* wav, long long ld_wav, const int32_t* n_samples, const long long* offsets,
                    int B, int n_max, float* data, void* stream);

/* ------------------------------------------------------------------------- *
 * The path's one collective: the all-gather of the waveform exchange buffers over RCCL (xGMI inside a node).
 * Replaces: the reference's Pool(8) result hand-back (sr/inference.py:288-292,351-354: every worker writes its own
 * files, the parent joins) -- north_star's "single RCCL all-gather of decoded waveforms".  With these four entries a
 * maintainer who binds the C ABI alone (no torch.distributed) can run the multi-GPU path: pack with dissc_pack_rows,
 * gather with dissc_allgather_waves, unpack on the host (layout above).
 * librccl.so is NOT a link dependency of this library: the entries resolve ncclGetUniqueId / ncclCommInitRank /
 * ncclAllGather / ncclCommDestroy at first use from the RCCL the process already holds (PyTorch's, when it was imported
 * first), else from $DISSC_RCCL_LIB, librccl.so.1, /opt/rocm/lib/librccl.so.1 -- DISSC_ENOTSUP when none loads.
 *   dissc_comm_unique_id   rank 0 makes the 128-byte id (DISSC_COMM_ID_BYTES) and hands it to the other ranks out of band
 *   dissc_comm_create      collective over the nranks processes, each on its own current HIP device (RCCL: one GPU per rank);
 *                          *comm is an ncclComm_t
 *   dissc_allgather_waves  nccl_comm: an ncclComm_t -- from dissc_comm_create or any other owner (e.g. the one PyTorch's
 *                          ProcessGroupNCCL holds); send: n_floats f32 on this rank's device, recv: nranks * n_floats f32, rank r's
 *                          block at r * n_floats (send may alias its own block: in place); enqueued on `stream`, returns at once
 *                          (ordering and completion are the stream's); n_floats must be the same on every rank
 *   dissc_comm_destroy     after the stream has drained
 * ------------------------------------------------------------------------- */
#define DISSC_COMM_ID_BYTES 128
int dissc_comm_unique_id(void* id_out);
int dissc_comm_create(const void* id, int nranks, int rank, void** comm_out);
int dissc_comm_destroy(void* comm);
int dissc_allgather_waves(void* nccl_comm, const float* send, size_t n_floats, float* recv, void* stream);

/* ------------------------------------------------------------------------- *
 * YAAPT F0 tracker, device front end.
 * Replaces the numerically heavy stages of amfm_decompy.pYAAPT.yaapt as the reference calls it
 *   (get_yaapt_f0, reference sr/dataset.py:27-43; eval.py:26-33; inside textless' SpeechEncoder for
 *   data/encode.py:32): band-pass FIR of the signal and of its square, the per-frame spectra behind NLFER and
 *   the spectral-harmonics-correlation candidates, and the NCCF candidates.  amfm_decompy is an un-vendored
 *   third party that is absent offline: the algorithm is restated in oracle/yaapt_ref.py, PARITY UNPINNED.
 *   The short sequential stages (median smoothing, dynamic programming) are host logic in dissc_amd/f0.py.
 * fir: HOST f32 [n_taps] band-pass coefficients (scipy.signal.firwin in the caller, like amfm_decompy).
 * ------------------------------------------------------------------------- */
typedef struct {
  int32_t fs;            /* 16000 */
  int32_t frame_len;     /* samples: frame_length 20 ms -> 320 */
  int32_t frame_hop;     /* frame_space 5 ms -> 80 */
  int32_t tda_len;       /* tda_frame_length 25 ms -> 400 */
  int32_t nfft;          /* fft_length 8192 */
  float f0_min, f0_max;  /* 60, 400 */
  int32_t shc_numharms;  /* 3 */
  float shc_window_hz, shc_pwidth_hz, shc_thresh1, shc_thresh2, f0_double, f0_half; /* 40, 50, 5, 1.25, 150, 150 */
  float nccf_thresh1, nccf_thresh2; /* 0.25 (reference override), 0.9 */
  int32_t nccf_pwidth;   /* 5 */
} DisscYaaptConfig;
typedef struct dissc_yaapt* dissc_yaapt_t;
int dissc_yaapt_create(const float* fir, int n_taps, const DisscYaaptConfig* cfg, dissc_yaapt_t* out);
void dissc_yaapt_destroy(dissc_yaapt_t y);
/* frames of the spectral stages / of the time-domain stage for n_samples input samples; SHC bins per frame */
int dissc_yaapt_frames(dissc_yaapt_t y, int n_samples);
int dissc_yaapt_tda_frames(dissc_yaapt_t y, int n_samples);
int dissc_yaapt_shc_bins(dissc_yaapt_t y);
size_t dissc_yaapt_workspace_bytes(dissc_yaapt_t y, int B, int Nmax);
/* wav f32 [B,Nmax] (already zero-padded by frame_len/2 at both ends, as the reference does), n_samples i32 [B]
 * (NULL = Nmax), F = dissc_yaapt_frames(Nmax) ->
 *   filt, nlfilt f32 [B,Nmax]   band-passed signal / squared signal
 *   energy f32 [B,F]            NLFER band sums (un-normalised; 0 beyond an utterance's frames)
 *   cand_pitch, cand_merit f32 [B,F,4]   SHC peak candidates per frame (pitch 0 / merit 1 = no candidate)
 *   shc_out f32 [B,F,shc_bins]  optional (NULL): the SHC itself, for tests */
int dissc_yaapt_spectral(dissc_yaapt_t y, const float* wav, const int32_t* n_samples, int B, int Nmax, float* filt,
                         float* nlfilt, float* energy, float* cand_pitch, float* cand_merit, float* shc_out,
                         void* workspace, size_t workspace_bytes, void* stream);
/* NCCF candidates of `sig` (filt or nlfilt): frame f = sig[f*hop : f*hop + tda_len], lags lag_min[b,f] <= lag <
 * lag_max[b,f] (i32 [B,F], from the spectral track) -> pitch, merit f32 [B,F,3]; phi_out f32 [B,F,tda_len]
 * optional (NULL).  Frames beyond dissc_yaapt_tda_frames(n_samples[b]) give pitch 0 / merit 0.001. */
int dissc_yaapt_nccf(dissc_yaapt_t y, const float* sig, const int32_t* n_samples, const int32_t* lag_min,
                     const int32_t* lag_max, int B, int Nmax, int F, float* pitch, float* merit, float* phi_out,
                     void* workspace, size_t workspace_bytes, void* stream);

/* The sequential stages of the tracker, one workgroup per utterance, fp64 (pYAAPT's spec_track, refine and both
 * dynamic-programming passes as restated in oracle/yaapt_ref.py [3P-unverified]).  All pointers are device pointers.
 *   dissc_yaapt_spec_track: energy f32 [B,F], cand_pitch / cand_merit f32 [B,F,4] (dissc_yaapt_spectral's outputs),
 *     n_frames / n_tda i32 [B] (dissc_yaapt_frames / _tda_frames of each utterance) ->
 *     en_norm f64 [B,F] (NLFER / its mean), vuv u8 [B,F], spec f64 [B,F] (smoothed spectral F0 track),
 *     spec_std f64 [B], lag_min / lag_max i32 [B,F] (the NCCF search range of every time-domain frame)
 *   dissc_yaapt_final_track: the NCCF candidates of the band-passed signal (tp1, tm1) and of its square (tp2, tm2),
 *     f32 [B,F,3] each, plus the outputs above -> f0 f32 [B,F] (0 = unvoiced, 0 beyond n_tda[b]) */
typedef struct {
  double nlfer_thresh1, nlfer_thresh2; /* 0.75, 0.1 */
  double dp5_k1;                       /* 11 */
  double merit_boost, merit_pivot, merit_extra; /* 0.20, 0.99, 0.4 */
  double dp_w1, dp_w2, dp_w3, dp_w4;   /* 0.15, 0.5, 0.1, 0.9 */
  double spec_pitch_min_std;           /* 0.05 */
  double f0_min, f0_max;               /* 60, 400 */
  int32_t median_value;                /* 7 (odd, 3..9) */
  int32_t nccf_pwidth;                 /* 5 */
  int32_t fs;                          /* 16000 */
  int32_t reserved;
} DisscYaaptTrackConfig;
size_t dissc_yaapt_track_workspace_bytes(int B, int F);
int dissc_yaapt_spec_track(const DisscYaaptTrackConfig* cfg, const float* energy, const float* cand_pitch,
                           const float* cand_merit, const int32_t* n_frames, const int32_t* n_tda, int B, int F,
                           double* en_norm, uint8_t* vuv, double* spec, double* spec_std, int32_t* lag_min,
                           int32_t* lag_max, void* workspace, size_t workspace_bytes, void* stream);
int dissc_yaapt_final_track(const DisscYaaptTrackConfig* cfg, const float* tp1, const float* tm1, const float* tp2,
                            const float* tm2, const double* en_norm, const uint8_t* vuv, const double* spec,
                            const double* spec_std, const int32_t* n_tda, int B, int F, float* f0, void* workspace,
                            size_t workspace_bytes, void* stream);

/* ------------------------------------------------------------------------- *
 * Prosody metrics on device-side F0 tracks (csrc/prosody_metrics.hip).
 * Replaces: the per-file numpy / scipy part of reference eval.py -- scipy.stats.wasserstein_distance on the two
 * zero-extended tracks (eval.py:96-102) and aligned_ffe with utils.interp's nearest-neighbour resampling
 * (eval.py:50-57, utils.py:39-45) -- restated in tests/eval_ref.py.
 * tracks f32 [n_rows, ld] on the device (dissc_yaapt_final_track's output, one row per waveform); the tables are
 * device i32 arrays of six columns per entry.  All arithmetic is IEEE double on the track values widened to double;
 * every pair / interval is reduced in a fixed order, so its result does not depend on the batch around it.
 * Asynchronous on `stream`, nothing is allocated.  The workspace queries return 0 today (every supported pair is
 * sorted in LDS); the arguments are the place of a global-memory form for longer pairs.
 *
 * dissc_track_emd: first Wasserstein distance of n_pairs pairs (row_a, n_a, len_a, row_b, n_b, len_b): sample a =
 *   tracks[row_a, 0:n_a] followed by len_a - n_a zeros (0 <= n_a <= min(len_a, ld), len_a >= 1), b alike; the sizes
 *   may differ.  emd_out f64 [n_pairs] = sum |cdf_a - cdf_b| * delta over the merged sorted values, cdf = count /
 *   size (scipy's definition); NaN for an entry that breaks the rules above.  max_pair_frames: an upper bound of
 *   len_a + len_b over the table, at most DISSC_EMD_MAX_PAIR_FRAMES (DISSC_EINVAL beyond: the pair would not fit
 *   the LDS of a workgroup); an entry above the bound given yields NaN.
 * dissc_track_ffe: F0-frame-error of n_intervals intervals (row_ref, lo_ref, hi_ref, row_syn, lo_syn, hi_syn),
 *   0 <= lo <= hi <= ld: the generated slice is resampled to the reference slice's length like utils.interp
 *   (nearest neighbour on two linspace(0, 1, .) grids, the lower index on a tie; a length-1 slice becomes
 *   target_len * value), ffe_out f64 [n_intervals] = share of frames with |(ref + 1e-4) / (syn + 1e-4) - 1| > 0.2,
 *   NaN for an empty reference slice.  status_out i32 [n_intervals]: 0, DISSC_FFE_EMPTY_SYN (empty generated slice,
 *   non-empty reference: the reference raises ValueError there; ffe_out is NaN) or DISSC_FFE_BAD_ENTRY.
 * ------------------------------------------------------------------------- */
#define DISSC_EMD_MAX_PAIR_FRAMES 40000
#define DISSC_FFE_EMPTY_SYN 1
#define DISSC_FFE_BAD_ENTRY 2
size_t dissc_track_emd_workspace_bytes(int n_pairs, int max_pair_frames);
int dissc_track_emd(const float* tracks, int n_rows, int ld, const int32_t* pairs, int n_pairs, int max_pair_frames,
                    double* emd_out, void* workspace, size_t workspace_bytes, void* stream);
size_t dissc_track_ffe_workspace_bytes(int n_intervals);
int dissc_track_ffe(const float* tracks, int n_rows, int ld, const int32_t* intervals, int n_intervals,
                    double* ffe_out, int32_t* status_out, void* workspace, size_t workspace_bytes, void* stream);

/* ------------------------------------------------------------------------- *
 * Band-limited sinc resampling.
 * Replaces: resampy.resample(data, sr, 16000) at reference data/preprocess.py:22 (and sr/dataset.py:226) --
 * an un-vendored third party; algorithm (Kaiser-windowed sinc table, linear table interpolation) restated in
 * oracle/preprocess_ref.py, PARITY UNPINNED.  All arrays fp64 on the device: x [n_orig] -> y [n_out],
 * ratio = sr_new / sr_orig, win / delta [nwin] = the (already ratio-scaled) filter table and its differences,
 * num_table = table entries per zero crossing (2^precision).
 * ------------------------------------------------------------------------- */
int dissc_resample(const double* x, int n_orig, double* y, int n_out, double ratio, const double* win,
                   const double* delta, int nwin, int num_table, void* stream);

/* ------------------------------------------------------------------------- *
 * Predictor training.
 * Replaces one iteration of the training loops: model.train() forward, LenSumLoss / PitchLoss, loss.backward(),
 *   torch.optim.Adam.step() -- reference train_len_predictor.py:57-68, train_f0_predictor.py:58-66,
 *   loss/len_loss.py:16-30, loss/pitch_loss.py:6-27, model/len_predictor.py:35-52, model/pitch_predictor.py:72-94,145-166.
 * kind: 0 LenPredictor, 1 PitchPredictor ("new"), 2 PitchPredictorBase.  tensors: the model's state_dict by name
 *   (HOST fp32, incl. the BatchNorm running statistics and "pe.pe"; num_batches_tracked is kept by the caller).
 * The random masks of train() mode are inputs: keep f32 [B,L] (1 = token embedding kept; NULL = all kept),
 *   pe_mult f32 [B,L,32] (PositionalEncoding dropout multipliers 0 or 1/(1-p); kind 1 only; NULL = none).
 * One step: seq i64 [B,L] (pad token = n_tokens), spk i64 [B], target f32 [B,L] (pad_value marks padding) -- device
 *   pointers; loss_out: device f32[1]; parameters, Adam moments and running statistics live in the handle.
 * ------------------------------------------------------------------------- */
typedef struct dissc_trainer* dissc_trainer_t;
int dissc_train_create(int kind, const DisscTensor* tensors, size_t n, dissc_trainer_t* out);
void dissc_train_destroy(dissc_trainer_t t);
int dissc_train_set_len_norm(dissc_trainer_t t, float mean, float std);          /* LenPredictor.norm_mean / norm_std */
int dissc_train_set_pitch_stats(dissc_trainer_t t, const float* id2mean, const float* id2std, int n);  /* host arrays */
size_t dissc_train_workspace_bytes(dissc_trainer_t t, int B, int L);
int dissc_train_step(dissc_trainer_t t, const int64_t* seq, const int64_t* spk, const float* target, const float* keep,
                     const float* pe_mult, int B, int L, float pad_value, float lr, float* loss_out, void* workspace,
                     size_t workspace_bytes, void* stream);
/* state access: tensors in a fixed order (trainable ones first); which = 0 value; trainable tensors only: 1 gradient
 * of the last step, 2 / 3 torch.optim.Adam's exp_avg / exp_avg_sq (DISSC_EINVAL for running statistics and "pe.pe") */
int dissc_train_num_tensors(dissc_trainer_t t);
const char* dissc_train_tensor_name(dissc_trainer_t t, int i);
long long dissc_train_tensor_numel(dissc_trainer_t t, int i);
long long dissc_train_steps(dissc_trainer_t t);
int dissc_train_read(dissc_trainer_t t, int i, int which, float* host_out, void* stream);
/* diagnostics: a buffer of this handle's LAST step, copied out of the caller's workspace (valid until the next step or
 * any other use of that workspace; DISSC_EINVAL before the first step).  layer: index in the engine's order (trunk, head
 * branches, scalar heads), or -1 = the embedding.  which: 0 conv output z, 1 activation a, 2 gradient w.r.t. a,
 * 3 gradient w.r.t. z -- [B][cout][ld] floats, ld = L rounded up to 4 (columns L .. ld-1 are padding and hold
 * nothing); 4 / 5 batch mean / 1/sqrt(var + eps) of the layer's BatchNorm, cout floats (DISSC_EINVAL for a layer
 * without BatchNorm).  layer -1: which 0 = x0, 2 = dx0, [B][64][ld].  A scalar head has which 0 (its output) and 3 (written
 * by the loss) only.  n: floats to copy, at most the buffer's size. */
int dissc_train_debug_read(dissc_trainer_t t, int layer, int which, float* host_out, size_t n, void* stream);

/* ------------------------------------------------------------------------- *
 * Log-mel spectrogram and the L1 distance between two of them (the vocoder's validation figure).
 * Replaces: mel_spectrogram, reference sr/dataset.py:46-69 (center=False), and the F.l1_loss on its outputs that
 *   sr/train.py:231-269 logs as validation/mel_spec_error.  Restated in tests/mel_ref.py.
 * dissc_mel_filterbank: librosa's default filterbank (Slaney scale, Slaney area normalisation), fp64
 *   [num_mels][n_fft / 2 + 1] into a HOST array; fmax <= 0 means sr / 2.  Host only, no GPU needed.
 * dissc_mel_create: host only as well (the packed bases go to the device with the handle's first launch, on the device
 *   current then; a handle serves that one device).  Supported: n_fft a multiple of 64 up to 2048, win <= n_fft,
 *   4 <= hop <= n_fft with n_fft - hop even (a multiple of 4 takes the faster 16-byte LDS reads), num_mels <= 128, 0 <= fmin < fmax <= sr / 2, and a tile of
 *   DISSC_MEL_TILE_FRAMES frames that fits the LDS; anything else is DISSC_EINVAL with a message.
 * dissc_mel_frames: n_samples / hop.
 * wav f32 [B][ld], n_samples_dev i32 [B] on the device (cut to ld).  An utterance needs n_samples > (n_fft - hop) / 2,
 *   or its mirror extension is undefined: the caller checks (the counts are on the device here); such an utterance has no
 *   frames, and a NaN sum.
 * dissc_mel_forward: mel_out f32 [B][num_mels][ldF], ldF >= ld / hop; columns at and beyond an utterance's frames are not
 *   written.  flags: DISSC_MEL_LINEAR = mel before the log.
 * dissc_mel_l1: a [B][lda], b [B][ldb], the same n_samples for both (cut to the shorter row) -> sum_out f64 [B] =
 *   sum over the utterance's frames x num_mels cells of |logmel(a) - logmel(b)|; neither mel is stored.  One fp32
 *   subtraction per cell, all additions in double in a fixed order: bit-reproducible, independent of the batch.
 * The gradient with respect to the samples (csrc/mel_grad.hip; the generator's mel loss, sr/train.py:154-176).  Nothing of a
 *   forward call is kept: re / im are recomputed per tile.  No atomics, a fixed summation order: bit-reproducible, an
 *   utterance's gradient does not depend on the batch.  Needs hop >= 8 and a tile's samples plus its overlap-add strip in
 *   the LDS (DISSC_EINVAL otherwise), and a 16-byte aligned workspace of dissc_mel_grad_workspace_bytes(h, B, Nmax)
 *   (Nmax: ld, or the shorter row).  The tile of the gradient is DISSC_MEL_GRAD_TILE_FRAMES frames.
 * dissc_mel_backward: the vector-Jacobian product of dissc_mel_forward (same wav, n_samples, flags): g_mel f32
 *   [B][num_mels][ldF], read only inside an utterance's frames -> grad_wav f32 [B][ldg], ldg >= ld; samples at and beyond
 *   n_samples, up to ld, are written as zero.  Log mode: a cell's cotangent is divided by the mel where mel > 1e-5f (the
 *   forward's own fp32 value and comparison) and dropped where it clamps.
 * dissc_mel_l1_grad: the fused training form.  a (target), b (generated), scale_dev f64 [B] = d loss / d sum_b ->
 *   sum_out f64 [B], the bits of dissc_mel_l1, and grad_b f32 [B][ldg] (ldg >= ldb) = scale_b d sum_b / d b, the bits of
 *   dissc_mel_backward(b) for the cotangent (float)scale_b * sign(logmel(b) - logmel(a)) with sign(0) = 0; neither mel
 *   is stored.
 * ------------------------------------------------------------------------- */
#define DISSC_MEL_TILE_FRAMES 64
#define DISSC_MEL_GRAD_TILE_FRAMES 64
#define DISSC_MEL_LINEAR 1
typedef struct dissc_mel* dissc_mel_t;
int dissc_mel_filterbank(int sr, int n_fft, int num_mels, double fmin, double fmax, double* out);
int dissc_mel_create(int sr, int n_fft, int num_mels, int hop, int win, double fmin, double fmax, dissc_mel_t* out);
void dissc_mel_destroy(dissc_mel_t h);
int dissc_mel_frames(dissc_mel_t h, int n_samples);
size_t dissc_mel_workspace_bytes(dissc_mel_t h, int B, int Nmax);
int dissc_mel_forward(dissc_mel_t h, const float* wav, int ld, const int32_t* n_samples_dev, int B, float* mel_out, int ldF,
                      int flags, void* workspace, size_t workspace_bytes, void* stream);
int dissc_mel_l1(dissc_mel_t h, const float* a, int lda, const float* b, int ldb, const int32_t* n_samples_dev, int B,
                 double* sum_out, void* workspace, size_t workspace_bytes, void* stream);
size_t dissc_mel_grad_workspace_bytes(dissc_mel_t h, int B, int Nmax);
int dissc_mel_backward(dissc_mel_t h, const float* wav, int ld, const int32_t* n_samples_dev, int B, const float* g_mel, int ldF,
                       int flags, float* grad_wav, int ldg, void* workspace, size_t workspace_bytes, void* stream);
int dissc_mel_l1_grad(dissc_mel_t h, const float* a, int lda, const float* b, int ldb, const int32_t* n_samples_dev, int B,
                      const double* scale_dev, double* sum_out, float* grad_b, int ldg, void* workspace, size_t workspace_bytes,
                      void* stream);

/* ------------------------------------------------------------------------- *
 * A differentiable, ragged, stride-1 "same" Conv1d layer (csrc/conv_grad.hip): the op 92 of the generator's 97 conv layers
 * are (conv_pre, the ResBlock convs, conv_post; reference sr/models.py:34-41, :98-114), for training the vocoder.
 *   y[b,:,t] = bias + sum_j w[:,:,j] . lrelu(x, in_slope)[b,:,t + j d - pad]  (+ add[b,:,t]),  pad = (k - 1) d / 2,
 *   with dissc_conv1d's conventions: x f32 [B][Cin][ldx], y / add / gy f32 [B][Cout][ldo], 16-byte aligned, ldx and ldo
 *   multiples of 4 and >= Lmax; lengths i32 [B] on the device or NULL (= Lmax); positions >= lengths[b] are read as zero
 *   and never written by the forward.
 * dissc_convgrad_create: HOST ONLY (no HIP call; the device buffers come with the first dissc_convgrad_set_weights).  k odd,
 *   k <= 11, (k - 1) dilation <= 60, 1 <= Cin, Cout <= 65535; anything else is DISSC_EINVAL with a message.  The handle
 *   snapshots the tuning options, as every handle does.
 * dissc_convgrad_set_weights: w_dev f32 [Cout][Cin][k] and bias_dev f32 [Cout] (NULL = no bias) are DEVICE pointers; packs the
 *   weights for the forward and, transposed and tap-flipped, for the data gradient, on the device.  The handle keeps only
 *   these packed copies: call it again whenever the weights changed, and before a backward if another layer that shares
 *   the handle ran in between.
 * dissc_convgrad_forward: the forward on the direct conv kernels, the bits of dissc_conv1d for the same weights; add may be
 *   NULL.
 * dissc_convgrad_partials: HOST ONLY.  The weight gradient's reduction over (utterance, time) is cut into chunks of
 *   DISSC_CONVGRAD_CHUNK positions; the (utterance, chunk) pairs, utterance-major with ceil(Lmax / chunk) chunks per
 *   utterance, are dealt in consecutive runs of *pairs_per_partial to *P partials, summed afterwards in a fixed order.
 *   Both are functions of (B, Lmax, Cin, Cout, k) only, never of lengths.
 * dissc_convgrad_workspace_bytes: bytes of the backward's workspace (the partials; at most 64 MB for every generator layer
 *   at B = 32 x 8 960 samples).
 * dissc_convgrad_backward: x and in_slope as in the forward, gy the gradient of y (read as zero beyond lengths).
 *   gx f32 [B][Cin][ldx] = (x > 0 ? 1 : in_slope) * conv^T(gy) (torch's rule at x = 0), zero from lengths[b] to ldx;
 *   gw f32 [Cout][Cin][k]; gb f32 [Cout].  Each may be NULL ("not needed"): its kernels are skipped.  The gradient of add is
 *   gy itself.  No atomics, fixed summation orders: bit-reproducible from call to call, and an utterance's gx does not
 *   depend on the batch it is in.  workspace: 16-byte aligned device memory, needed for gw / gb only.
 * ------------------------------------------------------------------------- */
#define DISSC_CONVGRAD_CHUNK 64
typedef struct dissc_convgrad* dissc_convgrad_t;
int dissc_convgrad_create(int Cin, int Cout, int k, int dilation, dissc_convgrad_t* out);
/* the same handle with (k - 1) dilation <= 72 admitted (ResBlock2 of HiFi-GAN V3: k = 7, dilation 12): spans above 60 run the
 * forward and the data gradient on the wide-span conv instances (256-column tiles for any row count) and the weight gradient on
 * instances with a 36-column halo; every span <= 60 runs what dissc_convgrad_create's handle runs.  What nn.conv1d creates. */
int dissc_convgrad_create_wide(int Cin, int Cout, int k, int dilation, dissc_convgrad_t* out);
/* dissc_convgrad_create_wide's handle with a precision: prec = 0 is exactly that handle; prec = 1 is the split-bf16 ("bf16x3")
 * layer: every fp32 operand v is split into hi = bf16(v), lo = bf16(v - hi) (round to nearest even) and every product is
 * hi*hi + hi*lo + lo*hi on v_mfma_f32_32x32x16_bf16 with fp32 accumulation.  Any other prec is DISSC_EINVAL.  HOST ONLY.  It
 * takes every shape create_wide takes; each DIRECTION of a prec = 1 handle runs split where there is an instance for it:
 *   forward        rows = Cout >= 32 and (k - 1) dilation <= 60 (conv_bf3_kernel; not the k = 1 layers of >= 256 rows and >= 128
 *                  columns, which have their own fp32 instance);
 *   data gradient  the same test with rows = Cin (conv_bf3_kernel on the transposed, tap-flipped weights, then the mask kernel);
 *   weight gradient  Cin >= 32, Cout >= 32 and (k - 1) dilation <= 60 (convgrad_wgrad_bf3_kernel, csrc/conv_grad_bf3.hip);
 * every other direction runs the fp32 kernels of the prec = 0 handle, with its bits.  The bias gradient is always the fp32
 * handle's.  set_weights packs the split A fragments on the device (convgrad_repack_bf3_kernel).  partials, workspace_bytes and
 * every contract of the backward (no atomics, fixed orders, gx independent of the batch) are those of the prec = 0 handle.
 * dissc_convgrad_precision_info: HOST ONLY.  split[0 .. 2] = 1 where the forward, the data gradient, the weight gradient of the
 * handle run split-bf16, 0 where they run fp32; answered by the functions the launches themselves consult. */
int dissc_convgrad_create_prec(int Cin, int Cout, int k, int dilation, int prec, dissc_convgrad_t* out);
int dissc_convgrad_precision_info(dissc_convgrad_t h, int32_t split[3]);
void dissc_convgrad_destroy(dissc_convgrad_t h);
int dissc_convgrad_set_weights(dissc_convgrad_t h, const float* w_dev, const float* bias_dev, void* stream);
int dissc_convgrad_forward(dissc_convgrad_t h, const float* x, const float* add, float* y, const int32_t* lengths, int B,
                           int ldx, int ldo, int Lmax, float in_slope, void* stream);
int dissc_convgrad_partials(dissc_convgrad_t h, int B, int Lmax, int* P, int* pairs_per_partial);
size_t dissc_convgrad_workspace_bytes(dissc_convgrad_t h, int B, int Lmax);
int dissc_convgrad_backward(dissc_convgrad_t h, const float* x, const float* gy, const int32_t* lengths, int B, int ldx,
                            int ldo, int Lmax, float in_slope, float* gx, float* gw, float* gb, void* workspace,
                            size_t workspace_bytes, void* stream);

/* ------------------------------------------------------------------------- *
 * A differentiable, ragged ConvTranspose1d layer (csrc/conv_grad_t.hip): the generator's five upsamplers ups[i]
 * (reference sr/models.py), the layers dissc_convgrad_* leaves out.  Added without an ABI bump, as the mel entries were.
 *   y[b,co,u] = bias[co] + sum_{ci,t,kk : stride t + kk - pad = u} w[ci,co,kk] lrelu(x, in_slope)[b,ci,t],  pad = (k - stride) / 2
 *   x f32 [B][Cin][ldx], y / gy f32 [B][Cout][ldo], 16-byte aligned, ldx and ldo multiples of 4, ldx >= Lmax and
 *   ldo >= stride Lmax.  lengths i32 [B] on the device or NULL (= Lmax) and Lmax are INPUT positions: utterance b has
 *   stride lengths[b] valid output positions; what lies beyond is read as zero and never written by the forward.
 * dissc_convtgrad_create: HOST ONLY.  1 <= stride <= 8, stride <= k <= 11, k - stride even, 1 <= Cin, Cout <= 65535; anything
 *   else is DISSC_EINVAL with a message that names the rule.
 * dissc_convtgrad_set_weights: w_dev f32 [Cin][Cout][k] (torch's ConvTranspose1d layout) and bias_dev f32 [Cout] (NULL = no
 *   bias) are DEVICE pointers; one kernel packs every phase group of the forward (the groups and packings of
 *   dissc_conv_transpose1d) and the data gradient's fragments.  Call it again whenever the weights changed.
 * dissc_convtgrad_forward: the bits of dissc_conv_transpose1d for the same weights.
 * dissc_convtgrad_partials / _workspace_bytes: HOST ONLY, as dissc_convgrad_*: chunks of DISSC_CONVGRAD_CHUNK INPUT positions.
 * dissc_convtgrad_backward: gx f32 [B][Cin][ldx] (times the leaky ReLU's derivative, torch's rule at x = 0; zero from
 *   lengths[b] to ldx), gw f32 [Cin][Cout][k], gb f32 [Cout]; each may be NULL and its kernels are skipped.  No atomics, fixed
 *   summation orders: bit-reproducible, and an utterance's gx does not depend on the batch it is in (it does on ldx: rows of
 *   fewer than 8 tiles of 32 x 128 split each reduction in two).
 * ------------------------------------------------------------------------- */
typedef struct dissc_convtgrad* dissc_convtgrad_t;
int dissc_convtgrad_create(int Cin, int Cout, int k, int stride, dissc_convtgrad_t* out);
void dissc_convtgrad_destroy(dissc_convtgrad_t h);
int dissc_convtgrad_set_weights(dissc_convtgrad_t h, const float* w_dev, const float* bias_dev, void* stream);
int dissc_convtgrad_forward(dissc_convtgrad_t h, const float* x, float* y, const int32_t* lengths, int B, int ldx, int ldo,
                            int Lmax_in, float in_slope, void* stream);
int dissc_convtgrad_partials(dissc_convtgrad_t h, int B, int Lmax_in, int* P, int* pairs_per_partial);
size_t dissc_convtgrad_workspace_bytes(dissc_convtgrad_t h, int B, int Lmax_in);
int dissc_convtgrad_backward(dissc_convtgrad_t h, const float* x, const float* gy, const int32_t* lengths, int B, int ldx,
                             int ldo, int Lmax_in, float in_slope, float* gx, float* gw, float* gb, void* workspace,
                             size_t workspace_bytes, void* stream);

/* ------------------------------------------------------------------------- *
 * A differentiable, ragged, STRIDED Conv1d layer (csrc/conv_grad_s.hip): the four Conv2d((5,1), stride (3,1)) layers of every
 * DiscriminatorP (reference sr/models.py:228-260) on the period-major rows of dissc_period_fold_fwd, the layers neither section
 * above can run.  Added without an ABI bump, as those were.
 *   y[b,co,q] = bias[co] + sum_{ci,kk} w[co,ci,kk] lrelu(x, in_slope)[b,ci,stride q + kk - pad],  pad = (k - 1) / 2
 *   x f32 [B][Cin][ldx], y / gy f32 [B][Cout][ldo], 16-byte aligned, ldx and ldo multiples of 4, ldx >= Lmax and
 *   ldo >= ceil(Lmax / stride).  lengths i32 [B] on the device or NULL (= Lmax) and Lmax are INPUT positions: utterance b has
 *   ceil(lengths[b] / stride) valid output positions (torch's own count for an input of lengths[b]: the last window reaches at
 *   most lengths[b] + 1, inside the conv's zero padding); input at and beyond lengths[b] is read as zero, y is never written at
 *   or beyond the output length and gy is read as zero there.
 * dissc_convsgrad_create: HOST ONLY.  k odd, 3 <= k <= 11, 2 <= stride <= min(k, 8), 1 <= Cin, Cout <= 65535; anything else is
 *   DISSC_EINVAL with a message that names the rule.
 * dissc_convsgrad_set_weights: w_dev f32 [Cout][Cin][k] and bias_dev f32 [Cout] (NULL = no bias) are DEVICE pointers; one kernel
 *   packs the A fragments of the forward and of the data gradient.  Call it again whenever the weights changed.
 * dissc_convsgrad_packed: the packings, for tests.  which = 0: the forward's, [ceil(Cout / 32)][k][ceil(Cin / 32) * 4][64][4]
 *   floats, element (blk, kk, c8, lane, e) = w[co = 32 blk + lane % 32][ci = 8 c8 + 2 e + lane / 32][kk]; which = 1: the data
 *   gradient's, [ceil(Cin / 32)][k][ceil(Cout / 32) * 4][64][4], = w[co = 8 c8 + 2 e + lane / 32][ci = 32 blk + lane % 32][kk];
 *   zero outside the weights.  Returns the number of floats (HOST ONLY with dst_dev NULL), after copying them to dst_dev
 *   otherwise; negative on error.
 * dissc_convsgrad_forward: one implicit-GEMM kernel on v_mfma_f32_32x32x2_f32 (Cin = 1 included, on zero-padded tiles).
 * dissc_convsgrad_partials / _workspace_bytes: HOST ONLY, as dissc_convgrad_*: Lmax in INPUT positions, chunks of
 *   DISSC_CONVGRAD_CHUNK OUTPUT positions, ceil(ceil(Lmax / stride) / chunk) per utterance.
 * dissc_convsgrad_backward: gx f32 [B][Cin][ldx] (times the leaky ReLU's derivative, torch's rule at x = 0; zero from
 *   lengths[b] to ldx), gw f32 [Cout][Cin][k], gb f32 [Cout]; each may be NULL and its kernels are skipped.  No atomics, fixed
 *   summation orders: bit-reproducible, and an utterance's y and gx depend neither on the batch it is in nor on the row strides.
 *
 * The period fold in front of the first layer (reference sr/models.py:245-250, period-major: every row is an independent 1-D
 * sequence, so the Conv2d stack over [B, C, H, p] is plain Conv1d layers on B p rows).
 * dissc_period_fold_fwd: wav f32 [B][ldw] with lengths[b] (i32 on the device, or NULL = T) valid samples -> x0 f32 [B p][ldh],
 *   x0[b p + w][h] = ypad_b[h p + w] for h < ceil(lengths[b] / p), ypad_b = utterance b reflect-padded at its own end
 *   (ypad[n + i] = y[n - 2 - i]); nothing is written beyond.  ldw >= T, ldh >= ceil(T / p).  The caller refuses the lengths
 *   torch's reflect pad refuses (0 < n <= p - n % p with n % p != 0).
 * dissc_period_fold_bwd: gwav [B][ldw] = the gather form, each sample its own place plus, where it is a reflect source, the
 *   padded place; zero from lengths[b] to ldw.  No atomics.
 * ------------------------------------------------------------------------- */
typedef struct dissc_convsgrad* dissc_convsgrad_t;
int dissc_convsgrad_create(int Cin, int Cout, int k, int stride, dissc_convsgrad_t* out);
void dissc_convsgrad_destroy(dissc_convsgrad_t h);
int dissc_convsgrad_set_weights(dissc_convsgrad_t h, const float* w_dev, const float* bias_dev, void* stream);
long long dissc_convsgrad_packed(dissc_convsgrad_t h, int which, float* dst_dev, void* stream);
int dissc_convsgrad_forward(dissc_convsgrad_t h, const float* x, float* y, const int32_t* lengths, int B, int ldx, int ldo,
                            int Lmax_in, float in_slope, void* stream);
int dissc_convsgrad_partials(dissc_convsgrad_t h, int B, int Lmax_in, int* P, int* pairs_per_partial);
size_t dissc_convsgrad_workspace_bytes(dissc_convsgrad_t h, int B, int Lmax_in);
int dissc_convsgrad_backward(dissc_convsgrad_t h, const float* x, const float* gy, const int32_t* lengths, int B, int ldx,
                             int ldo, int Lmax_in, float in_slope, float* gx, float* gw, float* gb, void* workspace,
                             size_t workspace_bytes, void* stream);
int dissc_period_fold_fwd(const float* wav, const int32_t* lengths, int B, int T, int period, int ldw, int ldh, float* x0,
                          void* stream);
int dissc_period_fold_bwd(const float* gx0, const int32_t* lengths, int B, int T, int period, int ldw, int ldh, float* gwav,
                          void* stream);

/* ------------------------------------------------------------------------- *
 * A differentiable, ragged, GROUPED, strided, wide-tap Conv1d layer (csrc/conv_grad_g.hip): the first six layers of every
 * DiscriminatorS (reference sr/models.py:285-307; k = 15 and 41, stride 1, 2 or 4, up to 16 groups), which the three sections
 * above cannot run.  Added without an ABI bump, as those were.
 *   y[b,co,q] = bias[co] + sum_{ci in group(co)} sum_kk w[co,ci,kk] lrelu(x, in_slope)[b,ci,stride q + kk - pad],
 *   pad = (k - 1) / 2: torch's F.conv1d(..., stride, padding=pad, groups).  Rows, lengths and strides as dissc_convsgrad_*: x f32
 *   [B][Cin][ldx], y / gy f32 [B][Cout][ldo], 16-byte aligned, ldx and ldo multiples of 4, ldx >= Lmax, ldo >= ceil(Lmax /
 *   stride); lengths i32 [B] on the device or NULL (= Lmax) and Lmax are INPUT positions, utterance b has ceil(lengths[b] /
 *   stride) outputs; input at and beyond lengths[b] is read as zero, y is never written at or beyond the output length and gy
 *   is read as zero there.
 * dissc_convggrad_create: HOST ONLY.  Accepted: k odd, 3 <= k <= 41; stride 1, 2 or 4; groups >= 1 dividing Cin and Cout;
 *   Cin / groups either 1 or a multiple of 8 up to 64; Cout / groups a multiple of 16 up to 128; 1 <= Cin, Cout <= 65535.
 *   Anything else is DISSC_EINVAL with a message that starts with the entry's name and names the rule.
 * dissc_convggrad_set_weights: w_dev f32 [Cout][Cin / groups][k] and bias_dev f32 [Cout] (NULL = no bias) are DEVICE pointers;
 *   one kernel packs the A fragments of the forward and of the data gradient.  Call it again whenever the weights changed.
 * dissc_convggrad_packed: the packings, for tests.  Taps are indexed by o' = kk - pad + PO, PO = pad rounded up to 4, four to a
 *   float4.  which = 0: the forward's, [groups][Cout / groups / 16][ceil(Cin / groups / 4)][K4 = (PO + pad) / 4 + 1][64][4]
 *   floats, element (g, rt, c4, k4, lane, e) = w[co = g cog + 16 rt + lane % 16][ci = 4 c4 + lane / 16][kk = 4 k4 + e - PO + pad];
 *   which = 1: the data gradient's, [groups][ceil(Cin / groups / 16)][Cout / groups / 4][K4][64][4], = w[co = g cog + 4 c4 +
 *   lane / 16][ci = 16 rt + lane % 16][kk]; zero outside the weights.  Returns the number of floats (HOST ONLY with dst_dev
 *   NULL), after copying them to dst_dev otherwise; negative on error.
 * dissc_convggrad_forward: one implicit-GEMM kernel per group on v_mfma_f32_16x16x4_f32, four accumulators per output added in a
 *   fixed order (Cin / groups = 1 included, on zero-padded tiles).
 * dissc_convggrad_partials / _workspace_bytes: HOST ONLY, as dissc_convsgrad_*: Lmax in INPUT positions, chunks of
 *   DISSC_CONVGRAD_CHUNK OUTPUT positions; the partials take at most 56 MB.
 * dissc_convggrad_backward: gx f32 [B][Cin][ldx] (times the leaky ReLU's derivative, torch's rule at x = 0; zero from
 *   lengths[b] to ldx), gw f32 [Cout][Cin / groups][k], gb f32 [Cout]; each may be NULL and its kernels are skipped.  No
 *   atomics, fixed summation orders: bit-reproducible, and an utterance's y and gx depend neither on the batch it is in nor on
 *   the row strides.
 *
 * The average pool between the scales, AvgPool1d(4, 2, padding=2) with count_include_pad (reference sr/models.py:315-318), on
 * B C rows x f32 [B][C][ldx] with lengths[b] (i32 on the device, or NULL = T) valid samples, each zero-padded at its own end.
 * dissc_mean_pool_fwd: out[j] = ((x[2 j - 2] + x[2 j - 1]) + (x[2 j] + x[2 j + 1])) * 0.25f for j <= floor(n / 2) (n >= 1;
 *   n = 0 has no output); nothing is written beyond.  ldx >= T, ldo >= T / 2 + 1, B C <= 65535.
 * dissc_mean_pool_bwd: gx[i] = 0.25f * (gy[floor(i / 2)] + gy[floor(i / 2) + 1]), gy read as zero at and beyond the output
 *   length; zero from lengths[b] to ldx.  The gather form: no atomics.
 * ------------------------------------------------------------------------- */
typedef struct dissc_convggrad* dissc_convggrad_t;
int dissc_convggrad_create(int Cin, int Cout, int k, int stride, int groups, dissc_convggrad_t* out);
void dissc_convggrad_destroy(dissc_convggrad_t h);
int dissc_convggrad_set_weights(dissc_convggrad_t h, const float* w_dev, const float* bias_dev, void* stream);
long long dissc_convggrad_packed(dissc_convggrad_t h, int which, float* dst_dev, void* stream);
int dissc_convggrad_forward(dissc_convggrad_t h, const float* x, float* y, const int32_t* lengths, int B, int ldx, int ldo,
                            int Lmax_in, float in_slope, void* stream);
int dissc_convggrad_partials(dissc_convggrad_t h, int B, int Lmax_in, int* P, int* pairs_per_partial);
size_t dissc_convggrad_workspace_bytes(dissc_convggrad_t h, int B, int Lmax_in);
int dissc_convggrad_backward(dissc_convggrad_t h, const float* x, const float* gy, const int32_t* lengths, int B, int ldx,
                             int ldo, int Lmax_in, float in_slope, float* gx, float* gw, float* gb, void* workspace,
                             size_t workspace_bytes, void* stream);
int dissc_mean_pool_fwd(const float* x, float* out, const int32_t* lengths, int B, int C, int T, int ldx, int ldo, void* stream);
int dissc_mean_pool_bwd(const float* gy, float* gx, const int32_t* lengths, int B, int C, int T, int ldx, int ldo, void* stream);

/* ------------------------------------------------------------------------- *
 * The rest of the generator's training step (csrc/gen_train.hip; composed in dissc_amd/nn.py's CodeGenerator): weight norm
 * of every layer at once, the embeddings, the MRF mean, the tanh tail.  Added without an ABI bump, as the sections above.
 * All device pointers f32 unless said otherwise; no atomics, fixed summation orders: bit-reproducible.
 *
 * Weight norm, w = g v / ||v|| per index of dim 0 (weight_norm(dim=0): for a ConvTranspose1d that is the INPUT channel;
 * reference sr/models.py wraps all 97 convs).  One launch per direction for up to 128 tensors.
 * dissc_wnorm_create: HOST ONLY.  n tensors of rows[i] x cols[i] (cols = the product of every dim but 0), each at least 1, at
 *   most 2^22 rows and 2^40 floats in all; anything else is DISSC_EINVAL with a message.  It fixes a flat layout: tensor i at
 *   the 16-byte aligned float offset off[i] (v, w and gv share it), its rows at row_off[i] in a flat per-row layout (g, gg
 *   and 1 / ||v|| share that); the row table goes to the device current at the first launch (a handle serves that device).
 * dissc_wnorm_offsets: HOST ONLY.  off / row_off: n entries each; the totals are the sizes of the two layouts (floats; the
 *   first a multiple of 4).  Each may be NULL.
 * dissc_wnorm_wave_cols: rows of up to this many columns are reduced by one wave, longer ones by a 256-thread workgroup.
 * dissc_wnorm_forward: writes w_flat (the alignment gaps are left alone) and 1 / ||v|| per row; v_flat and w_flat 16-byte
 *   aligned.  nbias > 0: the same launch copies bias_flat[0 .. nbias) to bias_out (the layers' biases next to their weights).
 * dissc_wnorm_backward: gw_ptrs is a HOST array of n DEVICE pointers, each layer's own weight gradient [rows][cols], 16-byte
 *   aligned; NULL = a zero gradient (its gv and gg are written as exact zeros).  The pointers travel in the kernel's
 *   arguments, 128 tensors per launch: nothing is uploaded per step.
 *   gg = (v . gw) / ||v||,  gv = (g / ||v||) (gw - v (v . gw) / ||v||^2).
 *   gb_ptrs (HOST array of n device pointers, or NULL = no biases): the same launch gathers bias_n[i] floats of each (NULL:
 *   zeros) into gb_flat, one after the other, each at the next multiple of 4 floats (the gaps are left alone).
 *   A row's sums (in double: a float product is then exact, and the kernels stay bandwidth bound): per-thread chains over
 *   (head to the next 16-byte boundary, float4s, tail), then a fixed butterfly; the order depends on cols and on the row's
 *   start modulo 4 floats, i.e. on (row index, cols) alone.  The backward sums ||v||^2 again in the pass that reads v for
 *   v . gw anyway, instead of taking the forward's fp32 1 / ||v|| (kept for the caller): gw - v (v . gw) / ||v||^2 cancels,
 *   entirely for a row of one column, and a norm rounded to fp32 in between would leave its rounding error there.
 *
 * Embeddings.  dissc_embed_concat_fwd: the generator's first kernel on DEVICE tables: x [B][C][ldx], C = E + (f0 ? 1 : 0) +
 *   (spkr ? E : 0), rows [dict_w[code] | f0 | spkr_w[spkr]]; code i64 [B][T], f0 f32 [B][T] or NULL, spkr i64 [B] or NULL; ids
 *   are clamped to the tables; nothing is written at or beyond lengths[b] (i32 [B] on the device, at most T, or NULL = T).
 * dissc_embed_concat_bwd: gx [B][C][ldx] ->  g_dict [n_codes][E] = sum over (b, t < lengths[b], code[b][t] = id) of
 *   gx[b][c][t], g_spkr [n_spk][E] = sum over (b: spkr[b] = id, t < lengths[b]) of gx[b][E + has_f0 + c][t]; both dense (rows
 *   of unused ids are exact zeros), ids clamped as the forward does; f0 gets no gradient.  One workgroup per table row, the
 *   summation order a function of (B, T) alone.  E <= 256; bad arguments are DISSC_EINVAL with a message, on the host.
 *
 * MRF mean over [B][C][ld] rows (ld a multiple of 4, 16-byte aligned; lengths i32 [B] on the device or NULL = Lmax):
 * dissc_mrf_mean_fwd: r = HOST array of nk (1 .. 4) device pointers; y = ((r0 + r1) + r2 ...) / nk with a true division;
 *   nothing written at or beyond lengths[b].
 * dissc_mrf_mean_bwd: gx = g / nk inside lengths[b], zero from there to ld; every branch takes the same tensor.
 * dissc_tanh_fwd: y [B][C][ldy] = tanh(x [B][C][ldx]) inside lengths; dissc_tanh_bwd: gx = gy (1 - y^2) from the saved
 *   output (y, gy with row stride ldy), zero from lengths[b] to ldx.
 * ------------------------------------------------------------------------- */
typedef struct dissc_wnorm* dissc_wnorm_t;
int dissc_wnorm_create(int n, const int* rows, const int* cols, dissc_wnorm_t* out);
void dissc_wnorm_destroy(dissc_wnorm_t h);
int dissc_wnorm_offsets(dissc_wnorm_t h, long long* off, long long* row_off, long long* total_floats, long long* total_rows);
int dissc_wnorm_wave_cols(void);
int dissc_wnorm_forward(dissc_wnorm_t h, const float* v_flat, const float* g_flat, float* w_flat, float* inv_norm,
                        const float* bias_flat, float* bias_out, int nbias, void* stream);
int dissc_wnorm_backward(dissc_wnorm_t h, const float* v_flat, const float* g_flat, const float* const* gw_ptrs, float* gv_flat, float* gg_flat, const float* const* gb_ptrs,
                         const int* bias_n, float* gb_flat, void* stream);
int dissc_embed_concat_fwd(const int64_t* code, const float* f0, const int64_t* spkr, const float* dict_w, const float* spkr_w,
                           const int32_t* lengths, int B, int T, int E, int n_codes, int n_spk, float* x, int ldx, void* stream);
int dissc_embed_concat_bwd(const float* gx, const int64_t* code, int has_f0, const int64_t* spkr, const int32_t* lengths, int B,
                           int T, int E, int n_codes, int n_spk, int ldx, float* g_dict, float* g_spkr, void* stream);
int dissc_mrf_mean_fwd(const float* const* r, int nk, float* y, const int32_t* lengths, int B, int C, int ld, int Lmax, void* stream);
int dissc_mrf_mean_bwd(const float* g, int nk, float* gx, const int32_t* lengths, int B, int C, int ld, int Lmax, void* stream);
int dissc_tanh_fwd(const float* x, float* y, const int32_t* lengths, int B, int C, int ldx, int ldy, int Lmax, void* stream);
int dissc_tanh_bwd(const float* y, const float* gy, float* gx, const int32_t* lengths, int B, int C, int ldx, int ldy, int Lmax,
                   void* stream);

/* ------------------------------------------------------------------------- *
 * The GAN losses on paired, ragged, pre-activation maps (csrc/gan_loss.hip; composed in dissc_amd/nn.py's
 * MultiPeriodDiscriminator, discriminator_loss, generator_loss and feature_loss; reference sr/models.py:352-383).  Added without
 * an ABI bump, as the sections above.
 *   A paired map is f32 [2 R][C][ld], 16-byte aligned, ld a multiple of 4: rows 0 .. R - 1 the real half, rows R .. 2 R - 1 the
 *   generated half, row r and row R + r with lengths[r] valid positions (i32 [R] on the device, clamped to 0 .. ld).  Positions at
 *   or beyond a length are never read for their value.  With v the valid positions and N = C sum_r lengths[r], a map's values are
 *     DISSC_GANLOSS_FM    2 / N sum_v |lrelu(real, slope) - lrelu(gen, slope)|            (feature_loss's term, times its 2)
 *     DISSC_GANLOSS_DISC  1 / N sum_v (1 - real)^2   and   1 / N sum_v gen^2              (discriminator_loss's r and g terms)
 *     DISSC_GANLOSS_GEN   1 / N sum_v (1 - gen)^2                                         (generator_loss's term)
 *   torch.mean of the reference at equal lengths.  N = 0: value 0, gradient 0.
 * All array arguments are HOST arrays of n entries (1 <= n <= DISSC_GANLOSS_MAX_MAPS), one per map: the map and lengths DEVICE
 *   pointers, R, C, ld, the op and the leaky ReLU's slope (read by FM only).  The records travel in the kernels' arguments:
 *   nothing is uploaded per call.  Anything else (a null pointer, n outside its range, R or C below 1, ld no positive multiple
 *   of 4, a map above 2^30 float4s per half, an unknown op) is DISSC_EINVAL with a message, before any launch.
 * dissc_ganloss_workspace_bytes: HOST ONLY, a function of the shapes alone (two doubles per workgroup of 1024 float4s per half,
 *   rounded up to 256 bytes); 0 on a bad argument.
 * dissc_ganloss_forward: out f32 [1 + 2 n] on the device: out[1 + m] and out[1 + n + m] are map m's first and second value
 *   (the second is 0 unless DISC), out[0] the sum of all of them in index order.  Stage 1 leaves one partial per workgroup in the
 *   workspace, stage 2 (one workgroup) sums each map's partials: lane l the partials l, l + 64, ... in index order, then a fixed
 *   butterfly.  Sums in double, no atomics: bit-reproducible, and a map's values do not depend on the list it is in.
 * dissc_ganloss_backward: gmaps[m] (DEVICE, [2 R][C][ld], or NULL = skip the map) receives the gradient with respect to the
 *   pre-activation map, both halves, exact zeros at and beyond every length.  The cotangent of map m's values is
 *   g_total[0] + g_vals[m] and g_total[0] + g_vals[n + m] (device pointers; either may be NULL = 0, not both).  The leaky ReLU's
 *   derivative is the slope at 0 (torch's rule), sign(0) = 0 (torch's abs); one rounding per element.
 * ------------------------------------------------------------------------- */
#define DISSC_GANLOSS_MAX_MAPS 64
#define DISSC_GANLOSS_FM 0
#define DISSC_GANLOSS_DISC 1
#define DISSC_GANLOSS_GEN 2
size_t dissc_ganloss_workspace_bytes(int n, const int* R, const int* C, const int* ld);
int dissc_ganloss_forward(int n, const float* const* maps, const int32_t* const* lengths, const int* R, const int* C,
                          const int* ld, const int* ops, const float* slopes, float* out, void* workspace, size_t workspace_bytes,
                          void* stream);
int dissc_ganloss_backward(int n, const float* const* maps, const int32_t* const* lengths, const int* R, const int* C,
                           const int* ld, const int* ops, const float* slopes, const float* g_total, const float* g_vals,
                           float* const* gmaps, void* stream);

/* ------------------------------------------------------------------------- *
 * Spectral norm of a list of weight matrices (csrc/spectral_norm.hip; composed in dissc_amd/nn.py's SpectralNorm and
 * MultiScaleDiscriminator; torch.nn.utils.spectral_norm as reference sr/models.py:288 applies it to discriminator 0 of the
 * MultiScaleDiscriminator).  Added without an ABI bump, as the sections above.  Tensor i is weight_orig seen as rows[i] x cols[i]
 * (cols = the product of every dim but 0), with the power iteration's vectors u (rows[i]) and v (cols[i]).
 * dissc_snorm_create: HOST ONLY.  1 .. 128 tensors, rows and cols at least 1, at most 2^22 rows, 2^26 columns and 2^32 floats in
 *   all; anything else is DISSC_EINVAL with a message.  It fixes three flat layouts, every entry 16-byte aligned: tensor i at the
 *   float offset off[i] (W, w and gW share it), its u at u_off[i], its v at v_off[i].  The tensor table and a workspace of
 *   doubles go to the device current at the first launch: a handle serves that device, and one stream at a time.
 * dissc_snorm_offsets: HOST ONLY.  off / u_off / v_off: n entries each; the totals are the sizes of the three layouts (floats,
 *   multiples of 4); state_floats = total_u + total_v + n rounded up to 4.  Each may be NULL.
 * dissc_snorm_chunk_rows / _span_cols / _wave_cols / _flat_span: HOST ONLY, the sizes at which the kernels change their walk: rows
 *   per partial chunk of W^T u; columns per workgroup span of W^T u and v; rows of up to wave_cols columns are reduced by one
 *   wave, longer ones by a 256-thread workgroup; elements per workgroup of the passes over a tensor as a flat array.
 * dissc_snorm_forward: with iterate = 1,  v = normalize(W^T u_in),  u = normalize(W v),  normalize(x) = x / max(||x||_2, 1e-12)
 *   (torch's F.normalize); with iterate = 0, u = u_in and v = v_in.  Then sigma = u . (W v) and w_out = W / sigma (a division).
 *   state_out = [u (total_u) | v (total_v) | sigma per tensor], freshly written; the alignment gaps of w_out and state_out are
 *   left alone, the inputs are never written (w_out / state_out equal to an input is DISSC_EINVAL).  All pointers 16-byte aligned.
 *   Six launches with an iteration, three without, whatever n.  Dots and norms in double, every sum in a fixed order, one rounding
 *   to float for u, v and sigma; no atomics: bit-reproducible, and a tensor's results do not depend on the list it is in.
 * dissc_snorm_backward: gw_orig (flat, as W) = gw / sigma - (sum gw o W / sigma^2) u v^T per tensor, u, v and sigma read from
 *   `state` as the forward wrote it (they are constants of the gradient, as torch holds them).  gw_ptrs is a HOST array of n DEVICE
 *   pointers, each tensor's own gradient [rows][cols], 16-byte aligned; NULL = a zero gradient (exact zeros are written).  The
 *   pointers travel in the kernels' arguments.  Three launches.
 * ------------------------------------------------------------------------- */
typedef struct dissc_snorm* dissc_snorm_t;
int dissc_snorm_create(int n, const int* rows, const int* cols, dissc_snorm_t* out);
void dissc_snorm_destroy(dissc_snorm_t h);
int dissc_snorm_offsets(dissc_snorm_t h, long long* off, long long* u_off, long long* v_off, long long* total_floats,
                        long long* total_u, long long* total_v, long long* state_floats);
int dissc_snorm_chunk_rows(void);
int dissc_snorm_span_cols(void);
int dissc_snorm_wave_cols(void);
int dissc_snorm_flat_span(void);
int dissc_snorm_forward(dissc_snorm_t h, const float* w_orig, const float* u_in, const float* v_in, int iterate, float* w_out,
                        float* state_out, void* stream);
int dissc_snorm_backward(dissc_snorm_t h, const float* w_orig, const float* state, const float* const* gw_ptrs, float* gw_orig,
                         void* stream);

/* ------------------------------------------------------------------------- *
 * AdamW over every leaf of an optimiser in one launch (csrc/adamw.hip; composed in dissc_amd/nn.py's AdamW).  Added without an ABI
 * bump, as the sections above.  The non-capturable single-tensor path of torch.optim.AdamW, amsgrad False, maximize False, per
 * element and in this order, every product and sum rounded on its own (nothing contracted):
 *   p *= 1 - lr wd;  m += (g - m)(1 - b1);  v = v b2 + ((1 - b2) g) g;  denom = sqrt(v) / sqrt(1 - b2^t) + eps;
 *   p -= (lr / (1 - b1^t)) (m / denom)
 * (m's line is torch's lerp_ for a weight 1 - b1 below 0.5, i.e. b1 > 0.5; at b1 <= 0.5 torch evaluates g - (g - m) b1, so the last
 * bits can differ there.)
 * Every scalar (1 - lr wd, 1 - b1, b2, 1 - b2, eps, lr / (1 - b1^t), sqrt(1 - b2^t)) is formed here in double and rounded once.
 * dissc_adamw_step: all six array arguments are HOST arrays of n entries (1 <= n <= dissc_adamw_max_tensors() = 16): the DEVICE
 *   pointers of p, g, m, v (four different f32 buffers of numel[i] >= 1 elements) and the step count t[i] >= 1 of THIS update,
 *   per tensor.  They travel in the kernel's arguments: nothing is uploaded per step.  A tensor whose four pointers are 16-byte
 *   aligned runs on float4s with a scalar tail, any other on scalars throughout; the bits are the same.  Workgroups take chunks of
 *   dissc_adamw_chunk() elements.  No atomics, each element written by one thread: bit-reproducible, and a tensor's results do not
 *   depend on the list it is in.  g is never written.  DISSC_EINVAL with a message before any launch: n outside its range, a null
 *   or repeated pointer, numel or t below 1, more than 2^30 chunks, lr / eps / weight_decay negative or NaN, a beta outside [0, 1).
 * ------------------------------------------------------------------------- */
int dissc_adamw_chunk(void);
int dissc_adamw_max_tensors(void);
int dissc_adamw_step(int n, float* const* p, const float* const* g, float* const* m, float* const* v, const long long* numel,
                     const long long* t, double lr, double b1, double b2, double eps, double weight_decay, void* stream);

/* ------------------------------------------------------------------------- *
 * The vocoder trainer's batch as one gather launch from a device-resident corpus (csrc/segment_gather.hip; composed in
 * dissc_amd/gan_train.py's SegmentSampler; CodeDataset.__getitem__ with eval_mode False, reference sr/dataset.py:240-267 and
 * 199-219).  Added without an ABI bump.
 * dissc_segment_create: HOST arrays; uploads to the current device, which the handle then serves.  U >= 1 utterances of
 *   frames[u] >= 1 frames after the trim, frames[u] hop < 2^31; packed one after the other: audio f32 (hop samples per frame),
 *   codes i32 and f0 f32 (one per frame), spkr i32 [U].  The frame offsets stay in the handle on both sides.
 * dissc_segment_interval_end: HOST ONLY.  The last legal start_step of an utterance at this segment, N' / hop - segment / hop with
 *   N' = frames hop 2^j the length after the doublings that reach the segment.
 * dissc_segment_gather: table is a HOST array of B (utterance, start_step) pairs of i32, 1 <= B <= dissc_segment_max_batch() =
 *   256, passed by value to the kernel.  Writes y f32 [B, 1, segment], code i64 [B, F], f0 f32 [B, 1, F], spkr i64 [B, 1], F =
 *   segment / hop, in one launch and nothing else: sample i of row b is sample (start_step hop + i) mod (frames hop) of its
 *   utterance, frame j is frame (start_step + j) mod frames.  DISSC_EINVAL with a message naming the row, before any launch: an
 *   utterance outside the corpus, a start_step outside [0, interval_end], B outside its range, a segment that is no positive
 *   multiple of hop below 2^30, another current device.
 * ------------------------------------------------------------------------- */
typedef struct dissc_segment* dissc_segment_t;
int dissc_segment_max_batch(void);
int dissc_segment_create(int U, const long long* frames, int hop, const float* audio, const int32_t* codes, const float* f0,
                         const int32_t* spkr, dissc_segment_t* out);
void dissc_segment_destroy(dissc_segment_t h);
int dissc_segment_interval_end(dissc_segment_t h, int utterance, int segment, long long* out);
int dissc_segment_gather(dissc_segment_t h, const int32_t* table, int B, int segment, float* y, int64_t* code, float* f0,
                         int64_t* spkr, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* DISSC_HIP_H */
