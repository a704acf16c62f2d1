/*
 * tsod.h -- C ABI of libtsod.so: the MI355X (gfx950) two-stage-detector forward path.
 *
 * Drop-in boundary.  The reference (3SAILab/two_stage_object_detection) is pure Python and has
 * no FFI of its own: its hot path bottoms out in torch / torchvision operators.  Each entry
 * point below replaces the operator(s) named in its comment (file:line in the reference), and
 * is what the reference's Python modules bind through ctypes (INTEGRATION.md shows the stub).
 *
 * Conventions (all entry points)
 *   - plain C, no exceptions; return 0 (TSOD_OK) or a negative tsod_status.
 *   - pointers are RAW DEVICE pointers (hipMalloc / torch tensor.data_ptr()), f32 unless said;
 *     activation and weight pointers must be 16-byte aligned.
 *   - asynchronous and stream-ordered on `stream` (a hipStream_t passed as void*; NULL = default).
 *   - stateless, re-entrant, no device allocation, no host synchronisation: the caller owns
 *     every buffer including workspaces (sizes from the *_workspace_bytes helpers), so every
 *     call is legal inside hipStreamBeginCapture / a torch.cuda.graph.
 *   - activations are NHWC ("pixel-major") f32: element (n,h,w,c) of a tensor with channel
 *     pitch P and channel offset O lives at ((n*H + h)*W + w)*P + O + c.  Pitch/offset let a
 *     conv read or write a channel slice of a wider buffer (HarDNet's concat is free).
 *   - boxes are xyxy pixel coordinates, f32.
 *   - the one exchange of the data-parallel job is an all-gather of [B,300,6] detection records per step.  bench.py and
 *     dist.py issue it through torch.distributed (backend "nccl" = RCCL over xGMI), which owns its communicator;
 *     tsod_allgather_f32 below is the same RCCL call for hosts without torch, RCCL bound at run time.
 */
#ifndef TSOD_H
#define TSOD_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define TSOD_VERSION 242 /* 0.2.0: conv descriptor grew (precision, second source), in-launch K-slice combine (zeroed
                            ticket area in the workspace), pitched tsod_detections_f32, new entry points;
                            0.2.1: conv tiles fed by LDS-DMA (bf16x3), balanced K schedule (split_k = -2);
                            0.2.2: tsod_allgather_f32 + communicator helpers (RCCL bound at run time);
                            0.3.0: tsod_bbox2loc_f32; a dual-source conv's c2 must be whole K-steps of the tile;
                            0.4.0: range words (conv descriptor grew: amax_in / amax_in2 / amax_out; tsod_absmax_f32 and the
                            *_amax_f32 entry points): the fp16x2 activation scale follows the tensor per forward */

typedef void *tsod_stream_t; /* hipStream_t */

typedef enum tsod_status {
    TSOD_OK = 0,
    TSOD_ERR_INVALID_ARG = -1, /* NULL pointer, non-positive size, inconsistent geometry */
    TSOD_ERR_UNSUPPORTED = -2, /* valid request this build has no kernel for */
    TSOD_ERR_ALIGNMENT = -3,   /* pointer / pitch / offset not aligned as documented */
    TSOD_ERR_WORKSPACE = -4,   /* workspace NULL or too small */
    TSOD_ERR_LAUNCH = -5       /* hipLaunchKernel reported an error */
} tsod_status;

const char *tsod_status_str(int status);
int tsod_version(void);
/* Number of compute units of the current device (used by the tile heuristics); <0 on error. */
int tsod_device_cu_count(void);

/* ------------------------------------------------------------------------------------------
 * Dense convolution / linear as implicit GEMM on v_mfma_f32_32x32x2_f32 (f32 in, f32 acc).
 * Replaces nn.Conv2d(groups=1) + eval nn.BatchNorm2d + nn.PReLU/ReLU6/ReLU [+ residual add]:
 *   models/resnet.py:62-74 (Bottleneck), :21-31 (BasicBlock), :136-138 (stem), :114-116 (downsample)
 *   models/hardnet.py:38-55 (ConvLayer)
 *   nets/rpn.py:86-88,107,111 (loc / score 1x1 convs)      nets/classify.py:13,15,48,50 (nn.Linear)
 *
 *   out[m, n] = act( (sum_k A[m,k] * Wp[n,k]) * scale[n] + shift[n] + residual[m,n] )
 *   m = (img, oh, ow);  k = (kh, kw, ci) over the input SEGMENTS (see below);  n = output channel.
 * ---------------------------------------------------------------------------------------- */
enum { TSOD_ACT_NONE = 0, TSOD_ACT_PRELU = 1, TSOD_ACT_RELU6 = 2, TSOD_ACT_RELU = 3 };
/* workgroup tile (rows x output channels); _W8 = 8 waves (512 threads) instead of 4; _S1 = single LDS stage
 * (half the LDS per workgroup: more workgroups per CU); _K64 = 64-float K-steps (half the barriers per FLOP);
 * _W1 / _W2 = one / two waves per workgroup, each computing a 64x64 block (no or cheap barriers, half the LDS reads per MFMA) */
enum { TSOD_TILE_AUTO = 0, TSOD_TILE_128x128 = 1, TSOD_TILE_128x64 = 2, TSOD_TILE_64x64 = 3, TSOD_TILE_64x128 = 4,
       TSOD_TILE_128x128_W8 = 5, TSOD_TILE_128x64_W8 = 6, TSOD_TILE_256x128_W8 = 7, TSOD_TILE_64x64_S1 = 8,
       TSOD_TILE_128x64_W8_S1 = 9, TSOD_TILE_64x64_S1_K64 = 10, TSOD_TILE_128x64_W8_S1_K64 = 11,
       TSOD_TILE_64x64_W1_S1 = 12, TSOD_TILE_128x64_W2_S1 = 13, TSOD_TILE_128x64_S1 = 14, TSOD_TILE_64x128_S1 = 15,
       TSOD_TILE_128x128_S1 = 16,
       /* fed by LDS-DMA (conv_dma_kernel; BF16X3 / FP16X2, see below): one channel segment, Cin (and a second source's c2) a
        * multiple of the K stage (16 / 32 / 64 floats), KH * KW <= 31 and K / stage + 8 <= 640 (one table entry per K-step of a
        * workgroup's K range) - or, FP16X2 only, a 1x1 stride-1 unpadded filter over several channel segments with K <= 2048;
        * anything else is TSOD_ERR_UNSUPPORTED for these tiles (TSOD_TILE_AUTO then resolves to another tile).  Filters with
        * more than one tap run their K-steps in (32-channel block, tap) order: another f32 summation order than the other
        * tiles, same weights */
       TSOD_TILE_D128x128 = 17, TSOD_TILE_D64x128 = 18, TSOD_TILE_D256x128 = 19,
       TSOD_TILE_D64x128_S2 = 20 /* two ring stages: two workgroups per CU */,
       TSOD_TILE_D128x256 = 21 /* two columns of waves share the activation stage */,
       TSOD_TILE_D128x128_K32 = 22 /* 8 waves (4 along M x 2 along K), 32-float stages, 3-stage ring: two waves per SIMD at one
                                      workgroup per CU - the small-M (batch-1) tile */,
       TSOD_TILE_D192x128 = 23 /* FP16X2 only: 6 waves along M, 16-float stages, 4-stage ring, one workgroup per CU.  A row-tile size
                                  of its own against tile-count cliffs: M = 4200 rows x 1024 channels (layer3's 1x1 expand conv at
                                  batch 1) is 264 tiles of 128 x 128 - one more chip-wave for 8 tiles - and 176 of these */,
       TSOD_TILE_D64x128_K64 = 24 /* FP16X2 only: 8 waves (2 along M x 4 along K), 64-float stages, 3-stage ring, one workgroup per CU:
                                     half the row granularity of D128x128_K32 at the same MFMAs per wave and phase - small-M layers
                                     fill the chip with whole tiles (four K quarters meet in LDS) instead of K-slices that meet in memory */,
       TSOD_TILE_COUNT = 25 };
/* arithmetic of the contraction.  F32: v_mfma_f32_32x32x2_f32 (a k-ordered f32 fma chain).  BF16X3: every f32 operand cut
 * exactly into three bf16 pieces (hi + mid + lo == x), six piece products per k accumulated in f32 on
 * v_mfma_f32_32x32x16_bf16: f32-level accuracy (error ~1.3e-7 of sum|a*b|) at 0.375x the matrix-pipe time; storage,
 * accumulation and epilogue are f32 either way.
 * Tiles built in each arithmetic (a named tile outside its arithmetic's list is TSOD_ERR_UNSUPPORTED):
 *   F32:    128x128 .. 128x128_S1 (1..16), none of the TSOD_TILE_D* tiles;
 *   BF16X3: 64x64, 64x64_S1, 128x64_W8_S1, 64x64_S1_K64, 128x64_S1, 64x128_S1, 128x128_S1,
 *           D128x128, D64x128, D256x128, D64x128_S2, D128x256, D128x128_K32;
 *   FP16X2: 64x64, 64x64_S1, 128x64_W8_S1, 64x64_S1_K64, 128x64_S1, 64x128_S1, 128x128_S1,
 *           D128x128, D256x128, D128x256, D128x128_K32, D192x128, D64x128_K64. */
enum { TSOD_PREC_F32 = 0, TSOD_PREC_BF16X3 = 1, TSOD_PREC_FP16X2 = 2 };
/* FP16X2: every f32 operand as TWO fp16 pieces of s * x
 * (hi = rne(s x), lo = rne(s x - hi), s a power of two per tensor), THREE piece products per f32 product on
 * v_mfma_f32_32x32x16_f16, f32 accumulation: the f32 kernel's accuracy with half the MFMAs of BF16X3 - while |s x| stays
 * below fp16's 65504 (the CALLER picks desc.a_scale_exp for its activations' range; beyond it the piece products are inf /
 * NaN, reported through desc.range_flag).
 * `w_packed` is then the image made by tsod_pack_conv_weight_fp16x2 with desc.w_scale_exp: [Cout][ceil(K/8)][hi | lo][8]
 * fp16 of 2^w_scale_exp * w, 32 bytes per 8 k.  The accumulators are scaled back by 2^-(a_scale_exp + w_scale_exp) before
 * the epilogue (exact), so scale / shift / residual / activation mean what they mean for the other arithmetics. */
/* With TSOD_PREC_BF16X3 the `w_packed` argument of tsod_conv2d_f32 is the PRE-SPLIT weight image made once by
 * tsod_pack_conv_weight_bf16x3 from the f32 packed weights [Cout][K]: [Cout][ceil(K/8)][hi | mid | lo][8] bf16, 48 bytes per
 * 8 k (tsod_conv_weight_bf16x3_bytes), every weight cut exactly (hi + mid + lo == w).  Activations are split on the fly. */
#define TSOD_MAX_SEGMENTS 16

typedef struct tsod_conv2d_desc {
    int32_t N, H, W;       /* input images, height, width */
    int32_t in_pitch;      /* floats between consecutive input pixels; multiple of 4 */
    int32_t n_seg;         /* 1..TSOD_MAX_SEGMENTS channel segments gathered from each input pixel */
    int32_t seg_off[TSOD_MAX_SEGMENTS]; /* first channel of segment s inside the pixel; multiple of 4 */
    int32_t seg_len[TSOD_MAX_SEGMENTS]; /* channels in segment s; multiple of 4.  Cin = sum(seg_len) */
    int32_t Cout;          /* output channels (any positive value) */
    int32_t out_pitch;     /* floats between consecutive output pixels (>= out_off + Cout) */
    int32_t out_off;       /* first output channel inside the output pixel */
    int32_t KH, KW;        /* filter size */
    int32_t stride;        /* same in h and w */
    int32_t pad_h, pad_w;  /* zero padding (top/left; bottom/right implied by OH/OW) */
    int32_t OH, OW;        /* output height / width */
    int32_t act;           /* TSOD_ACT_* */
    float slope;           /* PReLU negative slope (single-parameter nn.PReLU) */
    int32_t res_pitch;     /* residual pixel pitch (ignored when residual == NULL) */
    int32_t res_off;       /* residual channel offset */
    int32_t tile;          /* TSOD_TILE_*; AUTO = built-in heuristic */
    int32_t split_k;       /* 1 = whole tiles only; S > 1 = every tile cut into S K-slices; -1 = hybrid (full
                              chip-waves of whole tiles, left-over tiles K-sliced to fill the last wave);
                              -2 = balanced (TSOD_TILE_D* only): one workgroup per CU slot, each the same number of
                              K-steps of the tile-major K-step sequence; 0 = built-in cost model chooses */
    int32_t precision;     /* TSOD_PREC_* (0 = F32) */
    /* optional SECOND source (tsod_conv2d_dual_f32; c2 = 0: none).  k in [KH*KW*Cin, KH*KW*Cin + c2) contracts channel
     * in2_off + (k - KH*KW*Cin) of pixel (oh*stride2, ow*stride2) of in2 [N][H2][W2][in2_pitch]: a strided 1x1 tap, i.e. a
     * bottleneck's last 1x1 conv and its projection shortcut (models/resnet.py:70-74 with :114-116) as ONE GEMM
     *   out = act( [y | x_strided] . [W3*s3 | Wd*sd]^T + (b3 + bd) )
     * (the caller folds both BN scales into the stacked weights [Cout][KH*KW*Cin + c2] and adds the shifts).
     * Requires one channel segment and Cin, KH*KW*Cin AND c2 multiples of the tile's K-step (32; 64 for the _K64 tiles; the
     * stage of the TSOD_TILE_D* tiles): K-steps never straddle the sources nor run past c2.  A named tile that does not
     * divide them returns TSOD_ERR_UNSUPPORTED; TSOD_TILE_AUTO only considers tiles that do. */
    int32_t c2, in2_pitch, in2_off, stride2, H2, W2;
    /* TSOD_PREC_FP16X2 only (ignored otherwise): the activations are split as 2^a_scale_exp * x, the weight image holds
     * 2^w_scale_exp * w (the exponent it was packed with) */
    int32_t a_scale_exp, w_scale_exp;
    /* TSOD_PREC_FP16X2 only, optional (NULL: no report): a device int32 that the launch ORs 1 into when a workgroup ends its K
     * loop with a non-finite accumulator - which is what an activation outside the range produces in every output it feeds
     * (and what genuinely non-finite input produces).  The outputs of such a launch are not to be used; clear the word and
     * run the layer with TSOD_PREC_BF16X3 or a smaller a_scale_exp. */
    int32_t *range_flag;
    /* Range words (optional, NULL = off; see "Range words" below).  amax_out: this launch adds the abs-max of the values it
     * stores to the words.  amax_in (and amax_in2 for the second source): TSOD_PREC_FP16X2 only - the launch takes its
     * activation exponent from the words (2^e * absmax < 2^15) instead of a_scale_exp: the scale follows the tensor per forward,
     * so no input range can leave the arithmetic (range_flag then only reports non-finite input). */
    const uint32_t *amax_in, *amax_in2;
    uint32_t *amax_out;
} tsod_conv2d_desc;

/* Range words: the abs-max of an activation tensor, kept by its PRODUCERS for its consumers.  One tensor = TSOD_AMAX_WORDS
 * uint32 words TSOD_AMAX_STRIDE bytes apart (TSOD_AMAX_BYTES in all, 64-byte aligned), each the bit pattern of a non-negative
 * f32; the abs-max is the largest word.  The caller zero-fills the words once per forward (stream-ordered, e.g.
 * hipMemsetAsync) before the first producer runs; every producing launch adds one atomic max per workgroup (spread over the
 * words: a single word would serialise ~11.5 ns per workgroup); several producers may share the words of one buffer (HarDNet's
 * block buffers), a tensor that is a max-pool or RoI-pool of another may share its producer's.  Everything is stream-ordered and
 * capturable; nothing is read by the host. */
#define TSOD_AMAX_WORDS 64
#define TSOD_AMAX_STRIDE 64
#define TSOD_AMAX_BYTES (TSOD_AMAX_WORDS * TSOD_AMAX_STRIDE)
/* zero the words of `n_tensors` consecutive tensors (a memset node under stream capture): once per forward */
int tsod_amax_reset(uint32_t *words, int32_t n_tensors, tsod_stream_t stream);
/* abs-max of n floats into the words (for tensors no libtsod kernel produced: an image handed over in NHWC(4) layout) */
int tsod_absmax_f32(const float *x, int64_t n, uint32_t *amax_out, tsod_stream_t stream);

/* A device word the HOST can read without a device call (serving: one range-flag read per request, nets/.. serving.py).
 * tsod_host_mapped_pointer: the device-side address of page-locked, mapped host memory (hipHostMalloc, torch's pin_memory()) -
 * a query, made once; TSOD_ERR_UNSUPPORTED when the memory is not mapped into the current device.  tsod_word_publish_i32: one
 * thread stores *src_device to that address, stream-ordered and capturable (a kernel node, no blit); the host reads its own
 * memory once the forward's event has completed. */
int tsod_host_mapped_pointer(void *host, void **device);
int tsod_word_publish_i32(const int32_t *src_device, int32_t *dst_mapped, tsod_stream_t stream);

/* Packed weight layout Wp: [Cout][KH][KW][Cin] f32 (k = (kh*KW + kw)*Cin + ci, ci running over
 * the concatenated segments).  tsod_pack_conv_weight_f32 converts torch's [Cout][Cin_src][KH][KW]:
 * Cin >= Cin_src, extra input channels get zero weights (used to pad 3 -> 4 channels in the
 * stems); KW >= KW_src, extra taps on the right get zero weights (the 7x7 stem runs as 7x8). */
int tsod_pack_conv_weight_f32(const float *w_oihw, int32_t Cout, int32_t Cin_src, int32_t KH, int32_t KW_src,
                              int32_t Cin, int32_t KW, float *w_packed, tsod_stream_t stream);

size_t tsod_conv_weight_bf16x3_bytes(int32_t Cout, int32_t K);
int tsod_pack_conv_weight_bf16x3(const float *w_packed /* [Cout][K] f32 */, int32_t Cout, int32_t K, void *w_bf16x3,
                                 tsod_stream_t stream);
size_t tsod_conv_weight_fp16x2_bytes(int32_t Cout, int32_t K);
int tsod_pack_conv_weight_fp16x2(const float *w_packed /* [Cout][K] f32 */, int32_t Cout, int32_t K, int32_t w_scale_exp,
                                 void *w_fp16x2, tsod_stream_t stream);

/* Bytes of workspace tsod_conv2d_f32 needs for this descriptor (0 unless some tile is K-sliced).
 * Workspace contract: 16-byte aligned, private to one stream at a time, layout [one int32 arrival ticket per K-sliced
 * tile, padded to 256 bytes | partial-sum slabs].  K-slices are combined INSIDE the launch: every slice stores its slab
 * write-through, the slice that arrives last at the tile's ticket sums the slabs in slice order (bit-reproducible) and
 * applies the epilogue.  The tickets must be ZERO when a launch starts; every launch leaves them zero, so zero-fill the
 * buffer once when it is allocated and never lend it to another kernel in between. */
size_t tsod_conv2d_workspace_bytes(const tsod_conv2d_desc *d);
/* Resolve TSOD_TILE_AUTO / split_k == 0 to the concrete choice the heuristic makes. */
int tsod_conv2d_resolve(const tsod_conv2d_desc *d, int32_t *tile, int32_t *split_k);

int tsod_conv2d_f32(const tsod_conv2d_desc *d, const float *in, const float *w_packed,
                    const float *scale /* [Cout] or NULL (=1) */, const float *shift /* [Cout] or NULL (=0) */,
                    const float *residual /* or NULL */, float *out,
                    void *workspace, size_t workspace_bytes, tsod_stream_t stream);

/* The same with a second source tensor (desc.c2 > 0, see tsod_conv2d_desc); in2 == NULL iff desc.c2 == 0. */
int tsod_conv2d_dual_f32(const tsod_conv2d_desc *d, const float *in, const float *in2, const float *w_packed,
                         const float *scale, const float *shift, const float *residual, float *out,
                         void *workspace, size_t workspace_bytes, tsod_stream_t stream);

/* ------------------------------------------------------------------------------------------
 * A whole identity-shortcut ResNet bottleneck in ONE launch (models/resnet.py:57-76 with stride 1 and downsample None: the
 * blocks 1.. of `layer1 = _make_layer(64, 3)`, :99):
 *     out = PReLU(BN3(conv1x1(PReLU(BN2(conv3x3(PReLU(BN1(conv1x1(x)))))))) + x)        Cin -> 64 -> 64 -> Cout, Cout == Cin
 * The two 64-channel intermediates never leave the CU (LDS), so the block moves x (+ a one-pixel halo), x again for the
 * residual (an L2 / Infinity-Cache hit) and out, instead of 273 MB per image at 3x800x1333 in three launches.  FP16X2
 * arithmetic (see TSOD_PREC_FP16X2): x is split with the scale of amax_in (or the static a_scale_exp), the intermediates with
 * the scale of each tile's own abs-max.  This build: Cmid == 64, Cin == Cout, both multiples of 64.
 *
 * `wstream`: the three convs' weights as ONE stream of 8 KB steps in consumption order - Cin/32 steps of conv1 (k = 32 s ..),
 * 18 of conv2 (step = (tap kh*3+kw, channel half)), 2 per 64 output channels of conv3 - each step 64 output channels x 32 k of
 * fp16 pieces of 2^w_exp[i] * w (hi = rne(.), lo = rne(2^e w - hi)), stored as the MFMA fragments the kernel's lanes load
 * straight from L2 into registers: [channel block cb (2)][lane (64) = 32 hh + j][chunk c (2)][hi | lo][8 k], where lane (j, hh) of
 * block cb holds output channel base + 32 cb + pi(j), pi(j) = 16 ((j >> 2) & 1) + 4 (j >> 3) + (j & 3) (so that an accumulator
 * lane owns 16 consecutive channels), and k = 16 c + 8 hh ...  `bn`: f32 [s1(64) | b1(64) | s2(64) | b2(64) | s3(Cout) | b3(Cout)],
 * the folded BatchNorm scale / shift of the three convs.  No workspace. */
typedef struct tsod_bottleneck_desc {
    int32_t N, H, W;              /* images, height, width (input and output) */
    int32_t Cin, in_pitch;        /* x: [N][H][W][in_pitch], channels [0, Cin) */
    int32_t Cmid;                 /* 64 */
    int32_t Cout, out_pitch;      /* out: [N][H][W][out_pitch] */
    float slope;                  /* the block's one PReLU slope */
    int32_t w_exp[3];             /* exponents the three convs' weights were scaled with in wstream */
    int32_t a_scale_exp;          /* static exponent for x when amax_in == NULL */
    int32_t projection;           /* 0: identity shortcut (Cout == Cin).  1 (version 242): the block's 1x1 projection shortcut at stride 1
                                   * (models/resnet.py:114-116, layer1's first block) as part of ONE stacked-K GEMM:
                                   *   out = PReLU([y2 | x] . [W3 s3 | Wd sd]^T + (b3 + bd)),   Cin -> 64 -> 64 -> Cout, Cin % 64 == 0
                                   * wstream then carries 2 + Cin / 32 steps per 64 output channels of "conv3" (k = the 64 channels of
                                   * y2, then the Cin channels of x; both BatchNorm scales folded into the weights, ONE exponent
                                   * w_exp[2] for the stacked matrix: tsod_bottleneck_proj_wstream_bytes), bn's s3 is all ones and its
                                   * b3 the two shifts added up; the x chunks of a tile's own pixels are read a second time from L2
                                   * straight into MFMA fragments, there is no residual pass.  (The field sits in what was padding.) */
    int32_t *range_flag;          /* optional, as in tsod_conv2d_desc */
    const uint32_t *amax_in;      /* optional range words of x */
    uint32_t *amax_out;           /* optional range words of out */
} tsod_bottleneck_desc;
size_t tsod_bottleneck_wstream_bytes(int32_t Cin, int32_t Cout);
size_t tsod_bottleneck_proj_wstream_bytes(int32_t Cin, int32_t Cout);    /* desc.projection == 1 */
int tsod_bottleneck_fp16x2(const tsod_bottleneck_desc *d, const float *x, const void *wstream, const float *bn, float *out,
                           tsod_stream_t stream);

/* The ResNet stem in one launch (models/resnet.py:136-139: conv1 7x7 / 2 pad 3, 3 -> 64, no bias; bn1; relu = nn.PReLU (one
 * slope); maxpool 3x3 / 2 pad 1):  out[N][PH][PW][out_pitch] (channels [0, 64)) from the images x, which are either the reference's
 * NCHW [N][3][H][W] or the input step's NHWC with 4 floats per pixel (channel 3 is ignored).  OH = (H - 1) / 2 + 1, PH = (OH - 1) / 2 + 1
 * (same for W).  fp16x2 arithmetic (see TSOD_PREC_FP16X2) with the pixel scale taken per tile from the tile's own input patch: no
 * range words and no pass over the image are needed.  `wfrag` = tsod_stem_wfrag_bytes() bytes: the weights times 2^w_exp as two
 * fp16 pieces in the MFMA fragments the lanes load, [channel block cb (2)][chunk c (14)][hi | lo][lane (64) = 32 hh + j][8 k], where
 * lane (j, hh) holds output channel 32 cb + pi(j) (pi as in tsod_bottleneck_fp16x2) and k = 16 c + 8 hh .. + 7 with
 * k = 32 kh + 4 kw + ci (kw = 7 and ci = 3: zeros).  `bn`: f32 [scale(64) | shift(64)].  amax_out: the pooled map's range words. */
#define TSOD_STEM_NCHW 0
#define TSOD_STEM_NHWC4 1
typedef struct tsod_stem_desc {
    int32_t N, H, W;              /* images, input height, width */
    int32_t in_layout;            /* TSOD_STEM_NCHW / TSOD_STEM_NHWC4 */
    int32_t out_pitch;            /* floats per pooled pixel (>= 64, multiple of 4) */
    float slope;                  /* PReLU slope */
    int32_t w_exp;                /* the weights in wfrag are scaled by 2^w_exp */
    int32_t *range_flag;          /* optional, as in tsod_conv2d_desc (raised by non-finite input) */
    uint32_t *amax_out;           /* optional range words of out */
} tsod_stem_desc;
size_t tsod_stem_wfrag_bytes(void);
int tsod_stem_fp16x2(const tsod_stem_desc *d, const float *x, const void *wfrag, const float *bn, float *out, tsod_stream_t stream);

/* nn.Linear (nets/classify.py:13,15): out[M,N] = in[M,K] @ w[N,K]^T + bias.  K % 4 == 0. */
int tsod_linear_f32(const float *in, int32_t M, int32_t K, int32_t in_pitch, const float *w /* [N][K] */,
                    const float *bias /* [N] or NULL */, int32_t N, float *out, int32_t out_pitch,
                    void *workspace, size_t workspace_bytes, tsod_stream_t stream);
size_t tsod_linear_workspace_bytes(int32_t M, int32_t K, int32_t N);

/* ------------------------------------------------------------------------------------------
 * HBM-bound layer kernels (NHWC).
 * ---------------------------------------------------------------------------------------- */
/* nn.MaxPool2d(3, 2, 1): models/resnet.py:98,139.  C % 4 == 0; OH = (H-1)/2+1, OW = (W-1)/2+1. */
int tsod_maxpool3x3s2_f32(const float *in, int32_t N, int32_t H, int32_t W, int32_t C, int32_t in_pitch,
                          float *out, int32_t out_pitch, tsod_stream_t stream);

/* Depthwise 3x3, pad 1, stride 1|2, + per-channel scale/shift (folded BN or bias) + optional ReLU:
 * models/hardnet.py:21-36 (DWConvLayer) and :193-195 (tail).  w is [3][3][C]; C % 4 == 0. */
int tsod_dwconv3x3_f32(const float *in, int32_t N, int32_t H, int32_t W, int32_t C, int32_t in_pitch, int32_t in_off,
                       const float *w, const float *scale, const float *shift, int32_t stride, int32_t relu,
                       float *out, int32_t out_pitch, int32_t out_off, tsod_stream_t stream);

/* ... the same, adding the abs-max of what it stores to the range words `amax_out` (NULL: exactly tsod_dwconv3x3_f32) */
int tsod_dwconv3x3_amax_f32(const float *in, int32_t N, int32_t H, int32_t W, int32_t C, int32_t in_pitch, int32_t in_off,
                            const float *w, const float *scale, const float *shift, int32_t stride, int32_t relu,
                            float *out, int32_t out_pitch, int32_t out_off, uint32_t *amax_out, tsod_stream_t stream);

/* Grouped 3x3 conv, pad 1, stride 1|2, C -> C channels in `groups` groups + per-channel scale/shift (folded BN) + activation:
 * the conv2 of the ResNeXt bottleneck (models/resnet.py:46-47 with groups = 32, width_per_group = 4; factory :167-172).
 * w is [C][3][3][C/groups]; C/groups must be a multiple of 4.  act / slope as in tsod_conv2d_desc. */
int tsod_gconv3x3_f32(const float *in, int32_t N, int32_t H, int32_t W, int32_t C, int32_t in_pitch, int32_t groups,
                      const float *w, const float *scale, const float *shift, int32_t stride, int32_t act, float slope,
                      float *out, int32_t out_pitch, tsod_stream_t stream);

int tsod_gconv3x3_amax_f32(const float *in, int32_t N, int32_t H, int32_t W, int32_t C, int32_t in_pitch, int32_t groups,
                           const float *w, const float *scale, const float *shift, int32_t stride, int32_t act, float slope,
                           float *out, int32_t out_pitch, uint32_t *amax_out, tsod_stream_t stream);

/* nn.Conv2d(2G, G, 1, groups=G) + bias: models/hardnet.py:196.
 * out[.., g] = w[g][0]*in[.., 2g] + w[g][1]*in[.., 2g+1] + bias[g].  w is [G][2]. */
int tsod_gconv1x1_pair_f32(const float *in, int64_t pixels, int32_t G, int32_t in_pitch, const float *w,
                           const float *bias, float *out, int32_t out_pitch, tsod_stream_t stream);

int tsod_gconv1x1_pair_amax_f32(const float *in, int64_t pixels, int32_t G, int32_t in_pitch, const float *w,
                                const float *bias, float *out, int32_t out_pitch, uint32_t *amax_out, tsod_stream_t stream);

/* Layout changes at the module boundary (the reference's tensors are NCHW).
 * nchw_to_nhwc writes channels [0,C) of each pixel and zero-fills [C, C_pad) (C_pad <= out_pitch). */
int tsod_nchw_to_nhwc_f32(const float *in, int32_t N, int32_t C, int32_t H, int32_t W,
                          float *out, int32_t out_pitch, int32_t C_pad, tsod_stream_t stream);
/* ... adding the image batch's abs-max to the range words `amax_out` (NULL: exactly tsod_nchw_to_nhwc_f32) */
int tsod_nchw_to_nhwc_amax_f32(const float *in, int32_t N, int32_t C, int32_t H, int32_t W,
                               float *out, int32_t out_pitch, int32_t C_pad, uint32_t *amax_out, tsod_stream_t stream);
int tsod_nhwc_to_nchw_f32(const float *in, int32_t N, int32_t C, int32_t H, int32_t W, int32_t in_pitch,
                          int32_t in_off, float *out, tsod_stream_t stream);

/* ------------------------------------------------------------------------------------------
 * RPN proposal path.
 * ---------------------------------------------------------------------------------------- */
/* Fused anchor shift + fg softmax + box decode + clamp + min-size test.  Replaces
 *   utils/basic_anchors.py:27-57 (enumerate_shifted_anchor), nets/rpn.py:115-118 (softmax, fg),
 *   utils/loc_bbox_iou.py:29-61 (loc2bbox), nets/rpn.py:45-54 (clamp, min-size keep).
 * Anchor index a' = (y*Wf + x)*A + a.  locs holds 4 floats per anchor at
 * locs[(img*Hf*Wf + y*Wf + x)*loc_pitch + 4a ..], scores 2 logits (bg, fg) at
 * scores[(...)*score_pitch + 2a ..].  x is clamped to [0, clamp_x], y to [0, clamp_y]
 * (the caller passes img_size[1], img_size[2]: reference quirk Q1 lives in the caller).
 * Outputs: boxes [B][Hf*Wf*A][4]; fg [B][Hf*Wf*A] (softmax probability);
 *          keys [B][Hf*Wf*A] = fg where both sides >= min_size, else -inf;
 *          anchors_out (optional, may be NULL) [Hf*Wf*A][4] the shifted anchors. */
int tsod_rpn_decode_f32(const float *locs, int32_t loc_pitch, const float *scores, int32_t score_pitch,
                        const float *anchor_base /* [A][4] */, int32_t A, int32_t B, int32_t Hf, int32_t Wf,
                        int32_t feat_stride, float clamp_x, float clamp_y, float min_size,
                        float *boxes, float *fg, float *keys, float *anchors_out, tsod_stream_t stream);

/* The same decode for an explicit anchor tensor and ready-made fg scores: the head of
 * ProposalCreator.__call__ (nets/rpn.py:44-54) for one image.  anchor [n][4], loc [n][4], score [n] ->
 * boxes [n][4] (decoded, clamped), keys [n] = score where both sides >= min_size else -inf. */
int tsod_proposal_decode_f32(const float *anchor, const float *loc, const float *score, int64_t n, float clamp_x,
                             float clamp_y, float min_size, float *boxes, float *keys, tsod_stream_t stream);

/* utils/basic_anchors.py:27-57 as a stand-alone op: out [Hf*Wf*A][4] = base[a] + (x*s, y*s, x*s, y*s). */
int tsod_enumerate_anchors_f32(const float *anchor_base, int32_t A, int32_t Hf, int32_t Wf, int32_t feat_stride,
                               float *out, tsod_stream_t stream);

/* utils/loc_bbox_iou.py:29-61 as a stand-alone op: src [n][4] xyxy, loc [n][4] (dx,dy,dw,dh) -> out [n][4]. */
int tsod_loc2bbox_f32(const float *src, const float *loc, int64_t n, float *out, tsod_stream_t stream);

/* utils/loc_bbox_iou.py:63-88 (bbox2loc) as a stand-alone op, the inverse of loc2bbox: src [n][4], dst [n][4] xyxy ->
 * out [n][4] = ((cx_d - cx_s) / w_s, (cy_d - cy_s) / h_s, log(w_d / w_s), log(h_d / h_s)), w_s / h_s floored at f32 eps.
 * The same device function the two target creators below call. */
int tsod_bbox2loc_f32(const float *src, const float *dst, int64_t n, float *out, tsod_stream_t stream);

/* Per-image stable descending top-k.  Replaces torch.argsort(score, descending=True)[:n_pre] and
 * the gathers at nets/rpn.py:56-61.  keys [B][n]; entries equal to -inf are "filtered out" and
 * never selected; ties keep lower index first.  Outputs, per image b:
 *   counts[b]      = n_sel = min(n_pre, #keys > -inf)                       (int32)
 *   idx[b][k]      = source index of the k-th best, k < n_sel; -1 beyond    (int32, [B][n_pre])
 *   boxes_out[b][k]= boxes[b][idx] (zeros beyond n_sel)                     ([B][n_pre][4]) (may be NULL)
 *   keys_out[b][k] = keys[b][idx]  (-inf beyond n_sel)                      ([B][n_pre])    (may be NULL)
 * n_pre <= 16384.  Small problems (B * n^2 <= 3e8): one launch that ranks every key against every key of its image on the
 * whole chip.  Larger: one workgroup per image, LDS radix-select (rows of up to 81920 keys are held in registers after one
 * pass over memory, longer rows are re-read per pass), then a bitonic sort there - or, with scratch (the _ws_ form below),
 * the rank kernel over the selection. */
int tsod_sort_topk_desc_f32(const float *keys, const float *boxes, int32_t B, int32_t n, int32_t n_pre,
                            int32_t *counts, int32_t *idx, float *boxes_out, float *keys_out,
                            tsod_stream_t stream);
/* The same with caller-owned scratch (tsod_sort_topk_workspace_bytes; may be 0): the order of the selection is then
 * computed by RANK on the whole chip (every key counts the keys before it: the composite keys (score, index) are
 * distinct) instead of by a sorting network inside one workgroup per image.  Results are identical. */
size_t tsod_sort_topk_workspace_bytes(int32_t B, int32_t n, int32_t n_pre);
int tsod_sort_topk_desc_ws_f32(const float *keys, const float *boxes, int32_t B, int32_t n, int32_t n_pre,
                               int32_t *counts, int32_t *idx, float *boxes_out, float *keys_out, void *workspace,
                               size_t workspace_bytes, tsod_stream_t stream);

/* Batched greedy NMS on boxes already sorted by descending score + the pad/truncate tail.
 * Replaces torchvision.ops.nms (nets/rpn.py:63) and nets/rpn.py:65-69.
 *   boxes [B][n_max][4], counts[b] <= n_max valid rows per image.
 *   suppress j when IoU(i,j) > thr (strict), IoU = inter / (area_i + area_j - inter).
 *   keep_idx [B][n_post] int32: kept indices in order, then 0,1,2,... padding (quirk Q4).
 *   rois     [B][n_post][4]   : boxes[b][keep_idx]
 *   n_kept   [B] int32        : min(number surviving NMS, n_post) before padding
 *   status   [1] int32 (zeroed by the caller): bit 0 set when the pad ran past counts[b]
 *            (the reference raises IndexError there); the offending rows are zero-filled.
 * workspace: tsod_nms_workspace_bytes(B, n_max). */
size_t tsod_nms_workspace_bytes(int32_t B, int32_t n_max);
int tsod_nms_f32(const float *boxes, const int32_t *counts, int32_t B, int32_t n_max, float iou_thr,
                 int32_t n_post, int32_t *keep_idx, float *rois, int32_t *n_kept, int32_t *status,
                 void *workspace, size_t workspace_bytes, tsod_stream_t stream);

/* Dense pairwise IoU with eps in the denominator: utils/loc_bbox_iou.py:4-27.  out [Na][Nb]. */
int tsod_bbox_iou_f32(const float *a, int32_t Na, const float *b, int32_t Nb, float eps, float *out,
                      tsod_stream_t stream);

/* ------------------------------------------------------------------------------------------
 * RoI head.
 * ---------------------------------------------------------------------------------------- */
/* torchvision.ops.RoIPool((PH,PW), spatial_scale) (nets/classify.py:17,43) on an NHWC feature map.
 *   feat [B][Hf][Wf] pixels with pitch feat_pitch, C channels (C % 4 == 0);
 *   rois5 [K][5] = (batch_index, x1, y1, x2, y2) in feature coordinates before spatial_scale.
 *   out  [K][C][PH][PW]  (torchvision's layout). */
int tsod_roi_pool_f32(const float *feat, int32_t B, int32_t Hf, int32_t Wf, int32_t C, int32_t feat_pitch,
                      const float *rois5, int32_t K, float spatial_scale, int32_t PH, int32_t PW,
                      float *out, tsod_stream_t stream);

/* Fused RoI rescale + index + RoIPool + mean over the PHxPW bins.  Replaces
 *   nets/classify.py:29-38 (rescale: x / img_w * Wf, y / img_h * Hf; row index = roi_indices[b]),
 *   nets/classify.py:43 (RoIPool), models/hardnet.py:203-212 (AdaptiveAvgPool2d(1) + Flatten).
 *   rois [B][R][4] image coordinates; roi_indices [B] int32; out [B*R][C] (pitch out_pitch). */
int tsod_roi_pool_avg_f32(const float *feat, int32_t B, int32_t Hf, int32_t Wf, int32_t C, int32_t feat_pitch,
                          const float *rois, const int32_t *roi_indices, int32_t R, float img_h, float img_w,
                          float spatial_scale, int32_t PH, int32_t PW, float *out, int32_t out_pitch,
                          tsod_stream_t stream);

/* RoIAlign: the added `roi_op="align"` option of the head (the reference builds RoIPool).  Semantics of
 * torchvision.ops.roi_align(input, rois5, (PH,PW), spatial_scale, sampling_ratio, aligned): bilinear samples on a
 * sampling_ratio x sampling_ratio grid per bin (0 = adaptive: ceil(roi extent / P)), averaged; layouts as tsod_roi_pool_f32.
 * tsod_roi_align_avg_f32 is the fused form of tsod_roi_pool_avg_f32 (RoI rescale + index + align + mean over the bins). */
int tsod_roi_align_f32(const float *feat, int32_t B, int32_t Hf, int32_t Wf, int32_t C, int32_t feat_pitch,
                       const float *rois5, int32_t K, float spatial_scale, int32_t PH, int32_t PW, int32_t sampling_ratio,
                       int32_t aligned, float *out, tsod_stream_t stream);
int tsod_roi_align_avg_f32(const float *feat, int32_t B, int32_t Hf, int32_t Wf, int32_t C, int32_t feat_pitch,
                           const float *rois, const int32_t *roi_indices, int32_t R, float img_h, float img_w,
                           float spatial_scale, int32_t PH, int32_t PW, int32_t sampling_ratio, int32_t aligned,
                           float *out, int32_t out_pitch, tsod_stream_t stream);

/* Final detection records (nets/frcnn_training.py:311-319): per RoI the arg-max class
 * over all n_class logits (first max wins; a NaN logit counts as the largest, as in torch.max / torch.argmax: the record's
 * score is NaN and its class the first NaN's column), its raw logit, and loc2bbox(roi, loc of that class).
 *   cls_locs [K] rows of 4*n_class floats (row pitch loc_pitch), scores [K] rows of n_class (pitch score_pitch) - both may
 *   be column slices of one wider matrix, as the fused head GEMM writes them - rois [K][4]
 *   -> det [K][6] = (x1,y1,x2,y2,score,class). */
int tsod_detections_f32(const float *cls_locs, int32_t loc_pitch, const float *scores, int32_t score_pitch,
                        const float *rois, int32_t K, int32_t n_class, float *det, tsod_stream_t stream);

/* ---- inference-time filtering of the records (the step after the path) ------------------
 * The reference's demo keeps `nms(boxes_pred, labels_score_pred, iou_threshold=0.1)` over the records of an
 * image, class-agnostic, no score threshold (multi_inference.py:84).  These three calls are that step with the
 * two switches a deployment adds (score threshold / background class, per-class suppression):
 *   1. tsod_detection_keys_f32   keys[t] = score if (score >= score_thresh and class != background_class) else -inf
 *                                (background_class < 0: no class is dropped; NaN scores are dropped)
 *   2. tsod_sort_topk_desc_f32(keys, NULL, B, R, R, counts, idx, NULL, NULL)   stable descending order, -inf rows dropped
 *      tsod_gather_rows_f32      det_sorted[b][r][:] = det[b][idx[b][r]][:]  (zero rows where idx < 0)
 *   3. tsod_detection_nms_f32    greedy NMS over det_sorted [B][R][6] (columns 0-3 box, 5 class), suppress j when
 *                                IoU(i,j) > thr (strict) and - with per_class != 0 - class_i == class_j.
 *                                keep_idx [B][R] int32: surviving rows of det_sorted in score order, -1 after n_kept[b].
 *                                workspace: tsod_nms_workspace_bytes(B, R).  R <= 8192. */
int tsod_detection_keys_f32(const float *det, int64_t n, float score_thresh, int32_t background_class, float *keys,
                            tsod_stream_t stream);
int tsod_gather_rows_f32(const float *src, const int32_t *idx, int32_t B, int32_t n, int32_t m, int32_t C, float *out,
                         tsod_stream_t stream);
int tsod_detection_nms_f32(const float *det_sorted, const int32_t *counts, int32_t B, int32_t R, float iou_thr,
                           int32_t per_class, int32_t *keep_idx, int32_t *n_kept, void *workspace,
                           size_t workspace_bytes, tsod_stream_t stream);

/* ---- training-side box ops ---------------------------------------------------------------
 * The reference's two target creators are deterministic IoU arg-max assignments ("first n by index" sampling); both are
 * restated with their indexing quirks (oracle/targets.py T1-T4).  IoU is utils/loc_bbox_iou.py:4-27 (eps 1e-8), offsets
 * are bbox2loc (utils/loc_bbox_iou.py:63-88).
 *
 * tsod_anchor_targets_f32 = AnchorTargetCreator(n_sample, pos_iou_thresh, neg_iou_thresh, pos_ratio)(bbox, anchor),
 * nets/frcnn_training.py:19-103, with n_pos = int(pos_ratio * n_sample) computed by the caller:
 *   anchor [A][4], bbox [G][4] (G may be 0) ->
 *   label  [A] int64: -1 ignore / 0 negative / 1 positive     loc [A][4]: bbox2loc(anchor, bbox[argmax]) or zeros when
 *   argmax [A] int32: the gt index each anchor is assigned to  there is no positive
 * tsod_proposal_targets_f32 = ProposalTargetCreator(n_sample, pos_ratio, pos_iou_thresh, neg_iou_thresh_high,
 * neg_iou_thresh_low)(roi, bbox, label), nets/frcnn_training.py:105-177, pos_per_image = int(n_sample * pos_ratio):
 *   roi [R][4], bbox [G][4], gt_label [G] int64 -> the first counts[0] = S <= n_sample rows of
 *   sample_roi [n_sample][4], gt_roi_loc [n_sample][4], gt_roi_label [n_sample] int64;
 *   counts [4] int32 = (S, kept positives, kept negatives, status): status 1 = the reference raises IndexError here
 *   (quirk T2: a sampled negative's original index lies beyond the kept list).
 * Both need 0 <= n_pos (pos_per_image) <= n_sample, i.e. pos_ratio in [0, 1]: beyond it the reference's negative slices take a
 * negative bound (they drop only the last negatives), which is not restated - TSOD_ERR_INVALID_ARG.
 * tsod_anchor_targets_f32 also refuses G == 0 with pos_iou_thresh <= 0 (TSOD_ERR_INVALID_ARG, before any launch): every anchor
 * would be positive with no box to take offsets to; G > 0 with pos_iou_thresh <= 0 is legal (all positive, every box exists). */
size_t tsod_anchor_targets_workspace_bytes(int32_t A, int32_t G);
int tsod_anchor_targets_f32(const float *anchor, int32_t A, const float *bbox, int32_t G, float pos_iou_thresh,
                            float neg_iou_thresh, int32_t n_pos, int32_t n_sample, float *loc, int64_t *label,
                            int32_t *argmax, void *workspace, size_t workspace_bytes, tsod_stream_t stream);
size_t tsod_proposal_targets_workspace_bytes(int32_t R, int32_t G, int32_t n_sample);
int tsod_proposal_targets_f32(const float *roi, int32_t R, const float *bbox, int32_t G, const int64_t *gt_label,
                              int32_t n_sample, int32_t pos_per_image, float pos_iou_thresh, float neg_iou_thresh_high,
                              float neg_iou_thresh_low, float *sample_roi, float *gt_roi_loc, int64_t *gt_roi_label,
                              int32_t *counts, void *workspace, size_t workspace_bytes, tsod_stream_t stream);

/* The same two assignments for a whole batch in one pass: the image index rides on a grid dimension (the two one-workgroup
 * kernels run one workgroup per image), four launches (three when Gmax == 0) and two launches for all B images, no host
 * synchronisation, no float atomics, and no result depends on what the workspace held before the call.  Ground truth is padded
 * as for tsod_eval_match_f32: bbox [B][Gmax][4], gt_label [B][Gmax] int64, gt_counts [B] int32 ON THE DEVICE.  gt_counts[b] is
 * read by the kernels and clamped to [0, Gmax]; rows [gt_counts[b], Gmax) of image b are never read (they may hold anything, NaN
 * included).  Gmax == 0 is legal: bbox, gt_label and gt_counts may then be NULL and every image has no ground truth.
 * Image b's results are bit for bit those of the single-image entry points on (anchor, bbox[b][:gt_counts[b]]) and
 * (roi[b], bbox[b][:gt_counts[b]], gt_label[b][:gt_counts[b]]), quirks T1, T2 and T4 included: they are the same kernels and the
 * same launch sequences - a single-image call is a batch of one whose box count is passed by value.
 *
 * tsod_anchor_targets_batch_f32: anchor [A][4] is shared by the batch -> loc [B][A][4], label [B][A] int64, argmax [B][A] int32.
 *   workspace: tsod_anchor_targets_batch_workspace_bytes(B, A, Gmax) = B * (align16(4 A) + align16(4 max(Gmax, 1)) + 16)
 *   = B * tsod_anchor_targets_workspace_bytes(A, Gmax); 0 for B outside [1, 65535], A <= 0 or Gmax < 0.
 * tsod_proposal_targets_batch_f32: roi [B][R][4] -> sample_roi / gt_roi_loc [B][n_sample][4], gt_roi_label [B][n_sample] int64,
 *   counts [B][4] int32 = per image (S, kept positives, kept negatives, status), sample_src [B][n_sample] int32 or NULL (the rows
 *   of cat(roi[b], bbox[b][:gt_counts[b]]), as tsod_proposal_targets_src_f32).  One behaviour the single-image entry points do
 *   not have: rows [counts[b][0], n_sample) of image b are WRITTEN - zeros in sample_roi, gt_roi_loc and gt_roi_label, -1 in
 *   sample_src - so a caller that defers reading counts runs the head and the losses on defined memory.  An image with
 *   R + gt_counts[b] == 0 candidates keeps nothing: counts[b] = (0, 0, 0, 0).
 *   workspace:
 *   tsod_proposal_targets_batch_workspace_bytes(B, R, Gmax, n_sample) = B * (2 align16(4 (R + Gmax)) + align16(4 n_sample))
 *   = B * tsod_proposal_targets_workspace_bytes(R, Gmax, n_sample); 0 for B outside [1, 65535], R < 0, Gmax < 0, R + Gmax <= 0
 *   or n_sample <= 0.
 * Both refuse what the single-image entry points refuse (n_pos / pos_per_image > n_sample: TSOD_ERR_INVALID_ARG; anchor, roi,
 * bbox, loc, sample_roi, gt_roi_loc or the workspace not 16-byte aligned: TSOD_ERR_ALIGNMENT / TSOD_ERR_WORKSPACE; a short
 * workspace: TSOD_ERR_WORKSPACE) and B outside [1, 65535] (it is a grid dimension), before any launch; the anchor call also
 * refuses pos_iou_thresh <= 0, with which an image without ground truth would have positives and no box to take offsets to. */
size_t tsod_anchor_targets_batch_workspace_bytes(int32_t B, int32_t A, int32_t Gmax);
int tsod_anchor_targets_batch_f32(const float *anchor, int32_t A, const float *bbox, const int32_t *gt_counts, int32_t B,
                                  int32_t Gmax, float pos_iou_thresh, float neg_iou_thresh, int32_t n_pos, int32_t n_sample,
                                  float *loc, int64_t *label, int32_t *argmax, void *workspace, size_t workspace_bytes,
                                  tsod_stream_t stream);
size_t tsod_proposal_targets_batch_workspace_bytes(int32_t B, int32_t R, int32_t Gmax, int32_t n_sample);
int tsod_proposal_targets_batch_f32(const float *roi, int32_t R, const float *bbox, const int64_t *gt_label,
                                    const int32_t *gt_counts, int32_t B, int32_t Gmax, int32_t n_sample, int32_t pos_per_image,
                                    float pos_iou_thresh, float neg_iou_thresh_high, float neg_iou_thresh_low, float *sample_roi,
                                    float *gt_roi_loc, int64_t *gt_roi_label, int32_t *counts, int32_t *sample_src,
                                    void *workspace, size_t workspace_bytes, tsod_stream_t stream);

/* ---- the losses of the ground-truth-conditioned forward (FasterRCNNTrainer, nets/frcnn_training.py:179-342) ----------
 * Both are additive restatements of the reference's loss arithmetic on the outputs of the kernels above; one workgroup per
 * image, sums in f64 in a fixed order (deterministic, no atomics, no workspace), each loss rounded once to f32.
 * smooth L1 (nets/frcnn_training.py:220-238, sigma = rpn_sigma / roi_sigma): over the positives (label > 0) and their 4
 * offsets, d = |gt - pred|, d < 1/sigma^2 ? 0.5 sigma^2 d^2 : d - 0.5/sigma^2, summed and divided by 4 * n_pos - NaN without a
 * positive (0/0, as the reference).  Cross-entropy: log-sum-exp minus the target logit, mean over the counted rows - NaN when
 * there is none.  status[b] = number of labels of image b the reference would index out of bounds with (IndexError there);
 * such a label is never used as an index and its row does not count.
 *
 * tsod_rpn_losses_f32: nets/frcnn_training.py:262-274.  rpn_out [B*n_pix][pitch] is the fused RPN conv's output (loc in
 *   columns [0,4A), (bg, fg) logits in [4A,6A); anchor t = pixel*A + a, quirk Q9), read in place.
 *   gt_loc [B][n_pix*A][4], gt_label [B][n_pix*A] int64 in {-1 ignore, 0, 1} (tsod_anchor_targets_f32) ->
 *   out [B][2] = (loc loss, cls loss with ignore_index = -1), status [B].
 * tsod_roi_losses_f32: nets/frcnn_training.py:300-331.  cls_locs [B*S] rows of 4*n_class (pitch loc_pitch), scores [B*S]
 *   rows of n_class logits (pitch score_pitch) - column slices of the fused head GEMM's output like tsod_detections_f32's -
 *   sample_roi / gt_roi_loc [B][S][4], gt_roi_label [B][S] int64 in [0, n_class) ->
 *   anchors_pred [B][S][4] = loc2bbox(sample_roi, cls_loc[row, gt_label]) (the decode of tsod_loc2bbox_f32; NaN rows for an
 *   out-of-range label), classes_pred [B][S] int64 / classes_score_pred [B][S] = arg-max / max of the raw logits (first
 *   maximum wins, quirk Q11; a row holding a NaN logit gives (the first NaN's column, NaN), as torch.argmax / torch.max, and a
 *   NaN cls loss), out [B][2] = (loc loss, cls loss over all n_class logits), status [B]. */
int tsod_rpn_losses_f32(const float *rpn_out, int32_t pitch, int32_t A, int32_t B, int32_t n_pix, const float *gt_loc,
                        const int64_t *gt_label, float sigma, float *out, int32_t *status, tsod_stream_t stream);
int tsod_roi_losses_f32(const float *cls_locs, int32_t loc_pitch, const float *scores, int32_t score_pitch,
                        const float *sample_roi, const float *gt_roi_loc, const int64_t *gt_roi_label, int32_t B, int32_t S,
                        int32_t n_class, float sigma, float *anchors_pred, int64_t *classes_pred, float *classes_score_pred,
                        float *out, int32_t *status, tsod_stream_t stream);

/* ---- the backward of those losses into the eight head parameters (FasterRCNNTrainer(head_grads=True), frozen backbone) -----
 * What autograd computes behind the reference's losses[-1].backward() for rpn.loc / rpn.score / head.cls_loc / head.score.
 * `up` [5] f32 on the device = d out / d (rpn_loc, rpn_cls, roi_loc, roi_cls, total loss): loss k is weighted by up[k] + up[4],
 * times inv_B (the batch mean).  No host synchronisation, no float atomics: run to run bit-identical.  Torch's empty sets:
 * no positive / no counted row gives zero gradients from that term (its loss is NaN); |d| == 0 gives abs's zero subgradient.
 *
 * tsod_proposal_targets_src_f32: tsod_proposal_targets_f32 (the same checks, the same two launches) plus sample_src [n_sample]
 *   int32 = the row of cat(roi, bbox) each sample was taken from (the reference's keep_index, nets/frcnn_training.py:165): < R a
 *   proposal, >= R a ground-truth box.  Like it, and unlike the batched call, it leaves rows [counts[0], n_sample) untouched.
 * tsod_rpn_losses_grad_f32: d rpn_out [B*n_pix][d_pitch] of the two RPN losses, in the fused layout tsod_rpn_losses_f32 reads
 *   (loc columns [0,4A), logits [4A,6A), zero columns after); n_rows [B][2] int32 out = (positives, counted rows).
 * tsod_roi_losses_grad_f32: d both [B*S][d_pitch] of the two head losses in the fused head GEMM's layout (cls_loc columns
 *   [0,4 n_class), score columns [4 n_class, 5 n_class), zero after) and d sample_roi [B][S][4] through the regression target
 *   gt_roi_loc = bbox2loc(sample_roi, gt) (utils/loc_bbox_iou.py:63-88; zero rows for non-positive samples).
 * tsod_rpn_roi_scatter_f32: adds d sample_roi into the loc columns of d rpn_out along the index chain sample_src (< R) ->
 *   keep_idx [B][R] (tsod_nms_f32, with its padding) -> sort_idx [B][n_pre] (tsod_sort_topk_desc_f32) -> anchor t; the
 *   unclamped decode of anchors[t] with rpn_out's offsets is recomputed, the clamp passes where 0 <= v <= clamp (x: clamp_x,
 *   y: clamp_y, inclusive), then loc2bbox's backward.  Sample rows reaching one anchor are summed in ascending order by one
 *   thread.  S <= 1024.
 * tsod_wgrad_f32: dW[n][k] = sum_m dy[m][n] x[m][k], db[n] = sum_m dy[m][n] on the f32 matrix cores (v_mfma_f32_32x32x2_f32),
 *   dy [M][dy_pitch], x [M][x_pitch] (16-byte aligned, K and x_pitch multiples of 4).  Rows [0,n0) of the result go to dw0
 *   [n0][K] / db0 [n0], rows [n0,n0+n1) to dw1 / db1 (db may be NULL), rows past n0+n1 are dropped.  accumulate = 0 writes,
 *   1 adds to what is there.  M is split across workgroups (about 512 of them); the M-slices' partial tiles are summed in
 *   slice order by a second launch.  workspace: tsod_wgrad_workspace_bytes(M, N, K). */
int tsod_proposal_targets_src_f32(const float *roi, int32_t R, const float *bbox, int32_t G, const int64_t *gt_label,
                                  int32_t n_sample, int32_t pos_per_image, float pos_iou_thresh, float neg_iou_thresh_high,
                                  float neg_iou_thresh_low, float *sample_roi, float *gt_roi_loc, int64_t *gt_roi_label,
                                  int32_t *counts, int32_t *sample_src, void *workspace, size_t workspace_bytes,
                                  tsod_stream_t stream);
int tsod_rpn_losses_grad_f32(const float *rpn_out, int32_t pitch, int32_t A, int32_t B, int32_t n_pix, const float *gt_loc,
                             const int64_t *gt_label, float sigma, const float *up, float inv_B, int32_t *n_rows,
                             float *d_rpn_out, int32_t d_pitch, tsod_stream_t stream);
int tsod_roi_losses_grad_f32(const float *cls_locs, int32_t loc_pitch, const float *scores, int32_t score_pitch,
                             const float *sample_roi, const float *gt_roi_loc, const int64_t *gt_roi_label, int32_t B, int32_t S,
                             int32_t n_class, float sigma, const float *up, float inv_B, float *d_both, int32_t d_pitch,
                             float *d_sample_roi, tsod_stream_t stream);
int tsod_rpn_roi_scatter_f32(const float *d_sample_roi, const int32_t *sample_src, int32_t B, int32_t S, int32_t R,
                             const int32_t *keep_idx, const int32_t *sort_idx, int32_t n_pre, const float *rpn_out, int32_t pitch,
                             const float *anchors, int32_t A, int32_t n_pix, float clamp_x, float clamp_y, float *d_rpn_out,
                             int32_t d_pitch, tsod_stream_t stream);
size_t tsod_wgrad_workspace_bytes(int64_t M, int32_t N, int32_t K);
int tsod_wgrad_f32(const float *dy, int64_t M, int32_t N, int32_t dy_pitch, const float *x, int32_t K, int32_t x_pitch,
                   int32_t n0, float *dw0, float *db0, int32_t n1, float *dw1, float *db1, int32_t accumulate, void *workspace,
                   size_t workspace_bytes, tsod_stream_t stream);

/* ---- feature gradients: the backward of the RoI head's pooling into the feature map (FasterRCNNTrainer(features=...)) ------
 * The RoI term of d loss / d feature map, written into (or, accumulate = 1, added to) d_feat [B][Hf][Wf][d_feat_pitch] NHWC:
 * the arguments of tsod_roi_pool_avg_f32 / tsod_roi_align_avg_f32 plus d_out [B*R][d_out_pitch] = d loss / d (their output).
 * A gather: one thread owns a (pixel, channel quad) of d_feat and sums what reaches it in a fixed order (RoI groups whose
 * roi_indices name its image, in group order; the RoIs of a group ascending; bins, then samples and corners, in the forward's
 * order) - no atomics, bit-identical from run to run.  Any roi_indices mapping; RoIs of an index outside [0, B) contribute 0.
 * tsod_roi_pool_avg_grad_f32: torchvision's roi_pool backward - bin (ph, pw) gives d_out / (PH PW) to its arg-max pixel
 *   (recomputed from `feat` by a pre-pass with the forward's rule: from -FLT_MAX, strict '>', h outer, w inner; empty bins and
 *   bins without a value above -FLT_MAX give nothing).  The arg-max is recorded as a u16 map index: Hf * Wf <= 65535
 *   (TSOD_ERR_UNSUPPORTED otherwise), B * R <= 65535.  workspace: tsod_roi_pool_avg_grad_workspace_bytes(B, R, C, PH, PW)
 *   (B*R*PH*PW*C u16 of arg-max record + 16 B per RoI).
 * tsod_roi_align_avg_grad_f32: torchvision's roi_align backward - sample (iy, ix) of bin (ph, pw) gives w1..w4 x d_out /
 *   (PH PW count) to its four corners (the forward's positions, [-1, H] x [-1, W] skip, clamps and corner collapse); the
 *   feature values are not read.  workspace: tsod_roi_align_avg_grad_workspace_bytes(B, R) (16 B per RoI). */
size_t tsod_roi_pool_avg_grad_workspace_bytes(int32_t B, int32_t R, int32_t C, int32_t PH, int32_t PW);
int tsod_roi_pool_avg_grad_f32(const float *feat, int32_t B, int32_t Hf, int32_t Wf, int32_t C, int32_t feat_pitch,
                               const float *rois, const int32_t *roi_indices, int32_t R, float img_h, float img_w,
                               float spatial_scale, int32_t PH, int32_t PW, const float *d_out, int32_t d_out_pitch, float *d_feat,
                               int32_t d_feat_pitch, int32_t accumulate, void *workspace, size_t workspace_bytes,
                               tsod_stream_t stream);
size_t tsod_roi_align_avg_grad_workspace_bytes(int32_t B, int32_t R);
int tsod_roi_align_avg_grad_f32(int32_t B, int32_t Hf, int32_t Wf, int32_t C, const float *rois, const int32_t *roi_indices,
                                int32_t R, float img_h, float img_w, float spatial_scale, int32_t PH, int32_t PW,
                                int32_t sampling_ratio, int32_t aligned, const float *d_out, int32_t d_out_pitch, float *d_feat,
                                int32_t d_feat_pitch, int32_t accumulate, void *workspace, size_t workspace_bytes,
                                tsod_stream_t stream);

/* ---- the HarDNet tail's backward: depthwise 3x3 and the grouped pair 1x1 ---------------------------
 * NHWC f32 with pixel pitches and channel offsets like the forwards; no float atomics, bit-identical from run to run: the
 * parameter gradients are per-workgroup partial sums over pixel slices (slice count and in-workgroup tree fixed by the shape),
 * added in slice order by a second launch.
 * tsod_dwconv3x3_grad_f32: backward of y = relu?(scale[c] * dwconv3x3(x, w)[c] + shift[c]) (tsod_dwconv3x3_f32's arguments;
 *   scale / shift NULL = 1 / 0).  dy [N][OH][OW][dy_pitch]; g = dy * [y > 0] with relu (the mask is recomputed from x with the
 *   forward's tap order), else dy.
 *     dx [N][H][W][dx_pitch] (NULL: skipped) = scale * sum over the outputs that read the pixel of w[dh][dw] * g, dh then dw
 *        ascending: a gather by the thread that owns the pixel's channel quad; accumulate = 1 adds to what is there.
 *     dw [3][3][C] = scale[c] * sum_pixels g * x_tap;  dscale [C] = sum g * dwconv3x3(x, w) (may be NULL; must be NULL when scale
 *        is NULL);  dshift [C] = sum g.
 *     dw and dshift NULL together (then dscale NULL and dx not): no parameter gradient is computed - without relu the dx gather is
 *        the only launch and no workspace is read.
 *   workspace: tsod_dwconv3x3_grad_workspace_bytes(N, H, W, C, stride, relu_dx) - the partials, and with relu_dx (= relu and a
 *   non-NULL dx) room for g, which the dx gather reads.  16-byte aligned pointers, C / pitches / offsets multiples of 4.
 * tsod_gconv1x1_pair_grad_f32: backward of tsod_gconv1x1_pair_f32.  d_out [pixels][d_out_pitch];
 *   d_in [pixels][d_in_pitch] (columns [0, 2G): d_in[2g + j] = w[g][j] * d_out[g]), dw [G][2] = sum_pixels d_out[g] * in[2g + j],
 *   dbias [G] = sum_pixels d_out[g]; each of the three may be NULL (skipped).  in / d_in 8-byte aligned with even pitches.
 *   workspace: tsod_gconv1x1_pair_grad_workspace_bytes(pixels, G). */
size_t tsod_dwconv3x3_grad_workspace_bytes(int32_t N, int32_t H, int32_t W, int32_t C, int32_t stride, int32_t relu_dx);
int tsod_dwconv3x3_grad_f32(const float *x, int32_t N, int32_t H, int32_t W, int32_t C, int32_t in_pitch, int32_t in_off,
                            const float *w, const float *scale, const float *shift, int32_t stride, int32_t relu,
                            const float *dy, int32_t dy_pitch, int32_t dy_off, float *dx, int32_t dx_pitch, int32_t dx_off,
                            int32_t accumulate, float *dw, float *dscale, float *dshift, void *workspace,
                            size_t workspace_bytes, tsod_stream_t stream);
size_t tsod_gconv1x1_pair_grad_workspace_bytes(int64_t pixels, int32_t G);
int tsod_gconv1x1_pair_grad_f32(const float *in, int64_t pixels, int32_t G, int32_t in_pitch, const float *w,
                                const float *d_out, int32_t d_out_pitch, float *d_in, int32_t d_in_pitch, float *dw,
                                float *dbias, void *workspace, size_t workspace_bytes, tsod_stream_t stream);

/* ---- the backward of a HarDNet 1x1 ConvLayer --------------------------------------------------------
 * y[m][o] = relu6(scale[o] * sum_k w[o][k] x[m][k] + shift[o]) on pixel rows m: x is gathered from channel segments of an NHWC
 * buffer [M][x_pitch] (tsod_pw_segs: buffer offset, padded width - both multiples of 4 - and real width of every segment, in the
 * K order of w [N][K], K = the sum of the padded widths, zero columns at the pad channels), BN folded into scale / shift [N].
 * No float atomics; bit-identical from run to run.
 * tsod_dwconv3x3_grad_act_f32: tsod_dwconv3x3_grad_f32 (same arguments, same workspace query, same dw / dscale / dshift) whose
 *   dx gather keeps a value only where the x pixel it owns has 0 < x < 6: with x = a ConvLayer's output this dx is that layer's
 *   masked gradient g, one pass saved.
 * tsod_relu6_grad_mask_f32: g [rows][g_pitch] = dy [rows][dy_pitch] (columns [dy_off, dy_off + C)) * [0 < y < 6], y
 *   [rows][y_pitch] the forward's output (both comparisons strict: torch's hardtanh backward).  16-byte aligned, C / pitches /
 *   dy_off multiples of 4.
 * tsod_pw_wgrad_f32: dWraw = g^T x_gathered on v_mfma_f32_32x32x2_f32 (g [M][g_pitch], N columns), M cut into slices whose
 *   partial tiles a finishing launch adds in slice order; it writes dw [n_real][sum of real widths] = scale[o] * dWraw (pad
 *   rows and columns dropped), dscale [n_real] = sum_k w[o][k] * dWraw[o][k], dshift [n_real] = sum_m g[m][o]; each of the
 *   three may be NULL (not all).  Slices: enough for about 512 workgroups, at least 64 row pairs each, and never more slab
 *   floats than M (N + K), the operands.  workspace: tsod_pw_wgrad_workspace_bytes(M, N, K).
 * tsod_pw_dgrad_f32: dx [M][dx_pitch] columns of every segment with want != 0 (=, or accumulate = 1: +=)
 *   sum_o (g[m][o] * scale[o]) * w[o][k], o ascending, the old value added last; pad columns of a wanted segment are written as
 *   exact zeros, segments with want == 0 and everything between segments are not touched.  N, g_pitch multiples of 4. */
#define TSOD_PW_MAX_SEGMENTS 16
typedef struct tsod_pw_segs {
    int32_t n_seg;
    int32_t off[TSOD_PW_MAX_SEGMENTS];  /* first channel in the buffer */
    int32_t len[TSOD_PW_MAX_SEGMENTS];  /* padded width */
    int32_t real[TSOD_PW_MAX_SEGMENTS]; /* real width, 1..len */
    int32_t want[TSOD_PW_MAX_SEGMENTS]; /* tsod_pw_dgrad_f32: this segment's dx is wanted */
} tsod_pw_segs;
int tsod_dwconv3x3_grad_act_f32(const float *x, int32_t N, int32_t H, int32_t W, int32_t C, int32_t in_pitch, int32_t in_off,
                                const float *w, const float *scale, const float *shift, int32_t stride, int32_t relu,
                                const float *dy, int32_t dy_pitch, int32_t dy_off, float *dx, int32_t dx_pitch, int32_t dx_off,
                                int32_t accumulate, float *dw, float *dscale, float *dshift, void *workspace,
                                size_t workspace_bytes, tsod_stream_t stream);
int tsod_relu6_grad_mask_f32(const float *y, int64_t rows, int32_t C, int32_t y_pitch, const float *dy, int32_t dy_pitch,
                             int32_t dy_off, float *g, int32_t g_pitch, tsod_stream_t stream);
size_t tsod_pw_wgrad_workspace_bytes(int64_t M, int32_t N, int32_t K);
int tsod_pw_wgrad_f32(const float *g, int64_t M, int32_t N, int32_t g_pitch, const float *x, int32_t x_pitch,
                      const tsod_pw_segs *segs, const float *w, const float *scale, int32_t n_real, float *dw, float *dscale,
                      float *dshift, void *workspace, size_t workspace_bytes, tsod_stream_t stream);
int tsod_pw_dgrad_f32(const float *g, int64_t M, int32_t N, int32_t g_pitch, const float *w, const float *scale,
                      const tsod_pw_segs *segs, float *dx, int32_t dx_pitch, int32_t accumulate, tsod_stream_t stream);

/* ---- what a ResNet Bottleneck's backward adds to the 1x1 kernels above -----------------------------
 * y = prelu(z) with ONE slope a, finite and > 0 (the caller checks), so that the saved output y has z's sign.
 * No float atomics; bit-identical from run to run.
 * tsod_prelu_grad_f32: g [rows][g_pitch] = dy [rows][dy_pitch] (columns [dy_off, dy_off + C)) * (y > 0 ? 1 : slope), y
 *   [rows][y_pitch] the forward's output; *dslope_num = sum dy * y * [y < 0] (the slope's gradient times the slope), a two-stage
 *   sum: per-workgroup partials in the workspace, then one finishing workgroup.  dslope_num NULL: no sum, the workspace is not
 *   read.  An exact y == 0 takes the slope branch and adds nothing to the sum.  16-byte aligned, C / pitches / dy_off multiples
 *   of 4.  workspace: tsod_prelu_grad_workspace_bytes(rows, C) (0 for a shape that is refused).
 * tsod_conv3x3_dense_wgrad_f32: the parameter gradients of z = scale[o] * conv3x3(x, w, pad 1, stride 1) + shift[o] from the
 *   masked gradient g [N][H][W][g_pitch] (Cout columns), x [N][H][W][x_pitch] (C channels), w [Cout][3][3][C] unscaled (the
 *   forward's f32 pack), scale [Cout]: dWraw = g^T patches(x) on v_mfma_f32_32x32x2_f32 with K = 9 C gathered columns, N H W cut
 *   into slices by tsod_pw_wgrad_f32's rule; dw [Cout][3][3][C] = scale[o] * dWraw, dscale [Cout] = sum_k w[o][k] dWraw[o][k],
 *   dshift [Cout] = sum g; each of the three may be NULL (not all).  C, Cout, pitches multiples of 4; x, g, workspace 16-byte
 *   aligned.  stride: only 1 is built, anything else is TSOD_ERR_UNSUPPORTED.
 *   workspace: tsod_conv3x3_dense_wgrad_workspace_bytes(N, H, W, C, Cout) (0 for a shape that is refused).
 * The 3x3 conv's dx is tsod_conv2d_f32 on g with the weights w_rot[c][kh][kw][o] = scale[o] * w[o][2 - kh][2 - kw][c]. */
size_t tsod_prelu_grad_workspace_bytes(int64_t rows, int32_t C);
int tsod_prelu_grad_f32(const float *y, int64_t rows, int32_t C, int32_t y_pitch, const float *dy, int32_t dy_pitch,
                        int32_t dy_off, float slope, float *g, int32_t g_pitch, float *dslope_num, void *workspace,
                        size_t workspace_bytes, tsod_stream_t stream);
size_t tsod_conv3x3_dense_wgrad_workspace_bytes(int32_t N, int32_t H, int32_t W, int32_t C, int32_t Cout);
int tsod_conv3x3_dense_wgrad_f32(const float *g, int32_t N, int32_t H, int32_t W, int32_t Cout, int32_t g_pitch, const float *x,
                                 int32_t C, int32_t x_pitch, const float *w, const float *scale, int32_t stride, float *dw,
                                 float *dscale, float *dshift, void *workspace, size_t workspace_bytes, tsod_stream_t stream);

/* ---- what a projection Bottleneck's backward adds to those -----------------------------------------
 * A 3x3 at stride s (1 or 2), pad 1: x [N][H][W], outputs [N][OH][OW] with OH = (H - 1) / s + 1, OW = (W - 1) / s + 1.
 * No float atomics; bit-identical from run to run.
 * tsod_conv3x3_strided_wgrad_f32: tsod_conv3x3_dense_wgrad_f32's contract with g [N][OH][OW][g_pitch] over the output grid
 *   and x [N][H][W][x_pitch]; the slices cut N OH OW.  stride 1 or 2, anything else is TSOD_ERR_UNSUPPORTED; with stride 1 the
 *   bits of tsod_conv3x3_dense_wgrad_f32.  workspace: tsod_conv3x3_strided_wgrad_workspace_bytes(N, H, W, C, Cout, stride) (0 for
 *   a shape that is refused).
 * tsod_prelu_grad_d2s_f32: tsod_prelu_grad_f32 for y [N][H][W][y_pitch] (C channels) whose dy is never written out: it is read
 *   from p [N][(H - 1) / 2 + 2][(W - 1) / 2 + 2][p_pitch] (4 C columns), the stride-1, pad-1 conv of the stride-2 3x3's masked
 *   output gradient with the 2x2 phase pack [4 C][2][2][Cout] (rows ((ih & 1) 2 + (iw & 1)) C + c), as
 *   dy[n][ih][iw][c] = p[n][(ih >> 1) + 1][(iw >> 1) + 1][((ih & 1) 2 + (iw & 1)) C + c].  The grid, the sum and its order are
 *   tsod_prelu_grad_f32's for rows = N H W.  dslope_num may be NULL.  16-byte aligned, C and pitches multiples of 4.
 *   workspace: tsod_prelu_grad_d2s_workspace_bytes(N, H, W, C) (0 for a shape that is refused).
 * tsod_pixel_subsample_f32: xs [N][OH][OW][xs_pitch] (C columns) = x [N][H][W][x_pitch] at pixels (s oh, s ow), any s >= 1: the
 *   rows a strided 1x1 conv reads, so that tsod_pw_wgrad_f32 serves it.
 * tsod_pixel_upsample_add_f32: dx[n][s oh][s ow][c] = dx[n][s oh][s ow][c] + d[n][oh][ow][c] (dx the first operand, one add per
 *   touched element; every other element of dx is left as it is): that conv's input gradient added into the block's.
 *   Both: C and pitches multiples of 4, 16-byte aligned, N H W below 2^31. */
size_t tsod_conv3x3_strided_wgrad_workspace_bytes(int32_t N, int32_t H, int32_t W, int32_t C, int32_t Cout, int32_t stride);
int tsod_conv3x3_strided_wgrad_f32(const float *g, int32_t N, int32_t H, int32_t W, int32_t Cout, int32_t g_pitch, const float *x,
                                   int32_t C, int32_t x_pitch, const float *w, const float *scale, int32_t stride, float *dw,
                                   float *dscale, float *dshift, void *workspace, size_t workspace_bytes, tsod_stream_t stream);
size_t tsod_prelu_grad_d2s_workspace_bytes(int32_t N, int32_t H, int32_t W, int32_t C);
int tsod_prelu_grad_d2s_f32(const float *y, int32_t N, int32_t H, int32_t W, int32_t C, int32_t y_pitch, const float *p,
                            int32_t p_pitch, float slope, float *g, int32_t g_pitch, float *dslope_num, void *workspace,
                            size_t workspace_bytes, tsod_stream_t stream);
int tsod_pixel_subsample_f32(const float *x, int32_t N, int32_t H, int32_t W, int32_t C, int32_t x_pitch, int32_t stride,
                             float *xs, int32_t xs_pitch, tsod_stream_t stream);
int tsod_pixel_upsample_add_f32(float *dx, int32_t N, int32_t H, int32_t W, int32_t C, int32_t dx_pitch, int32_t stride,
                                const float *d, int32_t d_pitch, tsod_stream_t stream);

/* ---- the backward of ResNet's stem ------------------------------------------------------------------
 * z = scale[o] * conv7x7(x4, w, stride 2, pad 3)[o] + shift[o], y = prelu(z) [N][OH][OW] with OH = (H - 1) / 2 + 1, then
 * MaxPool2d(3, 2, 1) to [N][PH][PW] with PH = (OH - 1) / 2 + 1, PW = (OW - 1) / 2 + 1.  No float atomics; bit-identical from run
 * to run.
 * tsod_prelu_grad_pool_f32: tsod_prelu_grad_f32 for y [N][OH][OW][y_pitch] (C channels) whose dy is never written out: it is
 *   gathered from dp [N][PH][PW][dp_pitch], the gradient of the pooled map, as dy[n][oh][ow][c] = the sum, over the windows
 *   (ph, pw) that contain (oh, ow) in ascending (ph, pw), of dp[n][ph][pw][c] where the window's maximum is first met at
 *   (oh, ow).  Window ph covers rows 2 ph - 1 .. 2 ph + 1; "first": an ascending (kh, kw) scan of the window's taps inside the
 *   image with a strict > to replace (torch's max_pool2d backward); the winner is recomputed from y, no index tensor exists.
 *   Then g = dy * (y > 0 ? 1 : slope) and *dslope_num = sum dy * y * [y < 0]; the grid, the sum and its order are
 *   tsod_prelu_grad_f32's for rows = N OH OW, an exact y == 0 behaves as there.  dslope_num may be NULL.  Inputs are finite (the
 *   place of a NaN among the taps is not specified).  16-byte aligned, C and pitches multiples of 4; N OH OW C / 4 below 2^31
 *   (TSOD_ERR_UNSUPPORTED).  workspace: tsod_prelu_grad_pool_workspace_bytes(N, OH, OW, C) (0 for a shape that is refused).
 * tsod_conv7x7s2_wgrad_f32: the parameter gradients of z from the masked gradient g [N][OH][OW][g_pitch] (Cout columns), the
 *   staged image x4 [N][H][W][4], w [Cout][7][8][4] unscaled (the forward's f32 pack: kw = 7 and c = 3 are zero padding), scale
 *   [Cout].  dWraw[o][kh][kw][c] = sum_{n,oh,ow} g[n][oh][ow][o] x4[n][2 oh - 3 + kh][2 ow - 3 + kw][c] (taps outside the image
 *   are zeros) on v_mfma_f32_32x32x2_f32, one kernel row (8 x 4 floats, contiguous in x4) per column tile, over slices of pixel
 *   pairs numbered (n, oh, ow / 2) ascending: ceil(pairs / 256) pairs per slice, at least 64; the shape alone fixes them.  A
 *   finishing launch adds the slices in slice order and writes dw [Cout][7][8][4] = scale[o] * dWraw with exact zeros in the
 *   padding, dscale [Cout] = the sum over the 147 real taps of w * dWraw in ascending (kh, kw, c), dshift [Cout] = sum g.
 *   Each of the three may be NULL (not all).  Channel 3 of x4 and the pixels a kw = 7 tap would read reach no result, whatever
 *   they hold (a NaN included).  Cout must be 64 and N H W at most (2^31 - 1) / 4 (TSOD_ERR_UNSUPPORTED otherwise).  16-byte
 *   aligned pointers, g_pitch a multiple of 4.
 *   workspace: tsod_conv7x7s2_wgrad_workspace_bytes(N, H, W, Cout) = slices * 64 * 225 floats; 0 for a shape that is refused. */
size_t tsod_prelu_grad_pool_workspace_bytes(int32_t N, int32_t OH, int32_t OW, int32_t C);
int tsod_prelu_grad_pool_f32(const float *y, int32_t N, int32_t OH, int32_t OW, int32_t C, int32_t y_pitch, const float *dp,
                             int32_t dp_pitch, float slope, float *g, int32_t g_pitch, float *dslope_num, void *workspace,
                             size_t workspace_bytes, tsod_stream_t stream);
size_t tsod_conv7x7s2_wgrad_workspace_bytes(int32_t N, int32_t H, int32_t W, int32_t Cout);
int tsod_conv7x7s2_wgrad_f32(const float *g, int32_t N, int32_t H, int32_t W, int32_t Cout, int32_t g_pitch, const float *x4,
                             const float *w, const float *scale, float *dw, float *dscale, float *dshift, void *workspace,
                             size_t workspace_bytes, tsod_stream_t stream);

/* ---- the parameter gradients of HarDNet's first layer ----------------------------------------------
 * y[n][oh][ow][o] = relu6(scale[o] * sum_{kh,kw,c} w[o][kh][kw][c] x4[n][oh s - 1 + kh][ow s - 1 + kw][c] + shift[o]), s = stride
 * (1 or 2), pad 1, OH = (H - 1) / s + 1, OW = (W - 1) / s + 1.  x4 [N][H][W][4] (channel 3 is padding and is never read), y
 * [N][OH][OW][Cout_pad] the forward's saved output, dy [N][OH][OW][dy_pitch] (columns [dy_off, dy_off + Cout_pad)), w
 * [Cout_pad][3][3][4] the unscaled weight, scale [Cout_pad].  Cout_pad a multiple of 4, at most 64.  There is no dx.
 * tsod_conv3x3_wgrad_f32: g = dy * [0 < y < 6] (both strict) taken from y inside the kernel; dWraw = sum_{n,oh,ow} g * patch on
 *   v_mfma_f32_32x32x2_f32 over slices of whole output rows (at most 512 slices, at least 256 pixel pairs each; the shape alone
 *   fixes them), a finishing launch adds the slices in slice order and writes dw [Cout_pad][3][3][4] = scale[o] * dWraw, dscale
 *   [Cout_pad] = sum over the 27 real taps of w * dWraw (ascending kh, kw, c), dshift [Cout_pad] = sum g.  Rows o >= Cout_real
 *   and channel 3 of dw are exact zeros.  Each of the three may be NULL (not all).  No float atomics; bit-identical from run
 *   to run.  16-byte aligned pointers; dy_pitch and dy_off multiples of 4.
 *   workspace: tsod_conv3x3_wgrad_workspace_bytes(N, H, W, Cout_pad, stride) = slices * 32 ceil(Cout_pad / 32) * 33 floats; 0
 *   for a shape the entry point refuses. */
size_t tsod_conv3x3_wgrad_workspace_bytes(int32_t N, int32_t H, int32_t W, int32_t Cout_pad, int32_t stride);
int tsod_conv3x3_wgrad_f32(const float *x4, int32_t N, int32_t H, int32_t W, const float *y, const float *dy, int32_t dy_pitch,
                           int32_t dy_off, const float *w, const float *scale, int32_t Cout_pad, int32_t Cout_real,
                           int32_t stride, float *dw, float *dscale, float *dshift, void *workspace, size_t workspace_bytes,
                           tsod_stream_t stream);

/* ---- train-mode BatchNorm ------------------------------------------------------------------------
 * NHWC f32 rows [M][ld]; every tensor's channels are [off, off + C_pad) of its rows, C_pad a multiple of 4, C_real <= C_pad
 * real channels; pad channels of every output are written as exact zeros and never reach a real channel.  16-byte aligned
 * pointers, pitches and offsets multiples of 4 (TSOD_ERR_ALIGNMENT); NULL required pointers, M < 2 (torch refuses one value
 * per channel in training mode, so do these), C_real outside 1..C_pad or a slice beyond its pitch: TSOD_ERR_INVALID_ARG.  Sums
 * are kept in f64; a workgroup reduces TSOD_BN_ROWS_PER_WORKGROUP rows, its partials go to the workspace and a second stage
 * adds them in an order the shape alone fixes: no float atomics, bit-identical from run to run.
 * workspace (both entry points that take one): tsod_bn_train_workspace_bytes(M, C_pad); 0 for a shape they refuse.
 * tsod_bn_stats_f32: mean [C_pad], invstd [C_pad] = 1 / sqrt(var + eps) with the biased variance var (centred squares per
 *   workgroup, Chan's merge across them - never E[x^2] - E[x]^2), scale = gamma * invstd, shift = beta - mean * scale; gamma,
 *   beta [C_real].  scale and shift are [2][C_pad] floats: row 0 the f32 value (the folded epilogue's), row 1 the f32
 *   remainder of the f64 value - where |mean| invstd >> 1 the terms of scale * z + shift cancel and one f32 each would show
 *   in y.  running_mean / running_var [C_real] (each may be NULL) are updated in place: (1 - momentum) * old + momentum *
 *   (mean | var * M / (M - 1)); num_batches_tracked (one int64, may be NULL) is incremented.
 * tsod_bn_apply_f32: y = act(scale * z + shift), act TSOD_ACT_NONE or TSOD_ACT_RELU6 (else TSOD_ERR_UNSUPPORTED); scale,
 *   shift [2][C_pad] as above (value + remainder, added in f64, the result rounded once); amax_out: the range words of y's
 *   tensor (NULL: none), see "Range words".  M >= 1.
 * tsod_bn_train_grad_f32: g = the gradient of the BatchNorm's output (a ReLU6 mask already applied), z the saved input, mean /
 *   invstd [C_pad] what tsod_bn_stats_f32 gave, gamma [C_real], xhat = (z - mean) * invstd: dgamma [C_pad] = sum g xhat, dbeta
 *   [C_pad] = sum g, dz = gamma * invstd * (g - dbeta / M - xhat * dgamma / M).  Three launches: the workgroups' partial sums,
 *   their sum, the elementwise pass. */
#define TSOD_BN_ROWS_PER_WORKGROUP 128
size_t tsod_bn_train_workspace_bytes(int64_t M, int32_t C_pad);
int tsod_bn_stats_f32(const float *z, int64_t M, int32_t C_real, int32_t C_pad, int32_t ld, int32_t off, const float *gamma,
                      const float *beta, double eps, double momentum, float *running_mean, float *running_var,
                      int64_t *num_batches_tracked, float *mean, float *invstd, float *scale, float *shift, void *workspace,
                      size_t workspace_bytes, tsod_stream_t stream);
int tsod_bn_apply_f32(const float *z, int64_t M, int32_t C_real, int32_t C_pad, int32_t z_ld, int32_t z_off, const float *scale,
                      const float *shift, int32_t act, float *y, int32_t y_ld, int32_t y_off, uint32_t *amax_out,
                      tsod_stream_t stream);
int tsod_bn_train_grad_f32(const float *g, int32_t g_ld, int32_t g_off, const float *z, int32_t z_ld, int32_t z_off, int64_t M,
                           int32_t C_real, int32_t C_pad, const float *mean, const float *invstd, const float *gamma, float *dz,
                           int32_t dz_ld, int32_t dz_off, float *dgamma, float *dbeta, void *workspace, size_t workspace_bytes,
                           tsod_stream_t stream);

/* ---- what ResNet puts behind a train-mode BatchNorm -------------------------------------------------
 * The conventions, the grid, the summation rules and the error codes of the section above; every tensor has its own pitch and
 * offset.  PReLU with ONE slope by value; neither entry point checks it (the caller keeps it finite and > 0, so that the saved
 * output has the pre-activation's sign).
 * tsod_bn_apply_prelu_f32: y = prelu(scale * z + shift + R, slope).  scale, shift [2][C_pad]: tsod_bn_stats_f32's value +
 *   remainder pairs.  R is nothing (r == z2 == NULL), the residual tensor r [M][r_ld] (channels [r_off, r_off + C_pad)), or the
 *   second normalised operand scale2 * z2 + shift2 (z2 [M][z2_ld], channels [z2_off, z2_off + C_pad); scale2, shift2 [2][C_pad]
 *   pairs, both required with z2); r and z2 together: TSOD_ERR_INVALID_ARG.  (scale * z + shift) + R is added in f64 and
 *   rounded to f32 once, then o > 0 ? o : slope * o in f32.  amax_out: the range words of y's tensor (NULL: none).  M >= 1.
 * tsod_bn_prelu_train_grad_f32: tsod_prelu_grad_f32 and tsod_bn_train_grad_f32 in three launches (partials, their sum, the
 *   elementwise pass).  y the saved output of the PReLU, dy its gradient, z / mean / invstd / gamma as in
 *   tsod_bn_train_grad_f32.  g = y > 0 ? dy : slope * dy in f32 (an exact y == 0 takes the slope branch); dgamma, dbeta, dz:
 *   tsod_bn_train_grad_f32's on that g.  *dslope_num (NULL: none) = sum dy * y * [y < 0] in f64 (an exact 0 adds nothing): per
 *   real channel by the rule of the other two sums, then over the channels ascending - 64 contiguous runs of ceil(C_pad / 64)
 *   channels, each ascending, merged ascending - and rounded to f32 once.  g_out (NULL: none; channels [g_off, g_off + C_pad) of
 *   rows of g_ld floats): g written out, pad channels exact zeros.  M >= 2.
 *   workspace: tsod_bn_prelu_train_grad_workspace_bytes(M, C_pad) = three partials per workgroup and channel plus the totals;
 *   0 for a shape that is refused. */
int tsod_bn_apply_prelu_f32(const float *z, int64_t M, int32_t C_real, int32_t C_pad, int32_t z_ld, int32_t z_off,
                            const float *scale, const float *shift, const float *r, int32_t r_ld, int32_t r_off, const float *z2,
                            int32_t z2_ld, int32_t z2_off, const float *scale2, const float *shift2, float slope, float *y,
                            int32_t y_ld, int32_t y_off, uint32_t *amax_out, tsod_stream_t stream);
size_t tsod_bn_prelu_train_grad_workspace_bytes(int64_t M, int32_t C_pad);
int tsod_bn_prelu_train_grad_f32(const float *y, int32_t y_ld, int32_t y_off, const float *dy, int32_t dy_ld, int32_t dy_off,
                                 const float *z, int32_t z_ld, int32_t z_off, int64_t M, int32_t C_real, int32_t C_pad,
                                 const float *mean, const float *invstd, const float *gamma, float slope, float *dz,
                                 int32_t dz_ld, int32_t dz_off, float *dgamma, float *dbeta, float *dslope_num, float *g_out,
                                 int32_t g_ld, int32_t g_off, void *workspace, size_t workspace_bytes, tsod_stream_t stream);

/* ---- active dropout: nn.Dropout(p) under .train() on channel slices of an NHWC buffer ----------------
 * models/hardnet.py:182-183 (HarDNet-85: between the last HarDBlock and its transition ConvLayer).  The mask is the project's own
 * definition (torch's stream depends on its launch shape): a logical tensor [N][H][W][C], C the REAL channels of the slices in
 * the order of their `first` fields.
 *     e    = e0 + ((n H + h) W + w) C + c                         (uint64)
 *     word = lane (e & 3) of Philox4x32-10(counter (lo32(e >> 2), hi32(e >> 2), ordinal, 0), key (key[0], key[1]))
 *     thr  = (uint64) llround((double)p * 4294967296.0)           keep iff (uint64) word >= thr
 *     y    = keep ? x * scale : 0                                 scale = p < 1 ? (float)(1.0 / (1.0 - (double)p)) : 0.f
 * (one f32 multiply; a dropped NaN is 0).  The mask depends on nothing else: not on pitches, channel padding, where the slices
 * lie in the pixel, the grid or any chunking.  The backward is the same call on the gradient with the same key.
 * tsod_dropout_segs_f32: slice s = channels [off, off + real) of every pixel of src [N][H][W][src_pitch] and dst
 *   [N][H][W][dst_pitch], logical channels [first, first + real); `segs` is a HOST array of n_segs <=
 *   TSOD_DROPOUT_MAX_SEGMENTS records that travels by value with the launch, `key` a DEVICE pointer to two uint32 words read by
 *   the kernel (tsod_dropout_key_set writes them by a kernel of its own: stream-ordered, no copy).  dst == src is allowed
 *   (otherwise the two must not overlap).  Lanes [real, real rounded up to 4) of a slice are written as 0 in dst and never read
 *   from src; channels outside the slices are not touched.  16-byte accesses; a short last quad is loaded lane by lane.
 *   TSOD_ERR_INVALID_ARG: a NULL pointer, a non-positive size, p outside [0, 1] or NaN, a slice that does not fit a pitch with its
 *   pad lanes, logical channels beyond C, two slices that share a logical channel or a lane.  TSOD_ERR_ALIGNMENT: a pitch or
 *   an offset that is no multiple of 4, src / dst not 16-byte or key not 4-byte aligned.  TSOD_ERR_UNSUPPORTED: n_segs >
 *   TSOD_DROPOUT_MAX_SEGMENTS.
 * tsod_dropout_params / tsod_philox4x32_host: HOST functions - (thr, scale) of p as above (TSOD_ERR_INVALID_ARG as above), and
 *   the generator itself, ctr [4], key [2] -> out [4] (csrc/philox.h, the function the kernel calls). */
#define TSOD_DROPOUT_MAX_SEGMENTS 16
typedef struct tsod_dropout_seg {
    int32_t off;   /* first channel of the slice in the pixel; multiple of 4 */
    int32_t real;  /* real width, >= 1 */
    int32_t first; /* first logical channel */
} tsod_dropout_seg;
int tsod_dropout_segs_f32(const float *src, float *dst, int32_t N, int32_t H, int32_t W, int32_t src_pitch, int32_t dst_pitch,
                          const tsod_dropout_seg *segs, int32_t n_segs, int32_t C, float p, const uint32_t *key, uint32_t ordinal,
                          uint64_t e0, tsod_stream_t stream);
int tsod_dropout_key_set(uint32_t *key, uint32_t lo, uint32_t hi, tsod_stream_t stream);
int tsod_dropout_params(float p, uint64_t *thr, float *scale);
void tsod_philox4x32_host(const uint32_t *ctr, const uint32_t *key, uint32_t *out);

/* ---- detection mAP: COCOeval's evaluateImg + accumulate, area range "all", no crowd / ignore flags ------
 * The reference's calculate_metrics (nets/frcnn_training.py:372-565) defines no usable metric; this is the project's own.
 * IoU is tsod_bbox_iou_f32's expression (eps 1e-8, no +1), compared as IoU >= t in f32.  Three steps:
 *
 * tsod_eval_match_f32: one update.  det [B][R][6] = (x1,y1,x2,y2,score,class) rows; image b's candidates are rows j < counts[b]
 *   (keep == n_kept == NULL) or rows keep[b][j], j < n_kept[b] (tsod_detection_nms_f32's triple; counts == NULL).  Rows with a
 *   NaN score, a class outside [0, num_classes) or of ignore_class (< 0: none) are dropped.  Per image and class: descending
 *   score, ties to the lower j, the first max_dets kept; walking them in that order, each detection takes, for every threshold
 *   t of iou_thr [T] (device, f32) on its own, the not yet matched ground truth of its class with the largest IoU >= t (equal
 *   IoUs: the higher index).  gt_boxes [B][G][4] (16-byte aligned), gt_labels [B][G] int64, gt_counts [B]; G may be 0 (the
 *   three may then be NULL); labels outside [0, num_classes) or equal to ignore_class are not counted.
 *   Appends one tsod_eval_record per surviving detection to records [capacity] at *n_records (device int64, the running
 *   total, advanced by the call), ordered by image, then class, then the order above; adds each image's counted ground truth
 *   to npig [num_classes] (device int64, integer atomics).  Records past capacity are dropped: the caller keeps
 *   capacity >= *n_records + B * R.  workspace: tsod_eval_match_workspace_bytes(B, R).  Limits (TSOD_ERR_UNSUPPORTED beyond):
 *   B <= 65535, R <= 8192, G <= 1024, T <= 32, num_classes <= 262144.
 * tsod_sort_pairs_u64: stable ascending LSD radix sort of keys_in [n] on bits [begin_bit, end_bit) with an int32 payload
 *   (vals_in, or the identity 0..n-1 when NULL) -> keys_out, vals_out (neither may alias an input).  n_dev (device int64, may be
 *   NULL) makes the live count min(*n_dev, n) without a host read.  8-bit passes of histogram, per-digit scan and scatter;
 *   ranks inside a tile come from wave ballots in index order.  n <= 2^31 - 4097.  workspace:
 *   tsod_sort_pairs_workspace_bytes(n).
 * tsod_eval_accumulate_f64: every record so far (records [capacity], live count *n_records) sorted by (class, descending
 *   score) with ties in record order, then per (class c, threshold t): integer cumulative TP / FP, precision tp / (tp + fp)
 *   in f64 made monotone from the right, sampled for k = 0..100 at the first position where 100 tp >= k npig[c] (0 where
 *   there is none), AP[c][t] = the mean of the 101 samples.  Outputs [num_classes][T]: ap (f64, -1 when npig[c] == 0),
 *   tp / fp / fn = npig - tp (int64), recall = tp / npig (f64, -1 when npig[c] == 0).  No float atomics, fixed-order sums:
 *   run to run bit-identical.  workspace: tsod_eval_accumulate_workspace_bytes(capacity, num_classes). */
typedef struct tsod_eval_record {
    float score;
    int32_t cls;
    uint32_t tp_mask; /* bit t: a true positive at iou_thr[t] */
} tsod_eval_record;
size_t tsod_eval_match_workspace_bytes(int32_t B, int32_t R);
int tsod_eval_match_f32(const float *det, int32_t B, int32_t R, const int32_t *counts, const int32_t *keep, const int32_t *n_kept,
                        const float *gt_boxes, const int64_t *gt_labels, const int32_t *gt_counts, int32_t G,
                        const float *iou_thr, int32_t T, int32_t num_classes, int32_t max_dets, int32_t ignore_class,
                        tsod_eval_record *records, int64_t capacity, int64_t *n_records, int64_t *npig, void *workspace,
                        size_t workspace_bytes, tsod_stream_t stream);
size_t tsod_sort_pairs_workspace_bytes(int64_t n);
int tsod_sort_pairs_u64(const uint64_t *keys_in, const int32_t *vals_in, int64_t n, const int64_t *n_dev, int32_t begin_bit,
                        int32_t end_bit, uint64_t *keys_out, int32_t *vals_out, void *workspace, size_t workspace_bytes,
                        tsod_stream_t stream);
size_t tsod_eval_accumulate_workspace_bytes(int64_t capacity, int32_t num_classes);
int tsod_eval_accumulate_f64(const tsod_eval_record *records, int64_t capacity, const int64_t *n_records, const int64_t *npig,
                             int32_t num_classes, int32_t T, double *ap, int64_t *tp, int64_t *fp, int64_t *fn, double *recall,
                             void *workspace, size_t workspace_bytes, tsod_stream_t stream);

/* ---- COCO detection evaluation: the section-4.14 metric with COCOeval's area ranges, crowd regions,
 * ignore rules and detection caps, in one pass.  tsod_eval_match_f32 / tsod_eval_accumulate_f64 above are unchanged.
 *
 * tsod_eval_match_coco_f32: one update.  det, counts / keep / n_kept, gt_boxes, gt_labels, gt_counts, iou_thr [T],
 *   num_classes, ignore_class, the drop rules, the per-(image, class) order and the limits are tsod_eval_match_f32's.
 *   gt_crowd [B][G] uint8 (NULL: none is crowd), gt_area [B][G] f32 (NULL: the box's own area), area_lo / area_hi [A]
 *   (device, f32, 1 <= A <= 4), max_dets = the largest cap.  A box's area is (x2-x1)*(y2-y1) as an f32 product.  For every
 *   range a on its own, COCOeval's evaluateImg: a ground truth is ignored when it is crowd or area < lo[a] || area > hi[a]
 *   (f32, both bounds inclusive); the class's ground truth is walked not-ignored first, then ignored, each ascending; the
 *   first max_dets detections of the (image, class) are walked in order, every threshold t on its own: a ground truth
 *   already matched at t is skipped unless it is crowd; the walk stops where it reaches the ignored part holding a
 *   not-ignored best; a candidate needs IoU >= max(t, best so far), equal IoUs go to the later position.  IoU against a crowd
 *   ground truth is inter / (area_det + 1e-8), otherwise tsod_bbox_iou_f32's expression.  A detection matched to an ignored
 *   ground truth is ignored (neither TP nor FP), and so is an unmatched detection whose own area lies outside the range.
 *   Appends one tsod_eval_record_coco per surviving detection exactly as tsod_eval_match_f32 appends its records, and adds
 *   the not-ignored ground truth to npig [num_classes][A] (device int64, integer atomics).
 *   workspace: tsod_eval_match_coco_workspace_bytes(B, R) (0 for a refused B or R).  Dynamic LDS at the limits G = 1024,
 *   R = 8192: 143360 bytes.
 * tsod_eval_accumulate_coco_f64: every record so far, sorted as tsod_eval_accumulate_f64 sorts.  max_dets_list [M] (HOST,
 *   ascending from >= 1, 1 <= M <= 4, last entry <= max_dets, the value the match ran with; TSOD_ERR_INVALID_ARG otherwise).
 *   Matching is greedy in score order, so the result under cap m is the records with rank < max_dets_list[m].  Per (class c,
 *   range a, cap m, threshold t): ignored records add to neither count, integer cumulative TP / FP, precision tp / (tp + fp)
 *   in f64 made monotone from the right, sampled by the rule 100 tp >= k npig[c][a], k = 0..100.  Outputs
 *   [num_classes][A][M][T]: ap and recall = tp / npig (f64, -1 when npig[c][a] == 0), tp / fp / fn (int64).  Fixed-order sums:
 *   run to run bit-identical.  workspace: tsod_eval_accumulate_coco_workspace_bytes(capacity, num_classes). */
typedef struct tsod_eval_record_coco {
    float score;
    int32_t cls;
    int32_t rank;        /* 0-based place in the (image, class) order */
    uint32_t tp_mask[4]; /* [a] bit t: matched to a not-ignored ground truth of range a at iou_thr[t] */
    uint32_t ig_mask[4]; /* [a] bit t: ignored in range a at iou_thr[t] */
} tsod_eval_record_coco;
size_t tsod_eval_match_coco_workspace_bytes(int32_t B, int32_t R);
int tsod_eval_match_coco_f32(const float *det, int32_t B, int32_t R, const int32_t *counts, const int32_t *keep,
                             const int32_t *n_kept, const float *gt_boxes, const int64_t *gt_labels, const int32_t *gt_counts,
                             const uint8_t *gt_crowd, const float *gt_area, int32_t G, const float *iou_thr, int32_t T,
                             const float *area_lo, const float *area_hi, int32_t A, int32_t num_classes, int32_t max_dets,
                             int32_t ignore_class, tsod_eval_record_coco *records, int64_t capacity, int64_t *n_records,
                             int64_t *npig, void *workspace, size_t workspace_bytes, tsod_stream_t stream);
size_t tsod_eval_accumulate_coco_workspace_bytes(int64_t capacity, int32_t num_classes);
int tsod_eval_accumulate_coco_f64(const tsod_eval_record_coco *records, int64_t capacity, const int64_t *n_records,
                                  const int64_t *npig, int32_t num_classes, int32_t A, int32_t T, const int32_t *max_dets_list,
                                  int32_t M, int32_t max_dets, double *ap, int64_t *tp, int64_t *fp, int64_t *fn, double *recall,
                                  void *workspace, size_t workspace_bytes, tsod_stream_t stream);

/* ---- input step (the step before the path) ----------------------------------------------
 * dataset/dataloader.py:35-44 + dataset/transform.py:14-17: a decoded RGB image becomes an f32 CHW tensor with
 * values 0..255 and is resized to the detector's fixed size by torchvision v2 Resize, i.e. ATen's antialiased
 * bilinear interpolation (align_corners = false).  Here: u8 HWC in device memory -> f32, resized, already in the
 * layout the backbone reads (NHWC with a zero 4th channel, or NCHW).
 *   tsod_resize_aa_taps(in, out)      taps per output index of one axis (row length of the weight table)
 *   tsod_resize_aa_tables_f32         HOST function: first[out], count[out], weights[out][taps] of one axis in
 *                                     ATen's f32 arithmetic (triangle filter widened by the down-scale factor,
 *                                     normalised per output index); copy the tables to the device once per size pair
 *   tsod_resize_bilinear_aa_u8_f32    out[oy*stride_y + ox*stride_x + c*stride_c] =
 *                                       mul * sum_j wy[oy][j] * (sum_i wx[ox][i] * src[y0+j][x0+i][c]),  c < C;
 *                                     channels C..C_out-1 are written as 0.  Strides in floats:
 *                                     NHWC4 = (4*OW, 4, 1) with C_out = 4;  NCHW plane = (OW, 1, OH*OW) with C_out = C.
 *                                     mul = 1 reproduces the reference (values stay 0..255), 1/255 gives [0,1]. */
int32_t tsod_resize_aa_taps(int32_t in_size, int32_t out_size);
int tsod_resize_aa_tables_f32(int32_t in_size, int32_t out_size, int32_t *first, int32_t *count, float *weights);
int tsod_resize_bilinear_aa_u8_f32(const uint8_t *src, int32_t H, int32_t W, int32_t C, int64_t src_row_bytes,
                                   const int32_t *yfirst, const int32_t *ycount, const float *ywt,
                                   const int32_t *xfirst, const int32_t *xcount, const float *xwt, int32_t OH,
                                   int32_t OW, float mul, float *out, int64_t stride_y, int64_t stride_x,
                                   int64_t stride_c, int32_t C_out, tsod_stream_t stream);

/* ---- training augmentation: the reference's `transform` (dataset/transform.py:4-12) -----------------
 * RandomPhotometricDistort -> RandomHorizontalFlip -> ScaleJitter -> Resize -> SanitizeBoundingBoxes on an RGB u8 HWC
 * image (values 0..255) and its XYXY boxes.  The parameters are drawn on the host; these calls apply them.
 * tsod_photometric holds one image's colour draws: the ops whose bit is set in `flags` run in torchvision's order
 * (brightness, contrast if CONTRAST_FIRST, saturation, hue, contrast otherwise, channel permutation).  When any of the
 * four colour ops is set, the pixel is divided by `white` first, the colour ops clamp into [0, 1], and the result is
 * multiplied by `white`; white = 1 is the reference (its 0..255 image clamped into [0, 1]), 255 the evident intent.
 *   tsod_augment_gray_mean_partials  TSOD_AUGMENT_MEAN_PARTS fixed-order partial sums (f64, device) of the grayscale
 *                                    value of the image as contrast sees it; needed only when CONTRAST is set
 *   tsod_augment_resize_u8_f32       colour ops + channel permutation + (flip ? mirrored columns : identity) + one
 *                                    antialiased resize (the tables of tsod_resize_aa_tables_f32, same tap arithmetic as
 *                                    tsod_resize_bilinear_aa_u8_f32 with mul = 1) into out[oy*stride_y + ox*stride_x +
 *                                    c*stride_c], c < 3, channels 3..C_out-1 zero.  mean_partials: the output of
 *                                    tsod_augment_gray_mean_partials for the same image and params (NULL without CONTRAST)
 *   tsod_resize_bilinear_aa_f32      the same resize from an f32 image src[y*src_stride_y + x*src_stride_x +
 *                                    c*src_stride_c], c < C <= 4 (the augmentation's second resize)
 *   tsod_augment_boxes_f32           B images in one launch (one workgroup each).  Image b owns boxes [first, first +
 *                                    count) of `boxes` [N,4] / `labels` [N]: iparams[b] = {first, count, flip, 0},
 *                                    fparams[b] = {W, sx1, sy1, sx2, sy2, OW, OH, min_size}.  Per box: flip
 *                                    (x1, x2) -> (W - x2, W - x1), x *= sx1, y *= sy1, x *= sx2, y *= sy2, then kept iff
 *                                    x2 - x1 >= min_size, y2 - y1 >= min_size, every coordinate >= 0, x1, x2 <= OW,
 *                                    y1, y2 <= OH.  Kept boxes and labels are written in order from index `first` of the
 *                                    outputs; kept[b] = their count.
 *   tsod_augment_color_host          HOST function: the colour ops and permutation of tsod_photometric on n
 *                                    interleaved f32 RGB pixels, given contrast's mean (the arithmetic the kernels run) */
#define TSOD_AUGMENT_MEAN_PARTS 256
enum {
    TSOD_AUG_BRIGHTNESS = 1,
    TSOD_AUG_CONTRAST = 2,
    TSOD_AUG_SATURATION = 4,
    TSOD_AUG_HUE = 8,
    TSOD_AUG_CONTRAST_FIRST = 16,
    TSOD_AUG_PERMUTE = 32
};
typedef struct tsod_photometric {
    int32_t flags;
    float brightness, contrast, saturation, hue; /* factors of the ops that are set */
    float white;                                  /* > 0 */
    int32_t perm[3];                              /* out[c] = in[perm[c]] when PERMUTE is set; a permutation of 0,1,2 */
} tsod_photometric;
int tsod_augment_gray_mean_partials(const uint8_t *src, int32_t H, int32_t W, int64_t src_row_bytes,
                                    const tsod_photometric *params, double *partials, tsod_stream_t stream);
int tsod_augment_resize_u8_f32(const uint8_t *src, int32_t H, int32_t W, int64_t src_row_bytes,
                               const tsod_photometric *params, const double *mean_partials, int32_t flip,
                               const int32_t *yfirst, const int32_t *ycount, const float *ywt, const int32_t *xfirst,
                               const int32_t *xcount, const float *xwt, int32_t OH, int32_t OW, float *out,
                               int64_t stride_y, int64_t stride_x, int64_t stride_c, int32_t C_out, tsod_stream_t stream);
int tsod_resize_bilinear_aa_f32(const float *src, int32_t H, int32_t W, int32_t C, int64_t src_stride_y,
                                int64_t src_stride_x, int64_t src_stride_c, const int32_t *yfirst, const int32_t *ycount,
                                const float *ywt, const int32_t *xfirst, const int32_t *xcount, const float *xwt,
                                int32_t OH, int32_t OW, float *out, int64_t stride_y, int64_t stride_x, int64_t stride_c,
                                int32_t C_out, tsod_stream_t stream);
int tsod_augment_boxes_f32(const float *boxes, const int64_t *labels, int32_t B, const int32_t *iparams,
                           const float *fparams, float *boxes_out, int64_t *labels_out, int32_t *kept,
                           tsod_stream_t stream);
int tsod_augment_color_host(const float *rgb, int64_t n, const tsod_photometric *params, float mean, float *rgb_out);

/* ---- optimizer: one AdamW update of any number of f32 tensors in ONE launch ---------------------------
 * Replaces torch.optim.AdamW(...).step() [+ zero_grad] of the reference's train/train.py (amsgrad=False, maximize=False,
 * decoupled weight decay).  Per element, every operation rounded to f32 on its own (the library is built with
 * -ffp-contract=off), in the order of torch's single-tensor AdamW:
 *     p = p * decay                                                   decay = 1 - lr * weight_decay
 *     m = w < 0.5 ? m + (g - m) * w : g - (g - m) * (1 - w)           w = 1 - beta1          (torch's lerp_)
 *     v = v * beta2 + ((1 - beta2) * g) * g                           (mul_, then addcmul_)
 *     p = p + ((-step_size) * m) / (sqrt(v) / bias2_sqrt + eps)       (addcdiv_; IEEE divide and sqrt)
 *     g = 0 when zero_grad is set
 * tsod_adamw_group holds the scalars of one step for tensors that share hyper-parameters and step count t; the caller
 * prepares them in double precision and rounds each once to f32.
 *   tsod_adamw_step_f32       `table` and `chunks` are DEVICE memory.  table[i] describes tensor i; `group` indexes
 *                             `groups`, a HOST array of n_groups <= TSOD_ADAMW_MAX_GROUPS records that travels by value
 *                             with the launch (nothing on the host is read after the call returns).  chunks[c] =
 *                             {tensor, piece}: workgroup c updates elements [piece * TSOD_ADAMW_CHUNK, + TSOD_ADAMW_CHUNK)
 *                             of that tensor, clipped to its n.  Every element of every tensor must be covered by exactly
 *                             one chunk; records that point outside the table or the groups are skipped.  16-byte accesses
 *                             where the four pointers of a chunk are 16-byte aligned, 4-byte ones otherwise.  No atomics:
 *                             the result does not depend on the schedule.  n_groups > TSOD_ADAMW_MAX_GROUPS:
 *                             TSOD_ERR_UNSUPPORTED.
 *   tsod_adamw_step_host_f32  HOST function: the same update over n elements of host arrays (the arithmetic the kernel runs) */
#define TSOD_ADAMW_CHUNK 2048
#define TSOD_ADAMW_MAX_GROUPS 32
typedef struct tsod_adamw_tensor {
    float *param, *grad, *exp_avg, *exp_avg_sq;
    int64_t n;     /* elements */
    int32_t group; /* index into groups */
    int32_t reserved;
} tsod_adamw_tensor;
typedef struct tsod_adamw_chunk {
    int32_t tensor, piece;
} tsod_adamw_chunk;
typedef struct tsod_adamw_group {
    float decay;           /* 1 - lr * weight_decay */
    float one_minus_beta1; /* lerp weight w */
    float beta2, one_minus_beta2;
    float step_size;       /* lr / (1 - beta1^t) */
    float bias2_sqrt;      /* sqrt(1 - beta2^t) */
    float eps;
    float reserved;
} tsod_adamw_group;
int tsod_adamw_step_f32(const tsod_adamw_tensor *table, int32_t n_tensors, const tsod_adamw_chunk *chunks, int64_t n_chunks,
                        const tsod_adamw_group *groups, int32_t n_groups, int32_t zero_grad, tsod_stream_t stream);
int tsod_adamw_step_host_f32(float *param, float *grad, float *exp_avg, float *exp_avg_sq, int64_t n,
                             const tsod_adamw_group *group, int32_t zero_grad);

/* ---- gradient clipping by global norm, over the table and work list of tsod_adamw_step_f32 -------------
 * torch.nn.utils.clip_grad_norm_(parameters, max_norm) in front of the step: the 2-norm over every gradient of the table,
 * coef = min(1, max_norm / (norm + 1e-6)), g = g * coef.  The norm is two launches, the multiplication rides in the step.
 * No float atomics, no tickets: every sum order below depends on the element counts only, so the record is bit-identical
 * from run to run and equal to tsod_grad_norm_host_f32's.
 *   tsod_grad_norm_f32          launch 1, workgroup c = chunks[c] (256 threads): thread t owns quads t, t + 256, ... of its
 *                               chunk, quads counted from the chunk's first element (not from an aligned address), and adds
 *                               (double)g * (double)g - exact in f64 - over the elements of each quad in ascending order, a
 *                               last short quad included; the 256 sums go through a binary tree (t += t + 128, then + 64,
 *                               ... + 1) into one f64 partial per chunk, workspace[c].  16-byte loads where the chunk's
 *                               gradient pointer is 16-byte aligned, 4-byte loads otherwise: the same order, the same bits.
 *                               Launch 2, one workgroup: thread t adds partials t, t + 256, ... ascending, the same tree,
 *                               and thread 0 stores
 *                                   sum_sq
 *                                   norm = (float)sqrt(sum_sq)
 *                                   c    = max_norm / (norm + 1e-6f)          f32, one IEEE divide
 *                                   coef = c > 1 ? 1 : c
 *                               so a NaN norm gives a NaN coefficient and an infinite norm gives 0, as torch's
 *                               clamp(max=1) does.  Records that point outside the table are skipped (their partial is 0);
 *                               n_tensors == 0 or n_chunks == 0 stores {0, 0, 1}.  `result` and `workspace` are DEVICE
 *                               memory, 8-byte aligned (TSOD_ERR_ALIGNMENT); workspace_bytes >=
 *                               tsod_grad_norm_workspace_bytes(n_chunks) (8 per chunk), max_norm >= 0 and not a NaN,
 *                               non-NULL pointers, 0 <= n_chunks <= INT32_MAX (TSOD_ERR_INVALID_ARG otherwise).  Only
 *                               `grad` and `n` of a table record are read.
 *   tsod_adamw_step_clipped_f32 tsod_adamw_step_f32 with g' = g * clip->coef (one f32 multiply, the coefficient read from
 *                               DEVICE memory by the kernel) in front of the update; the gradient becomes 0 with zero_grad,
 *                               g' otherwise (as after torch's clip).  clip == NULL is tsod_adamw_step_f32 itself.
 *   tsod_grad_scale_f32         g = g * clip->coef over the same work list (only `grad` and `n` are read)
 *   tsod_grad_norm_host_f32     HOST function: the whole norm over n_tensors host arrays - the work list of tensor-by-tensor
 *                               chunks of TSOD_ADAMW_CHUNK elements (no chunk for an empty tensor), the thread-strided
 *                               order, both trees and the coefficient, in the same arithmetic: equal bits */
typedef struct tsod_grad_norm_result {
    double sum_sq; /* the f64 sum of squares */
    float norm;    /* before clipping */
    float coef;    /* what the gradients are multiplied by */
} tsod_grad_norm_result;
size_t tsod_grad_norm_workspace_bytes(int64_t n_chunks);
int tsod_grad_norm_f32(const tsod_adamw_tensor *table, int32_t n_tensors, const tsod_adamw_chunk *chunks, int64_t n_chunks,
                       float max_norm, tsod_grad_norm_result *result, void *workspace, size_t workspace_bytes,
                       tsod_stream_t stream);
int tsod_adamw_step_clipped_f32(const tsod_adamw_tensor *table, int32_t n_tensors, const tsod_adamw_chunk *chunks,
                                int64_t n_chunks, const tsod_adamw_group *groups, int32_t n_groups, int32_t zero_grad,
                                const tsod_grad_norm_result *clip, tsod_stream_t stream);
int tsod_grad_scale_f32(const tsod_adamw_tensor *table, int32_t n_tensors, const tsod_adamw_chunk *chunks, int64_t n_chunks,
                        const tsod_grad_norm_result *clip, tsod_stream_t stream);
int tsod_grad_norm_host_f32(const float *const *grads, const int64_t *numels, int32_t n_tensors, float max_norm,
                            tsod_grad_norm_result *result);

/* ---- detection overlay: the last step of the reference's multi_inference.py:104-154 on the GPU -------------
 * tsod_draw_groups_u8 paints up to TSOD_DRAW_MAX_GROUPS groups of boxes, with text tags, in place onto B u8 RGB images
 * [B][H][W][3] (row_bytes >= 3 W between rows, image_bytes >= H row_bytes between images) in ONE launch.  Integer arithmetic
 * only, no atomics: the result depends on the arguments alone.  Bytes of a row beyond 3 W and pixels that no item covers
 * are neither read nor written.
 *
 * A group (tsod_draw_group) is one style over one box array `boxes` f32 [B][R][pitch], columns 0..3 = x1 y1 x2 y2; pitch 4,
 * or 6 for detection records (x1 y1 x2 y2 score class).
 *   Rows drawn, in this order (the conventions of DetectionEvaluator.update): keep == NULL and counts == NULL: rows 0..R-1;
 *     counts i32 [B]: rows 0..counts[b]-1; keep i32 [B][R] with n_kept i32 [B]: rows keep[b][0 .. n_kept[b]).  A count
 *     outside [0, R] is clamped into it; a keep entry outside [0, R) draws nothing.
 *   Label index of a row: labels i64 [B][R] when given; else with pitch 6 column 5 converted to int32 (truncated towards
 *     zero, saturating, NaN -> 0); else (pitch 4) the row has no label and gets no tag.  label_offset is added (in 64 bits).
 *   Box to pixels: X1 = rintf(clamp(sx * x1)), Y1 = rintf(clamp(sy * y1)), X2 = rintf(clamp(sx * x2)), Y2 = rintf(clamp(sy *
 *     y2)), each product ONE f32 multiply, clamp to [-2^24, 2^24], bounds inclusive.  A row with a non-finite coordinate, a
 *     NaN product, X2 < X1 or Y2 < Y1 draws nothing: no outline and no tag.
 *   Outline: the pixels (x, y) of [X1, X2] x [Y1, Y2] with x - X1 < t, X2 - x < t, y - Y1 < t or Y2 - y < t (t = thickness;
 *     it grows inwards, a box thinner than 2 t is filled), blended with color[0..2] at alpha color[3].
 *   Blend, per channel: out = (a c + (255 - a) src + 127) / 255 in integers (a = 255 stores c); a = 0 leaves the pixel alone.
 *   Tag (tag != TSOD_DRAW_TAG_NONE and the row has a label): the group reads rows [string_first, string_first +
 *     string_count) of the table `strings` (u8 [n_strings][32], zero-terminated, at most 31 bytes are read; DEVICE memory,
 *     4-byte aligned; one group: string_first = 0, string_count = n_strings).  Line 1 is strings[string_first + index] when
 *     0 <= index < string_count, else "class_" followed by the decimal index ('-' first when negative) - with string_count
 *     == 0 every label takes that route.  With score_line (pitch 6) line 2 is "Conf: d.ddd" of the score s = column
 *     4: m = (int)rintf(fminf(fmaxf(s, 0), 1) * 1000), printed as m / 1000, '.', three digits of m % 1000; a NaN score
 *     prints "Conf: -.---".  Glyphs are 5x7 in a 6x8 cell (the glyph in the cell's upper left), every glyph pixel
 *     font_scale x font_scale image pixels.  With cols = the longer line's length and lines = 1 or 2, the tag is the
 *     rectangle of w = cols 6 font_scale + 2 padding by h = lines 8 font_scale + 2 padding pixels whose left edge is X1 and
 *       TSOD_DRAW_TAG_ABOVE: whose bottom row is Y1 - 1 (top = Y1 - h); when top < 0, top = Y1;
 *       TSOD_DRAW_TAG_BELOW: whose top row is Y2 + 1; when top + h > H, its bottom row is Y2 (top = Y2 - h + 1);
 *     then, when left > 0 and left + w > W, left = max(W - w, 0); what still lies outside the image is clipped.  The
 *     rectangle is blended with tag_bg[0..2] at alpha tag_bg[3]; then the set pixels of character k of line l - cell origin
 *     (left + padding + 6 k font_scale, top + padding + 8 l font_scale) - are stored opaque with text_rgb.
 *   Order: first every outline - groups ascending, rows in drawn order -, then every tag in the same order; a later item
 *     paints over an earlier one.
 * The kernel: one workgroup per 64x16 tile of one image collects the items that meet its tile into a list of
 * TSOD_DRAW_LIST_CAPACITY entries in LDS and every thread walks that list for its pixels; a tile met by more items paints
 * the list and refills it, in item order, before its single store per pixel.
 * TSOD_ERR_INVALID_ARG: images NULL; B, H or W <= 0; row_bytes < 3 W; image_bytes < H row_bytes; n_groups outside
 *   [0, TSOD_DRAW_MAX_GROUPS] (or groups NULL with n_groups > 0); n_strings < 0 (or strings NULL with n_strings > 0); in a
 *   group: R < 0, boxes NULL with R > 0, pitch not 4 or 6, keep without n_kept or the reverse, keep and counts together,
 *   thickness < 1, font_scale < 1, padding < 0, tag outside the enum, score_line not 0 / 1, score_line with pitch 4,
 *   string_first < 0, string_count < 0 or string_first + string_count > n_strings.
 * TSOD_ERR_UNSUPPORTED: H W or B R beyond 2^31 - 1, more than 2^31 - 1 tiles, thickness, font_scale or padding above
 *   TSOD_DRAW_MAX_STYLE (the geometry is 32-bit).  TSOD_ERR_ALIGNMENT: strings not 4-byte aligned.
 * n_groups == 0 or R == 0 in every group: TSOD_OK, nothing is launched.
 * tsod_draw_font5x7: HOST function, the font of csrc/font5x7.h: out[c][r] = row r (0 = top) of the glyph of byte c, 5 low
 *   bits, bit 4 the leftmost column.  Bytes without a glyph of their own (and bytes >= 128) print a filled block, 0x1f. */
#define TSOD_DRAW_MAX_GROUPS 4
#define TSOD_DRAW_LIST_CAPACITY 64
#define TSOD_DRAW_STRING_BYTES 32
#define TSOD_DRAW_MAX_STYLE 32767
enum { TSOD_DRAW_TAG_NONE = 0, TSOD_DRAW_TAG_ABOVE = 1, TSOD_DRAW_TAG_BELOW = 2 };
typedef struct tsod_draw_group {
    const float *boxes;     /* [B][R][pitch] */
    const int32_t *counts;  /* [B] or NULL */
    const int32_t *keep;    /* [B][R] or NULL */
    const int32_t *n_kept;  /* [B], with keep */
    const int64_t *labels;  /* [B][R] or NULL */
    int32_t R, pitch, label_offset;
    int32_t string_first, string_count; /* the group's rows of `strings` */
    float sx, sy;           /* box coordinates -> image pixels */
    uint8_t color[4];       /* outline R G B, alpha */
    int32_t thickness;
    int32_t tag;            /* TSOD_DRAW_TAG_* */
    uint8_t text_rgb[4];    /* tag text R G B, [3] unused */
    uint8_t tag_bg[4];      /* tag background R G B, alpha */
    int32_t font_scale, padding, score_line;
} tsod_draw_group;
int tsod_draw_groups_u8(uint8_t *images, int32_t B, int32_t H, int32_t W, int64_t row_bytes, int64_t image_bytes,
                        const tsod_draw_group *groups, int32_t n_groups, const uint8_t *strings, int32_t n_strings,
                        tsod_stream_t stream);
int tsod_draw_font5x7(uint8_t out[128][7]);

/* ---- training curves: the loss bookkeeping of the reference's train/train.py:147-160 and the figure of its
 * utils/draw.py:plot_training_metrics on the GPU.  Four calls; none reads device memory on the host, every result depends
 * on the arguments alone (integer atomicOr on LDS and min / max are the only order-free combinations used).  The library is
 * built with -ffp-contract=off: every f32 operation named below is ONE rounding.
 *
 * K1  tsod_ema_scan_f32: rows of n samples, x f32 [rows][x_pitch], out f32 [rows][out_pitch] (pitches in elements, >= n):
 *     out[r][0] = x[r][0];  out[r][i] = fadd(fmul(a, x[r][i]), fmul(b, out[r][i-1])) - two f32 products and one f32 sum,
 *     no FMA.  With a = (float)alpha and b = (float)(1.0 - alpha) (the subtraction in double) this is the reference's
 *     update_ema loop bit for bit.  Non-finite samples propagate by IEEE rules.  One wave per row: 64 samples are loaded
 *     coalesced, every lane forms its product, the wave walks the 64 steps on wave-uniform values (lane k's product is
 *     broadcast to step k), step k's value goes to word k of an LDS row and every lane stores its own, coalesced.  x and
 *     out may be the same array.
 *     TSOD_ERR_INVALID_ARG: rows or n < 0; x or out NULL with rows n > 0; a pitch < n.  rows == 0 or n == 0: TSOD_OK, no launch.
 *
 * K2  tsod_plot_limits_f32: the axis limits of a panel.  series: HOST array of n_series DEVICE pointers (f32), lengths:
 *     HOST array of their lengths; limits: DEVICE f32 [2] = (lo, hi).  With m / M the minimum / maximum over every FINITE
 *     sample of every series:  none finite -> (0, 1);  M == m -> (m - 0.5f, m + 0.5f);  otherwise pad = 0.1f * (0.5f * M -
 *     0.5f * m) (= 0.05 (M - m), formed from the halves so that it is finite for samples near +-FLT_MAX), lo = m - pad, hi =
 *     M + pad; lo and hi are then clamped into [-FLT_MAX, FLT_MAX].  Two launches on the stream (per-workgroup partial
 *     minima / maxima, then the rule); workspace: DEVICE, TSOD_PLOT_LIMITS_WORKSPACE_BYTES, 4-byte aligned.
 *     TSOD_ERR_INVALID_ARG: limits NULL; n_series outside [0, TSOD_PLOT_MAX_SERIES]; series or lengths NULL with n_series > 0;
 *     a length < 0; a NULL series with length > 0.  TSOD_ERR_WORKSPACE: workspace NULL or too small.  No series or only
 *     empty ones: (0, 1) is still written (one launch).
 *
 * K3  tsod_plot_series_u8: paints up to TSOD_PLOT_MAX_SERIES series, in order, into the plot rectangle [px0, px0 + pw) x
 *     [py0, py0 + ph) of ONE u8 RGB image [H][W][3] (row_bytes >= 3 W between rows).  Nothing outside the rectangle and no
 *     byte of a row beyond 3 W is read or written; a pixel no series covers is neither read nor written.
 *     A series (tsod_plot_series): y DEVICE f32 [n]; the abscissa of sample i is the integer x_i = x_first + i x_step
 *     (x_step >= 1), and x_lo <= x_first, x_first + (n - 1) x_step <= x_hi must hold; color = R G B alpha; width w in [0,
 *     TSOD_PLOT_MAX_WIDTH]; marker TSOD_PLOT_MARKER_*; marker_size odd, in [1, TSOD_PLOT_MAX_WIDTH].
 *     limits: DEVICE f32 [2] = (lo, hi), e.g. from K2.
 *       Column: c_i = px0 + floor((x_i - x_lo) (pw - 1) / (x_hi - x_lo)) in 64-bit integers; x_hi == x_lo: c_i = px0.
 *       Row:    r_i = py0 + (ph - 1) - (int)rintf(fminf(fmaxf((v - lo) * s, 0), ph - 1)) with s = (float)(ph - 1) / (hi -
 *               lo): one f32 difference hi - lo, one quotient, one difference v - lo, one product; fmaxf / fminf drop a NaN
 *               product (lo == hi), which so maps to the bottom row.
 *       Points: sample i is a point when y[i] is finite.  A non-finite sample is no point and the two segments that touch
 *               it are not drawn; a finite sample between two non-finite ones still paints its point.
 *       Line (w >= 1): the skeleton is every point's pixel (c_i, r_i) and, for consecutive points (c0, r0), (c1, r1) (c0 <=
 *               c1, the abscissa is monotone), the segment's pixels: c0 == c1: rows min(r0, r1) .. max(r0, r1) of the
 *               column.  Else with dx = c1 - c0, dy = r1 - r0 and B(c) = r0 + floor(((2 (c - c0) - 1) dy + dx) / (2 dx))
 *               (floor division, 64-bit): column c of c0 .. c1 paints the rows between (c == c0 ? r0 : B(c)) and (c == c1 ?
 *               r1 : B(c + 1)), both included.  (Both endpoints are painted, rows stay within min(r0, r1) .. max(r0, r1),
 *               consecutive columns share a row, a horizontal segment paints one row; the rows of column c are a function
 *               of (c0, r0, c1, r1, c) alone.)  Every skeleton pixel (c, r) covers the w x w pixels of columns c - w / 2 ..
 *               c - w / 2 + w - 1 and the same rows (integer division: odd w is centred).  w == 0 draws no line.
 *       Marker (marker != NONE), at every point, k = marker_size / 2, (u, v) = pixel - (c_i, r_i), |u| <= k, |v| <= k:
 *               SQUARE: all of them; CIRCLE: u u + v v <= k k + k; TRIANGLE (apex up): 2 |u| <= v + k.
 *       Coverage of a series = line pixels and marker pixels, clipped to the rectangle; every covered pixel is blended
 *               ONCE per series with the overlay's rule, out = (a c + (255 - a) src + 127) / 255 per channel; alpha 0
 *               leaves the series out.  A later series paints over an earlier one.
 *     The kernel: one workgroup per block of TSOD_PLOT_BLOCK_COLUMNS columns over the rectangle's height.  Per series it
 *     clears a row bitmask in LDS, finds by bisection (c_i is monotone in i) the samples whose column lies within a halo of
 *     its block, one more on each side, lets its threads stride over them setting row ranges with atomicOr, and after a
 *     barrier blends the set pixels: O(n + pixels) work, no pixel looks at all samples.
 *     TSOD_ERR_INVALID_ARG: image or limits NULL; H, W, pw or ph <= 0; row_bytes < 3 W; the rectangle not inside the image;
 *     x_hi < x_lo; n_series outside [0, TSOD_PLOT_MAX_SERIES] (or series NULL with n_series > 0); in a series: n < 0, y NULL
 *     with n > 0, x_step < 1, an abscissa outside [x_lo, x_hi], width or marker_size outside their ranges, an even
 *     marker_size, a marker outside the enum.  TSOD_ERR_UNSUPPORTED: H W beyond 2^31 - 1; ph > TSOD_PLOT_MAX_HEIGHT (the
 *     bitmask); |x_lo|, |x_hi| beyond 2^31 - 1.  n_series == 0 or n == 0 in every series: TSOD_OK, no launch.
 *
 * K4  tsod_plot_items_u8: paints n_items decorations (items: DEVICE array of tsod_plot_item, 8-byte aligned), in order,
 *     onto one image; everything is clipped to the image.
 *       TSOD_PLOT_ITEM_RECT: the pixels of [x, x + w) x [y, y + h), blended with color (alpha color[3]).  dash_period > 0
 *         keeps only the rows with (row - y) % dash_period < dash_on (a dashed vertical line); dash_period == 0: all rows.
 *       TSOD_PLOT_ITEM_TEXT: the bytes text[0 .. len) in the glyphs of csrc/font5x7.h (5x7 in a 6x8 cell, every glyph
 *         pixel scale x scale image pixels), set pixels blended with color; the string is len 6 scale pixels wide and its
 *         left edge is x (align 0), x - len 6 scale (align 1: x is its right edge) or x - (len 6 scale) / 2 (align 2); its
 *         top row is y.
 *       TSOD_PLOT_ITEM_NUMBER: the same, the string made on the device from limits (DEVICE f32 [2], the item's pointer): v
 *         = lo + ((float)tick * (hi - lo)) / (float)ticks, four f32 operations; p = fabsf(v) * 1000.f; when !(p < 1e9f) (too
 *         large to print, or not a number) the string is "-.---"; else m = (int)rintf(p) and the string is '-' (only when v
 *         < 0 and m > 0), the decimal digits of m / 1000, '.', and the three digits of m % 1000.
 *       An item of another kind, or with w, h, scale < 1 or len outside [0, TSOD_PLOT_STRING_BYTES], paints nothing.
 *     The kernel: one workgroup per 64x4 tile; it tests the items 256 at a time (one per thread) against its tile, keeps the
 *     hits as wave ballots and every thread walks the set bits, in item order, for its pixel; one load and one store per
 *     touched pixel.
 *     TSOD_ERR_INVALID_ARG: image NULL; H or W <= 0; row_bytes < 3 W; n_items < 0; items NULL with n_items > 0.
 *     TSOD_ERR_UNSUPPORTED: H W beyond 2^31 - 1.  TSOD_ERR_ALIGNMENT: items not 8-byte aligned.  n_items == 0: TSOD_OK, no launch. */
#define TSOD_PLOT_MAX_SERIES 4
#define TSOD_PLOT_MAX_WIDTH 15
#define TSOD_PLOT_MAX_HEIGHT 4096
#define TSOD_PLOT_BLOCK_COLUMNS 32
#define TSOD_PLOT_STRING_BYTES 32
#define TSOD_PLOT_LIMITS_WORKSPACE_BYTES 2048
enum { TSOD_PLOT_MARKER_NONE = 0, TSOD_PLOT_MARKER_CIRCLE = 1, TSOD_PLOT_MARKER_SQUARE = 2, TSOD_PLOT_MARKER_TRIANGLE = 3 };
enum { TSOD_PLOT_ITEM_RECT = 0, TSOD_PLOT_ITEM_TEXT = 1, TSOD_PLOT_ITEM_NUMBER = 2 };
typedef struct tsod_plot_series {
    const float *y;         /* [n], device */
    int32_t n, x_first, x_step;
    uint8_t color[4];       /* R G B, alpha */
    int32_t width, marker, marker_size;
} tsod_plot_series;
typedef struct tsod_plot_item {
    const float *limits;    /* NUMBER: device f32 [2] */
    int32_t kind;           /* TSOD_PLOT_ITEM_* */
    int32_t x, y, w, h;     /* RECT: the rectangle; TEXT / NUMBER: the anchor (x, y) */
    int32_t dash_period, dash_on; /* RECT */
    int32_t scale, align, len; /* TEXT / NUMBER (len: TEXT) */
    int32_t tick, ticks;    /* NUMBER */
    uint8_t color[4];       /* R G B, alpha */
    uint8_t text[32];       /* TEXT */
} tsod_plot_item;
int tsod_ema_scan_f32(const float *x, int32_t rows, int64_t n, int64_t x_pitch, float a, float b, float *out, int64_t out_pitch,
                      tsod_stream_t stream);
int tsod_plot_limits_f32(const float *const *series, const int64_t *lengths, int32_t n_series, float *limits, void *workspace,
                         size_t workspace_bytes, tsod_stream_t stream);
int tsod_plot_series_u8(uint8_t *image, int32_t H, int32_t W, int64_t row_bytes, int32_t px0, int32_t py0, int32_t pw, int32_t ph,
                        const tsod_plot_series *series, int32_t n_series, int64_t x_lo, int64_t x_hi, const float *limits,
                        tsod_stream_t stream);
int tsod_plot_items_u8(uint8_t *image, int32_t H, int32_t W, int64_t row_bytes, const tsod_plot_item *items, int32_t n_items,
                       tsod_stream_t stream);

/* ---- JPEG decoding: the reference's Image.open(path).convert("RGB") for baseline files, bit-equal
 * to Pillow (libjpeg-turbo's default islow / fancy upsampling / YCbCr path).  The bit-serial Huffman pass runs on the HOST
 * (csrc/jpeg_entropy.h) or, from the file's own unstuffed bytes, on the DEVICE (csrc/jpeg_huffman.hip, the section after this
 * one): the two write the same coefficients.  Everything that is arithmetic over pixels runs in two launches for a whole batch.
 *
 * HOST, re-entrant, no allocation, never reads outside [data, data + n):
 *   tsod_jpeg_parse: markers up to the first scan into *info.  Supported: 8-bit SOF0 / SOF1 (Huffman), one component (grey)
 *     or three (YCbCr) with luma sampling 1x1, 2x1 or 2x2 over 1x1 chroma in one interleaved scan.
 *     TSOD_ERR_UNSUPPORTED: any other SOF (progressive, lossless, arithmetic), another precision, two or four components,
 *     another sampling, a scan that does not hold every component in frame order, an Adobe APP14 marker with transform 0 on
 *     a three-component file (RGB-coded).  TSOD_ERR_INVALID_ARG: data or info NULL, no SOI, a segment length past the end, a
 *     cut-short or over-full DQT / DHT, zero dimensions, a scan before the frame, a table the scan names but no segment
 *     defined, spectral selection other than 0..63, the end of the data before a scan.
 *   tsod_jpeg_entropy_decode: the Huffman pass of the same file into coef[0 .. info.coef_total): int16, NOT dequantised, in
 *     natural (row-major) order inside each block of 64, component after component, the blocks of a component in raster
 *     order over its padded grid blocks_w x blocks_h (whole MCUs).  DC predictions are summed in wrapping 32-bit arithmetic
 *     and stored as their low 16 bits.  FF 00 is unstuffed; at every restart interval the next marker must be the expected
 *     RSTn (the DC predictors reset).  capacity (in int16) must be >= info.coef_total; nothing beyond coef_total is written.
 *     What tsod_jpeg_parse refuses is refused alike; TSOD_ERR_INVALID_ARG also for: coef NULL or capacity too small, entropy
 *     bits that end before the last MCU does, a code no table holds, a DC category above 15, a run (ZRL included) past
 *     coefficient 63, a wrong or missing restart marker.  After a negative status coef holds unspecified values inside
 *     [0, capacity).  A missing EOI after the last MCU is accepted.
 *
 * DEVICE, both in the pattern of tsod_adamw_step_f32: a table of per-image records and a flat work list, in device memory,
 * so that images of different sizes and samplings share ONE launch.  Each entry also takes the HOST copy of both arrays and
 * checks every record and every work item against the buffer sizes before it launches: every address the kernels form
 * comes from these checked integers, the only file-derived data they read are coefficient, quantiser and sample VALUES.
 * (The device copies must equal the host copies.)
 *   tsod_jpeg_idct_u8: plane sample = range(idct(coef * quant)): for every component the u8 plane [8 blocks_h][8 blocks_w]
 *     at planes + plane_offset[c].  The arithmetic, all in wrapping 32-bit integers (the kernel computes in uint32_t):
 *       d = (int32)coef * (int32)quant; two passes of the Loeffler-Ligtenberg-Moschytz 8-point inverse DCT with 13-bit
 *       constants 2446 3196 4433 6270 7373 9633 12299 15137 16069 16819 20995 25172 (libjpeg's jidctint.c): columns first,
 *       descaled by 11, then rows, descaled by 18 - descale(x, n) = (x + (1 << (n - 1))) >> n, arithmetic shift; the sample
 *       is looked up at j = v & 1023: j < 128 -> j + 128, j < 512 -> 255, j < 896 -> 0, else j - 896.
 *     Work item (image, component, first_block, 0): the blocks [first_block, first_block + TSOD_JPEG_IDCT_BLOCKS) of that
 *     component that exist; first_block is a multiple of TSOD_JPEG_IDCT_BLOCKS.  One workgroup of 256 per item, 8 lanes per
 *     block: a lane loads one coefficient row and one quantiser row (16 bytes each), the column pass runs on a transposed
 *     copy in LDS, the row pass ends in one 8-byte store.
 *   tsod_jpeg_to_rgb_u8: out + out_offset = packed u8 [H][W][3] from the planes.
 *       Grey: R = G = B = Y.  Otherwise chroma sample (x, y) of a plane cropped to its true size dw = ceil(W / hs), dh =
 *       ceil(H / vs), indices beyond it clamped to its edge:  hs == 1: a[y][x].  dw <= 2: a[y / vs][x / 2] (replication).
 *       hs == 2, vs == 1: i = x / 2; (3 a[y][i] + a[y][i - 1] + 1) >> 2 for even x, (3 a[y][i] + a[y][i + 1] + 2) >> 2 for odd.
 *       hs == 2, vs == 2: r = y / 2, t[i] = 3 a[r][i] + a[r - 1][i] for even y, 3 a[r][i] + a[r + 1][i] for odd;
 *       (3 t[i] + t[i - 1] + 8) >> 4 for even x, (3 t[i] + t[i + 1] + 7) >> 4 for odd.
 *       With cb, cr minus 128: R = Y + ((91881 cr + 32768) >> 16), G = Y + ((-22554 cb - 46802 cr + 32768) >> 16),
 *       B = Y + ((116130 cb + 32768) >> 16), each clamped to 0..255.
 *     Work item (image, tile_y, tile_x, 0): the pixels of rows [TSOD_JPEG_RGB_TILE_H tile_y, +TSOD_JPEG_RGB_TILE_H) and
 *     columns [TSOD_JPEG_RGB_TILE_W tile_x, +TSOD_JPEG_RGB_TILE_W) inside the image; a thread makes four pixels of one row.
 *   TSOD_ERR_INVALID_ARG: a NULL pointer with work to do; a negative count; a record with n_comp not 1 or 3, a non-positive
 *     size, a sampling other than the above, a block grid smaller than the image needs, an offset that is negative, not a
 *     multiple of its unit (coef and quant: 64 elements, plane: 8 bytes) or whose extent ends beyond its buffer; a work item
 *     outside [0, n_images) or outside its image.  TSOD_ERR_ALIGNMENT: coef, quant, table or work not 16-byte, planes not
 *     8-byte aligned.  n_work == 0: TSOD_OK, nothing is launched. */
#define TSOD_JPEG_IDCT_BLOCKS 32
#define TSOD_JPEG_RGB_TILE_W 256
#define TSOD_JPEG_RGB_TILE_H 4
typedef struct tsod_jpeg_info {
    int32_t H, W, n_comp, hmax, vmax, mcus_x, mcus_y, restart_interval;
    int32_t h[3], v[3], tq[3];     /* sampling factors and quantiser selector of each component */
    int32_t blocks_w[3], blocks_h[3]; /* the padded block grid: mcus_x h, mcus_y v */
    int32_t plane_w[3], plane_h[3]; /* 8 blocks_w, 8 blocks_h */
    int32_t reserved;
    int64_t coef_count[3];         /* 64 blocks_w blocks_h: coefficients, and bytes of the plane */
    int64_t coef_total;
    uint16_t quant[3][64];         /* each component's quantiser, natural order */
} tsod_jpeg_info;
typedef struct tsod_jpeg_image {
    int64_t coef_offset[3];        /* int16 elements from coef */
    int64_t plane_offset[3];       /* bytes from planes */
    int64_t quant_offset;          /* uint16 elements from quant: [n_comp][64] */
    int64_t out_offset;            /* bytes from out */
    int32_t H, W, n_comp, hs, vs;  /* hs x vs: the luma sampling (1x1 for grey) */
    int32_t blocks_w[3], blocks_h[3];
    int32_t reserved;
} tsod_jpeg_image;
int tsod_jpeg_parse(const uint8_t *data, size_t n, tsod_jpeg_info *info);
int tsod_jpeg_entropy_decode(const uint8_t *data, size_t n, int16_t *coef, size_t capacity);
int tsod_jpeg_idct_u8(const tsod_jpeg_image *table_host, const tsod_jpeg_image *table, int32_t n_images, const int32_t *work_host,
                      const int32_t *work, int32_t n_work, const int16_t *coef, int64_t coef_count, const uint16_t *quant,
                      int64_t quant_count, uint8_t *planes, int64_t plane_bytes, tsod_stream_t stream);
int tsod_jpeg_to_rgb_u8(const tsod_jpeg_image *table_host, const tsod_jpeg_image *table, int32_t n_images, const int32_t *work_host,
                        const int32_t *work, int32_t n_work, const uint8_t *planes, int64_t plane_bytes, uint8_t *out,
                        int64_t out_bytes, tsod_stream_t stream);

/* ---- The Huffman pass on the DEVICE ("entropy on the device"): an alternative to
 * tsod_jpeg_entropy_decode that uploads the file's own entropy-coded bytes instead of 6 bytes of coefficients per pixel.
 * The host does a byte-speed sweep (tsod_jpeg_scan_prepare), the device decodes (tsod_jpeg_huffman_i16) into the same
 * coefficient layout, bit for bit, that tsod_jpeg_idct_u8 reads.
 *
 * HOST, re-entrant, no allocation, never reads outside [data, data + n) nor writes outside the stated capacities:
 *   tsod_jpeg_scan_sizes: from the info of tsod_jpeg_parse and the file length n, the capacities tsod_jpeg_scan_prepare needs
 *     at most: *n_segments = min(ceil(mcus / restart_interval) or 1, n / 2 + 1), *stream_bytes = n + 4 *n_segments rounded up
 *     to 4.  TSOD_ERR_INVALID_ARG: a NULL pointer, an info with no MCUs.
 *   tsod_jpeg_scan_prepare: for a file tsod_jpeg_parse accepts,
 *     stream: the entropy-coded bytes with FF 00 unstuffed and the restart markers removed; every restart interval
 *       ("segment") starts on a 4-byte boundary of stream and is zero-padded to the next.  *stream_bytes: bytes written.
 *     segments[0 .. *n_segments): one record per restart interval (one for a file without restarts): first_mcu, n_mcu,
 *       stream_offset (bytes from stream, a multiple of 4), bit_length (8 x the segment's real bytes), flags (bit 0: a restart
 *       marker followed the segment - the decoder then requires fewer than 8 leftover bits), image = 0.
 *     tables[TSOD_JPEG_HUFF_TABLES]: the scan's code tables in the fixed layout below, tables[2 c] the DC and tables[2 c + 1]
 *       the AC table of component c; the tables of components the file does not have are zero.
 *     Markers are checked exactly as tsod_jpeg_entropy_decode checks them: every interval but the last is followed by at
 *     least one FF and the expected RSTn; a missing EOI after the last is accepted.  TSOD_ERR_INVALID_ARG: a NULL pointer, a
 *     capacity too small, a missing or wrong restart marker; what tsod_jpeg_parse refuses is refused alike.  After a negative
 *     status the buffers hold unspecified values inside their capacities.
 *
 * DEVICE, in the pattern of the two entries above (host and device copies of every list; every record and work item is
 * checked on the host against the buffer sizes before anything is launched):
 *   tsod_jpeg_huffman_i16: coef[0 .. coef_count) = 0, status[0 .. n_images) = 0 (one fill launch), then ONE launch over the
 *     work list decodes every segment of a batch of any sizes and samplings: coef as tsod_jpeg_entropy_decode writes it at
 *     table[i].coef_offset[c].  Of a table record only n_comp, hs, vs, blocks_w, blocks_h and coef_offset are read; image
 *     i's code tables are huff[TSOD_JPEG_HUFF_TABLES i ..].
 *     Work item (segment, 0, 0, 0): one workgroup of 256 lanes walks the segment in rounds of 256 consecutive subsequences
 *     of 32 subseq_words bits (the self-synchronising decoder of Weissenberger and Schmidt, workgroup-local).  The parser
 *     state between symbols is (bit position, block slot in the MCU, zigzag index) or one absorbing ERROR value.  A lane
 *     decodes every symbol that starts in its subsequence from an assumed state, then again whenever its predecessor's end
 *     state differs from the start it used (an ERROR end state is never taken over: the lane that meets a true error
 *     reports it itself), until a workgroup vote finds no change (at most 256 times: after iteration k lanes 0 .. k are
 *     final - the result never depends on the stream synchronising, only the time does).  Block counts and
 *     per-component DC sums (wrapping uint32) are scanned over the lanes with the carry of the earlier rounds, and a last
 *     pass stores the coefficients: natural order, a block's DC the low 16 bits of its running prediction.
 *     A coefficient is stored only for a block number below the segment's n_mcu x blocks-per-MCU and a zigzag index <= 63,
 *     at an address made from the checked records; stream loads are clamped to the segment's padded extent: a corrupt file
 *     never becomes an out-of-range address.  status[image] gets (atomic OR) TSOD_JPEG_STATUS_ERROR when a segment meets an
 *     invalid code, a DC category above 15, a run past 63 or the end of its bits inside a symbol before its last block,
 *     TSOD_JPEG_STATUS_BLOCKS when it ends with fewer blocks than its record says, TSOD_JPEG_STATUS_LEFTOVER when 8 or more
 *     bits are left before a restart marker; it is 0 exactly where tsod_jpeg_entropy_decode returns TSOD_OK.  The
 *     coefficients of an image with a nonzero status are unspecified (inside the image's own extents).
 *   TSOD_ERR_INVALID_ARG: subseq_words outside [1, 64]; a negative count; a NULL pointer with work to do; a record with
 *     n_comp not 1 or 3, another sampling, a block grid that is not whole MCUs, a coef_offset that is negative, not a multiple
 *     of 64 or whose extent ends beyond coef_count; fewer than TSOD_JPEG_HUFF_TABLES n_images tables; segments that are not
 *     sorted by image or do not tile the MCUs of every image exactly, in order; a stream_offset that is negative, not a
 *     multiple of 4 or whose padded extent ends beyond stream_bytes; a bit_length that is negative, not a multiple of 8 or
 *     above TSOD_JPEG_MAX_SEGMENT_BITS; flags other than 0 or 1; a work item outside [0, n_segments).
 *   TSOD_ERR_ALIGNMENT: table, segments, work or coef not 16-byte, stream, huff or status not 4-byte aligned.
 *   n_work == 0: TSOD_OK, nothing is launched.
 *
 * SPLIT over workgroups ("split over workgroups"): the same pass for segments that are long - a
 * file without restart markers is ONE segment, so one workgroup above.
 *   tsod_jpeg_huffman_split_i16: the arguments, the result and the status word of tsod_jpeg_huffman_i16; the work list is a
 *     chunk list.  A segment of `bits` bits has n = ceil(bits / (32 subseq_words)) subsequences and max(1, ceil(n /
 *     chunk_subseqs)) chunks; chunk c owns subsequences [c chunk_subseqs, min((c + 1) chunk_subseqs, n)).  Item (segment,
 *     chunk, list index of the segment's chunk 0, the segment's chunk count); the list holds every segment's chunks in order,
 *     segment after segment.  After the fill launch, three launches, ordered by the stream alone (no workgroup waits for
 *     another inside a kernel):
 *       sync, one workgroup per chunk: one lane per subsequence of the chunk and of up to `overlap` subsequences before it
 *         (warm-up: they belong to the chunk before and only bring the parse into step), every lane from an assumed state
 *         (subsequence 0 from the true one), the fixpoint above among them (at most as many passes as lanes).  The owned
 *         lanes' start state, end state and tally go to the workspace, with the chunk's entry (the start of its first owned
 *         lane), exit (the end of its last) and total.
 *       stitch, one workgroup per segment: chunk 0 is true.  Chunk c stands when the final exit of chunk c - 1 equals its
 *         entry; otherwise it is repaired: its first lane starts from that exit and the fixpoint runs over its own lanes from
 *         their stored states (at most chunk_subseqs passes).  An ERROR exit ends the walk: a true error was met, and nothing
 *         after it is looked at, as above.  The boundaries are compared 256 at a time across the lanes; only a mismatch is
 *         walked to.  An exclusive scan of the chunk totals gives every chunk its base; TSOD_JPEG_STATUS_BLOCKS is set from
 *         the segment's total; repaired[segment] (when not NULL) = the chunks repaired.  The repair is exact for any
 *         content, but serial per segment: `overlap` is what keeps it rare.
 *       write, one workgroup per chunk: the owned lanes' tallies scanned on top of the chunk's base, then the coefficients
 *         from every lane's final start, with the store rule and the status bits above.
 *     The result never depends on the parse synchronising inside the overlap, only the time does.  No record of the workspace
 *     is read before this call has written it.
 *   tsod_jpeg_huffman_split_workspace_bytes(n_subseqs, n_chunks, n_segments) = 48 n_chunks + 32 (n_subseqs + 256 n_segments),
 *     n_subseqs the sum of n over the segments (chunk_subseqs lane records per chunk: at most n + chunk_subseqs per segment);
 *     0 for a negative argument.
 *   TSOD_ERR_INVALID_ARG: what tsod_jpeg_huffman_i16 refuses; chunk_subseqs outside [1, 256]; overlap outside [0, 256 -
 *     chunk_subseqs]; a chunk list that is not, segment after segment, every segment's chunks 0 .. count - 1 with the count
 *     that (bit_length, subseq_words, chunk_subseqs) implies; workspace NULL or smaller than the helper says.
 *   TSOD_ERR_ALIGNMENT: as above, and workspace not 16-byte or repaired not 4-byte aligned.
 *   n_chunks == 0: TSOD_OK, nothing is launched. */
#define TSOD_JPEG_HUFF_TABLES 6
#define TSOD_JPEG_MAX_SEGMENT_BITS 0x7FF00000
#define TSOD_JPEG_STATUS_ERROR 1
#define TSOD_JPEG_STATUS_BLOCKS 2
#define TSOD_JPEG_STATUS_LEFTOVER 4
typedef struct tsod_jpeg_huff {
    uint16_t look[512];            /* (length << 8) | symbol for codes of at most 9 bits, 0: longer or absent */
    int32_t maxcode[17];           /* largest code of each length, -1 when the length has none */
    int32_t valoff[17];            /* vals index of a length's first code, minus that code */
    uint8_t vals[256];
} tsod_jpeg_huff;
typedef struct tsod_jpeg_segment {
    int64_t stream_offset;         /* bytes from stream, a multiple of 4 */
    int64_t bit_length;            /* 8 x the real bytes */
    int32_t image, first_mcu, n_mcu, flags;
} tsod_jpeg_segment;
int tsod_jpeg_scan_sizes(const tsod_jpeg_info *info, size_t n, int64_t *stream_bytes, int32_t *n_segments);
int tsod_jpeg_scan_prepare(const uint8_t *data, size_t n, uint8_t *stream, int64_t stream_capacity, int64_t *stream_bytes,
                           tsod_jpeg_segment *segments, int32_t segment_capacity, int32_t *n_segments, tsod_jpeg_huff *tables);
int tsod_jpeg_huffman_i16(const tsod_jpeg_image *table_host, const tsod_jpeg_image *table, int32_t n_images,
                          const tsod_jpeg_segment *segments_host, const tsod_jpeg_segment *segments, int32_t n_segments,
                          const int32_t *work_host, const int32_t *work, int32_t n_work, const uint8_t *stream, int64_t stream_bytes,
                          const tsod_jpeg_huff *huff, int64_t n_huff, int16_t *coef, int64_t coef_count, int32_t *status,
                          int32_t subseq_words, tsod_stream_t stream_handle);
size_t tsod_jpeg_huffman_split_workspace_bytes(int64_t n_subseqs, int32_t n_chunks, int32_t n_segments);
int tsod_jpeg_huffman_split_i16(const tsod_jpeg_image *table_host, const tsod_jpeg_image *table, int32_t n_images,
                                const tsod_jpeg_segment *segments_host, const tsod_jpeg_segment *segments, int32_t n_segments,
                                const int32_t *chunks_host, const int32_t *chunks, int32_t n_chunks, const uint8_t *stream,
                                int64_t stream_bytes, const tsod_jpeg_huff *huff, int64_t n_huff, int16_t *coef, int64_t coef_count,
                                int32_t *status, int32_t subseq_words, int32_t chunk_subseqs, int32_t overlap, void *workspace,
                                size_t workspace_bytes, int32_t *repaired, tsod_stream_t stream_handle);

/* ---- collective: thin wrapper over ncclAllGather (RCCL over xGMI) on the caller's stream.
 * `comm` is an ncclComm_t (from tsod_comm_init_rank below, or any communicator the host already owns); every rank sends
 * `count_per_rank` floats and receives n_ranks * count_per_rank in rank order.  Stream-ordered, no host synchronisation.
 * RCCL is bound at run time: TSOD_ERR_UNSUPPORTED when no librccl can be loaded.  The reference has no distributed code
 * (nothing to match); the payload is tsod_detections_f32's fixed-size records. */
int tsod_allgather_f32(void *comm, const float *send, float *recv, size_t count_per_rank, tsod_stream_t stream);
/* communicator helpers for a host without torch.distributed: rank 0 makes the 128-byte id and ships it to the others by any
 * means, then every rank calls init_rank (collective: blocks until all n_ranks have called it) */
int tsod_comm_unique_id(void *id128);
int tsod_comm_init_rank(void **comm, int32_t n_ranks, const void *id128, int32_t rank);
int tsod_comm_destroy(void *comm);

#ifdef __cplusplus
}
#endif
#endif /* TSOD_H */
