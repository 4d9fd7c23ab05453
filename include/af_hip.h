/*
 * af_hip.h — C ABI of libafhip.so: the MI355X (gfx950) kernels behind the AltFreezing
 * `i3d_ori` clip classifier forward.
 *
 * The reference has no FFI: its hot path is stock torch.nn modules called from Python
 * (SURVEY.md section 8b).  Each entry point below therefore names the reference *operator
 * sequence* it replaces (file:line under /root/reference/altfreezing unless noted); the
 * ctypes binding a maintainer would add is shown in INTEGRATION.md.
 *
 * Conventions
 *   - plain pointers and ints only; every buffer is caller-owned DEVICE memory (16-byte
 *     aligned) and must stay alive until the stream has drained;
 *   - activations are NDHWC (channels innermost), element type `dtype` (AF_F32/AF_BF16/AF_F16);
 *     accumulation is always fp32; BatchNorm is applied as a per-channel fp32 scale/shift
 *     in the producing kernel's epilogue;
 *   - kernels are enqueued asynchronously on `stream` (a hipStream_t passed as void*,
 *     NULL = the null stream); nothing here synchronises, allocates or frees device memory (scratch a launch
 *     may need is sized by af_conv_workspace_bytes() and passed in by the caller), except the *_timed entry
 *     points which record and wait for their own events; there is no mutable global state beyond per-device
 *     "attribute already set" flags, so launches on different streams / devices of one process do not interact;
 *   - return value 0 = success, negative = error; af_last_error() (thread-local text).
 */
#ifndef AF_HIP_H
#define AF_HIP_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define AF_ABI_VERSION 6

enum af_dtype { AF_F32 = 0, AF_BF16 = 1, AF_F16 = 2 };

enum af_status {
    AF_OK = 0,
    AF_ERR_ARG = -1,        /* bad pointer / dimension / unsupported configuration */
    AF_ERR_LAUNCH = -2,     /* hipLaunch / runtime error */
    AF_ERR_NO_DEVICE = -3
};

/* stem input geometry: [N][T+4][H+6][W+8][4] with zero halos (2 | 3 | 3-left,5-right) and a
 * zero 4th channel; written by af_pack_input_* and read by af_stem_conv_bn_relu. */
#define AF_STEM_PAD_T 2
#define AF_STEM_PAD_H 3
#define AF_STEM_PAD_W_LEFT 3
#define AF_STEM_PAD_W_TOTAL 8
#define AF_STEM_CPAD 4

typedef struct af_conv_desc {
    int32_t n, t, h, w, cin;        /* input  [n][t][h][w][cin]              */
    int32_t cout;
    int32_t kt, kh, kw;
    int32_t st, sh, sw;
    int32_t pt, ph, pw;
    int32_t to, ho, wo;             /* output [n][to][ho][wo][cout]; checked */
    int32_t relu;                   /* ReLU after scale/shift(+residual)     */
    int32_t dtype;                  /* af_dtype of in / weights / residual / out */
    int32_t tpool;                  /* 1: also apply MaxPool3d([2,1,1],stride [2,1,1]) (pathway0_pool,
                                       video_model_builder.py:474-480) to the result: out is then
                                       [n][to/2][ho][wo][cout]; to must be even (af_conv3d_bn_act only)
                                       2: also apply MaxPool3d((1,2,2)) (what FTCN-TT's temporal_only_conv puts
                                       after the BN of a conv that lost its stride 2): out is [n][to][ho/2][wo/2][cout];
                                       ho, wo even, no residual (the ReLU, if any, commutes with the max) */
} af_conv_desc;

typedef struct af_pool_desc {
    int32_t n, t, h, w, c;
    int32_t kt, kh, kw, st, sh, sw, pt, ph, pw;
    int32_t to, ho, wo;
    int32_t dtype;
    int32_t out_ld;                 /* af_maxpool3d: channel stride of the output rows (0 = c); lets the Slow
                                       pathway's pooled stem leave room for the lateral's channels */
} af_pool_desc;

int af_version(void);
const char* af_last_error(void);
/* number of visible HIP devices, or AF_ERR_NO_DEVICE */
int af_device_count(void);

/* ---- one-time weight transforms (model load) ------------------------------------------- */

/* nn.BatchNorm3d(eval) -> scale = gamma / sqrt(var + eps), shift = beta - mean * scale
 * (slowfast/models/batchnorm_helper.py:23-24; applied at stem_helper.py:175, resnet_helper.py:314-325,441) */
int af_fold_bn(const float* gamma, const float* beta, const float* mean, const float* var,
               float eps, int channels, float* scale, float* shift, void* stream);

/* nn.Conv3d weight OIDHW fp32 -> [cout_pad][kt*kh*kw][cin_pad] in `dtype` (K-major rows for the implicit GEMM);
 * cout is padded to a multiple of 64 rows and cin to the K-step (64 elements, fp32: 32) with zeros, so any
 * channel count that is a multiple of 8 (fp32: 4) runs (SlowFast's 8/16/32/80/320-channel layers).
 * Output bytes: af_packed_conv_weight_bytes().  The BN scale/shift arrays handed to the conv entry points must
 * have af_padded_channels(cout) entries (padding = anything finite). */
int64_t af_packed_conv_weight_bytes(int cout, int cin, int kt, int kh, int kw, int dtype);
int af_padded_channels(int cout);
int af_pack_conv_weight(const float* w_oidhw, int cout, int cin, int kt, int kh, int kw,
                        int dtype, void* packed, void* stream);
/* same, with each output-channel row multiplied by row_scale[cout] in fp32 before the rounding to `dtype`
 * (BatchNorm scale folded into the weights: needed when two convolutions share one accumulator, below) */
int af_pack_conv_weight_scaled(const float* w_oidhw, const float* row_scale, int cout, int cin, int kt, int kh, int kw,
                               int dtype, void* packed, void* stream);

/* stem weight (64,3,kt,7,7) fp32 -> [kt][7][chunk][64][16 B]: kw padded 7->8, cin 3->4 (zeros) */
int64_t af_packed_stem_weight_bytes(int cout, int kt, int kh, int dtype);
int af_pack_stem_weight(const float* w_oidhw, int cout, int kt, int kh, int kw, int dtype,
                        void* packed, void* stream);

/* ---- input prologue (replaces the callers' as_tensor/permute/sub/div, test/af_realtime.py:77-83) */

int64_t af_stem_input_bytes(int n, int t, int h, int w, int dtype);
/* (n,3,t,h,w)-logical fp32 tensor with arbitrary element strides -> padded stem input */
int af_pack_input_f32(const float* x, int n, int t, int h, int w,
                      int64_t stride_n, int64_t stride_c, int64_t stride_t, int64_t stride_h, int64_t stride_w,
                      int dtype, void* stem_in, void* stream);
/* caller-layout uint8 clips (n,t,h,w,3), 0..255 RGB -> (x - mean[c]) / std[c] -> padded stem input */
int af_pack_input_u8(const uint8_t* clips, int n, int t, int h, int w,
                     const float mean[3], const float std_[3], int dtype, void* stem_in, void* stream);

/* ---- layers ------------------------------------------------------------------------- */

/* Conv3d(3->64,[kt,7,7],s[1,2,2],p[kt/2,3,3],bias=False)+BN+ReLU  (stem_helper.py:156-177).
 * d->cin must be 3, in = padded stem input, out = [n][to][ho][wo][cout]. */
int af_stem_conv_bn_relu(const af_conv_desc* d, const void* stem_in, const void* w_packed,
                         const float* scale, const float* shift, void* out, void* stream);

/* The whole ResNetBasicStem (stem_helper.py:173-178) as one launch: conv + BN + ReLU +
 * MaxPool3d([1,3,3],stride [1,2,2],pad [0,1,1]); out = [n][to][(ho-1)/2+1][(wo-1)/2+1][64] where (to,ho,wo) are
 * the conv output dims in `d`.  16-bit dtypes only (all weight slices stay resident in LDS); the conv output
 * tensor is never materialised. */
int af_stem_conv_bn_relu_maxpool(const af_conv_desc* d, const void* stem_in, const void* w_packed,
                                 const float* scale, const float* shift, void* out, void* stream);

/* The same fused stem on the K-PACKED input ("rgb3": 3 real channels per pixel, 6 bytes; rows of
 * ((w + 8) * 6 rounded up to 16) bytes, frames / rows / left halo padded like the 4-channel layout): the 7 x 7 x 3 taps of a
 * (dt) plane fill 5.25 MFMA K-blocks instead of 7 - the stem is MFMA-bound on exactly that padding (kt = 5: 27 blocks instead
 * of 35).  af_stem_input_bytes_rgb3 includes the few rows of slack the last frame needs; the buffer is zero-filled once by
 * the caller, af_pack_input_*_rgb3 write the interior (same arguments and arithmetic as af_pack_input_*); weights:
 * af_pack_stem_weight_rgb3 -> af_packed_stem_weight_bytes_rgb3(kt, dtype) bytes.  16-bit dtypes, 64 output channels. */
int64_t af_stem_input_bytes_rgb3(int n, int t, int h, int w, int dtype);
int af_pack_input_f32_rgb3(const float* x, int n, int t, int h, int w,
                           int64_t stride_n, int64_t stride_c, int64_t stride_t, int64_t stride_h, int64_t stride_w,
                           int dtype, void* stem_in, void* stream);
int af_pack_input_u8_rgb3(const uint8_t* clips, int n, int t, int h, int w,
                          const float mean[3], const float std_[3], int dtype, void* stem_in, void* stream);
/* SlowFast's two inputs out of ONE read of the clip (added within ABI 6): caller-layout uint8 clips (n,t,h,w,3) ->
 * fast_in = all t frames, slow_in = frames 0, alpha, 2 alpha, ... (t / alpha frames; t % alpha != 0 is AF_ERR_ARG) - what
 * SlowFast's pack_pathway_output does with torch.index_select on the normalised tensor.  Each output is written in the layout
 * its stem reads: AF_PACK_C4 = the 4-channel padded layout of af_pack_input_u8 (af_stem_input_bytes), AF_PACK_RGB3 = the K-packed
 * layout of af_pack_input_u8_rgb3 (af_stem_input_bytes_rgb3; 16-bit dtypes only), with exactly the bytes those two entry points
 * write for the same frames: (x - mean[c]) / std[c], one rounding, interior cells only (the caller zero-fills both buffers once).
 * Both outputs 16-byte aligned.  A frame's pixels are loaded and normalised once and stored into both outputs. */
enum af_pack_layout { AF_PACK_C4 = 0, AF_PACK_RGB3 = 1 };
int af_pack_input_u8_pathways(const uint8_t* clips, int n, int t, int h, int w, const float mean[3], const float std_[3],
                              int alpha, int dtype, void* slow_in, int slow_layout, void* fast_in, int fast_layout, void* stream);
int64_t af_packed_stem_weight_bytes_rgb3(int kt, int dtype);
int af_pack_stem_weight_rgb3(const float* w_oidhw, int cout, int kt, int dtype, void* packed, void* stream);
int af_stem_conv_bn_relu_maxpool_rgb3(const af_conv_desc* d, const void* stem_in, const void* w_packed,
                                      const float* scale, const float* shift, void* out, void* stream);
/* the same with a pooled row stride of out_ld channels (>= 64): SlowFast's Slow stem writes its 64 channels in front of the
 * lateral's (FuseFastToSlow concatenates by channel, video_model_builder.py:136-143) (ABI 3) */
int af_stem_conv_bn_relu_maxpool_rgb3_ld(const af_conv_desc* d, const void* stem_in, const void* w_packed, const float* scale,
                                         const float* shift, void* out, int out_ld, void* stream);

/* Conv3d(bias=False)+BN[+residual add][+ReLU] as one implicit-GEMM launch: the a/b/c convs of
 * BottleneckTransform (resnet_helper.py:267-325), the projection shortcut and the add+ReLU of
 * ResBlock (resnet_helper.py:411-444), FuseFastToSlow's conv_f2s+bn+relu (video_model_builder.py:121-143).
 * Requires cin % 8 == 0 and cout % 8 == 0 (fp32: % 4); scale/shift have af_padded_channels(cout) entries.
 * `residual` (NULL or [n][to][ho][wo][cout]) is added before the ReLU.
 * `out_ld` = channel stride of `out` rows in elements (>= cout; lets FuseFastToSlow write into
 * the concatenated slow tensor), 0 means cout.
 * `workspace` / `workspace_bytes`: caller-owned device scratch (16-byte aligned) for the split-K path that small
 * batches take in long-K layers (a live call's 1-3 clips: a layer with a handful of tiles splits its K range over up
 * to 8 workgroups per tile, fp32 partial sums meet in the workspace).  af_conv_workspace_bytes(d) is the size this
 * layer can use (0: never splits); with NULL or fewer bytes the layer runs unsplit (same result to fp32 rounding).  The
 * workspace is free for reuse as soon as the NEXT launch on the same stream has been enqueued; launches that may run
 * concurrently (different streams) need one each. */
int64_t af_conv_workspace_bytes(const af_conv_desc* d);
int af_conv3d_bn_act(const af_conv_desc* d, const void* in, const void* w_packed,
                     const float* scale, const float* shift, const void* residual,
                     void* out, int out_ld, void* workspace, int64_t workspace_bytes, void* stream);

/* Block 0 of a stage as ONE launch: relu( bn_c(conv_c(b)) + bn_1(conv_1(x)) ), i.e. the last 1x1x1 of the
 * bottleneck plus the projection shortcut `branch1` (1x1x1, stride [1,s,s]) of ResBlock
 * (resnet_helper.py:411-444) accumulated into the same output tile: the shortcut tensor is never written
 * to or read back from HBM.  Both weights must be packed with their BN scale folded in
 * (af_pack_conv_weight_scaled); `scale` is then all ones and `shift` = shift_c + shift_1.
 * d2 describes the shortcut conv over in2 and must land on the same output positions as d. */
int af_conv3d_dual_bn_act(const af_conv_desc* d, const void* in, const void* w_packed,
                          const af_conv_desc* d2, const void* in2, const void* w2_packed,
                          const float* scale, const float* shift, void* out, int out_ld, void* stream);

/* A whole bottleneck block of a NARROW pathway as ONE launch (ABI 3):
 *     out = relu( shortcut(x) + bn_c(conv_c( relu(bn_b(conv_b( relu(bn_a(conv_a(x))) ))) )) )
 * = ResBlock.forward over BottleneckTransform (resnet_helper.py:255-326, 411-444) as SlowFast's Fast pathway instantiates it
 * (video_model_builder.py:146-387: dim_inner 8 / 16, trunk 32 / 64 channels).  da: kT x 1 x 1 (kT = 1 or 3) -> C/4, db: 1x3x3
 * C/4 -> C/4, dc: 1x1x1 C/4 -> C, all stride 1, 16-bit, C/4 = 8 or 16; the a and b tensors never leave the CU.
 * d1 == NULL: identity shortcut (x has C channels and is also the residual).  d1 != NULL (block 0 of the Fast pathway's s2:
 * 8 -> 32 channels): shortcut = bn_1(conv_1x1x1(x)), computed like af_conv3d_dual_bn_act does - wc_packed and w1_packed carry
 * their BN scale (af_pack_conv_weight_scaled), scale_c is all ones and shift_c = shift_c + shift_1.  `x` must not alias `out`.
 * af_block_abc_fusable() says whether a block takes this path. */
int af_block_abc_fusable(const af_conv_desc* da, const af_conv_desc* db, const af_conv_desc* dc, const af_conv_desc* d1);
int af_block_abc_bn_act(const af_conv_desc* da, const void* x, const void* wa_packed, const float* scale_a, const float* shift_a,
                        const af_conv_desc* db, const void* wb_packed, const float* scale_b, const float* shift_b,
                        const af_conv_desc* dc, const void* wc_packed, const float* scale_c, const float* shift_c,
                        const af_conv_desc* d1, const void* w1_packed, void* out, int out_ld, void* stream);

/* The 1x3x3 `b` conv (+BN+ReLU) and the 1x1x1 `c` conv (+BN) of a bottleneck + the ResBlock's residual add + ReLU
 * (resnet_helper.py:283-325, 438-444) as ONE launch: relu( bn_c(conv_c( relu(bn_b(conv_b(in))) )) + residual ).  The b
 * output of a frame (or band of rows) stays in LDS as the c conv's operand and never reaches HBM.  Available for the shapes
 * af_conv_bc_fusable() accepts (16-bit, stride 1, 128 or 256 mid channels, enough frames to fill the chip: the s3 / s4
 * bottlenecks at batch >= 12); `dc` describes the c conv over b's output ([n][t][h][w][db->cout]); `residual` may be NULL. */
int af_conv_bc_fusable(const af_conv_desc* db, const af_conv_desc* dc);
int af_conv3d_bc_bn_act(const af_conv_desc* db, const void* in, const void* wb_packed, const float* scale_b, const float* shift_b,
                        const af_conv_desc* dc, const void* wc_packed, const float* scale_c, const float* shift_c,
                        const void* residual, void* out, int out_ld, void* stream);

/* The END of one res block and the START of the next, across the block boundary, as ONE launch (s2, 16-bit):
 *     x     = relu( bn_c(conv1x1x1_c(b)) + residual )      resnet_helper.py:304-325, 438-444   -> out_x  [n][t][h][w][C]
 *     a_out = relu( bn_a(conv3x1x1_a(x)) )                  resnet_helper.py:267-281 (next block) -> out_a [n][t][h][w][64]
 * in the time-tiled layout of the 3x1x1 kernel (tile = all T frames of a few pixels: the temporal halo is inside the tile):
 * per 64-channel slab of the trunk the residual is fetched, the c conv's slab is computed and added in LDS, stored once and
 * multiplied by the three temporal taps there - the `a` conv no longer re-reads the trunk from HBM.  dc: 64 -> C channels
 * (C % 64 == 0), ReLU; da: C -> 64, kernel [3,1,1], pad [1,0,0]; T = 16 or 32; batches with >= 4 tiles per CU
 * (af_conv_ca_fusable says whether a pair qualifies).  Block 0 of a stage: instead of `residual`, the projection shortcut
 * (d1: 1x1x1, stride 1, 64 -> C over in1; both weight sets packed with their BN scale, scale_c = ones, shift_c = the summed
 * shifts - as for af_conv3d_dual_bn_act) is a second K segment of the c conv's accumulator; d1 / in1 / w1_packed are NULL otherwise. */
int af_conv_ca_fusable(const af_conv_desc* dc, const af_conv_desc* d1, const af_conv_desc* da);
int af_conv3d_ca_bn_act(const af_conv_desc* dc, const void* in_b, const void* wc_packed, const af_conv_desc* d1, const void* in1,
                        const void* w1_packed, const float* scale_c, const float* shift_c, const void* residual, void* out_x,
                        const af_conv_desc* da, const void* wa_packed, const float* scale_a, const float* shift_a, void* out_a,
                        void* stream);

/* The s2 -> s3 boundary as ONE launch (16-bit): the c conv of s2's last block with its residual and ReLU, pathway0_pool
 * (MaxPool3d [2,1,1], video_model_builder.py:566-569) and the 3x1x1 a conv of s3's block 0 (resnet_helper.py:267-281):
 *     x     = relu( bn_c(conv1x1x1_c(b)) + residual )                   [n][32][h][w][C]  (never stored)
 *     xp    = max(x[2t'], x[2t'+1])                                     -> out_x
 *     a_out = relu( bn_a(conv3x1x1_a(xp)) )                             -> out_a [n][16][h][w][128]
 * dc: 64 -> C (C % 64 == 0; run against fp64 up to C = 512), tpool = 1, t = 32, h even, w % 4 == 0; da: C -> 128, kernel [3,1,1], pad [1,0,0], t = 16.
 * x_sub = 1: out_x is the whole pooled trunk [n][16][h][w][C]; x_sub = 2: only its even (h, w) positions, packed as
 * [n][16][h/2][w/2][C] - all that a 1x1x1 convolution of stride (1,2,2) (the stage's projection shortcut, resnet_helper.py:
 * 411-431) reads; its caller then runs that convolution with stride 1 over the packed tensor.  (ABI 3) */
int af_conv_cpa_fusable(const af_conv_desc* dc, const af_conv_desc* da, int x_sub);
int af_conv3d_cpa_bn_act(const af_conv_desc* dc, const void* in_b, const void* wc_packed, const float* scale_c, const float* shift_c,
                         const void* residual, void* out_x, int x_sub, const af_conv_desc* da, const void* wa_packed,
                         const float* scale_a, const float* shift_a, void* out_a, void* stream);

/* which tile variant af_conv3d_[dual_]bn_act launches for `d` (+ optional `d2`) (>= 0) and its kernel name:
 * lets a profiler attribute per-layer device time and FLOPs to a kernel instantiation (bench.py roofline). */
int af_conv_variant(const af_conv_desc* d, const af_conv_desc* d2);
const char* af_conv_variant_name(int variant);

/* what that launch is cut into: *units = the work units of the layer (strips of conv133, tiles of conv311 / conv111 / a conv_igemm
 * tile, units of conv133g / conv311g), *workgroups = the grid the launch has on the current device (256 CUs assumed where there is
 * none).  The specialised kernels are persistent - workgroup b walks units b, b + workgroups, ... (conv133: a contiguous range) - so
 * units / workgroups is how many units a workgroup runs one behind the other; a conv_igemm tile launches one workgroup per tile
 * (times the K ranges of a split, which depend on the caller's workspace and are not counted).  Both numbers come from the
 * launchers' own geometry: a test sizes its input from them instead of restating it.  Returns af_conv_variant(d, d2), or < 0
 * (the narrow-layer path is not cut into units). */
int af_conv_work_units(const af_conv_desc* d, const af_conv_desc* d2, int64_t* units, int* workgroups);

/* ... and how the fused launches are cut, from their launchers' own geometry, with no launch (256 CUs assumed where there is no
 * device).  Each takes the descriptors of its *_fusable predicate and returns that predicate's answer; the outputs are written only
 * when it is 1 (< 0: a NULL output pointer).
 *   af_conv3d_ca_bn_act:  *tiles of all T frames x *pixels pixels (256 / T) on *workgroups persistent workgroups - workgroup b walks
 *                         tiles b, b + workgroups, ... -, *form = the kernel instantiation: AF_CA_PLAIN, AF_CA_PLAIN_CWL (the c
 *                         weights as an LDS image) or AF_CA_PROJECTION (d1 != NULL);
 *   af_conv3d_cpa_bn_act: *tiles of 2 rows x 4 columns x all frames on *workgroups persistent workgroups;
 *   af_block_abc_bn_act:  one workgroup per unit = (clip, band of *patch_rows rows, 14 columns, one of *time_segments ranges of
 *                         frames). */
#define AF_CA_PLAIN 0
#define AF_CA_PLAIN_CWL 1
#define AF_CA_PROJECTION 2
int af_conv_ca_work_units(const af_conv_desc* dc, const af_conv_desc* d1, const af_conv_desc* da, int64_t* tiles, int* workgroups,
                          int* form, int* pixels);
int af_conv_cpa_work_units(const af_conv_desc* dc, const af_conv_desc* da, int x_sub, int64_t* tiles, int* workgroups);
int af_block_abc_work_units(const af_conv_desc* da, const af_conv_desc* db, const af_conv_desc* dc, const af_conv_desc* d1,
                            int* patch_rows, int* time_segments, int64_t* units);
/* device-free: the (frame, band) units, bands per frame and workgroups that the fused stems launch for d; fused = 1 for
 * af_stem_conv_bn_relu_maxpool, 2 for ..._rgb3[_ld]; answers for 256 CUs where there is no device (as af_conv_work_units).
 * A frame of fewer pooled rows than 8, or a launch of at least as many frames as CUs, has one band; otherwise bands of at least 4
 * pooled rows, the last one possibly shorter.  The launchers take their bands and their grid from the same function; workgroup b
 * walks units b, b + workgroups, ... (the K-packed stem on a grid that is a multiple of 8: a contiguous eighth of the units per
 * XCD).  AF_OK, or AF_ERR_ARG (added within ABI 6) */
int af_stem_work_units(const af_conv_desc* d, int fused, int64_t* units, int* bands, int* workgroups);

/* nn.MaxPool3d on NDHWC (stem_helper.py:168-170 [1,3,3]/[1,2,2]/[0,1,1];
 * video_model_builder.py:474-480 [2,1,1]/[2,1,1]); padding behaves as -inf. */
int af_maxpool3d(const af_pool_desc* d, const void* in, void* out, void* stream);

/* ResNetBasicHead (head_helper.py:74-95): AvgPool3d(pool,stride 1) -> Linear(c -> num_classes).
 * pooled (optional, may be NULL): fp32 [n][to*ho*wo][c] pooled features (the input of the
 * nn.Linear that feature.py:105-114 hooks); logits: fp32 [n][to*ho*wo*num_classes]. */
int af_avgpool_fc(const af_pool_desc* d, const void* in, const float* fc_w, const float* fc_b,
                  int num_classes, float* pooled, float* logits, void* stream);
/* the same with the callers' score epilogue fused behind the Linear (ClassifierSvc.infer_scores, test/af_realtime.py:88-95;
 * = TEST2.py:186-204, demo.py:328-331): scores[row] = sigmoid(logit) for num_classes == 1, softmax(logits)[1] for
 * num_classes == 2 (fp32 [n * to*ho*wo]); scores may be NULL. */
int af_avgpool_fc_scores(const af_pool_desc* d, const void* in, const float* fc_w, const float* fc_b,
                         int num_classes, float* pooled, float* logits, float* scores, void* stream);

/* The two halves of the head separately, for multi-pathway heads (SlowFast: one AvgPool3d per pathway, pooled
 * vectors concatenated by channel - head_helper.py:79-85 - then one Linear): af_avgpool writes row r of the pooled
 * result at pooled[r * pooled_ld + 0 .. c) (pass `pooled + channel_offset` to concatenate);
 * af_linear: y[r][k] = dot(x[r][0..in_features), w[k]) + b[k] on fp32. */
int af_avgpool(const af_pool_desc* d, const void* in, float* pooled, int pooled_ld, void* stream);
int af_linear(const float* x, const float* w, const float* b, int rows, int in_features, int out_features,
              float* y, void* stream);
int af_linear_scores(const float* x, const float* w, const float* b, int rows, int in_features, int out_features,
                     float* y, float* scores, void* stream);

/* ---- FTCN-TT plugin (reference model/classifier/i3d_temporal_var_fix_dropout_tt_cfg.py, time_transformer.py) ---- */

/* Temporal stem: Conv3d(3->64,[kt,1,1],stride 1,pad [kt/2,0,0]) + BN + MaxPool3d((1,2,2)) + ReLU - what
 * `temporal_only_conv` (:207-288) makes of ResNetBasicStem's conv / bn (stem_helper.py:156-178); d describes the conv
 * with to/ho/wo = t, h/2, w/2 (the pool is fused).  stem_in: af_pack_input_* buffer; out: NDHWC [n][t][h/2][w/2][64].
 * The stem's own MaxPool3d([1,3,3],[1,2,2],[0,1,1]) follows as af_maxpool3d - or rides along:
 * af_tstem_conv_bn_pool_relu_maxpool (ABI 3, 16-bit) takes the same descriptor and writes the stem pool's output
 * [n][t][(h/2-1)/2+1][(w/2-1)/2+1][64] directly (the half-resolution tensor never exists; i3d_temporal_var_fix_dropout_tt_cfg.py
 * keeps ResNetBasicStem's pool_layer behind the converted conv / bn). */
int af_pack_tstem_weight(const float* w_oidhw, int cout, int kt, int dtype, void* out, void* stream);
long long af_packed_tstem_weight_bytes(int dtype);
int af_tstem_conv_bn_pool_relu(const af_conv_desc* d, const void* stem_in, const void* w_packed, const float* scale,
                               const float* shift, void* out, void* stream);
int af_tstem_conv_bn_pool_relu_maxpool(const af_conv_desc* d, const void* stem_in, const void* w_packed, const float* scale,
                                       const float* shift, void* out, void* stream);

/* TimeTransformer head (time_transformer.py:219-281), fp32.  The Linear layers are af_conv3d_bn_act over the token
 * rows (1x1x1, AF_F32, scale = ones, shift = bias, residual = the skip connection).
 * af_tokens_assemble: out[b][0] = cls + pos[0], out[b][1+t] = pooled[b][t] + pos[1+t]   (:270-273)
 * af_layernorm: nn.LayerNorm(dim) over `rows` rows (PreNorm :15-21; mlp_head :259), row strides in elements
 * af_attention: softmax(q k^T / sqrt(dim_head)) v per (clip, head), qkv rows = [q | k | v] (Attention.forward :52-71)
 * af_gelu: nn.GELU() (erf form) in place (FeedForward :27) */
int af_tokens_assemble(const float* pooled, const float* cls_token, const float* pos_embedding, int clips, int n_tok,
                       int dim, float* out, void* stream);
int af_layernorm(const float* x, long long x_row_stride, const float* gamma, const float* beta, int rows, int dim,
                 float eps, float* y, long long y_row_stride, void* stream);
int af_attention(const float* qkv, int clips, int n_tok, int heads, int dim_head, float* out, void* stream);
int af_gelu(float* x, long long n, void* stream);

/* ---- dualrun AU / landmark dual encoder (reference dualrun/model/dual_encoder.py) --------------------- */

/* BranchEncoder.forward (:73-107) of `branches` modalities (AU, landmarks, ...) for `clips` clips of `frames` <= 16
 * frames, fp32, ONE launch (grid = clips x branches): x[b] [clips][frames][din[b]]; lengths [clips] valid frames (NULL:
 * all; 0 counts as 1 like :162-166); pe [frames][d_model] sinusoidal table (:16-23);
 * z[clip * z_ld + b * d_model + 0..d_model) = the attention-pooled clip vector of branch b (already concatenated).
 * weights[b] is the flat fp32 image af_dual_branch_weight_floats() sizes: proj W^T, b | ln_in g, b | 3 x (depthwise
 * w [c][3], b) | pointwise W^T, b | per layer: norm1 g, b | in_proj W^T, b | out_proj W^T, b | norm2 g, b | linear1
 * W^T, b | linear2 W^T, b | pool v   (W^T = [in][out], af_transpose_f32 of the checkpoint's [out][in]). */
long long af_dual_branch_weight_floats(int din, int d_model, int depth, int ff);
int af_transpose_f32(const float* src, int rows, int cols, float* dst, void* stream);
int af_dual_branch_encoders(int branches, const float* const* x, const float* const* weights, const int* din,
                            const int* lengths, const float* pe, int clips, int frames, int d_model, int depth, int heads,
                            int ff, float pool_tau, float* z, int z_ld, void* stream);
/* DualEncoderAU_LMK.head (:115-121): LayerNorm(n) -> Linear(n,n) -> GELU -> Linear(n,1) on z [clips][n];
 * weights: gamma, beta, W1^T [n][n], b1, w2 [n], b2. */
int af_dual_head(const float* z, const float* weights, int clips, int n, float* logits, void* stream);

/* dualrun tri-modal model (reference dualrun/model/dual_rgb.py).
 * af_masked_mean_proj: AltFreezingRGBEncoder.forward with from_features (:27-44) + rgb_proj (:70, Linear without bias):
 *   v [clips][tv][vis] per-frame / per-window RGB features (the AltFreezing backbone's pooled 2048-vector, feature.py:105-114);
 *   lengths [clips] = valid frames of a key-padding mask over `tmask` frames (NULL: no mask = plain mean); tv == tmask, or
 *   tv == 1 (broadcast against the mask like torch does); wt = rgb_proj.weight^T [vis][d];
 *   z[clip * z_ld + 0..d) = (sum_t v[t] * valid[t] / max(sum valid, 1e-6)) @ wt.
 * af_mlp_head: DualEncoderRGB.head (:75-79) = LayerNorm(n) -> Linear(n, hidden) -> GELU -> Linear(hidden, 1) on z [clips][n];
 *   weights: gamma [n], beta [n], W1^T [n][hidden], b1 [hidden], w2 [hidden], b2; scores (optional) = sigmoid(logit).
 *   (af_dual_head is the hidden == n case without scores.) */
int af_masked_mean_proj(const float* v, int clips, int tv, int vis, const int* lengths, int tmask, const float* wt, int d,
                        float* z, int z_ld, void* stream);
int af_mlp_head(const float* z, const float* weights, int clips, int n, int hidden, float* logits, float* scores, void* stream);

/* GatedMoE.forward (dualrun/rgb/engine_rgb.py:369-384): fuses the RGB (AltFreezing) logit and the dual-encoder logit of n
 * clips: gate = sigmoid(W2 relu(W1 [z_rgb, z_dual, |z_rgb - z_dual|] + b1) + b2), p = gate * sigmoid(z_rgb / max(t_rgb, 1))
 * + (1 - gate) * sigmoid(z_dual / max(t_dual, 0.1)), z = logit(p) with eps 1e-6.  weights: t_rgb, t_dual, W1 [hidden][3],
 * b1, w2 [hidden], b2. */
int af_gated_moe(const float* z_rgb, const float* z_dual, const float* weights, int hidden, int n, float* z, float* gate,
                 void* stream);

/* ---- dualrun at video level: raw landmark / AU tracks -> clip features, clip logits -> track and video verdicts ---- */

/* One face track on the device: lmk = n rows of P >= 467 (x, y) fp32 points, a row every lmk_pitch >= 934 floats; au = n rows of
 * K fp32 action units (columns in the reference's sorted-key order), a row every au_pitch >= K floats. */
typedef struct af_dualv_track {
    const float* lmk;
    const float* au;
    int64_t lmk_pitch;
    int32_t au_pitch;
    int32_t n;
} af_dualv_track;

/* One clip: frames first .. first + len - 1 of track `track`, 1 <= len <= 16. */
typedef struct af_dualv_clip {
    int32_t track, first, len, reserved;
} af_dualv_clip;

#define AF_DUALV_MAX_T 16
#define AF_DUALV_LMK_DIM 132
#define AF_DUALV_MIN_POINTS 467      /* the key set reaches index 466 (make_lmk_features.py:52 computes it; its comment says 309) */
#define AF_DUALV_ZSCORE_NONE 0
#define AF_DUALV_ZSCORE_CLIP 1
#define AF_DUALV_ZSCORE_GLOBAL 2
#define AF_DUALV_APPLY_BOTH 0
#define AF_DUALV_APPLY_AU 1
#define AF_DUALV_APPLY_LMK 2

typedef struct af_dualv_opts {
    int32_t frames;                 /* T: rows per clip handed to the encoder, 1..16            */
    int32_t au_k;                   /* K raw action units per frame                             */
    int32_t zscore_mode;            /* AF_DUALV_ZSCORE_*                                        */
    int32_t zscore_apply;           /* AF_DUALV_APPLY_*                                         */
    int32_t use_delta, use_delta2;  /* append diff(X) / diff(diff(X)): F_au = K * (1 + d + d2)  */
    const float* au_mean;           /* [F_au], [F_au], [132], [132] device vectors: all four in */
    const float* au_std;            /* global mode, ignored otherwise                           */
    const float* lmk_mean;
    const float* lmk_std;
} af_dualv_opts;

/* dualrun's feature path per clip, ONE launch (grid = clips): make_lmk_features._seq_to_features (the 66 key points centred on
 * the nose, divided by ||mouth left - mouth right|| + 1e-6; a frame whose scale is not finite or < 1e-8 is dropped and the rest
 * compacted), make_au_features.seq_au_to_features (X | diff | diff of diff, each with its first row prepended), fixT per modality
 * (centre crop / repeat the last row) and fusion.normalize_features (clip: mean and unbiased std over the T rows, clamp 1e-6;
 * global: the given vectors, std floored at 1e-6; nan_to_num in both; none: untouched).  tracks [n_tracks] and clips [n_clips]
 * are DEVICE tables.  A [n_clips][T][F_au], L [n_clips][T][132], nvalid [n_clips] = landmark frames that survived; a clip
 * with none (or a clip record that leaves its track) gets nvalid 0 and zeros.  Arithmetic and its order: tests/dualvideo_ref.py. */
int af_dual_clip_features(const af_dualv_track* tracks, int n_tracks, const af_dualv_clip* clips, int n_clips,
                          const af_dualv_opts* opts, float* A, float* L, int32_t* nvalid, void* stream);

#define AF_DUALV_FAMILY_FUSION 0    /* fusion.track_reduce / agg_video on logits                 */
#define AF_DUALV_FAMILY_BEST 1      /* best.aggregate_video_predictions on sigmoid(logit)        */
#define AF_DUALV_TRACK_MEDIAN 0     /* fusion family: torch.median (the lower middle value)      */
#define AF_DUALV_TRACK_MEAN 1
#define AF_DUALV_VIDEO_MAX 0
#define AF_DUALV_VIDEO_MEDIAN 1
#define AF_DUALV_VIDEO_MEAN 2
#define AF_DUALV_BEST_TRACK_MEAN 0  /* best family: track_mode                                   */
#define AF_DUALV_BEST_TRACK_MEDIAN 1 /* np.median: the midpoint on an even count, fp64           */
#define AF_DUALV_BEST_TRACK_MAJORITY 2

/* Clip logits -> track and video verdicts, ONE launch (grid = videos).  video_tracks [videos + 1]: video v owns tracks
 * video_tracks[v] .. video_tracks[v + 1] - 1; track_clips [tracks + 1]: track t owns clip_index[track_clips[t] ..
 * track_clips[t + 1] - 1], clip numbers < clips in input order.  Clips with nvalid == 0 are skipped, a track left with none is
 * skipped (track_count 0), a video left with none gets NaN (fusion) or score 0, pred 0 (best).  sigmoid = fp32(1 / (1 + exp(-x)))
 * evaluated in fp64.  Fusion family writes track_logit, track_prob [tracks], video_logit, video_prob [videos]; best family
 * writes clip_prob [clips] (sigmoid of every clip the CSR names: best.py's y_score_clip), track_score [tracks] (fp64), track_pred
 * [tracks], video_score [videos] (fp64), video_pred [videos]; both write
 * track_count [tracks] = clips used.  Means are sequential sums in input order (fp32 for fusion, fp64 for best). */
int af_dual_video_reduce(const float* logits, const int32_t* nvalid, int clips, const int32_t* video_tracks, int videos,
                         const int32_t* track_clips, int tracks, const int32_t* clip_index, int family, int track_mode,
                         int video_mode, double prob_thresh, float* track_logit, float* track_prob, float* video_logit,
                         float* video_prob, float* clip_prob, double* track_score, int32_t* track_pred, double* video_score,
                         int32_t* video_pred, int32_t* track_count, void* stream);

/* ---- cli/test.py's LMKDisc path: landmarks alone, ragged clips, the mouth-line rotation, noisy-OR ---- */

#define AF_DUALV_PAD_FIXT 0         /* VideoDataset._fixT: what af_dual_clip_features does                         */
#define AF_DUALV_PAD_ZERO 1         /* vox_ds.collate_pad: the nvalid surviving rows, then T - nvalid rows of +0.0 */

/* af_dual_clip_features with two options and an optional A.  rot_invariant = 1 is make_lmk_features.py's --rot-invariant
 * (_frame_to_features / _rotate_to_mouth), applied to every surviving frame before padding and z-score: with (x, y) a normalised
 * point and dx, dy = mr_c - ml_c in fp32, c = dx / h and s = -dy / h, h = sqrt(dx dx + dy dy), evaluated in fp64 and rounded to
 * fp32 once (c = 1, s = 0 when dx = dy = 0); x' = fl(fl(x c) + fl(y (-s))), y' = fl(fl(x s) + fl(y c)).  A == NULL: landmarks
 * alone; au_k, the delta flags, the AU statistics and the tracks' au pointers are not read.  AF_DUALV_PAD_ZERO needs A == NULL and
 * AF_DUALV_ZSCORE_NONE; a clip longer than T is then a bad record (nvalid 0, zeros).  rot_invariant = 0 with AF_DUALV_PAD_FIXT
 * and A given equals af_dual_clip_features bit for bit.  Arithmetic and its order: tests/lmkdisc_ref.py. */
int af_dual_clip_features_ex(const af_dualv_track* tracks, int n_tracks, const af_dualv_clip* clips, int n_clips,
                             const af_dualv_opts* opts, int rot_invariant, int pad_mode, float* A, float* L, int32_t* nvalid,
                             void* stream);

/* cli/test.py:86-94, 205-256 on clip logits, ONE launch (grid = videos), the CSR of af_dual_video_reduce (every track is its own
 * entry: test.py keys by track path).  clip_score [clips] (fp64) = sigmoid(logit) as af_dual_video_reduce defines it, or
 * 1.0 - it with invert, for every clip the CSR names; track_score [tracks] = np.median of the scores of its clips with
 * nvalid > 0 (the midpoint on an even count), track_pred = score >= thresh, track_count = clips used (a track with none: score
 * 0, pred 0, and it is skipped); video_score [videos] = 1 - exp(sum_t log1p(-clip(track_score_t, 1e-6, 1 - 1e-6))), summed in
 * CSR order in fp64, 0.0 for a video left with no track; video_pred = score >= thresh; video_count [videos] = tracks used. */
int af_lmk_video_reduce(const float* logits, const int32_t* nvalid, int clips, const int32_t* video_tracks, int videos,
                        const int32_t* track_clips, int tracks, const int32_t* clip_index, int invert, double thresh,
                        double* clip_score, double* track_score, int32_t* track_pred, int32_t* track_count, double* video_score,
                        int32_t* video_pred, int32_t* video_count, void* stream);

/* ---- clip aligner --------------------------------------------------- */

/* Replaces the per-frame loop of FasterCropAlignXRay.__call__ / process_single
 * (altfreezing/test_tools/faster_crop_align_xray.py:62-66, 75-88):
 *     new_image = zeros((h, w, 3), uint8); new_image[y:y+ih, x:x+iw] = image; cv2.warpAffine(new_image, tfm, (size, size))
 * for the n_frames frames of one clip in one launch.  `crops`: device buffer holding the frames' HxWx3 uint8 crops
 * (tightly packed rows), frame i at byte `frames[i].offset`; `frames` (HOST memory, copied into the launch): crop size
 * (ih, iw) and paste position (x, y) on the h x w canvas - a crop that does not fit the canvas is an error, as numpy's
 * slice assignment is in the reference; `tfm`: the forward 2x3 matrix (host, row-major doubles) as passed to
 * cv2.warpAffine; `out`: device (n_frames, size, size, 3) uint8 - the layout af_pack_input_u8 takes.
 * Arithmetic: OpenCV's fixed-point INTER_LINEAR / BORDER_CONSTANT(0) warp (see csrc/af_align.hip). */
#define AF_ALIGN_MAX_FRAMES 64
typedef struct af_align_frame {
    int64_t offset;
    int32_t ih, iw;
    int32_t x, y;
} af_align_frame;
int af_warp_affine_clip_u8(const void* crops, const af_align_frame* frames, int n_frames, int canvas_h, int canvas_w,
                           const double* tfm, int size, void* out, void* stream);

/* Host-side staging for the aligner (no device work): copies n rectangles of uint8 rows (the part of each crop the warp can
 * sample) into one staging buffer, one memcpy per row.  dst_offset / rows / row_bytes describe the packed destination,
 * src_pitch the source's row pitch in bytes.  (ABI 3) */
typedef struct af_stage_rect {
    const void* src;
    int64_t dst_offset;
    int64_t src_pitch;
    int32_t rows, row_bytes;
} af_stage_rect;
int af_stage_rows_u8(void* dst, const af_stage_rect* rects, int n);

/* Host-side planning of ONE clip for the aligner (no device work; ABI 4): what FasterCropAlignXRay.__call__ does per frame between the
 * similarity fit and the warp (reference altfreezing/test_tools/faster_crop_align_xray.py:75-88: paste every crop on the common
 * canvas, warp), as one call instead of a Python loop per frame.  crops[i]: the HxWx3 uint8 crop (first byte, row pitch in bytes -
 * pixels of a row contiguous - height, width) and its paste offset (x, y) on the canvas_w x canvas_h canvas; tfm: the forward 2x3
 * matrix; size: the output edge.  Checks that every crop fits the canvas (AF_ERR_ARG with the frame in *bad_frame: numpy's slice
 * assignment raises there in the reference), cuts each crop to the rows the size x size destination can sample (bilinear taps +
 * fixed-point rounding: 3 pixels of margin; a crop cut to rows [r0, r1) is that shorter crop pasted r0 rows lower) and fills
 * rects[i] (what af_stage_rows_u8 copies into the staging buffer, 16-byte aligned pieces), frames[i] (what af_warp_affine_clip_u8
 * reads) and *total_bytes (staging bytes used). */
typedef struct af_align_crop {
    const void* src;
    int64_t pitch;
    int32_t h, w;
    int32_t x, y;
} af_align_crop;
int af_align_plan_u8(const af_align_crop* crops, int n, int canvas_h, int canvas_w, const double* tfm, int size,
                     af_stage_rect* rects, af_align_frame* frames, int64_t* total_bytes, int32_t* bad_frame);

/* Window-batch warp: the offline evaluator's clip loop (altfreezing/demo.py:304-339) aligns EVERY clip_size-frame window of a face
 * track, stride 1, so consecutive windows share all but one crop.  The crops of the track sit once in a caller-owned device pool;
 * one launch warps up to AF_WINDOW_MAX_BATCH windows x clip_size frames out of it into `out`, device (n_windows, clip_size, size,
 * size, 3) uint8 - the layout af_pack_input_u8 takes.  Same arithmetic as af_warp_affine_clip_u8, bit for bit.
 *
 * af_window_batch_plan_u8 (host only, no device work) fills the launch's table into `table`, a caller-owned HOST buffer (pinned,
 * for an asynchronous copy) of af_window_batch_table_bytes(n_windows, clip_size) bytes, 8-byte aligned; the caller copies it to
 * the device and hands af_warp_affine_windows_u8 the device copy with the same n_windows / clip_size / size.  The library
 * allocates nothing.
 *   windows[w]: the forward 2x3 matrix as passed to cv2.warpAffine (inverted here in OpenCV's order of operations) and the canvas;
 *   frames[w * clip_size + t]: byte offset of the frame's HxWx3 crop (tightly packed rows) in the pool, its size, its paste
 *     position on window w's canvas.  A crop that does not fit its window's canvas is AF_ERR_ARG with *bad_window / *bad_frame
 *     set (numpy's slice assignment raises there in the reference); 3 readable bytes must follow every crop (pool_bytes is checked:
 *     the kernel reads the two taps of a source row as 6 bytes and gives a tap outside the crop weight 0);
 *   size: a multiple of 4, at most AF_WINDOW_MAX_SIZE.
 * What the launch cannot check: the table is device memory, so af_warp_affine_windows_u8 trusts its offsets, crop sizes and paste
 * positions as the planner wrote them - hand it only a copy of a table af_window_batch_plan_u8 filled for this pool.  The kernel
 * compares the table's header with n_windows / clip_size / size and writes nothing on a mismatch; the call still returns AF_OK and
 * `out` keeps its old contents, which the caller cannot detect - plan and launch with the same three numbers. */
#define AF_WINDOW_MAX_BATCH 64
#define AF_WINDOW_MAX_SIZE 1024
typedef struct af_window_desc {
    double tfm[6];
    int32_t canvas_h, canvas_w;
} af_window_desc;
int64_t af_window_batch_table_bytes(int n_windows, int clip_size);
int af_window_batch_plan_u8(const af_window_desc* windows, const af_align_frame* frames, int n_windows, int clip_size, int size,
                            int64_t pool_bytes, void* table, int64_t table_bytes, int32_t* bad_window, int32_t* bad_frame);
int af_warp_affine_windows_u8(const void* pool, const void* table, int n_windows, int clip_size, int size, void* out, void* stream);

/* The window-batch warp out of RESIDENT FRAMES: the same launch, but every (window, frame) reads its crop as a sub-rectangle of a
 * decoded frame that already sits in a caller-owned device frame store (the frames a detector has just read), so no crop is cut,
 * staged or uploaded.  Same arithmetic and the same bytes as af_warp_affine_windows_u8 on crops cut from those frames.
 *   store: n_frames frames of height x width RGB pixels (3 packed bytes), frame i at byte i * frame_stride, rows row_pitch bytes
 *     apart (any value >= 3 * width, no alignment asked: 1 923 for a 641-wide frame); store_bytes: the readable bytes of the buffer.
 *   rects[w * clip_size + t]: the frame's index in the store, the rectangle's top-left pixel (rx, ry) and size (ih, iw) in that
 *     frame, and its paste position (x, y) on window w's canvas.
 * af_window_rects_plan_u8 (host only) fills the table (af_window_rects_table_bytes bytes, 8-byte aligned) and refuses with
 * AF_ERR_ARG: a rectangle that does not fit its window's canvas (*bad_window / *bad_frame set, as af_window_batch_plan_u8 does); a
 * rectangle that leaves its frame or names a frame outside the store; a rectangle whose last pixel is followed by fewer than 3
 * readable bytes.  Inside a frame those bytes are the frame's next pixels, so this only asks for 3 bytes of slack behind the last
 * frame of the store.  The kernel reads tap pairs as 6 bytes from an address clamped into the rectangle and gives a tap outside the
 * rectangle weight 0: the pixels next to a rectangle never reach the result.
 * The launch trusts the table as af_warp_affine_windows_u8 does, compares the header (a table of the pool form is a mismatch too)
 * and writes nothing on a mismatch.  (Added within ABI 6, like the pool form.)
 * Widened since, with af_window_rects_plan_stores_u8, whose planner this now shares: EVERY refusal of one (window, frame) - not the
 * canvas misfit alone - sets *bad_window / *bad_frame, and a refused table's header is stamped so that no launch takes it; a caller
 * that read bad_window >= 0 as "canvas misfit" must look at the named rectangle, or at af_last_error, first. */
typedef struct af_frame_store {
    int64_t store_bytes;
    int64_t frame_stride, row_pitch;
    int32_t n_frames, height, width, reserved;
} af_frame_store;
typedef struct af_frame_rect {
    int32_t frame;
    int32_t rx, ry;
    int32_t ih, iw;
    int32_t x, y;
    int32_t reserved;
} af_frame_rect;
int64_t af_window_rects_table_bytes(int n_windows, int clip_size);
int af_window_rects_plan_u8(const af_window_desc* windows, const af_frame_rect* rects, int n_windows, int clip_size, int size,
                            const af_frame_store* store, void* table, int64_t table_bytes, int32_t* bad_window, int32_t* bad_frame);
int af_warp_affine_window_rects_u8(const void* store, const void* table, int n_windows, int clip_size, int size, void* out, void* stream);
/* The same launch for a store whose pixels are B, G, R in memory (cv2.VideoCapture, a screen capture, what YuNet takes): the byte at
 * row * row_pitch + col * 3 is B, and `out` is still R, G, B - the bytes af_warp_affine_window_rects_u8 writes for the store with
 * every pixel's first and third byte exchanged.  Same table (af_window_rects_plan_u8 plans for both), same argument check, same
 * reads; the exchange is a choice of which accumulated channel goes to which byte of the store.  (Added within ABI 6.) */
int af_warp_affine_window_rects_bgr_u8(const void* store, const void* table, int n_windows, int clip_size, int size, void* out, void* stream);

/* The quality gate's pixel part for every face of a frame in ONE launch, out of rectangles of resident frames: the reference's
 *     small = cv2.resize(crop, (max(1, w // 2), max(1, h // 2)), interpolation=cv2.INTER_AREA)
 *     lap   = cv2.Laplacian(cv2.cvtColor(small, cv2.COLOR_RGB2GRAY), cv2.CV_64F).var()
 * (test/af_realtime.py:265-267, :191-192) as three exact integers per rectangle; the arithmetic is stated in csrc/af_quality.hip.
 *   store / desc: the frame store as for the window warp (device pixels, host description); no slack bytes are asked for;
 *   rects[i]: HOST array; frame, (rx, ry) and (ih, iw) name the rectangle, x / y / reserved are not read;
 *   bgr: 0 - a pixel's bytes are R, G, B; non-zero - B, G, R;
 *   sums: DEVICE array of n records: n_px = dw * dh, s1 = sum of the Laplacian, s2 = sum of its squares over the half-size grey
 *     image (dw = max(1, iw / 2), dh = max(1, ih / 2)); the variance is (n_px * s2 - s1 * s1) / n_px^2.  Cleared and filled on
 *     `stream`; integer sums, so identical from run to run whatever the order of the rectangles;
 *   grey: null, or (tests) a DEVICE buffer of grey_bytes >= sum of dw * dh bytes that receives the grey images one behind the other.
 * AF_ERR_ARG: more than AF_QUALITY_MAX_RECTS rectangles, a rectangle that leaves its frame or names a frame outside the store.
 * (Added within ABI 6.) */
#define AF_QUALITY_MAX_RECTS 64
typedef struct af_quality_sums {
    int64_t s1, s2;
    int32_t n_px, reserved;
} af_quality_sums;
int af_face_quality_u8(const void* store, const af_frame_store* desc, const af_frame_rect* rects, int n, int bgr, af_quality_sums* sums,
                       void* grey, int64_t grey_bytes, void* stream);

/* ---- several frame stores in one launch (added within ABI 6) ------------------------------------------------------------------
 * A server that steps many live calls keeps one frame store per call; these forms of the window warp and of the quality gate read
 * from up to AF_MAX_STORES stores in one launch.  A store is named by its device base pointer, its description and its byte order
 * (bgr: 0 - a pixel's bytes are R, G, B; non-zero - B, G, R); af_frame_rect.reserved is the index of a rectangle's store in `stores`
 * (a HOST array).  The per-store checks are those of the single-store forms; a store index outside [0, n_stores) is AF_ERR_ARG.
 *
 * af_window_rects_plan_stores_u8 (host only) fills a table of af_window_rects_table_bytes(n_windows, clip_size) bytes whose items
 * carry the absolute address of their rectangle's first pixel, its row pitch and its byte order; its `kind` differs from the pool
 * and the single-store forms, so af_warp_affine_window_stores_u8 writes nothing for a table of another form, and the other
 * launches write nothing for this one.  A refusal of one (window, frame) - canvas misfit, a rectangle that leaves its frame or its
 * store, fewer than 3 readable bytes behind a rectangle that ends its store, a bad store index - sets *bad_window / *bad_frame.
 * The output bytes of a window equal those of af_warp_affine_window_rects_u8 / _bgr_u8 on that window's store. */
#define AF_MAX_STORES 64
typedef struct af_store_ref {
    const void* base;              /* device pointer of the store's first byte */
    af_frame_store desc;
    int32_t bgr, reserved;
} af_store_ref;
int af_window_rects_plan_stores_u8(const af_window_desc* windows, const af_frame_rect* rects, int n_windows, int clip_size, int size,
                                   const af_store_ref* stores, int n_stores, void* table, int64_t table_bytes, int32_t* bad_window,
                                   int32_t* bad_frame);
int af_warp_affine_window_stores_u8(const void* table, int n_windows, int clip_size, int size, void* out, void* stream);
/* af_face_quality_u8 over rectangles of several stores: the same integer sums and grey bytes, rectangle i out of
 * stores[rects[i].reserved].  At most AF_QUALITY_MAX_RECTS rectangles and AF_MAX_STORES stores per launch. */
int af_face_quality_stores_u8(const af_store_ref* stores, int n_stores, const af_frame_rect* rects, int n, af_quality_sums* sums,
                              void* grey, int64_t grey_bytes, void* stream);
/* The same kernel in its full-size mode: the Laplacian sums of every rectangle AS IT IS, without the INTER_AREA half-size stage -
 * the second measurement the dataset evaluator takes of a crop (altfreezing/TEST2.py:296-299: variance_of_laplacian(crop_rgb) into
 * _qstat).  dw = iw, dh = ih, n_px = iw * ih; grey, Laplacian, sums, grey bytes (sum of iw * ih) and every refusal are those of
 * af_face_quality_stores_u8.  (Added within ABI 6.) */
int af_face_laplacian_stores_u8(const af_store_ref* stores, int n_stores, const af_frame_rect* rects, int n, af_quality_sums* sums,
                                void* grey, int64_t grey_bytes, void* stream);

/* ---- YUV 4:2:0 frames into frame stores (added within ABI 6) ---------------------------------------------------------------------
 * What a WebRTC stack (I420), a hardware decoder (NV12) or ffmpeg (yuv420p) hands over, converted on the device straight into slots
 * of frame stores: one launch converts up to AF_YUV_MAX_FRAMES frames that may differ in size, format, destination store and byte
 * order.  Arithmetic: OpenCV's cvtColor(..., COLOR_YUV2BGR_NV12 / _I420) - fixed-point BT.601, limited range, integer only, one
 * (U, V) per 2 x 2 block of Y without interpolation; stated in csrc/af_yuv.hip and equal, byte for byte, to the numpy restatement
 * tests/yuv_ref.py (unpinned against cv2 itself, absent where this is built).  Other layouts, depths and colours: af_yuv_to_rgb_ex_u8
 * below.
 *
 * af_yuv_frame (host description of one frame): y - DEVICE pointer of the Y plane, h rows of w bytes y_pitch apart; u - the first
 * chroma plane: the interleaved plane (h / 2 rows of w bytes) when `interleaved`, else the first of two planes of h / 2 rows of
 * w / 2 bytes, v the second; c_pitch - the row pitch of the chroma plane(s); swap_uv - the first chroma byte / plane is V (NV21,
 * YV12 in memory order); (store, slot) - the destination: slot `slot` of stores[store], whose height and width must be h and w.
 * af_yuv420_plan_u8 (host only, no device work) fills items[0 .. n) and refuses with AF_ERR_ARG: odd or non-positive h or w, a pitch
 * shorter than its row, a store index outside [0, n_stores), a store of another frame size, a slot that does not lie wholly inside
 * its store (store_bytes is checked), n above AF_YUV_MAX_FRAMES.  An item carries the absolute address of its destination's first
 * byte, the pitches, the flags (bgr: the store's byte order) and first_tile, the prefix sum of the tiles of the items before it.
 * af_yuv420_to_rgb_u8 takes a HOST table the planner filled (it travels to the kernel by value), checks sizes, pitches and the
 * first_tile prefix again and trusts the pointers.  The kernel reads no byte outside [plane, plane + pitch * (rows - 1) + row bytes)
 * and writes exactly the h * w * 3 bytes of each destination frame, whatever the alignment of planes, pitches and destination rows;
 * the planes must be ready on `stream` and stay unchanged until the launch has run. */
#define AF_YUV_MAX_FRAMES 64
typedef struct af_yuv_frame {
    const void* y;
    const void* u;
    const void* v;
    int64_t y_pitch, c_pitch;
    int32_t h, w;
    int32_t interleaved, swap_uv;
    int32_t store, slot;
} af_yuv_frame;
typedef struct af_yuv_item {
    const void* y;
    const void* c0;
    const void* c1;
    void* dst;
    int32_t y_pitch, c_pitch, dst_pitch;
    int32_t first_tile;
    uint16_t h, w;
    uint8_t interleaved, swap_uv, bgr, reserved;
} af_yuv_item;
int af_yuv420_plan_u8(const af_yuv_frame* frames, int n, const af_store_ref* stores, int n_stores, af_yuv_item* items);
int af_yuv420_to_rgb_u8(const af_yuv_item* items, int n, void* stream);

/* ---- YUV frames of more layouts, depths and colours into frame stores (added within ABI 6) -------------------------------------------
 * af_yuv420_to_rgb_u8's launch for what webcams (packed 4:2:2), MJPEG decoders (full range, planar 4:2:2 / 4:4:4), HD decoders (BT.709)
 * and 10-bit decoders (P010) hand over: one launch converts up to AF_YUV_MAX_FRAMES frames that may differ in size, layout, bit depth,
 * colour matrix, range, destination store and byte order.  It also converts the four 4:2:0 layouts of the launch above, to the same
 * bytes at colour 0.  Nothing is interpolated: a (U, V) serves its 2 x 2, 2 x 1 or single pixel(s).  The output is 8-bit.
 *
 * layout (AF_YUV_LAYOUT_*)   planes                                                             chroma
 *   420P   i420 / yv12       y (h, w), u, v (h / 2, w / 2)                                      2 x 2
 *   420SP  nv12 / nv21       y (h, w), u = interleaved (h / 2, w)                               2 x 2
 *   422P   i422              y (h, w), u, v (h, w / 2)                                          2 x 1
 *   422SP  nv16              y (h, w), u = interleaved (h, w)                                   2 x 1
 *   444P   i444              y, u, v (h, w)                                                     1 x 1
 *   422PK  yuy2 uyvy yvyu    y = one packed plane (h, 2 w): 4 bytes per pixel pair              2 x 1
 *   420SP16 p010             y (h, w), u = interleaved (h / 2, w) of uint16, value = v >> 6     2 x 2
 *   420P16  i010             y (h, w), u, v (h / 2, w / 2) of uint16, value = min(v, 1023)      2 x 2
 * order: planar and semi-planar layouts - 0: U is the first chroma byte / plane, 1: V is; 422PK - 0: Y0 U Y1 V, 1: U Y0 V Y1,
 * 2: Y0 V Y1 U.  w is even; h is even where chroma is halved vertically; pitches are in bytes; the planes and pitches of the uint16
 * layouts are even.  matrix - 0: BT.601, 1: BT.709; full_range - 0: limited (Y 16..235, or 64..940), 1: full.
 *
 * Arithmetic: OpenCV's form (color_yuv.simd.hpp), int32 with an arithmetic shift:
 *     y = max(0, Y - Yoff) * CY;  u = U - Cmid;  v = V - Cmid
 *     R = clamp((y + 2^19 + CVR v) >> 20)   G = clamp((y + 2^19 + CVG v + CUG u) >> 20)   B = clamp((y + 2^19 + CUB u) >> 20)
 * Yoff: 16 (limited 8-bit), 64 (limited 10-bit), 0 (full); Cmid: 128 or 512.  Row 0 of AF_YUV_COLOUR_TABLES is OpenCV's own table
 * (BT.601, limited, 8-bit), so the packed 4:2:2 layouts at colour 0 are OpenCV's COLOR_YUV2BGR_YUY2 / _UYVY / _YVYU.  Every other row
 * is this library's: from Kr, Kb = 0.299, 0.114 (BT.601) or 0.2126, 0.0722 (BT.709) as exact rationals, scaled by 255/219 and 255/224
 * (limited 8-bit), 255/876 and 255/896 (limited 10-bit), 1 (full 8-bit) or 255/1023 (full 10-bit), each coefficient rounded half up
 * to 2^-20.  Rows: { CY, CVR, CVG, CUG, CUB } at index 4 * ten_bit + 2 * full_range + matrix.  Stated in numpy by
 * tests/yuv_formats_ref.py, which re-derives the rows.
 *
 * af_yuv_plan_ex_u8 (host only) fills items[0 .. n) and refuses, with AF_ERR_ARG, what af_yuv420_plan_u8 refuses and an unknown
 * layout, order, matrix or range, and an odd address or pitch of a uint16 plane.  af_yuv_to_rgb_ex_u8 takes the HOST table (it travels
 * to the kernel by value), checks codes, sizes, pitches and the first_tile prefix again and trusts the pointers.  The kernel reads no
 * byte outside [plane, plane + pitch * (rows - 1) + row bytes) and writes exactly the h rows of 3 w bytes of each destination frame.
 * Not built: NV24 / NV42, packed 10-bit, 12-bit, BT.2020, chroma siting / interpolation. */
#define AF_YUV_LAYOUT_420P 0
#define AF_YUV_LAYOUT_420SP 1
#define AF_YUV_LAYOUT_422P 2
#define AF_YUV_LAYOUT_422SP 3
#define AF_YUV_LAYOUT_444P 4
#define AF_YUV_LAYOUT_422PK 5
#define AF_YUV_LAYOUT_420SP16 6
#define AF_YUV_LAYOUT_420P16 7
#define AF_YUV_LAYOUTS 8
#define AF_YUV_COLOUR_TABLES                                                                                  \
    {                                                                                                         \
        {1220542, 1673527, -852492, -409993, 2116026},     /* BT.601 limited  8-bit: OpenCV's */             \
        {1220945, 1879825, -558796, -223607, 2215014},     /* BT.709 limited  8-bit */                       \
        {1048576, 1470104, -748826, -360853, 1858077},     /* BT.601 full     8-bit */                       \
        {1048576, 1651297, -490864, -196424, 1945738},     /* BT.709 full     8-bit */                       \
        {305236, 418389, -213115, -102698, 528805},        /* BT.601 limited 10-bit */                       \
        {305236, 469956, -139699, -55902, 553753},         /* BT.709 limited 10-bit */                       \
        {261375, 366448, -186658, -89949, 463157},         /* BT.601 full    10-bit */                       \
        {261375, 411614, -122356, -48962, 485008},         /* BT.709 full    10-bit */                       \
    }
typedef struct af_yuv_frame_ex {
    const void* y;                 /* DEVICE pointers: the Y plane, or the packed plane of 422PK */
    const void* u;                 /* the first chroma plane in memory (the interleaved one of a semi-planar layout); NULL for 422PK */
    const void* v;                 /* the second chroma plane of a planar layout, else NULL */
    int64_t y_pitch, c_pitch;      /* bytes */
    int32_t h, w;
    int32_t layout, order;
    int32_t matrix, full_range;
    int32_t store, slot;
} af_yuv_frame_ex;
typedef struct af_yuv_item_ex {
    const void* y;
    const void* c0;
    const void* c1;
    void* dst;
    int32_t y_pitch, c_pitch, dst_pitch;
    int32_t first_tile;
    uint16_t h, w;
    uint8_t layout, order, bgr, colour;      /* colour: 2 * full_range + matrix */
} af_yuv_item_ex;
int af_yuv_plan_ex_u8(const af_yuv_frame_ex* frames, int n, const af_store_ref* stores, int n_stores, af_yuv_item_ex* items);
int af_yuv_to_rgb_ex_u8(const af_yuv_item_ex* items, int n, void* stream);

/* ---- cv2.resize of resident frames (added within ABI 6) -----------------------------------------------------------------------
 * cv2.resize(frame, (dw, dh)) with the default INTER_LINEAR on frames that sit in frame stores: one launch resizes up to
 * AF_RESIZE_MAX_FRAMES frames that may differ in store, size, destination and destination size - the step in front of a detector
 * that runs on downscaled frames (FaceDetector.scale_detect, demo2.py's yunet_res).  Arithmetic: the plain C++ path of OpenCV 4.x
 * resize.cpp for 8-bit images - a copy at equal size, (a + b + c + d + 2) >> 2 at exactly 2x in both axes, else the 11-bit
 * fixed-point bilinear form - stated in csrc/af_resize.hip and equal, byte for byte, to the numpy restatement tests/resize_ref.py
 * (unpinned against cv2 itself, absent where this is built; an IPP-enabled OpenCV may differ from the plain path).  Channels are
 * treated alike: a store's byte order passes through.
 *
 * af_resize_job (host): frame `frame` of stores[store] -> dh rows of dw pixels at the DEVICE pointer dst, rows dst_pitch bytes apart.
 * af_resize_table_bytes: an upper bound of the table's size for these jobs (-1: n or a size out of range).
 * af_resize_plan_u8 (host only, no device work) fills `table`, a caller-owned HOST buffer (pinned, for an asynchronous copy), 8-byte
 * aligned, and sets *used_bytes, the bytes to copy to the device.  Layout: af_resize_header; n af_resize_item (absolute addresses,
 * pitches, sizes, mode, byte offsets of the coefficient tables from the table's start, so the table may be copied anywhere); then
 * one af_resize_coef table per distinct (w -> dw) and per distinct (h -> dh) of the bilinear jobs, shared by the jobs of one
 * geometry.  The coefficients are computed here, on the host, in the fp64 / fp32 steps OpenCV takes.
 * AF_ERR_ARG: more than AF_RESIZE_MAX_FRAMES jobs, a store or frame index out of range, a bad store, dw or dh outside
 * [1, AF_RESIZE_MAX_SIDE], a destination pitch below 3 * dw, a null pointer, a table buffer that is too small.  A refused table's
 * header is stamped (kind = -1) so that no launch takes it.
 * af_resize_frames_u8 launches over a DEVICE copy of the table.  It trusts the table as the window launches trust theirs; the
 * kernel compares the header with n and writes nothing on a mismatch (the call still returns AF_OK).  Reads stay inside
 * [frame, frame + row_pitch * (h - 1) + 3 * w); writes are exactly dh rows of 3 * dw bytes, nothing in the pitch padding. */
#define AF_RESIZE_MAX_FRAMES 64
#define AF_RESIZE_MAX_SIDE 8192
#define AF_RESIZE_KIND 0x315a5352              /* "RSZ1" */
enum af_resize_mode { AF_RESIZE_COPY = 0, AF_RESIZE_AREA2 = 1, AF_RESIZE_LINEAR = 2 };
typedef struct af_resize_job {
    int32_t store, frame;
    void* dst;
    int64_t dst_pitch;
    int32_t dh, dw;
} af_resize_job;
typedef struct af_resize_header {
    int32_t kind, n, total_tiles, used_bytes;
    int32_t first_tile[AF_RESIZE_MAX_FRAMES + 1];      /* prefix sum of the jobs' tiles; [n ..] = total_tiles */
    int32_t reserved[3];
} af_resize_header;
typedef struct af_resize_item {
    const void* src;                                   /* first byte of the source frame */
    void* dst;
    int32_t src_pitch, dst_pitch;
    int32_t h, w, dh, dw;
    int32_t mode, runs_x;                              /* af_resize_mode; runs of 4 pixels per destination row */
    int32_t xtab, ytab;                                /* bilinear: byte offsets of the dw- and dh-entry coefficient tables */
} af_resize_item;
typedef struct af_resize_coef {
    int32_t idx;                                       /* first tap: column (clamped to [0, w - 1]) or row (-1 .. h - 1, clipped by the kernel) */
    int16_t a0, a1;                                    /* weights of the first and second tap, 11 fractional bits */
} af_resize_coef;
int64_t af_resize_table_bytes(const af_resize_job* jobs, int n);
int af_resize_plan_u8(const af_resize_job* jobs, int n, const af_store_ref* stores, int n_stores, void* table, int64_t table_bytes,
                      int64_t* used_bytes);
int af_resize_frames_u8(const void* table_dev, int n, void* stream);

/* ---- captured bitmaps into frame stores (added within ABI 6) --------------------------------------------------------------------
 * What a screen or window capture hands over - a BGRA (or RGBA, BGR, RGB) bitmap - into slots of frame stores in one launch that
 * does the three things the reference's capture code does on the host (test/win_capture.py:37, :110-115; test/capture_tile.py:190,
 * :199-201): the alpha byte is dropped, the client rectangle is cut out, and the rectangle is reduced with cv2.resize(...,
 * interpolation=cv2.INTER_AREA).  One launch takes up to AF_CAPTURE_MAX_FRAMES frames that may differ in size, format, mode, store
 * and byte order.  Arithmetic: OpenCV 4.x resize.cpp for 8-bit images, per channel, after the alpha drop (alpha never enters a
 * result), stated in csrc/af_capture.hip and equal, byte for byte, to the numpy restatement tests/capture_ref.py (unpinned against
 * cv2 itself, absent where this is built):
 *     COPY    dw == w and dh == h                     the three bytes
 *     AREA2   w == 2 dw and h == 2 dh                 (a + b + c + d + 2) >> 2
 *     BOX     w % dw == 0 and h % dh == 0 otherwise   fp32(integer box sum) * fp32(1 / (kx ky)), rounded half to even, saturated
 *     TABLE   everything else                         computeResizeAreaTab on both axes, fp32 accumulation in table order
 * Not built: upscaling (dw > w or dh > h is refused), bottom-up bitmaps, 16-bit and float captures.
 *
 * af_capture_frame (host description of one frame): src - DEVICE pointer of the first byte of the RECTANGLE, h rows of w pixels of
 * `channels` (3 or 4) bytes, rows `pitch` bytes apart; src_bgr - non-zero: the bytes of a pixel are B, G, R[, x], zero: R, G, B[, x];
 * (store, slot) - the destination; (dh, dw) - the destination size, which must be the frame size of stores[store].
 * af_capture_table_bytes: an upper bound of the table's size for these frames (-1: n or a size out of range).
 * af_capture_plan_u8 (host only, no device work) fills `table`, a caller-owned HOST buffer (pinned, for an asynchronous copy), 8-byte
 * aligned, and sets *used_bytes.  Layout: af_capture_header; n af_capture_item (absolute addresses, pitches, sizes, mode, swap - the
 * store's bgr differs from src_bgr - and byte offsets of the area tables from the table's start, so the table may be copied
 * anywhere); then one area table per distinct (w -> dw) and per distinct (h -> dh) of the TABLE jobs, shared by the jobs of one
 * geometry: int32 first[d + 1] (the taps of destination index i are [first[i], first[i + 1])), padded to 8 bytes, then the
 * af_capture_tap list in OpenCV's table order.  Cell bounds are fp64 and weights are cast to fp32, here on the host.
 * AF_ERR_ARG: more than AF_CAPTURE_MAX_FRAMES frames, a side outside [1, AF_CAPTURE_MAX_SIDE], dw > w or dh > h, a pitch below
 * w * channels, channels not 3 or 4, a bad store or slot, a store of another frame size, a null pointer, a table buffer that is too
 * small.  A refused table's header is stamped (kind = -1) so that no launch takes it.
 * af_capture_to_stores_u8 launches over a DEVICE copy of the table.  It trusts the table as the resize launch trusts its own; the
 * kernel compares the header with n and writes nothing on a mismatch (the call still returns AF_OK).  Whatever the alignment of
 * source, pitch and destination rows, reads stay inside [src, src + pitch * (h - 1) + w * channels) and writes are exactly dh rows
 * of 3 * dw bytes.  The source must be ready on `stream` and stay unchanged until the launch has run. */
#define AF_CAPTURE_MAX_FRAMES 64
#define AF_CAPTURE_MAX_SIDE 8192
#define AF_CAPTURE_KIND 0x31504143             /* "CAP1" */
enum af_capture_mode { AF_CAPTURE_COPY = 0, AF_CAPTURE_AREA2 = 1, AF_CAPTURE_BOX = 2, AF_CAPTURE_TABLE = 3 };
typedef struct af_capture_frame {
    const void* src;
    int64_t pitch;
    int32_t h, w;
    int32_t channels, src_bgr;
    int32_t store, slot;
    int32_t dh, dw;
} af_capture_frame;
typedef struct af_capture_header {
    int32_t kind, n, total_tiles, used_bytes;
    int32_t first_tile[AF_CAPTURE_MAX_FRAMES + 1];     /* prefix sum of the items' tiles; [n ..] = total_tiles */
    int32_t reserved[3];
} af_capture_header;
typedef struct af_capture_item {
    const void* src;                                   /* first byte of the rectangle */
    void* dst;                                         /* first byte of the store's slot */
    int32_t src_pitch, dst_pitch;
    int32_t h, w, dh, dw;
    int32_t mode, runs_x;                              /* af_capture_mode; runs of 4 pixels per destination row */
    int32_t xtab, ytab;                                /* TABLE: byte offsets of the two area tables */
    int32_t kx, ky;                                    /* BOX: w / dw and h / dh */
    float inv_area;                                    /* BOX: fp32(1) / fp32(kx * ky) */
    uint8_t channels, swap, dword, xk;                 /* dword: 4 channels, source address and pitch 4-byte aligned; xk - TABLE: the
                                                          most taps one destination column has (255: that many or more) */
} af_capture_item;
typedef struct af_capture_tap {
    int32_t idx;                                       /* source column or row, 0 .. size - 1 */
    float weight;
} af_capture_tap;
int64_t af_capture_table_bytes(const af_capture_frame* frames, int n);
int af_capture_plan_u8(const af_capture_frame* frames, int n, const af_store_ref* stores, int n_stores, void* table, int64_t table_bytes,
                       int64_t* used_bytes);
int af_capture_to_stores_u8(const void* table_dev, int n, void* stream);

/* ---- the speaker tile of a captured call grid (added within ABI 6) ---------------------------------------------------------------
 * LargestTilePicker's pixel work (test/capture_tile.py:55-95) on a frame that is resident on the device; the arithmetic is stated
 * in csrc/af_tile.hip and equals tests/tile_ref.py byte for byte (a numpy restatement of OpenCV 4.x's plain C++ path, unpinned
 * against cv2 itself, absent where this is built).
 *
 * af_tile_source: DEVICE pointer of the first byte of h rows of w packed 3-byte pixels, rows `pitch` bytes apart; bgr - non-zero:
 * B, G, R, zero: R, G, B.  A frame of an af_store_ref is base + frame * frame_stride with the store's row_pitch and bgr.  Both sides
 * are AF_TILE_MIN_SIDE .. AF_TILE_MAX_SIDE (the blur's reflected halo of 4 pixels needs 8).
 * `workspace`: DEVICE memory of af_tile_workspace_bytes(h, w) bytes, 256-byte aligned, owned by the caller and by one call at a
 * time.  Its first sizeof(af_tile_result) bytes are the call's answer, written on `stream`; the caller copies them back (the one
 * read-back of a sequence).  Nothing waits on the host.
 *
 * af_tile_candidates_u8: grey, GaussianBlur 5 x 5, Canny(50, 150) with the hysteresis as a labelling of the candidates, dilate
 * 3 x 3, the 8-connected components of the result with their boxes, the external ones (findContours RETR_EXTERNAL), _valid with
 * `params`, and for each of the at most AF_TILE_MAX_BOXES survivors the exact sums S1, S2 of the blurred grey over the inset roi
 * of n_px pixels, by ascending root (a component's smallest pixel index y * w + x): result.count, result.box[].  More survivors:
 * result.overflow != 0.  The host decides n_px == 0 or n_px * S2 - S1^2 < 50 n_px^2 and sorts.
 * af_tile_motion_u8: the unblurred grey into `grey` (h * w bytes), |grey - prev_grey| > 16, medianBlur 5, two 5 x 5 dilations,
 * the components of the result and the union x1, y1, x2, y2 of the boxes with w * h >= area_min (union_count of them; none: w, h,
 * 0, 0).  prev_grey null: only the grey is written (the reference's first frame).
 * af_tile_components_u8: the stage both end in, on any h x w mask (non-zero = set; `g`, h * w bytes or null, feeds the sums;
 * params null: no selection).  result.components counts the components.
 * af_tile_outputs (null, or any member null): tight h x w copies of the stages for tests - g (motion: the grey), cls (0 none, 1
 * candidate, 2 strong; motion: the threshold 0 / 1), edges (0 / 255; motion: the median 0 / 1), mask (0 / 255), labels (int32: the
 * root, -1 background), boxes (int32 x 4 per pixel, minx, miny, maxx, maxy at a root, w, h, -1, -1 elsewhere), external (bytes, 1 at
 * the root of an external component).
 * Every device loop is bounded by the pixel count; a bound that is hit sets bits in result.error (1: a find, 2: a union) instead of
 * spinning.  A caller treats error != 0 or overflow != 0 as a failure, never as an answer. */
#define AF_TILE_MAX_BOXES 64
#define AF_TILE_MIN_SIDE 8
#define AF_TILE_MAX_SIDE 8192
typedef struct af_tile_source {
    const void* pixels;
    int64_t pitch;
    int32_t h, w;
    int32_t bgr, reserved;
} af_tile_source;
typedef struct af_tile_params {                        /* LargestTilePicker._valid: ww >= min_w, hh >= min_h, ar_lo <= ww / hh <= ar_hi */
    int32_t min_w, min_h;                              /* in fp64, ww * hh >= area_min (the host's 0.10 * W * H) */
    double ar_lo, ar_hi, area_min;
} af_tile_params;
typedef struct af_tile_box {
    int32_t root, x, y, w, h, n_px;
    int64_t s1, s2;
} af_tile_box;
typedef struct af_tile_result {
    int32_t error, count, overflow, components;
    int32_t x1, y1, x2, y2;                            /* motion: the union */
    int32_t union_count, reserved[3];
    af_tile_box box[AF_TILE_MAX_BOXES];
} af_tile_result;
typedef struct af_tile_outputs {
    void *g, *cls, *edges, *mask, *labels, *boxes, *external;
} af_tile_outputs;
int64_t af_tile_workspace_bytes(int h, int w);
int af_tile_candidates_u8(const af_tile_source* src, const af_tile_params* params, void* workspace, int64_t workspace_bytes,
                          const af_tile_outputs* out, void* stream);
int af_tile_motion_u8(const af_tile_source* src, const void* prev_grey, void* grey, double area_min, void* workspace,
                      int64_t workspace_bytes, const af_tile_outputs* out, void* stream);
int af_tile_components_u8(const void* mask, int64_t pitch, int h, int w, const void* g, const af_tile_params* params, void* workspace,
                          int64_t workspace_bytes, const af_tile_outputs* out, void* stream);

/* ---- rank metrics of index rows over one scored pool (added within ABI 6) -----------------------------------------------------------
 * AUROC and average precision of many resamples of ONE pool of n scored items, on integers (csrc/af_eval.hip; the
 * numpy statement is tests/evalsuite_ref.py).  The caller sorts the pool once by descending score (stable) and uploads
 *   rank_of_item[n]   each item's position in that order,
 *   group_of_rank[n]  the tie-group id along the sorted scores: 0 at rank 0, non-decreasing, +1 where the score changes,
 *   label_of_rank[n]  non-zero: a positive, along the sorted scores.
 * A row is the indices idx[row_off[r] .. row_off[r + 1]) (items, repeats allowed; n_idx = the length of idx).  One workgroup per
 * row counts the draws of every rank in LDS with integer atomics - hence n <= AF_RANK_MAX_POOL - and scans the sorted order:
 *   u2      = sum_g pos_g (2 (N - fp_g) + neg_g)         exact; AUROC = u2 / (2 P N)
 *   ap_sum  = sum_g pos_g (tp_g / (tp_g + fp_g))         fp64, groups with pos_g == 0 skipped; AP = ap_sum / P
 *   tp_cut, fp_cut = the draws of rank < cut, by label   (cut in [0, n]: the pool items at or above a threshold)
 * ap_sum is added in a fixed order (a thread's groups in rank order over contiguous chunks of ceil(n / AF_RANK_THREADS) ranks, a
 * group belonging to the thread of its last rank, then the tree p[i] += p[i + h], h = AF_RANK_THREADS / 2 .. 1): runs repeat bit
 * for bit.  An index or rank outside [0, n), or a row that leaves [0, n_idx], is never used as an address: it is skipped and
 * counted into *error (one int32, DEVICE memory, zeroed by the call on `stream`); a caller treats non-zero as a failed call.
 * AF_ERR_ARG: a null pointer, n outside [1, AF_RANK_MAX_POOL], rows < 0, n_idx outside [0, 2^31), cut outside [0, n].
 *
 * af_rank_curve: ONE row -> the cumulative counts at every group's end, tps[g] / fps[g] for g < *n_groups (tps, fps: n int32
 * each; n_groups, error: one int32 each; all DEVICE memory) - the integer ROC curve a caller thins and normalises. */
#define AF_RANK_MAX_POOL 16384
#define AF_RANK_THREADS 256
typedef struct af_rank_row {
    int64_t u2;
    double ap_sum;
    int32_t P, N, tp_cut, fp_cut;
} af_rank_row;
int af_rank_metrics_rows(const int32_t* rank_of_item, const int32_t* group_of_rank, const uint8_t* label_of_rank, int n, const int32_t* idx,
                         int64_t n_idx, const int64_t* row_off, int rows, int cut, af_rank_row* out, int32_t* error, void* stream);
int af_rank_curve(const int32_t* rank_of_item, const int32_t* group_of_rank, const uint8_t* label_of_rank, int n, const int32_t* idx,
                  int64_t n_idx, int32_t* tps, int32_t* fps, int32_t* n_groups, int32_t* error, void* stream);

/* ---- bootstrap rows from numpy's PCG64 stream (added within ABI 6) ------------------------------------------------------------------
 * What `rows` rounds of rng.choice(A, count_a, True), rng.choice(B, count_b, True) of a numpy Generator over PCG64 return, drawn on
 * the device (csrc/af_draw.hip; the numpy statement is tests/pcg64_ref.py).  `start` is bit_generator.state: the 128-bit
 * state and increment in 64-bit halves, has_uint32 and uinteger.  The stream: s_j = s_(j-1) 0x2360ED051FC65DA44385DF649FCCF645 + inc
 * (mod 2^128), out_j = rotr64(hi64(s_j) ^ lo64(s_j), s_j >> 122); 32-bit words are the buffered uinteger where has_uint32 is set, then
 * the low and the high half of every output.  A draw with bound m takes a word w, rejects it where lo32(w m) < 2^32 mod m and takes the
 * next, else yields hi32(w m); a bound of 1 yields 0 and takes NO word.  Row r is count_a draws under bound_a, then count_b under
 * bound_b; rows follow one another on the stream.  Written, all DEVICE memory:
 *   idx[rows (count_a + count_b)]   items_a[draw] / items_b[draw], or with a null items pointer the draw itself (uint32 bits);
 *   row_off[rows + 1]               row_base + r (count_a + count_b): the row table af_rank_metrics_rows reads, so idx and row_off may
 *                                   point behind rows that are already there;
 *   result                          words consumed, outputs made, the buffer numpy would be left with, the rejections, `error`.
 * Three launches on `stream` (scan, resolve, emit), no workgroup waits on another.  `max_rejects` (1 .. AF_DRAW_MAX_REJECTS) is the
 * capacity of the list of words that EITHER bound would reject among the first rows (count_a + count_b) + ceil(max_rejects / 2) words;
 * a list that overflows, or more than ceil(max_rejects / 2) rejections, sets result->error, result->consumed = -1 and nothing is drawn.  error also counts draws outside `items` (there are
 * none).  A caller treats non-zero as a failed call.  The workspace (af_pcg64_draw_workspace_bytes(max_rejects), 8-byte aligned) is
 * scratch.  AF_ERR_ARG: a null pointer other than items (and idx where nothing is drawn), a bound outside [1, 2^32 - 1] (numpy draws 2^32 another way), a negative
 * count, rows (count_a + count_b) >= 2^31, items with bound != count, max_rejects out of range, a workspace too small. */
#define AF_DRAW_MAX_REJECTS 8192
typedef struct af_pcg64_state {
    uint64_t state_hi, state_lo, inc_hi, inc_lo;
    int32_t has_uint32;
    uint32_t uinteger;
} af_pcg64_state;
typedef struct af_draw_result {
    int64_t consumed;              /* 32-bit words taken from the stream, the buffered one included */
    int64_t outputs;               /* 64-bit outputs made: the caller advances the state by this many steps */
    int32_t has_uint32;            /* the buffer after the last word, */
    uint32_t uinteger;             /*   as numpy leaves it (the high half of the last output, stale or not) */
    int32_t rejected, listed;      /* words rejected; words listed by the scan */
    int32_t error, reserved;
} af_draw_result;
int64_t af_pcg64_draw_workspace_bytes(int max_rejects);
int af_pcg64_draw_rows(const af_pcg64_state* start, int64_t bound_a, int count_a, int64_t bound_b, int count_b, int rows,
                       const int32_t* items_a, const int32_t* items_b, int max_rejects, int32_t* idx, int64_t* row_off, int64_t row_base,
                       af_draw_result* result, void* workspace, int64_t workspace_bytes, void* stream);

/* ---- whole-forward op list ------------------------------------------------------------ */

enum af_op_kind { AF_OP_STEM = 0, AF_OP_CONV = 1, AF_OP_MAXPOOL = 2, AF_OP_HEAD = 3,
                  AF_OP_PACK_F32 = 4, AF_OP_PACK_U8 = 5, AF_OP_CONV_DUAL = 6, AF_OP_STEM_POOL = 7, AF_OP_AVGPOOL = 8, AF_OP_LINEAR = 9,
                  /* FTCN-TT: in/weight/scale/shift/out as commented in af_run_ops' switch (csrc/af_api.hip) */
                  AF_OP_TSTEM = 10, AF_OP_TOKENS = 11, AF_OP_LAYERNORM = 12, AF_OP_ATTENTION = 13, AF_OP_GELU = 14,
                  /* b + c of a bottleneck in one launch: conv / weight / scale / shift = the b conv, conv2 / weight2 / scale2 /
                     shift2 = the c conv, residual, out, out_ld (af_conv3d_bc_bn_act) */
                  AF_OP_CONV_BC = 15,
                  /* the K-packed stem path: same fields as PACK_F32 / PACK_U8 / STEM_POOL, rgb3 input layout */
                  AF_OP_PACK3_F32 = 16, AF_OP_PACK3_U8 = 17, AF_OP_STEM3_POOL = 18,
                  /* c of a block + a of the next in one launch: conv / weight / scale / shift / residual / out = the c conv and
                     the trunk, conv2 / weight2 / scale2 / shift2 / aux = the a conv and its output (af_conv3d_ca_bn_act) */
                  AF_OP_CONV_CA = 19,
                  /* a narrow bottleneck block in one launch: conv / weight / scale / shift = a, conv2 / weight2 / scale2 / shift2 = b,
                     conv3 / weight3 / scale3 / shift3 = c, in = the trunk (input and residual), out, out_ld; projection form:
                     pool is unused, in2 == in and (conv4, weight4) = the shortcut conv (af_block_abc_bn_act) */
                  AF_OP_BLOCK_ABC = 20,
                  /* TSTEM with the stem's 1x3x3 / stride-2 max-pool fused behind it (af_tstem_conv_bn_pool_relu_maxpool) */
                  AF_OP_TSTEM_POOL3 = 21,
                  /* c of s2's last block + temporal pool + a of s3's block 0: fields as CONV_CA (no conv3 segment), x_sub
                     (af_conv3d_cpa_bn_act) */
                  AF_OP_CONV_CPA = 22,
                  /* both SlowFast inputs from one uint8 clip (af_pack_input_u8_pathways): in = clips, conv.n / t / h / w = the Fast
                     input's dims, conv.dtype, mean, std_, out = the Slow input, aux = the Fast input, x_sub = alpha, pack_rgb3
                     (added within ABI 6) */
                  AF_OP_PACK_PATHWAYS_U8 = 23,
                  /* launches nothing: the slot of an op whose work another op of the list does (SlowFast's second input pack
                     in a uint8 run); keeps op indices the same for every input form */
                  AF_OP_NOP = 24 };

typedef struct af_op {
    int32_t kind;                    /* af_op_kind */
    int32_t out_ld;
    af_conv_desc conv;               /* STEM / CONV */
    af_pool_desc pool;               /* MAXPOOL / HEAD */
    const void* in;
    const void* weight;              /* packed conv weight | fc weight */
    const float* scale;              /* BN scale | fc bias */
    const float* shift;
    const void* residual;
    void* out;                       /* activation | logits */
    void* aux;                       /* HEAD: pooled features (optional) */
    int32_t num_classes;
    int32_t tag;                     /* caller-defined (e.g. layer class) - echoed by *_timed */
    /* CONV_DUAL only: the projection-shortcut segment */
    af_conv_desc conv2;
    const void* in2;
    const void* weight2;
    /* PACK_* only */
    int64_t in_strides[5];           /* n,c,t,h,w element strides of the fp32 source */
    float mean[3], std_[3];
    /* CONV only: split-K scratch (af_conv3d_bn_act) */
    void* workspace;
    int64_t workspace_bytes;
    /* HEAD / LINEAR only: optional per-row scores (af_avgpool_fc_scores) */
    float* scores;
    /* CONV_BC / CONV_CA: BatchNorm of the second conv */
    const float* scale2;
    const float* shift2;
    /* CONV_CA of a projection block only: the shortcut segment (NULL in3: plain block with a residual) */
    af_conv_desc conv3;
    const void* in3;
    const void* weight3;
    /* BLOCK_ABC: BatchNorm of the third conv; the projection shortcut of its block-0 form (weight4 == NULL: identity) (ABI 3) */
    const float* scale3;
    const float* shift3;
    af_conv_desc conv4;
    const void* weight4;
    /* CONV_CPA: 1 = the whole pooled trunk is stored, 2 = its even (h, w) positions, packed (ABI 3); PACK_PATHWAYS_U8: alpha */
    int32_t x_sub;
    /* PACK_PATHWAYS_U8: bit 0 = the Slow input (out) is AF_PACK_RGB3, bit 1 = the Fast input (aux) is; the former reserved0 */
    int32_t pack_rgb3;
} af_op;

/* Enqueue ops[0..n) in order on `stream` (AltFreezing: ResNet.forward, video_model_builder.py:561-578). */
int af_run_ops(const af_op* ops, int n_ops, void* stream);
/* Same, bracketing every op with hipEvents on `stream`; ms[i] = device time of op i.  Synchronises. */
int af_run_ops_timed(const af_op* ops, int n_ops, void* stream, float* ms);

/* ---- YuNet face detector (ABI 5) ---------------------------------------------------------
 * The live-call loop's detection stage: preprocessing/yunet/yunet.py YuNet.infer ->
 * cv2.FaceDetectorYN.detect on face_detection_yunet_2023mar.onnx (test/af_realtime.py), for a batch
 * of `batch` uint8 BGR frames of one size.  Each frame is zero-padded bottom / right to a multiple of
 * 32 and fed as float 0..255 (no mean, no scale, no channel swap); the whole network is fp32.
 * Decode and NMS restate OpenCV's FaceDetectorYN::postProcess and dnn::NMSBoxes (csrc/af_yunet.hip).
 *
 * `weights`: af_yunet_weight_floats() fp32 values packed by detector.py (pack_weights) from the ONNX file.
 * `frames`: frame b starts at frames + b * frame_stride, rows row_pitch bytes apart, 3 bytes per pixel.
 * `workspace`: af_yunet_workspace_bytes(desc) bytes of device scratch (16-byte aligned).
 * `out_rows`: [batch][top_k][15] f32 (x, y, w, h, 5 landmarks (x, y), score); rows past out_count[b]
 * are not written.  `out_count`: [batch] int32.  `raw` (optional, may be NULL): [batch][anchors][16]
 * f32, per anchor (stride 8, 16, 32 levels in order, row-major) the 16 head outputs cls, obj (after the
 * sigmoid), bbox[4], kps[10].  Every argument is checked on the host before the first launch.
 * AF_YUNET_LAUNCHES kernels are enqueued; *_timed also returns their device times (synchronises).
 * Cost of the per-frame sort: up to 16 384 candidates (score >= conf) are sorted in one pass in LDS; above that the sort
 * runs as candidates / 8 192 LDS passes of 16 384 keys, so a very low conf on a very large frame (all 1.38 M anchors of an
 * 8192 x 8192 frame at conf 0) costs one workgroup about 170 such passes.  At the default conf 0.6 real frames stay far
 * below 16 384.  A workspace serves one stream at a time: concurrent calls need separate workspaces. */
#define AF_YUNET_MAX_TOPK 8192
#define AF_YUNET_MAX_SIDE 8192
#define AF_YUNET_LAUNCHES 18
typedef struct af_yunet_desc {
    int32_t batch, height, width;
    int32_t top_k;
    int64_t frame_stride, row_pitch;   /* bytes */
    float conf_threshold, nms_threshold;
} af_yunet_desc;
int64_t af_yunet_weight_floats(void);
int64_t af_yunet_workspace_bytes(const af_yunet_desc* desc);
int af_yunet_detect(const af_yunet_desc* desc, const float* weights, const void* frames, void* workspace, int64_t workspace_bytes,
                    float* out_rows, int32_t* out_count, float* raw, void* stream);
int af_yunet_detect_timed(const af_yunet_desc* desc, const float* weights, const void* frames, void* workspace,
                          int64_t workspace_bytes, float* out_rows, int32_t* out_count, float* raw, void* stream, float* ms);

/* af_yunet_detect on a LIST of frames: `frames` is a HOST array of desc->batch device pointers, one per frame; the frames have one
 * size and one row_pitch, desc->frame_stride is not read, and desc->batch is at most AF_YUNET_MAX_LIST.  The pointers travel in the
 * launch arguments of the first kernel (the only one that reads pixels): no copy of the list or of the frames.  Everything else,
 * the outputs bit for bit, is af_yunet_detect on a contiguous copy of the same frames; the workspace is that of the same desc.
 * (Added within ABI 6.) */
#define AF_YUNET_MAX_LIST 64
int af_yunet_detect_frames(const af_yunet_desc* desc, const float* weights, const void* const* frames, void* workspace,
                           int64_t workspace_bytes, float* out_rows, int32_t* out_count, float* raw, void* stream);

/* ---- RetinaFace detector (ABI 6) ---------------------------------------------------------
 * The offline evaluator's face detector: test_tools/ct/detection (RetinaFace(cfg_mnet, phase="test"),
 * mobilenet0.25, and batch_detect's post_process with confidence 0.02, top_k 5000, NMS 0.4,
 * keep_top_k 750) for a batch of `batch` uint8 HWC frames of one size.  The mean (104, 117, 123) is
 * subtracted by channel index, whatever the channel order; the whole network is fp32 (csrc/af_retinaface.hip).
 *
 * `weights`: af_retinaface_weight_floats() fp32 values packed by retinaface.py (pack_weights), BN folded.
 * `frames`: frame b starts at frames + b * frame_stride, rows row_pitch bytes apart, 3 bytes per pixel.
 * `workspace`: af_retinaface_workspace_bytes(desc) bytes of device scratch (16-byte aligned).
 * `out_rows`: [batch][af_retinaface_max_rows(desc)][15] f32 (x1, y1, x2, y2, score, 5 landmarks (x, y)),
 * in descending score order; rows past out_count[b] are not written.  `out_count`: [batch] int32.
 * The rows are post_process's detections cut to min(keep_top_k, max_count) (max_count <= 0: no cut),
 * then to the leading rows with score >= min_score (get_valid_faces; min_score 0: no cut).
 * Exact score ties are ordered by descending anchor index (the reference leaves them unordered).
 * `raw` (optional, may be NULL): 16 * batch * anchors f32 as three planes, loc [batch][anchors][4],
 * conf [batch][anchors][2] (after the softmax), landms [batch][anchors][10]; anchors in PriorBox order
 * (level, row, col, anchor).
 * af_retinaface_postprocess runs the decode and post-process alone on caller-supplied planes of that
 * layout (`loc`, `conf` after the softmax, `landms`); it does not read `frames`.
 * AF_RETINAFACE_LAUNCHES kernels are enqueued by detect; *_timed also returns their device times
 * (synchronises).  A workspace serves one stream at a time. */
#define AF_RETINAFACE_MAX_SIDE 8192
#define AF_RETINAFACE_TOP_K 5000
#define AF_RETINAFACE_MAX_KEEP 5000
#define AF_RETINAFACE_LAUNCHES 54
#define AF_RETINAFACE_POST_LAUNCHES 5
typedef struct af_retinaface_desc {
    int32_t batch, height, width;
    int32_t keep_top_k;                /* 750 in batch_detect; 1 .. AF_RETINAFACE_MAX_KEEP */
    int64_t frame_stride, row_pitch;   /* bytes */
    int32_t max_count;                 /* get_valid_faces' max_count; <= 0: no cut */
    int32_t reserved;
    double min_score;                  /* get_valid_faces' thres: rows with score < min_score are dropped */
} af_retinaface_desc;
int64_t af_retinaface_weight_floats(void);
int64_t af_retinaface_anchors(const af_retinaface_desc* desc);
int32_t af_retinaface_max_rows(const af_retinaface_desc* desc);
int64_t af_retinaface_workspace_bytes(const af_retinaface_desc* desc);
int af_retinaface_detect(const af_retinaface_desc* desc, const float* weights, const void* frames, void* workspace,
                         int64_t workspace_bytes, float* out_rows, int32_t* out_count, float* raw, void* stream);
int af_retinaface_detect_timed(const af_retinaface_desc* desc, const float* weights, const void* frames, void* workspace,
                               int64_t workspace_bytes, float* out_rows, int32_t* out_count, float* raw, void* stream, float* ms);
int af_retinaface_postprocess(const af_retinaface_desc* desc, const float* loc, const float* conf, const float* landms,
                              void* workspace, int64_t workspace_bytes, float* out_rows, int32_t* out_count, void* stream);
int af_retinaface_postprocess_timed(const af_retinaface_desc* desc, const float* loc, const float* conf, const float* landms,
                                    void* workspace, int64_t workspace_bytes, float* out_rows, int32_t* out_count, void* stream,
                                    float* ms);

/* ---- device tracker (added within ABI 6) -----------------------------------------------------
 * tracker.ByteTracker.update for many trackers in one launch (csrc/af_track_core.h, csrc/af_track.hip; the numpy statement
 * is tests/bytetrack_ref.py): fp64, every sum in one written-down order, one wave per tracker.
 *
 * A tracker is af_bytetrack_state_bytes() bytes (8-byte aligned) that af_bytetrack_reset filled: reset writes a HOST block, a
 * device tracker is a copy of one.  A state block belongs to one call of a launch.  An update writes one record of
 * af_bytetrack_record_bytes() bytes per call:
 *   int32 frame_id, overflow, n_online, n_tracked, n_lost, n_removed, reserved[2];
 *   { double tlbr[4], score; int32 id, state, is_activated, reserved; } online[AF_TRACK_MAX_TRACKS];   the returned tracks, in order
 *   int32 tracked_ids[AF_TRACK_MAX_TRACKS], lost_ids[AF_TRACK_MAX_TRACKS], removed_ids[AF_TRACK_MAX_TRACKS];
 * removed_ids: the tracks removed by THIS update (a lost track that times out is named by two successive updates, as the
 * reference appends it to removed_stracks twice).  overflow: 0, or AF_TRACK_OVERFLOW_DETS (more than AF_TRACK_MAX_DETS rows
 * passed the start filter; the state is untouched), AF_TRACK_OVERFLOW_TRACKS (tracked + lost would exceed AF_TRACK_MAX_TRACKS;
 * the tracker refuses every later update until it is reset), AF_TRACK_NOT_RESET.  Nothing is written outside the state blocks
 * and the records.
 *
 * af_track_call.form: EMPTY (no detection: _nothing_detected); LIST (float32 rows x, y, w, h, score, ... `row_stride` floats
 * apart, a detector's rows where it left them: a row is scaled back as YuNet.scale_rows does it - x, w and column 4 by scale_x,
 * y, h by scale_y in fp64, cast to float32 - and enters when column 4 >= start_conf and max(w, h) >= start_min_size, compared in
 * float32; column 4 is its score, as af_realtime.py:385 reads it; no second association); LIST64
 * (fp64 rows x, y, w, h, score, no filter); ARRAY (fp64 rows x0, y0, x1, y1, score, divided by min(img_size[0] / img_info[1],
 * img_size[1] / img_info[0]), split at track_thresh, with the second association).  The number of rows is *count_ptr when
 * count_ptr is not NULL (device memory for af_bytetrack_update_calls), cut at max_rows, and `count` otherwise.
 * af_bytetrack_update_calls: `calls` is a HOST array of 1 .. AF_TRACK_MAX_CALLS entries that travels in the launch arguments;
 * states, rows, counts and records are device memory; one launch.  af_bytetrack_update_host runs the same source on the CPU
 * for one call over host memory.  af_track_probe_f64: q[i] = x[i] / y[i], r[i] = sqrt(x[i]) in device code, one launch. */
#define AF_TRACK_MAX_TRACKS 32
#define AF_TRACK_MAX_DETS 32
#define AF_TRACK_MAX_CALLS 64
#define AF_TRACK_FORM_EMPTY 0
#define AF_TRACK_FORM_LIST 1
#define AF_TRACK_FORM_ARRAY 2
#define AF_TRACK_FORM_LIST64 3
#define AF_TRACK_OVERFLOW_DETS 1
#define AF_TRACK_OVERFLOW_TRACKS 2
#define AF_TRACK_NOT_RESET 3
typedef struct af_track_call {
    void* state;
    const void* rows;
    const int32_t* count_ptr;
    int32_t count, max_rows, form, row_stride;
    int32_t img_info[2], img_size[2];
    float start_conf, start_min_size;
    double scale_x, scale_y;
} af_track_call;
int64_t af_bytetrack_state_bytes(void);
int64_t af_bytetrack_record_bytes(void);
int af_bytetrack_reset(void* state, double track_thresh, double match_thresh, int buffer_size);
int af_bytetrack_update_calls(const af_track_call* calls, int n_calls, void* records, void* stream);
int af_bytetrack_update_host(const af_track_call* call, void* record);
int af_track_probe_f64(const double* x, const double* y, double* q, double* r, int n, void* stream);

/* ---- the dataset evaluator's chunk stage on the device (added within ABI 6) -------------------------------------------------------
 * What runner.VideoRunner does on the host per kept frame of a chunk - the detection rhythm, the smart start, the budget,
 * filter_detections, ByteTracker.update, the id-switch count, the five-point pick with the mesh_every cache and get_crop_box
 * (runner.py: the loop's host stage and track_stage) - for all frames of a chunk, in order, as ONE launch of one wave on
 * the detector's rows where they lie (csrc/af_runner_core.h, csrc/af_runner.hip; the numpy statement is tests/runner_chunk_ref.py).
 *
 * A run is af_runner_state_bytes() bytes (8-byte aligned): the tracker's state block first, then the loop's scalars, prev_boxes /
 * prev_ids and the five-point cache (one entry per tracker slot, tagged with the track id it belongs to, so a reused slot never
 * serves another track's points).  af_runner_reset fills a HOST block; a device run is a copy of one.
 *
 * af_runner_chunk (host, travels in the launch arguments): rows - float32, frame j's rows at rows + j * max_rows * row_stride,
 * row i `row_stride` (>= 15) floats on (x, y, w, h, score, five points); counts[j] rows of frame j, cut at max_rows; rows_floats
 * - the floats readable behind `rows` (n_frames * max_rows * row_stride must fit); frame_idx[j] - the frame's index in the video;
 * first_slot - frame j lies in slot first_slot + j of the frame store; the thresholds as the loop compares them: float32 for the
 * detection filters and the start (a clause whose threshold is not positive is skipped; bottom_limit is
 * float32(frame_h * (1 - exclude_bottom_frac)), formed by the caller, <= 0: no clause), fp64 for min_track_side and crop_scale.
 *
 * The chunk record, af_runner_record_bytes(n_frames) bytes (8-byte aligned):
 *   af_runner_header;  af_runner_frame frames[AF_RUNNER_MAX_FRAMES];  af_runner_cand cands[n_frames * AF_TRACK_MAX_TRACKS];
 * header: the loop's scalars after the chunk; overflow - 0 or an AF_TRACK_* code with overflow_frame the chunk position of the
 * frame that refused (more than AF_TRACK_MAX_DETS rows past the filter: the state is untouched by that frame; more than
 * AF_TRACK_MAX_TRACKS tracked + lost faces: the run refuses every later chunk); nothing of a later frame is written;
 * n_cands; tiles_half / tiles_full - the tile totals of the quality launch in its two modes; bad - set by
 * af_face_quality_table_u8 when it skipped a candidate.
 * frames[j].flags: AF_RUNNER_NEED_DETECT, _DROPPED (before the start), _PROCESSED, _NOT_REACHED (behind the budget stop),
 * _REFUSED; n_rows - the rows the filter left; ids[0 .. n_ids) - the tracks that passed min_track_side, in the tracker's order.
 * cands, in track_stage's order: the frame's position in the chunk and its slot, the track id, the float32 box and five points
 * in frame coordinates, the crop box (x1, y1, x2, y2), the first tile of its half-size and of its full-size image, flags
 * (AF_RUNNER_CAND_BAD: the quality launch skipped it).
 * af_runner_track_chunk: state, rows, counts and record are DEVICE memory; one workgroup of 64 lanes; nothing is written outside
 * the state block and the record.  af_runner_track_chunk_host: the same source on the CPU over host memory.
 *
 * af_face_quality_table_u8: the quality launch (af_face_quality_stores_u8, or with `full` af_face_laplacian_stores_u8) with
 * rectangles, slots and tile prefixes read from a chunk record in DEVICE memory: candidate k (k < min(n_cands, capacity)) is the
 * rectangle (x1, y1) .. (x2, y2) of slot cands[k].slot of `store`, its sums go to sums[k]; sums[0 .. capacity) are cleared in
 * front of the launch on `stream`.  A fixed grid strides over the record's tile total.  The kernel re-checks every candidate: a
 * rectangle that leaves its frame, a slot outside the store or a tile prefix that does not fit is skipped - never read - and
 * flagged (cands[k].flags, header.bad).  grey: null, or (tests) a DEVICE buffer of capacity * grey_stride bytes; candidate k's
 * grey image goes to grey + k * grey_stride when it fits grey_stride. */
#define AF_RUNNER_MAX_FRAMES 64
#define AF_RUNNER_NEED_DETECT 1
#define AF_RUNNER_DROPPED 2
#define AF_RUNNER_PROCESSED 4
#define AF_RUNNER_NOT_REACHED 8
#define AF_RUNNER_REFUSED 16
#define AF_RUNNER_CAND_BAD 1
typedef struct af_runner_header {
    int32_t started, consec, processed_after_start, stop;
    int32_t id_switches, frames_seen, overflow, overflow_frame;
    int32_t n_cands, tiles_half, tiles_full, bad;
    int32_t n_frames, reserved[3];
} af_runner_header;
typedef struct af_runner_frame {
    int32_t flags, n_rows, n_ids, reserved;
    int32_t ids[AF_TRACK_MAX_TRACKS];
} af_runner_frame;
typedef struct af_runner_cand {
    int32_t frame_pos, slot, tid, flags;
    float tlbr[4];
    float lm5[10];
    int32_t box[4];
    int32_t tile_half, tile_full;
} af_runner_cand;
typedef struct af_runner_chunk {
    void* state;
    const float* rows;
    const int32_t* counts;
    void* record;
    int64_t rows_floats;
    int32_t n_frames, max_rows, row_stride, first_slot;
    int32_t frame_h, frame_w, detect_every, start_after_n;
    int32_t mesh_every, budget_frames;
    float start_conf, start_min_size, min_det_side, min_det_area, bottom_limit, reserved;
    double min_track_side, crop_scale;
    int32_t frame_idx[AF_RUNNER_MAX_FRAMES];
} af_runner_chunk;
int64_t af_runner_state_bytes(void);
int64_t af_runner_record_bytes(int n_frames);
int af_runner_reset(void* host_state, double track_thresh, double match_thresh, int buffer_size, int started);
int af_runner_track_chunk(const af_runner_chunk* chunk, void* stream);
int af_runner_track_chunk_host(const af_runner_chunk* chunk);
int af_face_quality_table_u8(const af_store_ref* store, void* record, int capacity, int full, af_quality_sums* sums, void* grey,
                             int64_t grey_stride, void* stream);

/* ---- a live tick's face stage on the device (added within ABI 6) ------------------------------------------------------------------
 * What RealtimeCall / CallServer do on the host per call between the tracker and the quality launch - live.track_candidates: the
 * self-view exclusion, the five-point pick, the mesh_every cache and get_crop_box (af_realtime.py:390-437) - behind
 * the tracker's update in the SAME launch, one wave per call (csrc/af_live_core.h, csrc/af_live.hip; the statement is
 * live.track_candidates itself, driven as tests/live_cands_ref.py drives it).
 *
 * A call's state is af_live_state_bytes() bytes (8-byte aligned): the tracker's state block first - every af_bytetrack_* entry
 * works on it - then the five-point cache, one entry per tracker slot tagged with the track id it belongs to.  af_live_reset fills
 * a HOST block; a device state is a copy of one.
 *
 * af_live_call (host, travels in the launch arguments): `track` is the tracker's call on that state, in any of its forms, and is
 * run unchanged.  The candidate stage then walks the tracks the update returned, in the tracker's order:
 *   exclusion  exclude = (x1n, y1n, x2n, y2n): a track whose fp64 centre (0.5 * (x1 + x2), 0.5 * (y1 + y2)) has
 *              x1n * frame_w <= cx <= x2n * frame_w and y1n * frame_h <= cy <= y2n * frame_h, all in fp64, is neither alive nor kept;
 *   rows       with the LIST form the frame's rows are ALL *count_ptr (or count) rows, cut at max_rows, not only those past the
 *              start filter (row_stride >= 15; max_rows * row_stride <= rows_floats); column c of a row is scaled back as
 *              YuNet.scale_rows does it - by scale_x for even c, scale_y for odd c, 1 for column 14, an fp64 product cast to float32 -
 *              and a row's box is the float32 (x, y, x + w, y + h).  With any other form, or with no row, there are no points;
 *   pick       the row of highest IoU (+ 1 convention, fp64 on the widened float32 boxes) with the float32 cast of the track's
 *              box, the first of equals, if that IoU is 0.4 or more: its columns 5 .. 14 are the track's five points;
 *   cache      on a frame with frame_idx % mesh_every == 0, or for a track without a cache entry: the picked points, which are
 *              cached (flag REFRESHED), or, without any, the track is skipped (NO_POINTS) even when an entry exists; otherwise the
 *              cached points.  Before the frame the entries of the tids in purged[0 .. n_purged) are dropped;
 *   crop box   get_crop_box((frame_h, frame_w), the float32 box, crop_scale) in fp64; an empty one is skipped (EMPTY_BOX).
 * An excluded track carries only EXCLUDED; every other one is alive and kept; the CANDIDATE ones are the frame's candidates.
 *
 * Per call the launch writes the tracker's record (af_bytetrack_record_bytes()) and one af_live_record: the header - frame_idx,
 * slot (the ring slot of the frame, as handed in), n_online, n_cands, tiles (the tile total of the half-size quality launch),
 * overflow (the tracker's code; then n_online is 0), bad (set by af_face_quality_records_u8) - and one entry per returned track:
 * tid, flags, the float32 box, the ten float32 points, the crop box (x1, y1, x2, y2), the first tile of its half-size image (of
 * every entry the tiles of the candidates in front of it, so the prefixes ascend) and its index among the frame's candidates
 * (-1 for the others).  Entries behind n_online are zero.  Nothing is written outside the
 * states and the records.
 * af_live_update_calls: `calls` is a HOST array of 1 .. AF_TRACK_MAX_CALLS entries; states, rows, counts and records are DEVICE
 * memory; as many launches as the calls need (af_live_calls_per_launch() calls fit one launch's arguments).
 * af_live_update_host: the same source on the CPU for one call over host memory.
 *
 * af_face_quality_records_u8: af_face_quality_stores_u8 with its rectangles read from af_live_records in DEVICE memory.  jobs
 * (HOST, 0 .. AF_QUALITY_MAX_RECTS of them): job j's candidates are those of jobs[j].record, rectangles of frame jobs[j].slot of
 * stores[jobs[j].store].  Candidate k of job j adds to sums[j * AF_TRACK_MAX_TRACKS + k]; all n_jobs * AF_TRACK_MAX_TRACKS sums
 * are cleared on `stream` first.  A fixed grid: a workgroup reads the jobs' tile totals, forms their prefix and finds the job and
 * then the candidate of each of its tiles by bisection.  It re-checks every candidate against its store: a slot outside the
 * store, a rectangle that leaves its frame or a tile prefix that does not fit is skipped - never read - and flagged (the entry's
 * AF_LIVE_BAD, the header's bad).  Stores of different sizes, pitches and byte orders may share a launch.  grey: null, or (tests)
 * a DEVICE buffer of n_jobs * AF_TRACK_MAX_TRACKS * grey_stride bytes; the half-size grey image of candidate k of job j goes to
 * grey + (j * AF_TRACK_MAX_TRACKS + k) * grey_stride when it fits grey_stride. */
#define AF_LIVE_EXCLUDED 1
#define AF_LIVE_NO_POINTS 2
#define AF_LIVE_EMPTY_BOX 4
#define AF_LIVE_CANDIDATE 8
#define AF_LIVE_REFRESHED 16
#define AF_LIVE_BAD 32
typedef struct af_live_call {
    af_track_call track;
    int64_t rows_floats;
    int32_t frame_idx, slot, mesh_every, frame_h, frame_w, n_purged;
    double crop_scale;
    double exclude[4];
    int32_t purged[AF_TRACK_MAX_TRACKS];
} af_live_call;
typedef struct af_live_entry {
    int32_t tid, flags;
    float tlbr[4];
    float lm5[10];
    int32_t box[4];
    int32_t first_tile, cand;
} af_live_entry;
typedef struct af_live_record {
    int32_t frame_idx, slot, n_online, n_cands;
    int32_t tiles, bad, overflow, reserved;
    af_live_entry online[AF_TRACK_MAX_TRACKS];
} af_live_record;
typedef struct af_live_quality_job {
    void* record;                  /* device pointer of an af_live_record */
    int32_t store, slot;
} af_live_quality_job;
int64_t af_live_state_bytes(void);
int64_t af_live_record_bytes(void);
int af_live_calls_per_launch(void);
int af_live_reset(void* host_state, double track_thresh, double match_thresh, int buffer_size);
int af_live_update_calls(const af_live_call* calls, int n_calls, void* track_records, void* records, void* stream);
int af_live_update_host(const af_live_call* call, void* track_record, void* record);
int af_face_quality_records_u8(const af_store_ref* stores, int n_stores, const af_live_quality_job* jobs, int n_jobs, af_quality_sums* sums,
                               void* grey, int64_t grey_stride, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* AF_HIP_H */
