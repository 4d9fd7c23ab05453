// RetinaFace (mobilenet0.25, test_tools/ct/detection/alignment.py: RetinaFace(cfg_mnet, phase="test")) and batch_detect's
// post_process for a batch of uint8 HWC frames of one size: the offline evaluator's detector (detect_all).  fp32 throughout,
// activations NHWC, BN folded into the convolutions on the host (retinaface.py: pack_weights).
//
// Launch sequence (af_retinaface_detect, one stream, no host synchronisation or allocation):
//   1. rf_stem            : uint8 frame - (104, 117, 123) by channel index -> 3x3/2 conv 3->8 + LeakyReLU(0.1)
//   2. 13 x (rf_dw, rf_conv<1x1>): MobileNetV1's conv_dw: depthwise 3x3 (stride 1 or 2) + LeakyReLU, then 1x1 on MFMA
//   3. FPN                : three 1x1 (+ nearest up-sampled coarser level in the epilogue) and two 3x3 merges, MFMA
//   4. SSH x 3            : five dense 3x3 per level, MFMA; the three concat branches are stored at their channel offsets
//                           with the ReLU applied in the epilogue
//   5. heads x 3          : one 1x1 64 -> 32 (bbox 8 | class 4 | landmarks 20) per level whose epilogue writes the
//                           (level, row, col, anchor)-ordered loc / conf / landms planes directly
//   6. rf_decode          : softmax, PriorBox, decode / decode_landm, * [W, H]; anchors with score > 0.02 append a sort key
//   7. rf_sort            : per frame, the candidates sorted by (score desc, anchor index desc), cut to top_k = 5000
//   8. rf_nms_mask        : per frame, the upper-triangular "suppresses" bitmask of py_cpu_nms's overlap test (ovr > 0.4)
//   9. rf_nms_scan        : per frame, one wave walks the bitmask greedily and stops after min(keep_top_k, max_count) kept
//                           boxes or at the first kept score below min_score
// The dense convolutions are implicit GEMMs on v_mfma_f32_16x16x4_f32 (exact fp32 products and sums): A[pixel][k] with
// k = (tap, input channel), B[k][output channel] packed by the host so that each lane loads one float4 per 16 k.
#include "af_detect.h"

#include <algorithm>

namespace af {
namespace retinaface {

using detect::kSortHalf;
using detect::kSortLdsBytes;
using detect::kSortThreads;

constexpr int kThreads = 256;
constexpr int kMB = 4;                       // 16-pixel blocks per wave in rf_conv
constexpr int kTopK = AF_RETINAFACE_TOP_K;
constexpr int kWords = (kTopK + 63) / 64;    // bitmask words per NMS row
constexpr float kConf = 0.02f, kNms = 0.4f, kVar0 = 0.1f, kVar1 = 0.2f;
constexpr int kBlocks = 13;
// MobileNetV1 stage1..3 after the first conv_bn: (cin, cout, stride) of each conv_dw
constexpr int kBlockCin[kBlocks] = {8, 16, 32, 32, 64, 64, 128, 128, 128, 128, 128, 128, 256};
constexpr int kBlockCout[kBlocks] = {16, 32, 32, 64, 64, 128, 128, 128, 128, 128, 128, 256, 256};
constexpr int kBlockStride[kBlocks] = {1, 2, 1, 2, 1, 2, 1, 1, 1, 1, 1, 2, 1};
constexpr int kTapBlock[3] = {4, 10, 12};    // blocks whose output is the FPN input of stride 8, 16, 32
constexpr int kLaunches = 1 + 2 * kBlocks + 5 + 15 + 3 + 4;
constexpr int kPostLaunches = 5;
static_assert(AF_RETINAFACE_LAUNCHES == kLaunches, "header launch count");
static_assert(AF_RETINAFACE_POST_LAUNCHES == kPostLaunches, "header post-process launch count");
static_assert(kTopK <= kSortHalf, "the chunked sort keeps kSortHalf keys");
static_assert(kWords <= 128, "a scan lane holds two bitmask words");

// ---- weight blob layout (retinaface.py pack_weights builds the same order)
// stem: [ky][kx][ci][8] + bias[8]; depthwise: [9][C] + bias[C]; MFMA conv: ks*ks*cinp*cout packed B fragments + bias[cout]
constexpr int cin_pad(int c) { return (c + 15) / 16 * 16; }
constexpr int64_t mfma_floats(int ks, int cin, int cout) { return (int64_t)ks * ks * cin_pad(cin) * cout + cout; }
constexpr int64_t dw_floats(int c) { return 10LL * c; }
constexpr int64_t kStemFloats = 27 * 8 + 8;
struct Layout {
    int64_t stem, dw[kBlocks], pw[kBlocks], fpn_out[3], fpn_merge[2], ssh[3][5], head[3], total;
};
constexpr int kSshCin[5] = {64, 64, 16, 16, 16};
constexpr int kSshCout[5] = {32, 16, 16, 16, 16};
static Layout make_layout() {
    Layout L{};
    int64_t o = 0;
    L.stem = o;
    o += kStemFloats;
    for (int i = 0; i < kBlocks; ++i) {
        L.dw[i] = o;
        o += dw_floats(kBlockCin[i]);
        L.pw[i] = o;
        o += mfma_floats(1, kBlockCin[i], kBlockCout[i]);
    }
    const int fin[3] = {64, 128, 256};
    for (int l = 0; l < 3; ++l) {
        L.fpn_out[l] = o;
        o += mfma_floats(1, fin[l], 64);
    }
    for (int l = 0; l < 2; ++l) {
        L.fpn_merge[l] = o;
        o += mfma_floats(3, 64, 64);
    }
    for (int l = 0; l < 3; ++l)
        for (int k = 0; k < 5; ++k) {
            L.ssh[l][k] = o;
            o += mfma_floats(3, kSshCin[k], kSshCout[k]);
        }
    for (int l = 0; l < 3; ++l) {
        L.head[l] = o;
        o += mfma_floats(1, 64, 32);
    }
    L.total = o;
    return L;
}

enum Act { kNone = 0, kLeaky = 1, kRelu = 2 };

template <int ACT> __device__ __forceinline__ float act_f(float v) {
    if (ACT == kLeaky) return v > 0.f ? v : v * 0.1f;      // torch leaky_relu: x > 0 ? x : x * negative_slope
    if (ACT == kRelu) return relu_f(v);
    return v;
}

struct StemArgs {
    const uint8_t* frames;
    long long frame_stride, row_pitch;
    int h, w, ho, wo;
    const float* wt;     // [ky][kx][ci][8] + bias[8]
    float* out;          // [B][ho][wo][8]
    int* counts;         // per-frame candidate counters, zeroed here
};

// conv_bn(3, 8, 2, leaky=0.1) on the mean-subtracted frame; taps outside the frame are 0 (padding after the subtraction)
__global__ __launch_bounds__(kThreads) void rf_stem(StemArgs a) {
    const int b = blockIdx.y;
    if (blockIdx.x == 0 && threadIdx.x == 0) a.counts[b] = 0;
    const int p = blockIdx.x * kThreads + threadIdx.x;
    if (p >= a.ho * a.wo) return;
    const int y = p / a.wo, x = p - y * a.wo;
    const uint8_t* img = a.frames + (long long)b * a.frame_stride;
    const float mean[3] = {104.f, 117.f, 123.f};
    float s[8];
#pragma unroll
    for (int o = 0; o < 8; ++o) s[o] = a.wt[216 + o];
#pragma unroll
    for (int ky = 0; ky < 3; ++ky) {
        const int iy = 2 * y - 1 + ky;
        if (iy < 0 || iy >= a.h) continue;
#pragma unroll
        for (int kx = 0; kx < 3; ++kx) {
            const int ix = 2 * x - 1 + kx;
            if (ix < 0 || ix >= a.w) continue;
            const uint8_t* px = img + (long long)iy * a.row_pitch + ix * 3;
#pragma unroll
            for (int ci = 0; ci < 3; ++ci) {
                const float v = (float)px[ci] - mean[ci];
#pragma unroll
                for (int o = 0; o < 8; ++o) s[o] = fmaf(v, a.wt[((ky * 3 + kx) * 3 + ci) * 8 + o], s[o]);
            }
        }
    }
    float4* dst = reinterpret_cast<float4*>(a.out + ((size_t)b * a.ho * a.wo + p) * 8);
    dst[0] = make_float4(act_f<kLeaky>(s[0]), act_f<kLeaky>(s[1]), act_f<kLeaky>(s[2]), act_f<kLeaky>(s[3]));
    dst[1] = make_float4(act_f<kLeaky>(s[4]), act_f<kLeaky>(s[5]), act_f<kLeaky>(s[6]), act_f<kLeaky>(s[7]));
}

struct DwArgs {
    const float* in;     // [B][hi][wi][C]
    const float* wt;     // [9][C] + bias[C]
    float* out;          // [B][ho][wo][C]
    int hi, wi, ho, wo, stride;
};

// depthwise 3x3 (pad 1) + LeakyReLU(0.1): one thread per output pixel x 4 channels
template <int C>
__global__ __launch_bounds__(kThreads) void rf_dw(DwArgs a) {
    constexpr int G = C / 4;
    const int b = blockIdx.y;
    const int it = blockIdx.x * kThreads + threadIdx.x;
    if (it >= a.ho * a.wo * G) return;
    const int g = it % G, p = it / G, y = p / a.wo, x = p - y * a.wo;
    const float* in = a.in + (size_t)b * a.hi * a.wi * C;
    float4 acc = *reinterpret_cast<const float4*>(a.wt + 9 * C + 4 * g);
#pragma unroll
    for (int ky = 0; ky < 3; ++ky) {
        const int iy = y * a.stride - 1 + ky;
        if (iy < 0 || iy >= a.hi) continue;
#pragma unroll
        for (int kx = 0; kx < 3; ++kx) {
            const int ix = x * a.stride - 1 + kx;
            if (ix < 0 || ix >= a.wi) continue;
            const float4 v = *reinterpret_cast<const float4*>(in + ((size_t)iy * a.wi + ix) * C + 4 * g);
            const float4 k = *reinterpret_cast<const float4*>(a.wt + (ky * 3 + kx) * C + 4 * g);
            acc.x = fmaf(v.x, k.x, acc.x); acc.y = fmaf(v.y, k.y, acc.y); acc.z = fmaf(v.z, k.z, acc.z); acc.w = fmaf(v.w, k.w, acc.w);
        }
    }
    *reinterpret_cast<float4*>(a.out + ((size_t)b * a.ho * a.wo + p) * C + 4 * g) =
        make_float4(act_f<kLeaky>(acc.x), act_f<kLeaky>(acc.y), act_f<kLeaky>(acc.z), act_f<kLeaky>(acc.w));
}

// one output segment of rf_conv: channels [c0, next segment's c0) go to ptr + b * bstride + pixel * ld + (ch - c0)
struct Seg {
    float* ptr;
    long long bstride;
    int ld, c0;
};

struct ConvArgs {
    const float* in;     // [B][h][w][CIN]
    const float* wt;     // packed B fragments [chunk][cout / 16][64 lanes][4] + bias[cout]
    int h, w, cout, act;
    const float* add;    // optional: + add[b][y >> 1][x >> 1][ch] (ld cout) after the activation (FPN's nearest up-sampling)
    int ah, aw;
    int nseg;
    Seg seg[3];
};

// stride-1 KSxKS conv (pad KS / 2) + bias + activation on MFMA.  A wave computes kMB x 16 consecutive pixels of one frame
// by NB x 16 output channels; the 4 waves of a block take consecutive pixel runs; blockIdx.y picks the channel group.
template <int KS, int CIN, int NB, int ACT>
__global__ __launch_bounds__(kThreads) void rf_conv(ConvArgs a) {
    constexpr int CINP = cin_pad(CIN), CH = CINP / 16, PAD = KS / 2;
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, col = lane & 15, kq = lane >> 4;
    const int b = blockIdx.z, hw = a.h * a.w;
    const int base = (blockIdx.x * (kThreads / 64) + wave) * kMB * 16;
    if (base >= hw) return;
    const int nb0 = blockIdx.y * NB, nbt = a.cout / 16;
    const float* in = a.in + (size_t)b * hw * CIN;
    int py[kMB], px[kMB];
#pragma unroll
    for (int m = 0; m < kMB; ++m) {
        const int p = base + m * 16 + col;
        py[m] = p < hw ? p / a.w : -(1 << 20);         // a pixel past the map reads only zero taps
        px[m] = p < hw ? p - py[m] * a.w : 0;
    }
    f32x4 acc[kMB][NB];
#pragma unroll
    for (int m = 0; m < kMB; ++m)
#pragma unroll
        for (int n = 0; n < NB; ++n) acc[m][n] = f32x4{0.f, 0.f, 0.f, 0.f};
    const float4* wb = reinterpret_cast<const float4*>(a.wt);
#pragma unroll 1
    for (int tap = 0; tap < KS * KS; ++tap) {
        const int dy = tap / KS - PAD, dx = tap % KS - PAD;
        const float* src[kMB];
#pragma unroll
        for (int m = 0; m < kMB; ++m) {
            const int y = py[m] + dy, x = px[m] + dx;
            src[m] = (y >= 0 && y < a.h && x >= 0 && x < a.w) ? in + ((size_t)y * a.w + x) * CIN : nullptr;
        }
#pragma unroll
        for (int c = 0; c < CH; ++c) {
            const int ci = c * 16 + kq * 4;
            float4 av[kMB], bv[NB];
#pragma unroll
            for (int m = 0; m < kMB; ++m)
                av[m] = (src[m] && ci < CIN) ? *reinterpret_cast<const float4*>(src[m] + ci) : make_float4(0.f, 0.f, 0.f, 0.f);
#pragma unroll
            for (int n = 0; n < NB; ++n) bv[n] = wb[((size_t)(tap * CH + c) * nbt + nb0 + n) * 64 + lane];
#pragma unroll
            for (int m = 0; m < kMB; ++m)
#pragma unroll
                for (int n = 0; n < NB; ++n) {
                    acc[m][n] = __builtin_amdgcn_mfma_f32_16x16x4f32(av[m].x, bv[n].x, acc[m][n], 0, 0, 0);
                    acc[m][n] = __builtin_amdgcn_mfma_f32_16x16x4f32(av[m].y, bv[n].y, acc[m][n], 0, 0, 0);
                    acc[m][n] = __builtin_amdgcn_mfma_f32_16x16x4f32(av[m].z, bv[n].z, acc[m][n], 0, 0, 0);
                    acc[m][n] = __builtin_amdgcn_mfma_f32_16x16x4f32(av[m].w, bv[n].w, acc[m][n], 0, 0, 0);
                }
        }
    }
    const float* bias = a.wt + (size_t)KS * KS * CINP * a.cout;
#pragma unroll
    for (int n = 0; n < NB; ++n) {
        const int ch = (nb0 + n) * 16 + col;
        const float bs = bias[ch];
        int s = 0;
        while (s + 1 < a.nseg && ch >= a.seg[s + 1].c0) ++s;
        const Seg sg = a.seg[s];
        float* outb = sg.ptr + (size_t)b * sg.bstride + (ch - sg.c0);
#pragma unroll
        for (int m = 0; m < kMB; ++m)
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                const int p = base + m * 16 + kq * 4 + r;
                if (p >= hw) continue;
                float v = act_f<ACT>(acc[m][n][r] + bs);
                if (a.add) {
                    const int y = p / a.w, x = p - y * a.w;
                    v += a.add[(((size_t)b * a.ah + (y >> 1)) * a.aw + (x >> 1)) * a.cout + ch];
                }
                outb[(size_t)p * sg.ld] = v;
            }
    }
}

struct DecodeArgs {
    const float* loc;    // [B][A][4]
    float* conf;         // [B][A][2]: logits (softmax = 1, replaced in place by the softmax) or probabilities
    const float* landms; // [B][A][10]
    int softmax;
    int h, w, anchors;
    int lvl_w[3], lvl_off[4];
    int* counts;
    unsigned long long* keys;   // [B][A]
    float* rows;                // [B][A][16]: x1 y1 x2 y2 score l0x .. l4y, indexed by anchor
};

// PriorBox.forward for one anchor: computed in double as the reference's Python floats, rounded to fp32 by torch.Tensor
__device__ __forceinline__ float4 prior(int a, const DecodeArgs& d) {
    const int l = a < d.lvl_off[1] ? 0 : a < d.lvl_off[2] ? 1 : 2;
    const int idx = a - d.lvl_off[l], pix = idx >> 1, k = idx & 1;
    const int i = pix / d.lvl_w[l], j = pix - i * d.lvl_w[l];
    const double step = (double)(8 << l), min_size = (double)(16 << (2 * l + k));
    return make_float4((float)(((double)j + 0.5) * step / (double)d.w), (float)(((double)i + 0.5) * step / (double)d.h),
                       (float)(min_size / (double)d.w), (float)(min_size / (double)d.h));
}

// softmax, decode / decode_landm in the reference's fp32 operation order (no contraction), * [W, H, W, H], score > 0.02
__global__ __launch_bounds__(kThreads) void rf_decode(DecodeArgs d) {
    const int b = blockIdx.y, a = blockIdx.x * kThreads + threadIdx.x;
    if (a >= d.anchors) return;
    const size_t ia = (size_t)b * d.anchors + a;
    float score;
    if (d.softmax) {
        const float c0 = d.conf[ia * 2], c1 = d.conf[ia * 2 + 1];
        const float mx = fmaxf(c0, c1), e0 = expf(__fsub_rn(c0, mx)), e1 = expf(__fsub_rn(c1, mx)), s = __fadd_rn(e0, e1);
        score = __fdiv_rn(e1, s);
        d.conf[ia * 2] = __fdiv_rn(e0, s);
        d.conf[ia * 2 + 1] = score;
    } else {
        score = d.conf[ia * 2 + 1];
    }
    if (!(score > kConf)) return;
    const float4 p = prior(a, d);
    const float W = (float)d.w, H = (float)d.h;
    const float* lc = d.loc + ia * 4;
    const float cx = __fadd_rn(p.x, __fmul_rn(__fmul_rn(lc[0], kVar0), p.z));
    const float cy = __fadd_rn(p.y, __fmul_rn(__fmul_rn(lc[1], kVar0), p.w));
    const float bw = __fmul_rn(p.z, expf(__fmul_rn(lc[2], kVar1)));
    const float bh = __fmul_rn(p.w, expf(__fmul_rn(lc[3], kVar1)));
    const float x1 = __fsub_rn(cx, __fdiv_rn(bw, 2.f)), y1 = __fsub_rn(cy, __fdiv_rn(bh, 2.f));
    float row[16];
    row[0] = __fmul_rn(x1, W);
    row[1] = __fmul_rn(y1, H);
    row[2] = __fmul_rn(__fadd_rn(bw, x1), W);
    row[3] = __fmul_rn(__fadd_rn(bh, y1), H);
    row[4] = score;
    const float* lm = d.landms + ia * 10;
#pragma unroll
    for (int n = 0; n < 5; ++n) {
        row[5 + 2 * n] = __fmul_rn(__fadd_rn(p.x, __fmul_rn(__fmul_rn(lm[2 * n], kVar0), p.z)), W);
        row[6 + 2 * n] = __fmul_rn(__fadd_rn(p.y, __fmul_rn(__fmul_rn(lm[2 * n + 1], kVar0), p.w)), H);
    }
    row[15] = 0.f;
    float4* dst = reinterpret_cast<float4*>(d.rows + ia * 16);
#pragma unroll
    for (int k = 0; k < 4; ++k) dst[k] = make_float4(row[4 * k], row[4 * k + 1], row[4 * k + 2], row[4 * k + 3]);
    // ascending u64 order = score descending (positive float bits, inverted), then anchor index descending
    const unsigned long long key = ((unsigned long long)(~__float_as_uint(score)) << 32) | (unsigned)(~(unsigned)a);
    const int slot = atomicAdd(d.counts + b, 1);
    d.keys[(size_t)b * d.anchors + slot] = key;      // slot < anchors: each anchor appends at most once
}

__global__ void rf_zero_counts(int* counts, int n) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i < n) counts[i] = 0;
}

struct SortArgs {
    const int* counts;
    const unsigned long long* keys;
    const float* rows;
    int anchors;
    int* m;                     // [B] candidates after the top_k cut
    unsigned long long* skeys;  // [B][kTopK]
    float4* sboxes;             // [B][kTopK]
};

// Per frame (one block): the candidate keys are sorted in LDS (detect::sort_keys); the first min(n, top_k) keys and their
// boxes are written in order.
__global__ __launch_bounds__(kSortThreads) void rf_sort(SortArgs a) {
    extern __shared__ unsigned long long lds[];
    const int b = blockIdx.x, tid = threadIdx.x;
    const int n = min(a.counts[b], a.anchors);
    detect::sort_keys(a.keys + (size_t)b * a.anchors, n, lds);
    const int m = min(n, kTopK);
    for (int i = tid; i < m; i += kSortThreads) {
        const unsigned long long key = lds[i];
        const unsigned anchor = ~(unsigned)key;
        a.skeys[(size_t)b * kTopK + i] = key;
        a.sboxes[(size_t)b * kTopK + i] = *reinterpret_cast<const float4*>(a.rows + ((size_t)b * a.anchors + anchor) * 16);
    }
    if (tid == 0) a.m[b] = m;
}

// py_cpu_nms's overlap test in fp32, in its operation order: areas with +1, ovr = inter / (a_i + a_j - inter)
__device__ __forceinline__ float area_of(float4 q) {
    return __fmul_rn(__fadd_rn(__fsub_rn(q.z, q.x), 1.f), __fadd_rn(__fsub_rn(q.w, q.y), 1.f));
}
__device__ __forceinline__ bool suppresses(float4 p, float ap, float4 q, float aq) {
    const float xx1 = fmaxf(p.x, q.x), yy1 = fmaxf(p.y, q.y), xx2 = fminf(p.z, q.z), yy2 = fminf(p.w, q.w);
    const float iw = fmaxf(0.f, __fadd_rn(__fsub_rn(xx2, xx1), 1.f)), ih = fmaxf(0.f, __fadd_rn(__fsub_rn(yy2, yy1), 1.f));
    const float inter = __fmul_rn(iw, ih);
    const float ovr = __fdiv_rn(inter, __fsub_rn(__fadd_rn(ap, aq), inter));
    return !(ovr <= kNms);
}

struct MaskArgs {
    const int* m;
    const float4* sboxes;
    unsigned long long* mask;   // [B][kTopK][kWords]: bit j of row i = box i suppresses box j (j > i)
};

// grid (kWords column blocks, kWords row blocks, B), 64 threads: thread t of block (cb, rb) fills word cb of row rb * 64 + t
__global__ __launch_bounds__(64) void rf_nms_mask(MaskArgs a) {
    __shared__ float4 cbox[64];
    __shared__ float carea[64];
    const int b = blockIdx.z, rb = blockIdx.y, cb = blockIdx.x, t = threadIdx.x;
    const int m = a.m[b];
    if (cb < rb || cb * 64 >= m) return;
    const float4* bx = a.sboxes + (size_t)b * kTopK;
    const int jc = cb * 64 + t;
    if (jc < m) {
        cbox[t] = bx[jc];
        carea[t] = area_of(cbox[t]);
    }
    __syncthreads();
    const int i = rb * 64 + t;
    if (i >= m) return;
    const float4 p = bx[i];
    const float ap = area_of(p);
    const int jn = min(64, m - cb * 64);
    unsigned long long bits = 0;
    for (int k = (cb == rb ? t + 1 : 0); k < jn; ++k)
        if (suppresses(p, ap, cbox[k], carea[k])) bits |= 1ull << k;
    a.mask[((size_t)b * kTopK + i) * kWords + cb] = bits;
}

struct ScanArgs {
    const int* m;
    const unsigned long long* skeys;
    const unsigned long long* mask;
    const float* rows;
    int anchors, limit, max_rows;
    double min_score;
    float* out_rows;     // [B][max_rows][15]
    int* out_count;      // [B]
};

// greedy NMS over the bitmask by one wave per frame: lane l holds the "removed" words l and l + 64
__global__ __launch_bounds__(64) void rf_nms_scan(ScanArgs a) {
    const int b = blockIdx.x, lane = threadIdx.x;
    const int m = a.m[b], nwords = (m + 63) / 64;
    const unsigned long long* mk = a.mask + (size_t)b * kTopK * kWords;
    const float* rows = a.rows + (size_t)b * a.anchors * 16;
    float* out = a.out_rows + (size_t)b * a.max_rows * 15;
    unsigned long long r0 = 0, r1 = 0;
    int nk = 0;
    for (int i = 0; i < m && nk < a.limit; ++i) {
        const int wi = i >> 6;
        const unsigned long long lo = __shfl(r0, wi & 63), hi = __shfl(r1, wi & 63);
        if (((wi < 64 ? lo : hi) >> (i & 63)) & 1ull) continue;
        const unsigned long long key = a.skeys[(size_t)b * kTopK + i];
        const float* r = rows + (size_t)(~(unsigned)key) * 16;
        if ((double)r[4] < a.min_score) break;          // scores descend: get_valid_faces drops the tail
        if (lane < 15) out[(size_t)nk * 15 + lane] = r[lane];
        const unsigned long long* row = mk + (size_t)i * kWords;
        if (lane >= wi && lane < nwords) r0 |= row[lane];
        if (lane + 64 >= wi && lane + 64 < nwords) r1 |= row[lane + 64];
        ++nk;
    }
    if (lane == 0) a.out_count[b] = nk;
}

// ---- host side
struct Plan {
    int B, h, w;
    int h1, w1, lh[3], lw[3];     // stride-2 map; levels (stride 8, 16, 32)
    int anchors, lvl_off[4];
    size_t x_off, t_off, tap_off[3], o3_off, o2_off, m2_off, o1_off, m1_off, cat_off, c51_off, c72_off, planes_off;   // floats
    size_t counts_off, keys_off, rows_off, m_off, skeys_off, sboxes_off, mask_off, total_bytes;                      // bytes
};

static inline int cdiv2(int v) { return (v + 1) / 2; }

static Plan make_plan(const af_retinaface_desc& d) {
    Plan p{};
    p.B = d.batch;
    p.h = d.height;
    p.w = d.width;
    p.h1 = cdiv2(p.h);
    p.w1 = cdiv2(p.w);
    int hh = cdiv2(cdiv2(p.h1)), ww = cdiv2(cdiv2(p.w1));    // stride 8 = ceil(h / 8)
    for (int l = 0; l < 3; ++l) {
        p.lh[l] = hh;
        p.lw[l] = ww;
        p.lvl_off[l] = p.anchors;
        p.anchors += 2 * hh * ww;
        hh = cdiv2(hh);
        ww = cdiv2(ww);
    }
    p.lvl_off[3] = p.anchors;
    const size_t B = p.B;
    // largest backbone tensor that is not an FPN tap (ping-pong pair: x = block input / 1x1 output, t = depthwise output)
    size_t xmax = (size_t)p.h1 * p.w1 * 8, tmax = 0;
    {
        int h = p.h1, w = p.w1;
        for (int i = 0; i < kBlocks; ++i) {
            if (kBlockStride[i] == 2) {
                h = cdiv2(h);
                w = cdiv2(w);
            }
            tmax = std::max(tmax, (size_t)h * w * kBlockCin[i]);
            xmax = std::max(xmax, (size_t)h * w * kBlockCout[i]);
        }
    }
    size_t off = 0;
    auto take = [&](size_t floats) { const size_t o = off; off += (floats + 3) & ~(size_t)3; return o; };
    p.x_off = take(B * xmax);
    p.t_off = take(B * tmax);
    const int tap_ch[3] = {64, 128, 256};
    for (int l = 0; l < 3; ++l) p.tap_off[l] = take(B * p.lh[l] * p.lw[l] * tap_ch[l]);
    const size_t s8 = (size_t)p.lh[0] * p.lw[0], s16 = (size_t)p.lh[1] * p.lw[1], s32 = (size_t)p.lh[2] * p.lw[2];
    p.o3_off = take(B * s32 * 64);
    p.o2_off = take(B * s16 * 64);
    p.m2_off = take(B * s16 * 64);
    p.o1_off = take(B * s8 * 64);
    p.m1_off = take(B * s8 * 64);
    p.cat_off = take(B * s8 * 64);
    p.c51_off = take(B * s8 * 16);
    p.c72_off = take(B * s8 * 16);
    p.planes_off = take(B * p.anchors * 16);
    size_t bytes = off * 4;
    auto takeb = [&](size_t n) { const size_t o = bytes; bytes += (n + 15) & ~(size_t)15; return o; };
    p.counts_off = takeb(B * 4);
    p.keys_off = takeb(B * p.anchors * 8);
    p.rows_off = takeb(B * p.anchors * 64);
    p.m_off = takeb(B * 4);
    p.skeys_off = takeb(B * kTopK * 8);
    p.sboxes_off = takeb(B * kTopK * 16);
    p.mask_off = takeb(B * kTopK * kWords * 8);
    p.total_bytes = bytes;
    return p;
}

static int max_rows(const af_retinaface_desc& d) { return d.max_count > 0 ? std::min(d.keep_top_k, d.max_count) : d.keep_top_k; }

static int check_desc(const af_retinaface_desc* d, bool frames) {
    const int rc = detect::check_frames(d, "retinaface", AF_RETINAFACE_MAX_SIDE, frames);
    if (rc != AF_OK) return rc;
    AF_REQUIRE(d->keep_top_k >= 1 && d->keep_top_k <= AF_RETINAFACE_MAX_KEEP, "retinaface: keep_top_k %d out of [1, %d]",
               d->keep_top_k, AF_RETINAFACE_MAX_KEEP);
    AF_REQUIRE(d->min_score == d->min_score, "retinaface: NaN min_score");
    return AF_OK;
}

template <int KS, int CIN, int NB, int ACT>
static void launch_conv(int hw, int B, int cout, hipStream_t s, const ConvArgs& ca) {
    const dim3 grid((hw + kThreads / 64 * kMB * 16 - 1) / (kThreads / 64 * kMB * 16), cout / (16 * NB), B);
    hipLaunchKernelGGL((rf_conv<KS, CIN, NB, ACT>), grid, dim3(kThreads), 0, s, ca);
}

static ConvArgs conv_args(const float* in, const float* wt, int h, int w, int cout, int act, float* out, int ld = 0, int off = 0) {
    ConvArgs c{};
    c.in = in;
    c.wt = wt;
    c.h = h;
    c.w = w;
    c.cout = cout;
    c.act = act;
    c.nseg = 1;
    if (!ld) ld = cout;
    c.seg[0] = Seg{out + off, (long long)h * w * ld, ld, 0};
    return c;
}

// dispatch of the (kernel size, cin, cout, activation) combinations the network uses
static int run_conv(int ks, int cin, int B, hipStream_t s, const ConvArgs& c) {
    const int hw = c.h * c.w, cout = c.cout;
#define RF_CASE(KS_, CIN_, NB_, ACT_)                                                     \
    if (ks == KS_ && cin == CIN_ && NB_ == std::min(4, cout / 16) && cout % 16 == 0 && c.act == ACT_) { \
        launch_conv<KS_, CIN_, NB_, ACT_>(hw, B, cout, s, c);                              \
        AF_CHECK_LAUNCH("rf_conv");                                                        \
        return AF_OK;                                                                      \
    }
    RF_CASE(1, 8, 1, kLeaky)
    RF_CASE(1, 16, 2, kLeaky)
    RF_CASE(1, 32, 2, kLeaky)
    RF_CASE(1, 32, 4, kLeaky)
    RF_CASE(1, 64, 4, kLeaky)
    RF_CASE(1, 128, 4, kLeaky)
    RF_CASE(1, 256, 4, kLeaky)
    RF_CASE(3, 64, 4, kLeaky)
    RF_CASE(3, 64, 2, kRelu)
    RF_CASE(3, 64, 1, kLeaky)
    RF_CASE(3, 16, 1, kRelu)
    RF_CASE(3, 16, 1, kLeaky)
    RF_CASE(1, 64, 2, kNone)
#undef RF_CASE
    return set_error(AF_ERR_ARG, "retinaface: no conv kernel for %dx%d %d -> %d act %d", ks, ks, cin, cout, c.act);
}

template <int C>
static void launch_dw(int ho, int wo, int B, hipStream_t s, const DwArgs& da) {
    hipLaunchKernelGGL((rf_dw<C>), dim3((ho * wo * (C / 4) + kThreads - 1) / kThreads, B), dim3(kThreads), 0, s, da);
}

// decode + sort + NMS mask + scan (launches 6..9 of the sequence above)
static int post(const Plan& p, hipStream_t s, Marks& mark, const af_retinaface_desc* d, char* ws, const float* loc, float* conf,
                const float* landms, int softmax, float* out_rows, int32_t* out_count) {
    int* counts = (int*)(ws + p.counts_off);
    unsigned long long* keys = (unsigned long long*)(ws + p.keys_off);
    float* rows = (float*)(ws + p.rows_off);
    int* mm = (int*)(ws + p.m_off);
    unsigned long long* skeys = (unsigned long long*)(ws + p.skeys_off);
    float4* sboxes = (float4*)(ws + p.sboxes_off);
    unsigned long long* mask = (unsigned long long*)(ws + p.mask_off);
    DecodeArgs da{loc, conf, landms, softmax, p.h, p.w, p.anchors, {p.lw[0], p.lw[1], p.lw[2]},
                  {p.lvl_off[0], p.lvl_off[1], p.lvl_off[2], p.lvl_off[3]}, counts, keys, rows};
    hipLaunchKernelGGL(rf_decode, dim3((p.anchors + kThreads - 1) / kThreads, p.B), dim3(kThreads), 0, s, da);
    AF_CHECK_LAUNCH("rf_decode");
    mark();
    AF_SET_MAX_LDS(rf_sort, kSortLdsBytes, "rf_sort");
    SortArgs sa{counts, keys, rows, p.anchors, mm, skeys, sboxes};
    hipLaunchKernelGGL(rf_sort, dim3(p.B), dim3(kSortThreads), kSortLdsBytes, s, sa);
    AF_CHECK_LAUNCH("rf_sort");
    mark();
    MaskArgs ma{mm, sboxes, mask};
    hipLaunchKernelGGL(rf_nms_mask, dim3(kWords, kWords, p.B), dim3(64), 0, s, ma);
    AF_CHECK_LAUNCH("rf_nms_mask");
    mark();
    ScanArgs na{mm, skeys, mask, rows, p.anchors, max_rows(*d), max_rows(*d), d->min_score, out_rows, out_count};
    hipLaunchKernelGGL(rf_nms_scan, dim3(p.B), dim3(64), 0, s, na);
    AF_CHECK_LAUNCH("rf_nms_scan");
    mark();
    return AF_OK;
}

static int detect(const af_retinaface_desc* d, const float* weights, const void* frames, void* workspace, int64_t workspace_bytes,
                  float* out_rows, int32_t* out_count, float* raw, hipStream_t s, hipEvent_t* ev) {
    int rc = check_desc(d, true);
    if (rc != AF_OK) return rc;
    AF_REQUIRE(weights && frames && workspace && out_rows && out_count, "retinaface: null pointer");
    AF_REQUIRE(aligned16(weights) && aligned16(workspace) && aligned16(raw), "retinaface: weights / workspace / raw not 16-byte aligned");
    const Plan p = make_plan(*d);
    static const Layout L = make_layout();
    AF_REQUIRE(workspace_bytes >= (int64_t)p.total_bytes, "retinaface: workspace %lld bytes < %lld", (long long)workspace_bytes,
               (long long)p.total_bytes);
    char* ws = (char*)workspace;
    float* act = (float*)workspace;
    Marks mark{s, ev, 0};
    mark();
    const int B = p.B;

    StemArgs sa{(const uint8_t*)frames, d->frame_stride, d->row_pitch, p.h, p.w, p.h1, p.w1, weights + L.stem, act + p.x_off,
                (int*)(ws + p.counts_off)};
    hipLaunchKernelGGL(rf_stem, dim3((p.h1 * p.w1 + kThreads - 1) / kThreads, B), dim3(kThreads), 0, s, sa);
    AF_CHECK_LAUNCH("rf_stem");
    mark();

    // backbone: x -> dw -> t -> 1x1 -> x (or an FPN tap, which the next block then reads)
    const float* cur = act + p.x_off;
    int h = p.h1, w = p.w1;
    for (int i = 0; i < kBlocks; ++i) {
        const int st = kBlockStride[i], ho = st == 2 ? cdiv2(h) : h, wo = st == 2 ? cdiv2(w) : w;
        DwArgs da{cur, weights + L.dw[i], act + p.t_off, h, w, ho, wo, st};
        switch (kBlockCin[i]) {
            case 8: launch_dw<8>(ho, wo, B, s, da); break;
            case 16: launch_dw<16>(ho, wo, B, s, da); break;
            case 32: launch_dw<32>(ho, wo, B, s, da); break;
            case 64: launch_dw<64>(ho, wo, B, s, da); break;
            case 128: launch_dw<128>(ho, wo, B, s, da); break;
            default: launch_dw<256>(ho, wo, B, s, da); break;
        }
        AF_CHECK_LAUNCH("rf_dw");
        mark();
        float* out = act + p.x_off;
        for (int l = 0; l < 3; ++l)
            if (kTapBlock[l] == i) out = act + p.tap_off[l];
        rc = run_conv(1, kBlockCin[i], B, s, conv_args(act + p.t_off, weights + L.pw[i], ho, wo, kBlockCout[i], kLeaky, out));
        if (rc != AF_OK) return rc;
        mark();
        cur = out;
        h = ho;
        w = wo;
    }

    // FPN: output3; output2 + up(output3) -> merge2; output1 + up(merge2) -> merge1
    rc = run_conv(1, 256, B, s, conv_args(act + p.tap_off[2], weights + L.fpn_out[2], p.lh[2], p.lw[2], 64, kLeaky, act + p.o3_off));
    if (rc != AF_OK) return rc;
    mark();
    ConvArgs o2 = conv_args(act + p.tap_off[1], weights + L.fpn_out[1], p.lh[1], p.lw[1], 64, kLeaky, act + p.o2_off);
    o2.add = act + p.o3_off;
    o2.ah = p.lh[2];
    o2.aw = p.lw[2];
    rc = run_conv(1, 128, B, s, o2);
    if (rc != AF_OK) return rc;
    mark();
    rc = run_conv(3, 64, B, s, conv_args(act + p.o2_off, weights + L.fpn_merge[1], p.lh[1], p.lw[1], 64, kLeaky, act + p.m2_off));
    if (rc != AF_OK) return rc;
    mark();
    ConvArgs o1 = conv_args(act + p.tap_off[0], weights + L.fpn_out[0], p.lh[0], p.lw[0], 64, kLeaky, act + p.o1_off);
    o1.add = act + p.m2_off;
    o1.ah = p.lh[1];
    o1.aw = p.lw[1];
    rc = run_conv(1, 64, B, s, o1);
    if (rc != AF_OK) return rc;
    mark();
    rc = run_conv(3, 64, B, s, conv_args(act + p.o1_off, weights + L.fpn_merge[0], p.lh[0], p.lw[0], 64, kLeaky, act + p.m1_off));
    if (rc != AF_OK) return rc;
    mark();

    // SSH + heads per level; the heads write the three planes (the caller's raw buffer when given)
    float* planes = raw ? raw : act + p.planes_off;
    float* loc = planes;
    float* conf = planes + (size_t)B * p.anchors * 4;
    float* landms = planes + (size_t)B * p.anchors * 6;
    const size_t feat[3] = {p.m1_off, p.m2_off, p.o3_off};
    for (int l = 0; l < 3; ++l) {
        const int lh = p.lh[l], lw = p.lw[l];
        const float* x = act + feat[l];
        float* cat = act + p.cat_off;
        float* c51 = act + p.c51_off;
        float* c72 = act + p.c72_off;
        const ConvArgs ssh[5] = {
            conv_args(x, weights + L.ssh[l][0], lh, lw, 32, kRelu, cat, 64, 0),
            conv_args(x, weights + L.ssh[l][1], lh, lw, 16, kLeaky, c51),
            conv_args(c51, weights + L.ssh[l][2], lh, lw, 16, kRelu, cat, 64, 32),
            conv_args(c51, weights + L.ssh[l][3], lh, lw, 16, kLeaky, c72),
            conv_args(c72, weights + L.ssh[l][4], lh, lw, 16, kRelu, cat, 64, 48),
        };
        for (int k = 0; k < 5; ++k) {
            rc = run_conv(3, kSshCin[k], B, s, ssh[k]);
            if (rc != AF_OK) return rc;
            mark();
        }
        ConvArgs hd = conv_args(cat, weights + L.head[l], lh, lw, 32, kNone, loc);
        const long long A = p.anchors, o = p.lvl_off[l];
        hd.nseg = 3;
        hd.seg[0] = Seg{loc + o * 4, A * 4, 8, 0};
        hd.seg[1] = Seg{conf + o * 2, A * 2, 4, 8};
        hd.seg[2] = Seg{landms + o * 10, A * 10, 20, 12};
        rc = run_conv(1, 64, B, s, hd);
        if (rc != AF_OK) return rc;
        mark();
    }
    return post(p, s, mark, d, ws, loc, conf, landms, 1, out_rows, out_count);
}

static int postprocess(const af_retinaface_desc* d, const float* loc, const float* conf, const float* landms, void* workspace,
                       int64_t workspace_bytes, float* out_rows, int32_t* out_count, hipStream_t s, hipEvent_t* ev) {
    int rc = check_desc(d, false);
    if (rc != AF_OK) return rc;
    AF_REQUIRE(loc && conf && landms && workspace && out_rows && out_count, "retinaface_postprocess: null pointer");
    AF_REQUIRE(aligned16(workspace), "retinaface_postprocess: workspace not 16-byte aligned");
    const Plan p = make_plan(*d);
    AF_REQUIRE(workspace_bytes >= (int64_t)p.total_bytes, "retinaface_postprocess: workspace %lld bytes < %lld",
               (long long)workspace_bytes, (long long)p.total_bytes);
    Marks mark{s, ev, 0};
    mark();
    int* counts = (int*)((char*)workspace + p.counts_off);
    hipLaunchKernelGGL(rf_zero_counts, dim3((p.B + 255) / 256), dim3(256), 0, s, counts, p.B);
    AF_CHECK_LAUNCH("rf_zero_counts");
    mark();
    // conf is only read when softmax == 0
    return post(p, s, mark, d, (char*)workspace, loc, const_cast<float*>(conf), landms, 0, out_rows, out_count);
}

}  // namespace retinaface
}  // namespace af

extern "C" int64_t af_retinaface_weight_floats(void) { return af::retinaface::make_layout().total; }

extern "C" int64_t af_retinaface_anchors(const af_retinaface_desc* d) {
    if (af::retinaface::check_desc(d, false) != AF_OK) return 0;
    return af::retinaface::make_plan(*d).anchors;
}

extern "C" int32_t af_retinaface_max_rows(const af_retinaface_desc* d) {
    if (af::retinaface::check_desc(d, false) != AF_OK) return 0;
    return af::retinaface::max_rows(*d);
}

extern "C" int64_t af_retinaface_workspace_bytes(const af_retinaface_desc* d) {
    if (af::retinaface::check_desc(d, false) != AF_OK) return 0;
    return (int64_t)af::retinaface::make_plan(*d).total_bytes;
}

extern "C" int af_retinaface_detect(const af_retinaface_desc* d, const float* weights, const void* frames, void* workspace,
                                    int64_t workspace_bytes, float* out_rows, int32_t* out_count, float* raw, void* stream) {
    return af::retinaface::detect(d, weights, frames, workspace, workspace_bytes, out_rows, out_count, raw, (hipStream_t)stream,
                                  nullptr);
}

extern "C" int af_retinaface_detect_timed(const af_retinaface_desc* d, const float* weights, const void* frames, void* workspace,
                                          int64_t workspace_bytes, float* out_rows, int32_t* out_count, float* raw, void* stream,
                                          float* ms) {
    int rc = af::retinaface::check_desc(d, true);
    if (rc != AF_OK) return rc;
    hipStream_t s = (hipStream_t)stream;
    return af::timed("retinaface_detect_timed", s, AF_RETINAFACE_LAUNCHES, ms, [&](hipEvent_t* ev) {
        return af::retinaface::detect(d, weights, frames, workspace, workspace_bytes, out_rows, out_count, raw, s, ev);
    });
}

extern "C" int af_retinaface_postprocess(const af_retinaface_desc* d, const float* loc, const float* conf, const float* landms,
                                         void* workspace, int64_t workspace_bytes, float* out_rows, int32_t* out_count, void* stream) {
    return af::retinaface::postprocess(d, loc, conf, landms, workspace, workspace_bytes, out_rows, out_count, (hipStream_t)stream,
                                       nullptr);
}

extern "C" int af_retinaface_postprocess_timed(const af_retinaface_desc* d, const float* loc, const float* conf, const float* landms,
                                               void* workspace, int64_t workspace_bytes, float* out_rows, int32_t* out_count,
                                               void* stream, float* ms) {
    int rc = af::retinaface::check_desc(d, false);
    if (rc != AF_OK) return rc;
    hipStream_t s = (hipStream_t)stream;
    return af::timed("retinaface_postprocess_timed", s, AF_RETINAFACE_POST_LAUNCHES, ms, [&](hipEvent_t* ev) {
        return af::retinaface::postprocess(d, loc, conf, landms, workspace, workspace_bytes, out_rows, out_count, s, ev);
    });
}
