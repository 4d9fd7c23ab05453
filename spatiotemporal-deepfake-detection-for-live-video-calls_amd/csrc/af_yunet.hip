// YuNet-2023mar face detector (the live-call loop's per-frame detection stage): the whole network, OpenCV FaceDetectorYN's
// decode and dnn::NMSBoxes, for a batch of uint8 BGR frames of one size.  fp32 throughout, activations NHWC.
//
// Launch sequence (af_yunet_detect, one stream, no host synchronisation or allocation):
//   1. yunet_stem_unit0_pool : uint8 frame -> 3x3/2 conv + ReLU -> DP unit 0 -> MaxPool 2x2  (stride-2 maps stay in LDS)
//   2. yunet_dp_unit x 13     : 1x1 conv (linear, MFMA) + depthwise 3x3 + bias + ReLU; optional neck prologue x = a + up2(b);
//                               epilogue stores the full map, the 2x2-pooled map or both
//   3. yunet_head_decode x 3  : per level 1x1 64->16 (cls, obj, bbox 4, kps 10) + depthwise 3x3, sigmoid on cls / obj,
//                               decode, append candidates with score >= conf to the frame's list (key = score, anchor index)
//   4. yunet_sort_nms         : per frame, sort (score desc, anchor index asc), drop score <= conf, cut to top_k, greedy NMS
// A "DP unit" is YuNet's ConvDPUnit: Conv1x1 (bias, no activation) -> depthwise Conv3x3 (pad 1, bias) -> ReLU.  Zero padding
// of the depthwise conv applies to the 1x1 conv's OUTPUT (bias included), so halo pixels outside the map are 0 in LDS.
#include "af_detect.h"

namespace af {
namespace yunet {

using detect::kSortHalf;
using detect::kSortLdsBytes;
using detect::kSortThreads;

constexpr int kT = 16;                 // output tile edge, in pixels of the unit's own resolution
constexpr int kHalo = kT + 2;          // 1x1-conv tile incl. the depthwise conv's 1-pixel halo
constexpr int kThreads = 256;
constexpr int kUnits = 14;             // unit 0 lives in the stem kernel
constexpr int kUnitCin[kUnits] = {16, 16, 16, 32, 32, 64, 64, 64, 64, 64, 64, 64, 64, 64};
constexpr int kUnitCout[kUnits] = {16, 16, 32, 32, 64, 64, 64, 64, 64, 64, 64, 64, 64, 64};
constexpr int kHeadCh = 16;            // cls, obj, bbox[4], kps[10]
constexpr int kStemFloats = 27 * 16 + 16;
constexpr int kHeadFloats = 64 * kHeadCh + kHeadCh + 9 * kHeadCh + kHeadCh;
constexpr int kLaunches = 1 + (kUnits - 1) + 3 + 1;

static_assert(AF_YUNET_MAX_TOPK * 16 <= kSortLdsBytes, "kept boxes must fit the sort kernel's LDS");
static_assert(AF_YUNET_MAX_TOPK <= kSortHalf, "the chunked sort keeps kSortHalf keys");
static_assert(AF_YUNET_LAUNCHES == kLaunches, "header launch count");

constexpr int unit_floats(int u) { return kUnitCin[u] * kUnitCout[u] + kUnitCout[u] + 9 * kUnitCout[u] + kUnitCout[u]; }
constexpr int unit_offset(int u) { return u == 0 ? kStemFloats : unit_offset(u - 1) + unit_floats(u - 1); }
constexpr int kHeadOffset = unit_offset(kUnits);
constexpr int kWeightFloats = kHeadOffset + 3 * kHeadFloats;

struct StemArgs {
    const uint8_t* frames;
    long long frame_stride, row_pitch;
    int h, w;            // the frame
    int h2, w2;          // stride-2 map (padded frame / 2)
    int h4, w4;          // stride-4 output
    const float* wt;     // stem [ky][kx][ci][16] + bias, then unit 0
    float* out;          // [B][h4][w4][16]
    int* counts;         // per-frame candidate counters, zeroed here
};

struct UnitArgs {
    const float* in;     // [B][h][w][cin]
    const float* up;     // neck prologue: [B][h/2][w/2][cin] added with nearest x2 upsampling, or null
    const float* wt;     // 1x1 [cin][cout], bias [cout], depthwise [9][cout], bias [cout]
    float* out_full;     // [B][h][w][cout] or null
    float* out_pool;     // [B][h/2][w/2][cout] or null (h, w even)
    int h, w;
};

struct HeadArgs {
    const float* in;     // [B][h][w][64]
    const float* wt;     // 1x1 [64][16], bias [16], depthwise [9][16], bias [16]
    int h, w, stride, level_off, anchors;
    float conf;
    float* raw;          // [B][anchors][16] (cls, obj after sigmoid; bbox; kps) or null
    int* counts;
    unsigned long long* keys;
    long long keys_ld;
    float* rows;         // [B][anchors][16] decoded rows (15 used), indexed by anchor
};

struct NmsArgs {
    const int* counts;
    unsigned long long* keys;
    long long keys_ld;
    const float* rows;
    int anchors, top_k;
    float conf, nms;
    float* out_rows;     // [B][top_k][15]
    int* out_count;      // [B]
};

// 1x1 conv of 16 output channels [g*16, g*16+16) over the (kT+2)^2 halo tile into LDS mid[pixel][16]; pixels outside the
// h x w map are 0 (the depthwise conv's zero padding).  Weights are wave-uniform (scalar loads).
template <int CIN, int COUT>
__device__ __forceinline__ void pw_tile(const float* __restrict__ in, const float* __restrict__ up, const float* __restrict__ pw,
                                        const float* __restrict__ pb, int g, int y0, int x0, int h, int w, float* mid) {
    const int wh = w >> 1;
    for (int p = threadIdx.x; p < kHalo * kHalo; p += kThreads) {
        const int i = p / kHalo, j = p - i * kHalo, y = y0 + i, x = x0 + j;
        float4* dst = reinterpret_cast<float4*>(mid + p * 16);
        if (y < 0 || y >= h || x < 0 || x >= w) {
#pragma unroll
            for (int k = 0; k < 4; ++k) dst[k] = make_float4(0.f, 0.f, 0.f, 0.f);
            continue;
        }
        float acc[16];
#pragma unroll
        for (int k = 0; k < 16; ++k) acc[k] = pb[g * 16 + k];
        const float4* src = reinterpret_cast<const float4*>(in + ((size_t)y * w + x) * CIN);
        const float4* us = up ? reinterpret_cast<const float4*>(up + ((size_t)(y >> 1) * wh + (x >> 1)) * CIN) : nullptr;
#pragma unroll 4
        for (int c4 = 0; c4 < CIN / 4; ++c4) {
            float4 v = src[c4];
            if (us) {
                const float4 u = us[c4];
                v.x += u.x; v.y += u.y; v.z += u.z; v.w += u.w;
            }
            const float vv[4] = {v.x, v.y, v.z, v.w};
#pragma unroll
            for (int k = 0; k < 4; ++k) {
                const float* wr = pw + (c4 * 4 + k) * COUT + g * 16;
#pragma unroll
                for (int o = 0; o < 16; ++o) acc[o] = fmaf(vv[k], wr[o], acc[o]);
            }
        }
#pragma unroll
        for (int k = 0; k < 4; ++k) dst[k] = make_float4(acc[4 * k], acc[4 * k + 1], acc[4 * k + 2], acc[4 * k + 3]);
    }
}

// The same 1x1 tile on v_mfma_f32_16x16x4_f32 (exact fp32 products and sums, another summation order): each wave takes
// blocks of 16 halo pixels; A[pixel = lane & 15][k], B[k][channel = lane & 15], 16 k per float4 chunk (lane >> 4 picks the
// 4 k of a lane, instruction j its element j); D row = 4 * (lane >> 4) + r.  The bias is added after the K loop.
template <int CIN, int COUT>
__device__ __forceinline__ void pw_tile_mfma(const float* __restrict__ in, const float* __restrict__ up, const float* __restrict__ pw,
                                             const float* __restrict__ pb, int g, int y0, int x0, int h, int w, float* mid) {
    constexpr int kPix = kHalo * kHalo, kBlocks = (kPix + 15) / 16;
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, col = lane & 15, kq = lane >> 4;
    const int wh = w >> 1;
    float bw[CIN / 16][4];
#pragma unroll
    for (int c = 0; c < CIN / 16; ++c)
#pragma unroll
        for (int j = 0; j < 4; ++j) bw[c][j] = pw[(c * 16 + kq * 4 + j) * COUT + g * 16 + col];
    const float bias = pb[g * 16 + col];
    for (int blk = wave; blk < kBlocks; blk += kThreads / 64) {
        const int pa = blk * 16 + col, ia = pa / kHalo, ja = pa - ia * kHalo, ya = y0 + ia, xa = x0 + ja;
        const bool va = pa < kPix && ya >= 0 && ya < h && xa >= 0 && xa < w;
        f32x4 acc = {0.f, 0.f, 0.f, 0.f};
        const float4* src = va ? reinterpret_cast<const float4*>(in + ((size_t)ya * w + xa) * CIN) : nullptr;
        const float4* us = (va && up) ? reinterpret_cast<const float4*>(up + ((size_t)(ya >> 1) * wh + (xa >> 1)) * CIN) : nullptr;
#pragma unroll
        for (int c = 0; c < CIN / 16; ++c) {
            float4 v = va ? src[c * 4 + kq] : make_float4(0.f, 0.f, 0.f, 0.f);
            if (us) {
                const float4 u = us[c * 4 + kq];
                v.x += u.x; v.y += u.y; v.z += u.z; v.w += u.w;
            }
            acc = __builtin_amdgcn_mfma_f32_16x16x4f32(v.x, bw[c][0], acc, 0, 0, 0);
            acc = __builtin_amdgcn_mfma_f32_16x16x4f32(v.y, bw[c][1], acc, 0, 0, 0);
            acc = __builtin_amdgcn_mfma_f32_16x16x4f32(v.z, bw[c][2], acc, 0, 0, 0);
            acc = __builtin_amdgcn_mfma_f32_16x16x4f32(v.w, bw[c][3], acc, 0, 0, 0);
        }
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            const int p = blk * 16 + kq * 4 + r;
            if (p >= kPix) continue;
            const int i = p / kHalo, j = p - i * kHalo, y = y0 + i, x = x0 + j;
            mid[p * 16 + col] = (y >= 0 && y < h && x >= 0 && x < w) ? acc[r] + bias : 0.f;
        }
    }
}

// depthwise 3x3 + bias + ReLU of one 2x2 quad x 4 channels from an LDS tile mid[pixel][16] of row length `ld` pixels:
// win(r, c) = mid pixel (r0 + r, c0 + c), r, c in [0, 4); out[dy][dx] = output pixel (r0 + dy, c0 + dx) of the halo-less grid
__device__ __forceinline__ void dw_quad(const float* mid, int ld, int r0, int c0, int c4, const float* __restrict__ dw,
                                        const float* __restrict__ db, int ch, int cstride, float4 out[2][2]) {
    float4 win[4][4];
#pragma unroll
    for (int r = 0; r < 4; ++r)
#pragma unroll
        for (int c = 0; c < 4; ++c) win[r][c] = *reinterpret_cast<const float4*>(mid + ((r0 + r) * ld + c0 + c) * 16 + c4 * 4);
    const float4 bias = *reinterpret_cast<const float4*>(db + ch);
#pragma unroll
    for (int dy = 0; dy < 2; ++dy)
#pragma unroll
        for (int dx = 0; dx < 2; ++dx) {
            float4 a = bias;
#pragma unroll
            for (int ky = 0; ky < 3; ++ky)
#pragma unroll
                for (int kx = 0; kx < 3; ++kx) {
                    const float4 k = *reinterpret_cast<const float4*>(dw + (ky * 3 + kx) * cstride + ch);
                    const float4 v = win[dy + ky][dx + kx];
                    a.x = fmaf(v.x, k.x, a.x); a.y = fmaf(v.y, k.y, a.y); a.z = fmaf(v.z, k.z, a.z); a.w = fmaf(v.w, k.w, a.w);
                }
            out[dy][dx] = make_float4(relu_f(a.x), relu_f(a.y), relu_f(a.z), relu_f(a.w));
        }
}

__device__ __forceinline__ float4 max4(float4 a, float4 b, float4 c, float4 d) {
    return make_float4(max_nan(max_nan(a.x, b.x), max_nan(c.x, d.x)), max_nan(max_nan(a.y, b.y), max_nan(c.y, d.y)),
                       max_nan(max_nan(a.z, b.z), max_nan(c.z, d.z)), max_nan(max_nan(a.w, b.w), max_nan(c.w, d.w)));
}

// Stem (3x3/2 conv 3->16 + ReLU) + unit 0 (16->16 at stride 2) + MaxPool: one block = a 16x16 tile of the stride-4 output,
// i.e. 32x32 stride-2 pixels + halo = 34x34x16 f32 (74 KB) in LDS.  Pixels of the padded frame beyond the real one read 0.
// `img`: the first byte of frame blockIdx.z - the one thing in which the two kernels below differ.
__device__ __forceinline__ void stem_unit0_pool_tile(const StemArgs& a, const uint8_t* img) {
    extern __shared__ float mid[];   // [34 * 34][16]
    constexpr int L = 2 * kT + 2;
    const int b = blockIdx.z;
    if (blockIdx.x == 0 && blockIdx.y == 0 && threadIdx.x == 0) a.counts[b] = 0;
    const float* sw = a.wt;
    const float* sb = sw + 27 * 16;
    const float* pw = a.wt + kStemFloats;
    const float* pb = pw + 16 * 16;
    const float* dw = pb + 16;
    const float* db = dw + 9 * 16;
    const int y0 = blockIdx.y * 2 * kT - 1, x0 = blockIdx.x * 2 * kT - 1;
    for (int p = threadIdx.x; p < L * L; p += kThreads) {
        const int i = p / L, j = p - i * L, y = y0 + i, x = x0 + j;
        float4* dst = reinterpret_cast<float4*>(mid + p * 16);
        if (y < 0 || y >= a.h2 || x < 0 || x >= a.w2) {
#pragma unroll
            for (int k = 0; k < 4; ++k) dst[k] = make_float4(0.f, 0.f, 0.f, 0.f);
            continue;
        }
        float s[16];
#pragma unroll
        for (int k = 0; k < 16; ++k) s[k] = sb[k];
#pragma unroll
        for (int ky = 0; ky < 3; ++ky) {
            const int iy = 2 * y - 1 + ky;
            if (iy < 0 || iy >= a.h) continue;
#pragma unroll
            for (int kx = 0; kx < 3; ++kx) {
                const int ix = 2 * x - 1 + kx;
                if (ix < 0 || ix >= a.w) continue;
                const uint8_t* px = img + (long long)iy * a.row_pitch + ix * 3;
                const float c[3] = {(float)px[0], (float)px[1], (float)px[2]};
#pragma unroll
                for (int ci = 0; ci < 3; ++ci)
#pragma unroll
                    for (int o = 0; o < 16; ++o) s[o] = fmaf(c[ci], sw[((ky * 3 + kx) * 3 + ci) * 16 + o], s[o]);
            }
        }
        float t[16];
#pragma unroll
        for (int k = 0; k < 16; ++k) t[k] = pb[k];
#pragma unroll
        for (int ci = 0; ci < 16; ++ci) {
            const float v = relu_f(s[ci]);
#pragma unroll
            for (int o = 0; o < 16; ++o) t[o] = fmaf(v, pw[ci * 16 + o], t[o]);
        }
#pragma unroll
        for (int k = 0; k < 4; ++k) dst[k] = make_float4(t[4 * k], t[4 * k + 1], t[4 * k + 2], t[4 * k + 3]);
    }
    __syncthreads();
    for (int it = threadIdx.x; it < kT * kT * 4; it += kThreads) {
        const int c4 = it & 3, q = it >> 2, qy = q / kT, qx = q - qy * kT;
        const int py = blockIdx.y * kT + qy, px = blockIdx.x * kT + qx;
        if (py >= a.h4 || px >= a.w4) continue;
        float4 o[2][2];
        dw_quad(mid, L, 2 * qy, 2 * qx, c4, dw, db, c4 * 4, 16, o);
        *reinterpret_cast<float4*>(a.out + (((size_t)b * a.h4 + py) * a.w4 + px) * 16 + c4 * 4) = max4(o[0][0], o[0][1], o[1][0], o[1][1]);
    }
}

__global__ __launch_bounds__(kThreads) void yunet_stem_unit0_pool(StemArgs a) {
    stem_unit0_pool_tile(a, a.frames + (long long)blockIdx.z * a.frame_stride);
}

// The same kernel for frames that lie anywhere (af_yunet_detect_frames): frame b starts at list.p[b].  The list travels by value
// in the launch arguments (512 bytes), so the launch needs no copy of it; a.frames / a.frame_stride are not read.
struct FrameList { const uint8_t* p[AF_YUNET_MAX_LIST]; };

__global__ __launch_bounds__(kThreads) void yunet_stem_unit0_pool_frames(StemArgs a, FrameList list) {
    stem_unit0_pool_tile(a, list.p[blockIdx.z]);
}

// One DP unit over a 16x16 output tile, 16 output channels at a time (a 18x18x16 f32 LDS tile, 20 KB): 1x1 conv into LDS, then
// each thread one 2x2 quad x 4 channels of the depthwise conv, stored full and / or 2x2-max-pooled.
template <int CIN, int COUT>
__global__ __launch_bounds__(kThreads) void yunet_dp_unit(UnitArgs a) {
    __shared__ float mid[kHalo * kHalo * 16];
    const int b = blockIdx.z;
    const float* in = a.in + (size_t)b * a.h * a.w * CIN;
    const float* up = a.up ? a.up + (size_t)b * (a.h >> 1) * (a.w >> 1) * CIN : nullptr;
    const float* pw = a.wt;
    const float* pb = pw + CIN * COUT;
    const float* dw = pb + COUT;
    const float* db = dw + 9 * COUT;
    const int c4 = threadIdx.x & 3, q = threadIdx.x >> 2, qy = q / (kT / 2), qx = q - qy * (kT / 2);
    const int fy = blockIdx.y * kT + 2 * qy, fx = blockIdx.x * kT + 2 * qx;
#pragma unroll 1
    for (int g = 0; g < COUT / 16; ++g) {
        pw_tile_mfma<CIN, COUT>(in, up, pw, pb, g, blockIdx.y * kT - 1, blockIdx.x * kT - 1, a.h, a.w, mid);
        __syncthreads();
        if (fy < a.h && fx < a.w) {
            const int ch = g * 16 + c4 * 4;
            float4 o[2][2];
            dw_quad(mid, kHalo, 2 * qy, 2 * qx, c4, dw, db, ch, COUT, o);
            if (a.out_full) {
#pragma unroll
                for (int dy = 0; dy < 2; ++dy)
#pragma unroll
                    for (int dx = 0; dx < 2; ++dx)
                        if (fy + dy < a.h && fx + dx < a.w)
                            *reinterpret_cast<float4*>(a.out_full + (((size_t)b * a.h + fy + dy) * a.w + fx + dx) * COUT + ch) = o[dy][dx];
            }
            if (a.out_pool) {
                const int hp = a.h >> 1, wp = a.w >> 1;
                *reinterpret_cast<float4*>(a.out_pool + (((size_t)b * hp + (fy >> 1)) * wp + (fx >> 1)) * COUT + ch) =
                    max4(o[0][0], o[0][1], o[1][0], o[1][1]);
            }
        }
        __syncthreads();
    }
}

__device__ __forceinline__ float sigmoid_f(float x) { return 1.f / (1.f + expf(-x)); }

// Head of one level + OpenCV's decode: one thread per anchor of a 16x16 tile.
__global__ __launch_bounds__(kThreads) void yunet_head_decode(HeadArgs a) {
    __shared__ float mid[kHalo * kHalo * 16];
    const int b = blockIdx.z;
    const float* pw = a.wt;
    const float* pb = pw + 64 * kHeadCh;
    const float* dw = pb + kHeadCh;
    const float* db = dw + 9 * kHeadCh;
    pw_tile<64, kHeadCh>(a.in + (size_t)b * a.h * a.w * 64, nullptr, pw, pb, 0, blockIdx.y * kT - 1, blockIdx.x * kT - 1, a.h,
                         a.w, mid);
    __syncthreads();
    const int ty = threadIdx.x / kT, tx = threadIdx.x - ty * kT;
    const int r = blockIdx.y * kT + ty, c = blockIdx.x * kT + tx;
    if (r >= a.h || c >= a.w) return;
    float o[kHeadCh];
#pragma unroll
    for (int k = 0; k < kHeadCh; ++k) o[k] = db[k];
#pragma unroll
    for (int ky = 0; ky < 3; ++ky)
#pragma unroll
        for (int kx = 0; kx < 3; ++kx) {
            const float* m = mid + ((ty + ky) * kHalo + tx + kx) * 16;
#pragma unroll
            for (int k = 0; k < kHeadCh; ++k) o[k] = fmaf(m[k], dw[(ky * 3 + kx) * kHeadCh + k], o[k]);
        }
    o[0] = sigmoid_f(o[0]);
    o[1] = sigmoid_f(o[1]);
    const int seq = a.level_off + r * a.w + c;
    if (a.raw) {
        float4* dst = reinterpret_cast<float4*>(a.raw + ((size_t)b * a.anchors + seq) * 16);
#pragma unroll
        for (int k = 0; k < 4; ++k) dst[k] = make_float4(o[4 * k], o[4 * k + 1], o[4 * k + 2], o[4 * k + 3]);
    }
    // FaceDetectorYN::postProcess: MIN / MAX clamps, sqrt, `score < threshold` skips
    const float cls = fmaxf(fminf(o[0], 1.f), 0.f), obj = fmaxf(fminf(o[1], 1.f), 0.f);
    const float score = sqrtf(cls * obj);
    if (!(score >= a.conf)) return;
    const float s = (float)a.stride, fc = (float)c, fr = (float)r;
    const float cx = (fc + o[2]) * s, cy = (fr + o[3]) * s;
    const float bw = expf(o[4]) * s, bh = expf(o[5]) * s;
    float row[16];
    row[0] = cx - bw / 2.f;
    row[1] = cy - bh / 2.f;
    row[2] = bw;
    row[3] = bh;
#pragma unroll
    for (int n = 0; n < 5; ++n) {
        row[4 + 2 * n] = (o[6 + 2 * n] + fc) * s;
        row[5 + 2 * n] = (o[7 + 2 * n] + fr) * s;
    }
    row[14] = score;
    row[15] = 0.f;
    float4* dst = reinterpret_cast<float4*>(a.rows + ((size_t)b * a.anchors + seq) * 16);
#pragma unroll
    for (int k = 0; k < 4; ++k) dst[k] = make_float4(row[4 * k], row[4 * k + 1], row[4 * k + 2], row[4 * k + 3]);
    // sort key: ascending u64 order = score descending (non-negative float bits, inverted), then anchor index ascending
    const unsigned long long key = ((unsigned long long)(~__float_as_uint(score)) << 32) | (unsigned)seq;
    const int slot = atomicAdd(a.counts + b, 1);
    a.keys[(size_t)b * a.keys_ld + slot] = key;     // slot < anchors: each anchor appends at most once
}

// dnn::NMSBoxes' overlap of two Rect2i: 1 - jaccardDistance, the distance in double, cast to float
__device__ __forceinline__ float rect_overlap(int4 p, int4 q) {
    const long long ap = (long long)p.z * p.w, aq = (long long)q.z * q.w;
    if (ap + aq <= 0) return 1.f;
    const int x1 = max(p.x, q.x), y1 = max(p.y, q.y);
    const int iw = min(p.x + p.z, q.x + q.z) - x1, ih = min(p.y + p.w, q.y + q.w) - y1;
    const double inter = (iw > 0 && ih > 0) ? (double)iw * (double)ih : 0.0;
    const float dist = (float)(1.0 - inter / ((double)(ap + aq) - inter));
    return 1.f - dist;
}

// Per frame (one block): the candidate keys are sorted in LDS (detect::sort_keys; top_k <= AF_YUNET_MAX_TOPK = kSortHalf).
// Then one wave runs the greedy NMS over the sorted list; it stops at the first score <= conf or after top_k candidates.
__global__ __launch_bounds__(kSortThreads) void yunet_sort_nms(NmsArgs a) {
    extern __shared__ unsigned long long lds[];
    const int b = blockIdx.x, tid = threadIdx.x;
    const int n = min(a.counts[b], a.anchors);
    unsigned long long* gk = a.keys + (size_t)b * a.keys_ld;
    const float* rows = a.rows + (size_t)b * a.anchors * 16;
    float* out = a.out_rows + (size_t)b * a.top_k * 15;
    if (n <= 1) {                                          // FaceDetectorYN: NMS only for two or more faces
        if (n == 1 && tid < 15) out[tid] = rows[(size_t)(unsigned)gk[0] * 16 + tid];
        if (tid == 0) a.out_count[b] = n;
        return;
    }
    detect::sort_keys(gk, n, lds);
    const int m = min(n, a.top_k);                         // <= kSortHalf
    for (int i = tid; i < m; i += kSortThreads) gk[i] = lds[i];
    __syncthreads();
    if (tid >= 64) return;
    int4* kept = reinterpret_cast<int4*>(lds);             // <= top_k <= AF_YUNET_MAX_TOPK boxes
    int nk = 0;
    for (int i = 0; i < m; ++i) {
        const unsigned long long key = gk[i];
        if (!(__uint_as_float(~(unsigned)(key >> 32)) > a.conf)) break;
        const float* r = rows + (size_t)(unsigned)key * 16;
        const int4 box = make_int4((int)r[0], (int)r[1], (int)r[2], (int)r[3]);
        int sup = 0;
        for (int j = tid; j < nk && !sup; j += 64) sup = !(rect_overlap(box, kept[j]) <= a.nms);
        if (!__any(sup)) {
            if (tid == 0) kept[nk] = box;
            if (tid < 15) out[(size_t)nk * 15 + tid] = r[tid];
            ++nk;
        }
        __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
        __builtin_amdgcn_wave_barrier();
    }
    if (tid == 0) a.out_count[b] = nk;
}

// ---- host side
struct Plan {
    int B, h, w, ph, pw;     // frames, padded size
    int anchors, lvl_h[3], lvl_w[3], lvl_off[3];
    long long keys_ld;
    // activation offsets (floats) per frame-batch
    size_t t189, t193, t197, t201, t206, t210, t214, t215, t219, t223, t224, t228, t232, t236, t246, t256;
    size_t act_floats, counts_off, keys_off, rows_off, total_bytes;
};

static Plan make_plan(const af_yunet_desc& d) {
    Plan p{};
    p.B = d.batch;
    p.h = d.height;
    p.w = d.width;
    p.ph = ((d.height - 1) / 32 + 1) * 32;
    p.pw = ((d.width - 1) / 32 + 1) * 32;
    for (int l = 0; l < 3; ++l) {
        const int s = 8 << l;
        p.lvl_h[l] = p.ph / s;
        p.lvl_w[l] = p.pw / s;
        p.lvl_off[l] = p.anchors;
        p.anchors += p.lvl_h[l] * p.lvl_w[l];
    }
    p.keys_ld = (p.anchors + 1) & ~1;                       // keeps every frame's keys 16-byte aligned
    const size_t B = p.B, s4 = (size_t)(p.ph / 4) * (p.pw / 4), s8 = s4 / 4, s16 = s8 / 4, s32 = s16 / 4;
    size_t off = 0;
    auto take = [&](size_t pixels, int ch) { const size_t o = off; off += B * pixels * ch; off = (off + 3) & ~(size_t)3; return o; };
    p.t189 = take(s4, 16);
    p.t193 = take(s4, 16);
    p.t197 = take(s4, 32);
    p.t201 = take(s4, 32);
    p.t206 = take(s8, 64);
    p.t210 = take(s8, 64);
    p.t214 = take(s8, 64);
    p.t215 = take(s16, 64);
    p.t219 = take(s16, 64);
    p.t223 = take(s16, 64);
    p.t224 = take(s32, 64);
    p.t228 = take(s32, 64);
    p.t232 = take(s32, 64);
    p.t236 = take(s32, 64);
    p.t246 = take(s16, 64);
    p.t256 = take(s8, 64);
    p.act_floats = off;
    size_t bytes = off * 4;
    p.counts_off = bytes;
    bytes += ((B * 4 + 15) / 16) * 16;
    p.keys_off = bytes;
    bytes += B * p.keys_ld * 8;
    p.rows_off = bytes;
    bytes += B * (size_t)p.anchors * 16 * 4;
    p.total_bytes = bytes;
    return p;
}

static int check_desc(const af_yunet_desc* d) {
    const int rc = detect::check_frames(d, "yunet", AF_YUNET_MAX_SIDE);
    if (rc != AF_OK) return rc;
    AF_REQUIRE(d->top_k >= 1 && d->top_k <= AF_YUNET_MAX_TOPK, "yunet: top_k %d out of [1, %d]", d->top_k, AF_YUNET_MAX_TOPK);
    AF_REQUIRE(d->conf_threshold == d->conf_threshold && d->nms_threshold == d->nms_threshold, "yunet: NaN threshold");
    return AF_OK;
}

template <int CIN, int COUT>
static void launch_unit(dim3 grid, hipStream_t s, const UnitArgs& ua) {
    hipLaunchKernelGGL((yunet_dp_unit<CIN, COUT>), grid, dim3(kThreads), 0, s, ua);
}

// `list`: null (frame b at frames + b * d->frame_stride), or d->batch frame pointers, checked by the caller (then `frames` is list[0])
static int detect(const af_yunet_desc* d, const float* weights, const void* frames, void* workspace, int64_t workspace_bytes,
                  float* out_rows, int32_t* out_count, float* raw, hipStream_t s, hipEvent_t* ev, const void* const* list = nullptr) {
    int rc = check_desc(d);
    if (rc != AF_OK) return rc;
    AF_REQUIRE(weights && frames && workspace && out_rows && out_count, "yunet: null pointer");
    AF_REQUIRE(aligned16(weights) && aligned16(workspace) && aligned16(raw), "yunet: weights / workspace / raw not 16-byte aligned");
    const Plan p = make_plan(*d);
    AF_REQUIRE(workspace_bytes >= (int64_t)p.total_bytes, "yunet: workspace %lld bytes < %lld", (long long)workspace_bytes,
               (long long)p.total_bytes);
    float* act = (float*)workspace;
    int* counts = (int*)((char*)workspace + p.counts_off);
    unsigned long long* keys = (unsigned long long*)((char*)workspace + p.keys_off);
    float* rows = (float*)((char*)workspace + p.rows_off);
    Marks mark{s, ev, 0};
    mark();

    const int h4 = p.ph / 4, w4 = p.pw / 4;
    constexpr int kStemLds = (2 * kT + 2) * (2 * kT + 2) * 16 * 4;
    AF_SET_MAX_LDS(yunet_stem_unit0_pool, kStemLds, "yunet_stem_unit0_pool");
    StemArgs sa{(const uint8_t*)frames, d->frame_stride, d->row_pitch, d->height, d->width, p.ph / 2, p.pw / 2, h4, w4,
                weights, act + p.t189, counts};
    const dim3 stem_grid((w4 + kT - 1) / kT, (h4 + kT - 1) / kT, p.B);
    if (list) {
        FrameList fl{};
        for (int b = 0; b < p.B; ++b) fl.p[b] = (const uint8_t*)list[b];
        AF_SET_MAX_LDS(yunet_stem_unit0_pool_frames, kStemLds, "yunet_stem_unit0_pool_frames");
        hipLaunchKernelGGL(yunet_stem_unit0_pool_frames, stem_grid, dim3(kThreads), kStemLds, s, sa, fl);
    } else {
        hipLaunchKernelGGL(yunet_stem_unit0_pool, stem_grid, dim3(kThreads), kStemLds, s, sa);
    }
    AF_CHECK_LAUNCH("yunet_stem_unit0_pool");
    mark();

    struct U { int unit; size_t in, up, full, pool; int h, w; };
    const size_t N = ~(size_t)0;
    const int hs[5] = {h4, h4 / 2, h4 / 4, h4 / 8}, ws[5] = {w4, w4 / 2, w4 / 4, w4 / 8};
    const U units[kUnits - 1] = {
        {1, p.t189, N, p.t193, N, hs[0], ws[0]},  {2, p.t193, N, p.t197, N, hs[0], ws[0]},  {3, p.t197, N, p.t201, N, hs[0], ws[0]},
        {4, p.t201, N, N, p.t206, hs[0], ws[0]},  {5, p.t206, N, p.t210, N, hs[1], ws[1]},  {6, p.t210, N, p.t214, p.t215, hs[1], ws[1]},
        {7, p.t215, N, p.t219, N, hs[2], ws[2]},  {8, p.t219, N, p.t223, p.t224, hs[2], ws[2]},
        {9, p.t224, N, p.t228, N, hs[3], ws[3]},  {10, p.t228, N, p.t232, N, hs[3], ws[3]}, {11, p.t232, N, p.t236, N, hs[3], ws[3]},
        {12, p.t223, p.t236, p.t246, N, hs[2], ws[2]},   // 242 = 223 + up2(236) -> 246
        {13, p.t214, p.t246, p.t256, N, hs[1], ws[1]},   // 252 = 214 + up2(246) -> 256
    };
    for (const U& u : units) {
        UnitArgs ua{act + u.in, u.up == N ? nullptr : act + u.up, weights + unit_offset(u.unit), u.full == N ? nullptr : act + u.full,
                    u.pool == N ? nullptr : act + u.pool, u.h, u.w};
        const dim3 grid((u.w + kT - 1) / kT, (u.h + kT - 1) / kT, p.B);
        switch (kUnitCin[u.unit] * 1000 + kUnitCout[u.unit]) {
            case 16016: launch_unit<16, 16>(grid, s, ua); break;
            case 16032: launch_unit<16, 32>(grid, s, ua); break;
            case 32032: launch_unit<32, 32>(grid, s, ua); break;
            case 32064: launch_unit<32, 64>(grid, s, ua); break;
            default: launch_unit<64, 64>(grid, s, ua); break;
        }
        AF_CHECK_LAUNCH("yunet_dp_unit");
        mark();
    }

    const size_t head_in[3] = {p.t256, p.t246, p.t236};
    for (int l = 0; l < 3; ++l) {
        HeadArgs ha{act + head_in[l], weights + kHeadOffset + l * kHeadFloats, p.lvl_h[l], p.lvl_w[l], 8 << l, p.lvl_off[l], p.anchors,
                    d->conf_threshold, raw, counts, keys, p.keys_ld, rows};
        hipLaunchKernelGGL(yunet_head_decode, dim3((p.lvl_w[l] + kT - 1) / kT, (p.lvl_h[l] + kT - 1) / kT, p.B), dim3(kThreads), 0, s, ha);
        AF_CHECK_LAUNCH("yunet_head_decode");
        mark();
    }

    AF_SET_MAX_LDS(yunet_sort_nms, kSortLdsBytes, "yunet_sort_nms");
    NmsArgs na{counts, keys, p.keys_ld, rows, p.anchors, d->top_k, d->conf_threshold, d->nms_threshold, out_rows, out_count};
    hipLaunchKernelGGL(yunet_sort_nms, dim3(p.B), dim3(kSortThreads), kSortLdsBytes, s, na);
    AF_CHECK_LAUNCH("yunet_sort_nms");
    mark();
    return AF_OK;
}

}  // namespace yunet
}  // namespace af

extern "C" int64_t af_yunet_weight_floats(void) { return af::yunet::kWeightFloats; }

extern "C" int64_t af_yunet_workspace_bytes(const af_yunet_desc* d) {
    if (af::yunet::check_desc(d) != AF_OK) return 0;
    return (int64_t)af::yunet::make_plan(*d).total_bytes;
}

extern "C" int af_yunet_detect(const af_yunet_desc* d, const float* weights, const void* frames, void* workspace,
                               int64_t workspace_bytes, float* out_rows, int32_t* out_count, float* raw, void* stream) {
    return af::yunet::detect(d, weights, frames, workspace, workspace_bytes, out_rows, out_count, raw, (hipStream_t)stream, nullptr);
}

extern "C" int af_yunet_detect_frames(const af_yunet_desc* d, const float* weights, const void* const* frames, void* workspace,
                                      int64_t workspace_bytes, float* out_rows, int32_t* out_count, float* raw, void* stream) {
    using namespace af;
    AF_REQUIRE(d && frames, "yunet_detect_frames: null argument");
    AF_REQUIRE(d->batch >= 1 && d->batch <= AF_YUNET_MAX_LIST, "yunet_detect_frames: %d frames (at most %d per call)", d->batch, AF_YUNET_MAX_LIST);
    for (int b = 0; b < d->batch; ++b) AF_REQUIRE(frames[b], "yunet_detect_frames: frame %d is a null pointer", b);
    af_yunet_desc one = *d;
    one.frame_stride = d->row_pitch * d->height;            // not read by the kernel; keeps the shared layout check quiet
    return yunet::detect(&one, weights, frames[0], workspace, workspace_bytes, out_rows, out_count, raw, (hipStream_t)stream, nullptr, frames);
}

extern "C" int af_yunet_detect_timed(const af_yunet_desc* d, const float* weights, const void* frames, void* workspace,
                                     int64_t workspace_bytes, float* out_rows, int32_t* out_count, float* raw, void* stream, float* ms) {
    int rc = af::yunet::check_desc(d);
    if (rc != AF_OK) return rc;
    hipStream_t s = (hipStream_t)stream;
    return af::timed("yunet_detect_timed", s, AF_YUNET_LAUNCHES, ms, [&](hipEvent_t* ev) {
        return af::yunet::detect(d, weights, frames, workspace, workspace_bytes, out_rows, out_count, raw, s, ev);
    });
}
