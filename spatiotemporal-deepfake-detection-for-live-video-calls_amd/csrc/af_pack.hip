// One-time weight transforms (model load) and the input prologue.  All HBM-bound elementwise work.
#include "af_common.h"

namespace af {

__global__ void fold_bn_kernel(const float* gamma, const float* beta, const float* mean, const float* var,
                               float eps, int c, float* scale, float* shift) {
    int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i < c) {
        // same operation order as ATen's eval batch_norm: invstd = 1/sqrt(var+eps); w*invstd; b - mean*that
        float invstd = 1.0f / sqrtf(var[i] + eps);
        float s = gamma[i] * invstd;
        scale[i] = s;
        shift[i] = beta[i] - mean[i] * s;
    }
}

// OIDHW fp32 -> [o_pad][tap][i_pad] in DT: cout padded to 64 rows, cin to the K-step (64 / 32 elements); zeros
template <int DT>
__global__ void pack_conv_weight_kernel(const float* __restrict__ w, const float* __restrict__ row_scale, int cout,
                                        int cin, int taps, int coutp, int cinp, typename Elem<DT>::type* __restrict__ out) {
    long long idx = (long long)blockIdx.x * blockDim.x + threadIdx.x;      // over output elements
    long long total = (long long)coutp * taps * cinp;
    if (idx >= total) return;
    int i = (int)(idx % cinp); long long r = idx / cinp;
    int tap = (int)(r % taps); int o = (int)(r / taps);
    float v = 0.f;
    if (o < cout && i < cin) {
        v = w[((long long)o * cin + i) * taps + tap];
        if (row_scale) v *= row_scale[o];           // BN scale folded in fp32, before the one rounding
    }
    out[idx] = Elem<DT>::from_f32(v);
}

// (cout,3,kt,kh,7) fp32 -> [kt][kh][NCH][cout][EPC]: K-row (dt,dh) = 8 pixels x 4 channels, zero padded
template <int DT>
__global__ void pack_stem_weight_kernel(const float* __restrict__ w, int cout, int coutp, int kt, int kh, int kw,
                                        typename Elem<DT>::type* __restrict__ out) {
    constexpr int EPC = Elem<DT>::EPC;
    constexpr int NCH = 32 / EPC;
    long long idx = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    long long total = (long long)kt * kh * NCH * coutp * EPC;
    if (idx >= total) return;
    int e = (int)(idx % EPC); long long r = idx / EPC;
    int o = (int)(r % coutp); r /= coutp;
    int ch = (int)(r % NCH); r /= NCH;
    int dh = (int)(r % kh); int dt = (int)(r / kh);
    int k = ch * EPC + e;               // 0..31 within the K-row
    int dw = k >> 2, c = k & 3;
    float v = 0.f;
    if (dw < kw && c < 3 && o < cout) v = w[((((long long)o * 3 + c) * kt + dt) * kh + dh) * kw + dw];
    out[idx] = Elem<DT>::from_f32(v);
}

// interior of the padded stem input; one thread per pixel (4 channels = one 8/16-byte store)
template <int DT, typename Src>
__global__ void pack_input_kernel(Src src, int n, int t, int h, int w, char* __restrict__ out) {
    constexpr int ES = 16 / Elem<DT>::EPC;
    long long idx = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    long long total = (long long)n * t * h * w;
    if (idx >= total) return;
    int x = (int)(idx % w); long long r = idx / w;
    int y = (int)(r % h); r /= h;
    int z = (int)(r % t); long long b = r / t;
    f32x4 v;
    v[0] = src(b, 0, z, y, x); v[1] = src(b, 1, z, y, x); v[2] = src(b, 2, z, y, x); v[3] = 0.f;
    const long long Tp = t + 2 * AF_STEM_PAD_T, Hp = h + 2 * AF_STEM_PAD_H, Wp = w + AF_STEM_PAD_W_TOTAL;
    long long o = (((b * Tp + z + AF_STEM_PAD_T) * Hp + y + AF_STEM_PAD_H) * Wp + x + AF_STEM_PAD_W_LEFT) * 4;
    Vec4<DT>::store(out + o * ES, v);
}

struct SrcF32 {
    const float* p; long long sn, sc, st, sh, sw;
    __device__ float operator()(long long b, int c, int z, int y, int x) const {
        return p[b * sn + c * sc + z * st + y * sh + x * sw];
    }
};
struct SrcU8 {
    const uint8_t* p; int t, h, w; float mean[3], stdv[3];
    __device__ float operator()(long long b, int c, int z, int y, int x) const {
        // (float(u8) - mean) / std : the callers' x.sub(mean).div(std) on float32 (af_realtime.py:83)
        float v = (float)p[(((b * t + z) * h + y) * w + x) * 3 + c];
        return (v - mean[c]) / stdv[c];
    }
};

// ---- SlowFast: both pathway inputs out of ONE read of the uint8 clip (af_pack_input_u8_pathways) ----
// A destination: rows [n][frames + 2 PAD_T][h + 2 PAD_H] of row_bytes each, pixel x of a row at byte (x + PAD_W_LEFT) * pixel size;
// pixel = 4 channels of DT (the padded layout of pack_input_kernel) or, rgb3, 3 x 16 bit (that of pack_input3_kernel, af_stem3.hip)
struct PackDst {
    char* p; long long row_bytes; int frames, rgb3;
    __device__ char* row(long long b, int z, int y, int h) const {
        return p + ((b * (frames + 2 * AF_STEM_PAD_T) + z + AF_STEM_PAD_T) * (h + 2 * AF_STEM_PAD_H) + y + AF_STEM_PAD_H) * row_bytes;
    }
};
struct PathwaysArgs { const uint8_t* clips; int n, t, h, w, alpha; float mean[3], stdv[3]; PackDst fast, slow; };

// NPX normalised pixels x0 .. x0 + NPX - 1 of one row.  NPX = 8 (x0 % 8 == 0): the 48 bytes of an rgb3 run start 18 bytes behind a
// 16-byte boundary, so they leave as 2 + 4 + 8 + 16 + 16 + 2 bytes, every store aligned to its own size; 4 channels: one 8- or
// 16-byte store per pixel, as pack_input_kernel writes them
template <int DT, int NPX>
__device__ __forceinline__ void store_pixels(const PackDst& d, char* row, int x0, const float (&v)[NPX][3]) {
    typedef typename Elem<DT>::type elem_t;
    constexpr int ES = sizeof(elem_t);
    if constexpr (DT != AF_F32) {
        if (d.rgb3) {
            char* o = row + (x0 + AF_STEM_PAD_W_LEFT) * 6;
            elem_t e[NPX * 3];
#pragma unroll
            for (int j = 0; j < NPX * 3; ++j) e[j] = Elem<DT>::from_f32(v[j / 3][j % 3]);
            if constexpr (NPX == 8) {
                typedef elem_t e2 __attribute__((ext_vector_type(2)));
                typedef elem_t e4 __attribute__((ext_vector_type(4)));
                typedef elem_t e8 __attribute__((ext_vector_type(8)));
                *reinterpret_cast<elem_t*>(o) = e[0];
                *reinterpret_cast<e2*>(o + 2) = e2{e[1], e[2]};
                *reinterpret_cast<e4*>(o + 6) = e4{e[3], e[4], e[5], e[6]};
                *reinterpret_cast<e8*>(o + 14) = e8{e[7], e[8], e[9], e[10], e[11], e[12], e[13], e[14]};
                *reinterpret_cast<e8*>(o + 30) = e8{e[15], e[16], e[17], e[18], e[19], e[20], e[21], e[22]};
                *reinterpret_cast<elem_t*>(o + 46) = e[23];
            } else {
#pragma unroll
                for (int j = 0; j < NPX * 3; ++j) reinterpret_cast<elem_t*>(o)[j] = e[j];
            }
            return;
        }
    }
    char* o = row + (long long)(x0 + AF_STEM_PAD_W_LEFT) * 4 * ES;
#pragma unroll
    for (int k = 0; k < NPX; ++k) Vec4<DT>::store(o + k * 4 * ES, f32x4{v[k][0], v[k][1], v[k][2], 0.f});
}

// One thread per run of NPX pixels of a clip row: the run is loaded once (VEC: 24 bytes as three 8-byte loads - w % 8 == 0 and an
// 8-byte aligned clip make every run of every row aligned; otherwise a pixel's 3 bytes), normalised once and stored into the Fast
// input and, for every alpha-th frame, into the Slow input as well.  Only interior cells are written; no LDS.
template <int DT, bool VEC>
__global__ void __launch_bounds__(256) pack_pathways_kernel(PathwaysArgs a) {
    constexpr int NPX = VEC ? 8 : 1;
    const int runs = a.w / NPX;
    const long long total = (long long)a.n * a.t * a.h * runs;
    for (long long idx = (long long)blockIdx.x * 256 + threadIdx.x; idx < total; idx += (long long)gridDim.x * 256) {
        const int x0 = (int)(idx % runs) * NPX; const long long r = idx / runs;       // r: row of the clip tensor
        const int y = (int)(r % a.h); const long long f = r / a.h;
        const int z = (int)(f % a.t); const long long b = f / a.t;
        const uint8_t* src = a.clips + (r * a.w + x0) * 3;
        float v[NPX][3];
        if constexpr (VEC) {
            const uint2 q0 = reinterpret_cast<const uint2*>(src)[0], q1 = reinterpret_cast<const uint2*>(src)[1],
                        q2 = reinterpret_cast<const uint2*>(src)[2];
            const unsigned wd[6] = {q0.x, q0.y, q1.x, q1.y, q2.x, q2.y};
#pragma unroll
            for (int j = 0; j < 24; ++j)
                v[j / 3][j % 3] = ((float)((wd[j >> 2] >> (8 * (j & 3))) & 0xffu) - a.mean[j % 3]) / a.stdv[j % 3];
        } else {
#pragma unroll
            for (int c = 0; c < 3; ++c) v[0][c] = ((float)src[c] - a.mean[c]) / a.stdv[c];
        }
        store_pixels<DT, NPX>(a.fast, a.fast.row(b, z, y, a.h), x0, v);
        if (z % a.alpha == 0) store_pixels<DT, NPX>(a.slow, a.slow.row(b, z / a.alpha, y, a.h), x0, v);
    }
}

static inline unsigned grid_for(long long total, int block) { return (unsigned)((total + block - 1) / block); }

}  // namespace af

using namespace af;

extern "C" int af_fold_bn(const float* gamma, const float* beta, const float* mean, const float* var, float eps,
                          int channels, float* scale, float* shift, void* stream) {
    AF_REQUIRE(gamma && beta && mean && var && scale && shift && channels > 0, "fold_bn: bad argument");
    hipLaunchKernelGGL(fold_bn_kernel, dim3(grid_for(channels, 256)), dim3(256), 0, (hipStream_t)stream, gamma, beta,
                       mean, var, eps, channels, scale, shift);
    AF_CHECK_LAUNCH("fold_bn_kernel");
    return AF_OK;
}

static inline int pad_cout(int cout) { return (cout + 63) / 64 * 64; }
static inline int pad_cin(int cin, int dtype) { const int bk = dtype == AF_F32 ? 32 : 64; return (cin + bk - 1) / bk * bk; }

extern "C" int64_t af_packed_conv_weight_bytes(int cout, int cin, int kt, int kh, int kw, int dtype) {
    if (!dtype_ok(dtype) || cout <= 0 || cin <= 0 || kt <= 0 || kh <= 0 || kw <= 0) return AF_ERR_ARG;
    return (int64_t)pad_cout(cout) * pad_cin(cin, dtype) * kt * kh * kw * dtype_size(dtype);
}

extern "C" int af_padded_channels(int cout) { return cout > 0 ? pad_cout(cout) : AF_ERR_ARG; }

extern "C" int af_pack_conv_weight_scaled(const float* w, const float* row_scale, int cout, int cin, int kt, int kh,
                                          int kw, int dtype, void* packed, void* stream) {
    AF_REQUIRE(w && packed && dtype_ok(dtype) && cout > 0 && cin > 0 && kt > 0 && kh > 0 && kw > 0,
               "pack_conv_weight: bad argument");
    const int taps = kt * kh * kw, coutp = pad_cout(cout), cinp = pad_cin(cin, dtype);
    const long long total = (long long)coutp * cinp * taps;
    hipStream_t s = (hipStream_t)stream;
    dim3 g(grid_for(total, 256)), b(256);
    if (dtype == AF_F32) hipLaunchKernelGGL((pack_conv_weight_kernel<AF_F32>), g, b, 0, s, w, row_scale, cout, cin, taps, coutp, cinp, (float*)packed);
    else if (dtype == AF_BF16) hipLaunchKernelGGL((pack_conv_weight_kernel<AF_BF16>), g, b, 0, s, w, row_scale, cout, cin, taps, coutp, cinp, (__bf16*)packed);
    else hipLaunchKernelGGL((pack_conv_weight_kernel<AF_F16>), g, b, 0, s, w, row_scale, cout, cin, taps, coutp, cinp, (_Float16*)packed);
    AF_CHECK_LAUNCH("pack_conv_weight_kernel");
    return AF_OK;
}

extern "C" int af_pack_conv_weight(const float* w, int cout, int cin, int kt, int kh, int kw, int dtype, void* packed,
                                   void* stream) {
    return af_pack_conv_weight_scaled(w, nullptr, cout, cin, kt, kh, kw, dtype, packed, stream);
}

static inline int pad_stem_cout(int cout) { return cout <= 16 ? 16 : 64; }     // channel tiles of the stem kernels

extern "C" int64_t af_packed_stem_weight_bytes(int cout, int kt, int kh, int dtype) {
    if (!dtype_ok(dtype) || cout <= 0 || cout > 64 || kt <= 0 || kh <= 0) return AF_ERR_ARG;
    return (int64_t)kt * kh * 32 * pad_stem_cout(cout) * dtype_size(dtype);
}

extern "C" int af_pack_stem_weight(const float* w, int cout, int kt, int kh, int kw, int dtype, void* packed,
                                   void* stream) {
    AF_REQUIRE(w && packed && dtype_ok(dtype) && cout > 0 && cout <= 64 && kt > 0 && kh > 0 && kw > 0 && kw <= 8,
               "pack_stem_weight: bad argument");
    const int coutp = pad_stem_cout(cout);
    const long long total = (long long)kt * kh * 32 * coutp;
    hipStream_t s = (hipStream_t)stream;
    dim3 g(grid_for(total, 256)), b(256);
    if (dtype == AF_F32) hipLaunchKernelGGL((pack_stem_weight_kernel<AF_F32>), g, b, 0, s, w, cout, coutp, kt, kh, kw, (float*)packed);
    else if (dtype == AF_BF16) hipLaunchKernelGGL((pack_stem_weight_kernel<AF_BF16>), g, b, 0, s, w, cout, coutp, kt, kh, kw, (__bf16*)packed);
    else hipLaunchKernelGGL((pack_stem_weight_kernel<AF_F16>), g, b, 0, s, w, cout, coutp, kt, kh, kw, (_Float16*)packed);
    AF_CHECK_LAUNCH("pack_stem_weight_kernel");
    return AF_OK;
}

extern "C" int64_t af_stem_input_bytes(int n, int t, int h, int w, int dtype) {
    if (!dtype_ok(dtype) || n <= 0 || t <= 0 || h <= 0 || w <= 0) return AF_ERR_ARG;
    return (int64_t)n * (t + 2 * AF_STEM_PAD_T) * (h + 2 * AF_STEM_PAD_H) * (w + AF_STEM_PAD_W_TOTAL) * AF_STEM_CPAD *
           dtype_size(dtype);
}

template <typename Src>
static int launch_pack_input(const Src& src, int n, int t, int h, int w, int dtype, void* out, hipStream_t s) {
    const long long total = (long long)n * t * h * w;
    dim3 g(grid_for(total, 256)), b(256);
    if (dtype == AF_F32) hipLaunchKernelGGL((pack_input_kernel<AF_F32, Src>), g, b, 0, s, src, n, t, h, w, (char*)out);
    else if (dtype == AF_BF16) hipLaunchKernelGGL((pack_input_kernel<AF_BF16, Src>), g, b, 0, s, src, n, t, h, w, (char*)out);
    else hipLaunchKernelGGL((pack_input_kernel<AF_F16, Src>), g, b, 0, s, src, n, t, h, w, (char*)out);
    AF_CHECK_LAUNCH("pack_input_kernel");
    return AF_OK;
}

extern "C" int af_pack_input_f32(const float* x, int n, int t, int h, int w, int64_t stride_n, int64_t stride_c,
                                 int64_t stride_t, int64_t stride_h, int64_t stride_w, int dtype, void* stem_in,
                                 void* stream) {
    AF_REQUIRE(x && stem_in && dtype_ok(dtype) && n > 0 && t > 0 && h > 0 && w > 0, "pack_input_f32: bad argument");
    AF_REQUIRE(aligned16(stem_in), "pack_input_f32: output must be 16-byte aligned");
    SrcF32 src{x, stride_n, stride_c, stride_t, stride_h, stride_w};
    return launch_pack_input(src, n, t, h, w, dtype, stem_in, (hipStream_t)stream);
}

extern "C" int af_pack_input_u8(const uint8_t* clips, int n, int t, int h, int w, const float mean[3],
                                const float std_[3], int dtype, void* stem_in, void* stream) {
    AF_REQUIRE(clips && stem_in && mean && std_ && dtype_ok(dtype) && n > 0 && t > 0 && h > 0 && w > 0,
               "pack_input_u8: bad argument");
    AF_REQUIRE(aligned16(stem_in), "pack_input_u8: output must be 16-byte aligned");
    SrcU8 src;
    src.p = clips; src.t = t; src.h = h; src.w = w;
    for (int i = 0; i < 3; ++i) { src.mean[i] = mean[i]; src.stdv[i] = std_[i]; }
    return launch_pack_input(src, n, t, h, w, dtype, stem_in, (hipStream_t)stream);
}

static PackDst pack_dst(void* p, int frames, int w, int layout, int dtype) {
    const bool rgb3 = layout == AF_PACK_RGB3;
    return PackDst{(char*)p, rgb3 ? (long long)rgb3_row_bytes(w) : (long long)(w + AF_STEM_PAD_W_TOTAL) * AF_STEM_CPAD * dtype_size(dtype),
                   frames, rgb3 ? 1 : 0};
}

extern "C" int af_pack_input_u8_pathways(const uint8_t* clips, int n, int t, int h, int w, const float mean[3], const float std_[3],
                                         int alpha, int dtype, void* slow_in, int slow_layout, void* fast_in, int fast_layout,
                                         void* stream) {
    AF_REQUIRE(clips && slow_in && fast_in && mean && std_, "pack_input_u8_pathways: null pointer");
    AF_REQUIRE(dtype_ok(dtype) && n > 0 && t > 0 && h > 0 && w > 0 && alpha > 0, "pack_input_u8_pathways: bad argument");
    AF_REQUIRE(t % alpha == 0, "pack_input_u8_pathways: %d frames are not a multiple of alpha = %d", t, alpha);
    for (int layout : {slow_layout, fast_layout}) {
        AF_REQUIRE(layout == AF_PACK_C4 || layout == AF_PACK_RGB3, "pack_input_u8_pathways: unknown layout %d", layout);
        AF_REQUIRE(layout == AF_PACK_C4 || dtype != AF_F32, "pack_input_u8_pathways: the rgb3 layout is 16-bit only");
    }
    AF_REQUIRE(aligned16(slow_in) && aligned16(fast_in), "pack_input_u8_pathways: outputs must be 16-byte aligned");
    PathwaysArgs a;
    a.clips = clips; a.n = n; a.t = t; a.h = h; a.w = w; a.alpha = alpha;
    for (int i = 0; i < 3; ++i) { a.mean[i] = mean[i]; a.stdv[i] = std_[i]; }
    a.fast = pack_dst(fast_in, t, w, fast_layout, dtype);
    a.slow = pack_dst(slow_in, t / alpha, w, slow_layout, dtype);
    const bool vec = w % 8 == 0 && (reinterpret_cast<uintptr_t>(clips) & 7u) == 0;
    const long long blocks = ((long long)n * t * h * (vec ? w / 8 : w) + 255) / 256, cap = (long long)device_cus() * 8;
    dim3 g((unsigned)(blocks < cap ? blocks : cap)), b(256);
    hipStream_t s = (hipStream_t)stream;
    with_dtype(dtype, [&](auto dt) {
        if (vec) hipLaunchKernelGGL((pack_pathways_kernel<decltype(dt)::value, true>), g, b, 0, s, a);
        else hipLaunchKernelGGL((pack_pathways_kernel<decltype(dt)::value, false>), g, b, 0, s, a);
    });
    AF_CHECK_LAUNCH("pack_pathways_kernel");
    return AF_OK;
}
