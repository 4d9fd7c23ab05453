// cv2.resize(frame, (dw, dh)) with the default INTER_LINEAR for frames that sit in frame stores: one launch resizes up to
// AF_RESIZE_MAX_FRAMES frames, which may differ in source store, size, destination and destination size, into a detector's batch.
//
// Arithmetic: the plain C++ path of OpenCV 4.x resize.cpp for 8-bit images, restated (like the warp, the quality gate and the YUV
// conversion it cannot be pinned against cv2 itself where this is built, only against tests/resize_ref.py and its hand-worked
// anchors; an OpenCV built with IPP may take another path and differ from it):
//     (dw, dh) == (w, h)            a copy
//     inv = dw / w in fp64, scale_x = 1.0 / inv (not w / dw: the two can differ in the last bit); the same for y
//     |scale_x - 2| < DBL_EPSILON and |scale_y - 2| < DBL_EPSILON: OpenCV switches INTER_LINEAR to the fast area path,
//                                   (a + b + c + d + 2) >> 2 over each 2 x 2 block, per channel
//     otherwise, per destination column dx:
//         fx = float32((dx + 0.5) * scale_x - 0.5)   (fp64 product and difference, one rounding);  sx = floor(fx);  fx = float32(fx - sx)
//         sx < 0: sx = 0, fx = 0;   sx >= w - 1: sx = w - 1, fx = 0 (the second tap then has weight 0)
//         a1 = rint(fx * 2048f), a0 = rint((1f - fx) * 2048f)   (fp32 products, half to even, int16)
//         H[dx] = S[sx] * a0 + S[sx + 1] * a1                   (int32)
//       per destination row dy: the same fy, sy, b0, b1 without the clamp of fy; the rows sy and sy + 1 are each clipped to [0, h - 1]
//         out = (((b0 * (H0 >> 4)) >> 16) + ((b1 * (H1 >> 4)) >> 16) + 2) >> 2      (int32, cannot leave 0..255)
// The coefficients (index, a0, a1) are computed by the planner on the host, with floating-point contraction off: on the device
// hipcc would fuse (dx + 0.5) * scale_x - 0.5 into an fma and change bits.  The device does integer arithmetic only.  Channels are
// treated alike, so the byte order of a store passes through unchanged.
//
// Shape: memory-bound; the runs, tiles and fixed grid of af_frame_runs.h, which also holds the argument for the writes.
//
// No stray access, reads: every source byte address is row * pitch + 3 * col + c with 0 <= row < h, 0 <= col < w, c < 3, or a
// dword that covers 4 such bytes of one row at a 4-byte aligned address, never rounded down or widened past them.
#include <cfloat>
#include <cmath>
#include "af_frame_runs.h"

namespace af {

static_assert(sizeof(af_resize_header) % 8 == 0 && sizeof(af_resize_item) % 8 == 0 && sizeof(af_resize_coef) == 8, "table layout");

// N bytes (a multiple of 4) from p as little-endian dwords: dword loads when p is 4-byte aligned, else byte loads.  Reads [p, p + N).
template <int N>
__device__ __forceinline__ void rs_load(const unsigned char* p, unsigned (&d)[N / 4]) {
    if (((unsigned)(uintptr_t)p & 3) == 0) {
#pragma unroll
        for (int i = 0; i < N / 4; ++i) d[i] = ((const unsigned*)p)[i];
    } else {
#pragma unroll
        for (int i = 0; i < N / 4; ++i)
            d[i] = (unsigned)p[4 * i] | ((unsigned)p[4 * i + 1] << 8) | ((unsigned)p[4 * i + 2] << 16) | ((unsigned)p[4 * i + 3] << 24);
    }
}
template <int N>
__device__ __forceinline__ unsigned rs_byte(const unsigned (&d)[N], int k) { return (d[k >> 2] >> (8 * (k & 3))) & 255u; }

// one channel of one pixel: the horizontal pass of both rows, then the vertical one
__device__ __forceinline__ unsigned rs_linear(int s00, int s01, int s10, int s11, int a0, int a1, int b0, int b1) {
    const int h0 = s00 * a0 + s01 * a1, h1 = s10 * a0 + s11 * a1;
    return (unsigned)((((b0 * (h0 >> 4)) >> 16) + ((b1 * (h1 >> 4)) >> 16) + 2) >> 2);
}

__global__ __launch_bounds__(RUN_TILE) void resize_frames_kernel(const unsigned char* __restrict__ table, int n) {
    for (int tile = blockIdx.x, total = launch_tiles<AF_RESIZE_KIND, af_resize_header>(table, n); tile < total; tile += gridDim.x) {
        const TileRun<af_resize_item> r = tile_run<af_resize_header, af_resize_item>(table, n, tile);
        if (!r.npx) continue;
        const af_resize_item& it = r.it;
        const int dy = r.dy, x0 = r.x0, npx = r.npx;
        const unsigned char* src = (const unsigned char*)it.src;
        unsigned px[4] = {0, 0, 0, 0}, out[3];
        if (it.mode == AF_RESIZE_COPY) {
            const unsigned char* s = src + (long long)dy * it.src_pitch + 3 * x0;
            if (npx == RUN_PX) {
                rs_load<12>(s, out);                                 // x0 + 4 <= dw = w: the 12 bytes lie inside the row
            } else {
                for (int i = 0; i < npx; ++i) px[i] = (unsigned)s[3 * i] | ((unsigned)s[3 * i + 1] << 8) | ((unsigned)s[3 * i + 2] << 16);
                pack_run(px, out);
            }
        } else if (it.mode == AF_RESIZE_AREA2) {
            const unsigned char* s0 = src + (long long)(2 * dy) * it.src_pitch + 6 * x0;     // rows 2 dy, 2 dy + 1 < h = 2 dh
            const unsigned char* s1 = s0 + it.src_pitch;
            if (npx == RUN_PX) {
                unsigned r0[6], r1[6];                               // source pixels 2 x0 .. 2 x0 + 7 <= 2 dw - 1 = w - 1
                rs_load<24>(s0, r0);
                rs_load<24>(s1, r1);
#pragma unroll
                for (int i = 0; i < 4; ++i)
#pragma unroll
                    for (int c = 0; c < 3; ++c)
                        px[i] |= area2(rs_byte(r0, 6 * i + c), rs_byte(r0, 6 * i + 3 + c), rs_byte(r1, 6 * i + c), rs_byte(r1, 6 * i + 3 + c)) << (8 * c);
            } else {
                for (int i = 0; i < npx; ++i)
                    for (int c = 0; c < 3; ++c)
                        px[i] |= area2(s0[6 * i + c], s0[6 * i + 3 + c], s1[6 * i + c], s1[6 * i + 3 + c]) << (8 * c);
            }
            pack_run(px, out);
        } else {
            const af_resize_coef yc = ((const af_resize_coef*)(table + it.ytab))[dy];
            const int ra = min(max(yc.idx, 0), it.h - 1), rb = min(max(yc.idx + 1, 0), it.h - 1);
            const unsigned char* s0 = src + (long long)ra * it.src_pitch;
            const unsigned char* s1 = src + (long long)rb * it.src_pitch;
            const af_resize_coef* xt = (const af_resize_coef*)(table + it.xtab) + x0;
#pragma unroll
            for (int i = 0; i < 4; ++i) {
                if (i < npx) {
                    const af_resize_coef xc = xt[i];                 // 0 <= idx <= w - 1 by the planner
                    const int o0 = 3 * xc.idx, o1 = 3 * min(xc.idx + 1, it.w - 1);
#pragma unroll
                    for (int c = 0; c < 3; ++c)
                        px[i] |= rs_linear(s0[o0 + c], s0[o1 + c], s1[o0 + c], s1[o1 + c], xc.a0, xc.a1, yc.a0, yc.a1) << (8 * c);
                }
            }
            pack_run(px, out);
        }
        store_run12(run_dst(r), out, npx);
    }
}

// cv2.resize's scale of one axis: 1 / (dst / src), not src / dst
static inline double resize_scale(int src, int dst) {
    const double inv = (double)dst / (double)src;
    return 1.0 / inv;
}

// The coefficient table of one axis, src -> dst pixels.  clamp_x: the horizontal rule (index and weight clamped at both ends);
// without it the vertical one (the index may be -1 or src - 1: the kernel clips the two rows).
static void resize_coefs(int src, int dst, bool clamp_x, af_resize_coef* out) {
#pragma clang fp contract(off)
    const double scale = resize_scale(src, dst);
    for (int d = 0; d < dst; ++d) {
        float f = (float)((d + 0.5) * scale - 0.5);
        int s = (int)std::floor(f);
        f -= (float)s;
        if (clamp_x) {
            if (s < 0) { s = 0; f = 0.f; }
            if (s >= src - 1) { s = src - 1; f = 0.f; }
        }
        out[d].idx = s;
        out[d].a0 = (int16_t)lrintf((1.f - f) * 2048.f);
        out[d].a1 = (int16_t)lrintf(f * 2048.f);
    }
}

// one axis' table, src -> dst: dst coefficients at `offset`
struct ResizeGeom { int src, dst; int32_t offset; int64_t prepare() const { return (int64_t)dst * sizeof(af_resize_coef); } };

static int resize_plan(const af_resize_job* jobs, int n, const af_store_ref* stores, int n_stores, void* table, int64_t table_bytes, int64_t* used_bytes) {
    RunPlan<af_resize_header, af_resize_item> plan;
    int rc = plan.begin("resize_plan", n, n_stores);
    if (rc != AF_OK) return rc;
    std::vector<ResizeGeom> xs, ys;
    for (int i = 0; i < n; ++i) {
        const af_resize_job& j = jobs[i];
        const af_store_ref* st;
        unsigned char* src;
        rc = store_frame("resize_plan", "job", i, stores, n_stores, j.store, j.frame, false, true, &st, &src);
        if (rc != AF_OK) return rc;
        const af_frame_store& s = st->desc;
        AF_REQUIRE(j.dst, "resize_plan: job %d: null destination", i);
        AF_REQUIRE(j.dw >= 1 && j.dh >= 1 && j.dw <= AF_RESIZE_MAX_SIDE && j.dh <= AF_RESIZE_MAX_SIDE,
                   "resize_plan: job %d: a destination of %dx%d (1 to %d in both directions)", i, j.dw, j.dh, AF_RESIZE_MAX_SIDE);
        AF_REQUIRE(j.dst_pitch >= 3 * (int64_t)j.dw && j.dst_pitch <= 0x7fffffff, "resize_plan: job %d: destination pitch %lld is shorter than a row of %d bytes",
                   i, (long long)j.dst_pitch, 3 * j.dw);
        af_resize_item& it = plan.items[i];
        it.src = src;
        it.dst = j.dst;
        it.src_pitch = (int32_t)s.row_pitch; it.dst_pitch = (int32_t)j.dst_pitch;
        it.h = s.height; it.w = s.width; it.dh = j.dh; it.dw = j.dw;
        it.runs_x = row_runs(j.dw);
        if (j.dw == s.width && j.dh == s.height) {
            it.mode = AF_RESIZE_COPY;
        } else if (std::fabs(resize_scale(s.width, j.dw) - 2.0) < DBL_EPSILON && std::fabs(resize_scale(s.height, j.dh) - 2.0) < DBL_EPSILON &&
                   s.width == 2 * j.dw && s.height == 2 * j.dh) {    // OpenCV's test, and what it implies spelled out: the kernel's bounds rest on it
            it.mode = AF_RESIZE_AREA2;
        } else {
            it.mode = AF_RESIZE_LINEAR;
            it.xtab = axis_table_at(xs, s.width, j.dw, &plan.used).offset;
            it.ytab = axis_table_at(ys, s.height, j.dh, &plan.used).offset;
        }
        plan.add_tiles(i, j.dh, j.dw);
    }
    rc = plan.finish("resize_plan", AF_RESIZE_KIND, table, table_bytes, used_bytes);
    if (rc != AF_OK) return rc;
    unsigned char* t = (unsigned char*)table;
    for (const ResizeGeom& g : xs) resize_coefs(g.src, g.dst, true, (af_resize_coef*)(t + g.offset));
    for (const ResizeGeom& g : ys) resize_coefs(g.src, g.dst, false, (af_resize_coef*)(t + g.offset));
    return AF_OK;
}

}  // namespace af

extern "C" int64_t af_resize_table_bytes(const af_resize_job* jobs, int n) {
    if (!jobs || n < 0 || n > AF_RESIZE_MAX_FRAMES) return -1;
    int64_t bytes = (int64_t)sizeof(af_resize_header) + (int64_t)n * sizeof(af_resize_item);
    for (int i = 0; i < n; ++i) {
        if (jobs[i].dw < 1 || jobs[i].dh < 1 || jobs[i].dw > AF_RESIZE_MAX_SIDE || jobs[i].dh > AF_RESIZE_MAX_SIDE) return -1;
        bytes += ((int64_t)jobs[i].dw + jobs[i].dh) * (int64_t)sizeof(af_resize_coef);
    }
    return bytes;
}

extern "C" int af_resize_plan_u8(const af_resize_job* jobs, int n, const af_store_ref* stores, int n_stores, void* table, int64_t table_bytes,
                                 int64_t* used_bytes) {
    using namespace af;
    AF_REQUIRE(jobs && stores, "resize_plan: null argument");
    return plan_into<af_resize_header>("resize_plan", table, table_bytes, used_bytes,
                                       [&] { return resize_plan(jobs, n, stores, n_stores, table, table_bytes, used_bytes); });
}

extern "C" int af_resize_frames_u8(const void* table_dev, int n, void* stream) {
    return af::launch_runs("resize_frames", "resize_frames_kernel", af::resize_frames_kernel, table_dev, n, AF_RESIZE_MAX_FRAMES, stream);
}
