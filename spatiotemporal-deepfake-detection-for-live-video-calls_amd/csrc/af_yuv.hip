// YUV 4:2:0 frames (NV12 / NV21 / I420 / YV12) -> packed B, G, R or R, G, B bytes, written straight into frame stores: what a
// WebRTC stack or a hardware decoder hands over becomes the bytes cv2.VideoCapture would have handed over, on the device.
//
// Arithmetic: OpenCV's cvtColor(..., COLOR_YUV2BGR_NV12 / _I420), the fixed-point BT.601 limited-range conversion of
// color_yuv.simd.hpp, restated (like the warp and the quality gate it cannot be pinned against cv2 itself where this is built, only
// against tests/yuv_ref.py, its anchors and its sums over the whole (Y, U, V) cube):
//     y = max(0, Y - 16) * 1220542;  u = U - 128;  v = V - 128
//     R = clamp((y + 2^19 + 1673527 v) >> 20)   G = clamp((y + 2^19 - 852492 v - 409993 u) >> 20)   B = clamp((y + 2^19 + 2116026 u) >> 20)
// in int32 (the largest magnitude is 5.6e8) with arithmetic shifts; a 2 x 2 block of Y shares one (U, V), nothing is interpolated.
// Full range, BT.709, 4:2:2 / 4:4:4 and 10-bit formats are af_yuv_formats.hip's; not built: NV24 / NV42, 12-bit, BT.2020, chroma
// siting / interpolation.
//
// Shape: memory-bound, 1.5 bytes in and 3 bytes out per pixel.  A lane owns a run of 8 pixels of two rows (one chroma row): 8 + 8
// bytes of Y, 8 of chroma in, 24 + 24 bytes out.  The runs of an item are numbered row pair by row pair; a workgroup of 256 lanes
// takes 256 consecutive runs (a tile), and the tiles of all items of a launch form one flat list with a `first_tile` prefix per
// item, as face_quality_stores_kernel maps its tiles to rectangles.  The table of items travels by value as the kernel argument.
//
// Alignment.  Nothing is assumed beyond what an address shows: every access picks, per row, the widest naturally aligned form its
// address allows.  A destination row is 3 w bytes with w even, so rows are 2-byte aligned in general (at w = 6 row 1 starts at byte
// 18); a 24-byte run then goes out as halfword, five dwords built across the dword seam, halfword.  Source planes may have odd
// pitches and fall back to halfword or byte loads.
//
// No stray access.  A full run reads exactly the bytes [8 j, 8 j + 8) of its Y rows and of an interleaved chroma row (or [4 j, 4 j
// + 4) of each planar one) and writes exactly [24 j, 24 j + 24) of its two destination rows, with 8 j + 8 <= w.  The last run of a
// row when w is no multiple of 8 holds 2, 4 or 6 pixels and moves them pixel pair by pixel pair with accesses of exactly the pair's
// bytes.  No load is rounded down to an aligned address or widened past the pair, so no byte outside a plane's rows or outside the
// h * w * 3 destination bytes is touched.
#include "af_common.h"
#include "af_yuv_runs.h"

namespace af {

constexpr int YUV_CY = 1220542, YUV_CUB = 2116026, YUV_CUG = -409993, YUV_CVG = -852492, YUV_CVR = 1673527;
constexpr int YUV_SHIFT = 20, YUV_HALF = 1 << 19;

struct YuvArgs {
    int32_t n, total_tiles;
    af_yuv_item item[AF_YUV_MAX_FRAMES];
};
static_assert(sizeof(af_yuv_item) == 56, "argument budget");
static_assert(sizeof(YuvArgs) <= 4096, "kernel arguments");

static inline int64_t yuv_tiles(int h, int w) {
    const int64_t runs = (int64_t)(h / 2) * ((w + YUV_RUN - 1) / YUV_RUN);
    return (runs + YUV_TILE - 1) / YUV_TILE;
}

// the chroma terms of one (U, V): what is added to y for R, G and B
struct Chroma {
    int r, g, b;
};
__device__ __forceinline__ Chroma chroma_terms(int U, int V) {
    const int u = U - 128, v = V - 128;
    return Chroma{YUV_HALF + YUV_CVR * v, YUV_HALF + YUV_CVG * v + YUV_CUG * u, YUV_HALF + YUV_CUB * u};
}

// one pixel's three bytes in the destination's order, as the low 24 bits
__device__ __forceinline__ unsigned pixel_bytes(int Y, const Chroma& c, int bgr) {
    const int y = max(0, Y - 16) * YUV_CY;
    const unsigned R = clamp_u8((y + c.r) >> YUV_SHIFT), G = clamp_u8((y + c.g) >> YUV_SHIFT), B = clamp_u8((y + c.b) >> YUV_SHIFT);
    return bgr ? (B | (G << 8) | (R << 16)) : (R | (G << 8) | (B << 16));
}

// 8 pixels of one row: y[2] are the row's 8 Y bytes, c[4] the four chroma terms -> 24 bytes as six dwords
__device__ __forceinline__ void convert_run(const unsigned (&y)[2], const Chroma (&c)[4], int bgr, unsigned (&out)[6]) {
    unsigned px[8];
#pragma unroll
    for (int i = 0; i < 8; ++i) px[i] = pixel_bytes((int)((y[i >> 2] >> (8 * (i & 3))) & 255u), c[i >> 1], bgr);
#pragma unroll
    for (int q = 0; q < 2; ++q) {                                 // four pixels are three dwords
        out[3 * q + 0] = px[4 * q] | (px[4 * q + 1] << 24);
        out[3 * q + 1] = (px[4 * q + 1] >> 8) | (px[4 * q + 2] << 16);
        out[3 * q + 2] = (px[4 * q + 2] >> 16) | (px[4 * q + 3] << 8);
    }
}

__global__ __launch_bounds__(YUV_TILE) void yuv420_to_rgb_kernel(const YuvArgs a) {
    const int tile = blockIdx.x;
    if (tile >= a.total_tiles) return;
    int k = 0;
    while (k + 1 < a.n && a.item[k + 1].first_tile <= tile) ++k;  // tens of items: a scan
    const af_yuv_item it = a.item[k];
    const int w = it.w, h = it.h;
    const int runs_x = (w + YUV_RUN - 1) / YUV_RUN;
    const int run = (tile - it.first_tile) * YUV_TILE + (int)threadIdx.x;      // at most 16383 * 4096 runs per item
    if (run >= (h / 2) * runs_x) return;
    const int rp = run / runs_x, j = run - rp * runs_x;
    const int x0 = j * YUV_RUN;
    const int bgr = it.bgr, swap = it.swap_uv;

    const unsigned char* y0 = (const unsigned char*)it.y + (long long)(2 * rp) * it.y_pitch + x0;
    const unsigned char* y1 = y0 + it.y_pitch;
    unsigned char* d0 = (unsigned char*)it.dst + (long long)(2 * rp) * it.dst_pitch + (long long)x0 * 3;
    unsigned char* d1 = d0 + it.dst_pitch;
    // interleaved: pixel pair p has its two chroma bytes at c0[2 p], c0[2 p + 1]; planar: one byte in each plane at [p]
    const unsigned char* c0 = (const unsigned char*)it.c0 + (long long)rp * it.c_pitch + (it.interleaved ? x0 : x0 / 2);
    const unsigned char* c1 = it.interleaved ? nullptr : (const unsigned char*)it.c1 + (long long)rp * it.c_pitch + x0 / 2;

    if (x0 + YUV_RUN <= w) {
        // A full run: x0 + 8 <= w, so the 8 Y bytes of each row, the 8 interleaved chroma bytes (pairs x0 / 2 .. x0 / 2 + 3 of the
        // w / 2 pairs of the row) or the 4 + 4 planar ones all lie inside their plane's row; load_bytes reads exactly those bytes.
        unsigned ya[2], yb[2];
        load_bytes<8>(y0, ya);
        load_bytes<8>(y1, yb);
        Chroma c[4];
        if (it.interleaved) {
            unsigned uv[2];
            load_bytes<8>(c0, uv);
#pragma unroll
            for (int p = 0; p < 4; ++p) {
                const int first = (int)((uv[p >> 1] >> (16 * (p & 1))) & 255u), second = (int)((uv[p >> 1] >> (16 * (p & 1) + 8)) & 255u);
                c[p] = swap ? chroma_terms(second, first) : chroma_terms(first, second);
            }
        } else {
            unsigned ua[1], va[1];
            load_bytes<4>(c0, ua);
            load_bytes<4>(c1, va);
#pragma unroll
            for (int p = 0; p < 4; ++p) {
                const int first = (int)((ua[0] >> (8 * p)) & 255u), second = (int)((va[0] >> (8 * p)) & 255u);
                c[p] = swap ? chroma_terms(second, first) : chroma_terms(first, second);
            }
        }
        unsigned out[6];
        convert_run(ya, c, bgr, out);
        store_run(d0, out);
        convert_run(yb, c, bgr, out);
        store_run(d1, out);
    } else {
        // The tail of a row: (w - x0) / 2 = 1, 2 or 3 pixel pairs, each with byte loads of its own bytes only.
        const int pairs = (w - x0) / 2;
        for (int p = 0; p < pairs; ++p) {
            const int first = it.interleaved ? c0[2 * p] : c0[p], second = it.interleaved ? c0[2 * p + 1] : c1[p];
            const Chroma c = swap ? chroma_terms(second, first) : chroma_terms(first, second);
            store_pair(d0 + 6 * p, pixel_bytes(y0[2 * p], c, bgr), pixel_bytes(y0[2 * p + 1], c, bgr));
            store_pair(d1 + 6 * p, pixel_bytes(y1[2 * p], c, bgr), pixel_bytes(y1[2 * p + 1], c, bgr));
        }
    }
}

static int yuv_check_item(const char* who, int i, const af_yuv_item& it) {
    AF_REQUIRE(it.y && it.c0 && it.dst && (it.interleaved || it.c1), "%s: item %d: null plane or destination", who, i);
    AF_REQUIRE(it.h > 0 && it.w > 0 && it.h % 2 == 0 && it.w % 2 == 0 && it.h <= 32766 && it.w <= 32766,
               "%s: item %d: a 4:2:0 frame is even and positive in both directions (at most 32766), not %dx%d", who, i, (int)it.w, (int)it.h);
    AF_REQUIRE(it.y_pitch >= it.w, "%s: item %d: Y pitch %d is shorter than a row of %d bytes", who, i, it.y_pitch, (int)it.w);
    const int crow = it.interleaved ? it.w : it.w / 2;
    AF_REQUIRE(it.c_pitch >= crow, "%s: item %d: chroma pitch %d is shorter than a row of %d bytes", who, i, it.c_pitch, crow);
    AF_REQUIRE(it.dst_pitch >= 3 * (int)it.w, "%s: item %d: destination pitch %d is shorter than a row of %d bytes", who, i, it.dst_pitch, 3 * (int)it.w);
    return AF_OK;
}

}  // namespace af

extern "C" int af_yuv420_plan_u8(const af_yuv_frame* frames, int n, const af_store_ref* stores, int n_stores, af_yuv_item* items) {
    using namespace af;
    AF_REQUIRE(frames && stores && items, "yuv420_plan: null argument");
    AF_REQUIRE(n >= 0 && n <= AF_YUV_MAX_FRAMES, "yuv420_plan: %d frames (at most %d per launch)", n, AF_YUV_MAX_FRAMES);
    AF_REQUIRE(n_stores > 0 && n_stores <= AF_MAX_STORES, "yuv420_plan: %d stores (1 to %d per launch)", n_stores, AF_MAX_STORES);
    int64_t tiles = 0;
    for (int i = 0; i < n; ++i) {
        const af_yuv_frame& f = frames[i];
        AF_REQUIRE(f.h > 0 && f.w > 0 && f.h % 2 == 0 && f.w % 2 == 0 && f.h <= 32766 && f.w <= 32766,
                   "yuv420_plan: frame %d: a 4:2:0 frame is even and positive in both directions (at most 32766), not %dx%d", i, f.w, f.h);
        AF_REQUIRE(f.y && f.u && (f.interleaved || f.v), "yuv420_plan: frame %d: null plane", i);
        AF_REQUIRE(f.y_pitch >= f.w && f.y_pitch <= 0x7fffffff, "yuv420_plan: frame %d: Y pitch %lld is shorter than a row of %d bytes", i,
                   (long long)f.y_pitch, f.w);
        const int crow = f.interleaved ? f.w : f.w / 2;
        AF_REQUIRE(f.c_pitch >= crow && f.c_pitch <= 0x7fffffff, "yuv420_plan: frame %d: chroma pitch %lld is shorter than a row of %d bytes", i,
                   (long long)f.c_pitch, crow);
        const af_store_ref* ref;
        unsigned char* dst;
        // one slot is written, so the store need not hold all its frames (whole = false): the slot's own bytes are checked below
        const int rc = store_frame("yuv420_plan", "frame", i, stores, n_stores, f.store, f.slot, true, false, &ref, &dst);
        if (rc != AF_OK) return rc;
        const af_store_ref& st = *ref;
        const af_frame_store& s = st.desc;
        AF_REQUIRE(s.height == f.h && s.width == f.w, "yuv420_plan: frame %d of %dx%d does not fit store %d of %d frames of %dx%d", i, f.w, f.h, f.store,
                   s.n_frames, s.width, s.height);
        AF_REQUIRE((int64_t)f.slot * s.frame_stride + frame_span(s) <= s.store_bytes, "yuv420_plan: frame %d: slot %d leaves store %d of %d frames, %lld bytes", i,
                   f.slot, f.store, s.n_frames, (long long)s.store_bytes);
        af_yuv_item& it = items[i];
        it.y = f.y; it.c0 = f.u; it.c1 = f.interleaved ? nullptr : f.v;
        it.dst = dst;
        it.y_pitch = (int32_t)f.y_pitch; it.c_pitch = (int32_t)f.c_pitch; it.dst_pitch = (int32_t)s.row_pitch;
        it.first_tile = (int32_t)tiles;
        it.h = (uint16_t)f.h; it.w = (uint16_t)f.w;
        it.interleaved = f.interleaved ? 1 : 0; it.swap_uv = f.swap_uv ? 1 : 0; it.bgr = st.bgr ? 1 : 0; it.reserved = 0;
        tiles += yuv_tiles(f.h, f.w);
        AF_REQUIRE(tiles <= 0x7fffffff, "yuv420_plan: too many pixels");
    }
    return AF_OK;
}

extern "C" int af_yuv420_to_rgb_u8(const af_yuv_item* items, int n, void* stream) {
    using namespace af;
    AF_REQUIRE(items, "yuv420_to_rgb: null argument");
    AF_REQUIRE(n >= 0 && n <= AF_YUV_MAX_FRAMES, "yuv420_to_rgb: %d frames (at most %d per launch)", n, AF_YUV_MAX_FRAMES);
    if (n == 0) return AF_OK;
    YuvArgs a;
    a.n = n;
    int64_t tiles = 0;
    for (int i = 0; i < n; ++i) {
        const int rc = yuv_check_item("yuv420_to_rgb", i, items[i]);
        if (rc != AF_OK) return rc;
        AF_REQUIRE(items[i].first_tile == tiles, "yuv420_to_rgb: item %d: first_tile %d, %lld by the sizes before it (hand in a table af_yuv420_plan_u8 filled)",
                   i, items[i].first_tile, (long long)tiles);
        a.item[i] = items[i];
        tiles += yuv_tiles(items[i].h, items[i].w);
        AF_REQUIRE(tiles <= 0x7fffffff, "yuv420_to_rgb: too many pixels");
    }
    a.total_tiles = (int32_t)tiles;
    hipLaunchKernelGGL(yuv420_to_rgb_kernel, dim3((unsigned)tiles), dim3(YUV_TILE), 0, (hipStream_t)stream, a);
    AF_CHECK_LAUNCH("yuv420_to_rgb_kernel");
    return AF_OK;
}
