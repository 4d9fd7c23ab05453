// Clip aligner warp: the per-frame
//     new_image = zeros(h, w, 3); new_image[y:y+ih, x:x+iw] = crop; cv2.warpAffine(new_image, tfm, (size, size))
// loop of FasterCropAlignXRay.process_single (reference altfreezing/test_tools/faster_crop_align_xray.py:75-88),
// for all frames of a clip in one launch, straight from the uploaded crops (the zero canvas is never built: a tap
// outside the pasted crop is 0 whether it falls on the canvas or beyond it - BORDER_CONSTANT 0).
//
// Arithmetic: OpenCV's fixed-point bilinear warp (imgwarp.cpp warpAffine / WarpAffineInvoker / remapBilinear, 3.x-4.10):
// the forward matrix is inverted in double on the host in OpenCV's order of operations; a destination pixel's source
// coordinate is X = (cvRound((M1*y + M2)*1024) + 16 + cvRound(M0*x*1024)) >> 5 in 1/32 pixel (doubles, no FMA
// contraction: __dmul_rn / __dadd_rn), weights (32-fx)(32-fy)*32 etc. (15-bit, sum 32768), dst = (sum + 16384) >> 15.
// Integer work: bit-exact against oracle/aligner_oracle.py; against cv2 itself the parity is unpinned (cv2 is absent
// from the build image and the reference holds no aligned frame).
// HBM-bound byte work: one thread per destination pixel, 4 x 3 source bytes in, 3 bytes out; a clip is ~5 MB.
// (warp_affine_windows_kernel further down does the same for many windows of a track in one launch, four pixels per thread.)
#include "af_common.h"
#include <cmath>
#include <string.h>

namespace af {

struct AlignArgs {
    const unsigned char* crops;
    unsigned char* out;
    double m[6];                 // dst -> src map (already inverted)
    int size, n;
    int canvas_h, canvas_w;
    af_align_frame f[AF_ALIGN_MAX_FRAMES];
};

__device__ __forceinline__ int cv_round_sat(double v) {       // saturate_cast<int>(double): round half to even, saturated
    const double r = rint(v);
    return r <= -2147483648.0 ? (int)0x80000000 : r >= 2147483647.0 ? 0x7fffffff : (int)r;
}

__global__ __launch_bounds__(256) void warp_affine_clip_kernel(const AlignArgs a) {
    const int p = blockIdx.x * 256 + threadIdx.x, fr = blockIdx.y;
    if (p >= a.size * a.size) return;
    const int y = p / a.size, x = p - y * a.size;
    const af_align_frame f = a.f[fr];
    const int adelta = cv_round_sat(__dmul_rn(__dmul_rn(a.m[0], (double)x), 1024.0));
    const int bdelta = cv_round_sat(__dmul_rn(__dmul_rn(a.m[3], (double)x), 1024.0));
    const int X0 = cv_round_sat(__dmul_rn(__dadd_rn(__dmul_rn(a.m[1], (double)y), a.m[2]), 1024.0)) + 16;
    const int Y0 = cv_round_sat(__dmul_rn(__dadd_rn(__dmul_rn(a.m[4], (double)y), a.m[5]), 1024.0)) + 16;
    const long long X = ((long long)X0 + adelta) >> 5, Y = ((long long)Y0 + bdelta) >> 5;
    long long sxl = X >> 5, syl = Y >> 5;
    const int sx = (int)(sxl < -32768 ? -32768 : sxl > 32767 ? 32767 : sxl);      // saturate_cast<short>
    const int sy = (int)(syl < -32768 ? -32768 : syl > 32767 ? 32767 : syl);
    const int fx = (int)(X & 31), fy = (int)(Y & 31);
    int acc[3] = {0, 0, 0};
    const unsigned char* img = a.crops + f.offset;
#pragma unroll
    for (int dy = 0; dy < 2; ++dy)
#pragma unroll
        for (int dx = 0; dx < 2; ++dx) {
            const int cx = sx + dx, cy = sy + dy;                     // canvas coordinates of the tap
            const int ix = cx - f.x, iy = cy - f.y;                   // crop coordinates
            if ((unsigned)cx < (unsigned)a.canvas_w && (unsigned)cy < (unsigned)a.canvas_h &&
                (unsigned)ix < (unsigned)f.iw && (unsigned)iy < (unsigned)f.ih) {
                const int w = (dx ? fx : 32 - fx) * (dy ? fy : 32 - fy) * 32;
                const unsigned char* s = img + ((long long)iy * f.iw + ix) * 3;
                acc[0] += w * s[0]; acc[1] += w * s[1]; acc[2] += w * s[2];
            }
        }
    unsigned char* o = a.out + (((long long)fr * a.size + y) * a.size + x) * 3;
#pragma unroll
    for (int c = 0; c < 3; ++c) {
        const int v = (acc[c] + (1 << 14)) >> 15;
        o[c] = (unsigned char)(v > 255 ? 255 : v);
    }
}

// warpAffine(): forward 2x3 matrix -> dst-to-src map, in double, same order of operations (volatile: no contraction)
static void invert_affine_cv(const double* tfm, double* inv) {
    volatile double M[6];
    for (int i = 0; i < 6; ++i) M[i] = tfm[i];
    volatile double D = M[0] * M[4] - M[1] * M[3];
    D = D != 0 ? 1.0 / D : 0.0;
    volatile double A11 = M[4] * D, A22 = M[0] * D;
    M[0] = A11; M[1] = M[1] * -D; M[3] = M[3] * -D; M[4] = A22;
    volatile double t0 = -M[0] * M[2], t1 = M[1] * M[5], t2 = -M[3] * M[2], t3 = M[4] * M[5];
    volatile double b1 = t0 - t1, b2 = t2 - t3;
    M[2] = b1; M[5] = b2;
    for (int i = 0; i < 6; ++i) inv[i] = M[i];
}

// ---- window-batch warp: every (window, frame) of up to AF_WINDOW_MAX_BATCH sliding windows of one face track in one launch ----
// The windows of a track share their crops (stride 1: 31 of 32), so the crops sit once in a device pool and each window brings
// its own dst -> src map and paste offsets.  Those tables are too big for kernel arguments: af_window_batch_plan_u8 writes them
// into a caller-owned host buffer (layout below), the caller copies it to the device once per batch.
// Same integers as warp_affine_clip_kernel.  What differs is how they are produced: a block owns WB_ROWS rows of one
// (window, frame); the column terms adelta[x] / bdelta[x] and the row terms X0[y] / Y0[y] (the only double arithmetic) are
// tabulated in LDS once per block, as OpenCV tabulates them; a thread makes four consecutive pixels and stores them as one
// 12-byte store; the two taps of a source row are read as 6 contiguous bytes (a dword and a half-word load, unaligned) from a
// clamped address, and a tap outside the crop gets weight 0 instead of a branch.
// Two forms of one kernel body, told apart by the work item's type.  af_align_frame: a tightly packed crop in a pool (row pitch
// iw * 3).  WindowRect: a sub-rectangle of a frame that is resident in a device frame store, with the frame's own row pitch in
// bytes (any value: 1 923 for a 641-wide frame; the 6-byte tap reads are unaligned in both forms).  The bytes around a rectangle
// are the frame's other pixels, not padding: only the clamp of (row, column) into the rectangle together with the zero weight of
// a tap outside it keeps them out of the result, and only the last rectangle of the store needs 3 readable bytes behind it.
// The WindowRect form also comes for frames whose pixels are B, G, R in memory (what a capture API delivers): kBgr only chooses
// which of the three accumulated channels goes to which byte of the R, G, B store - the reads and the arithmetic are the same.
constexpr int WB_ROWS = 32, WB_THREADS = 256;
constexpr int32_t WB_KIND_POOL = 0, WB_KIND_RECTS = 1, WB_KIND_STORES = 2;    // WindowTableHeader::kind
struct WindowTableHeader { int32_t n_windows, clip_size, size, kind; };
struct WindowXform { double m[6]; };                             // dst -> src map (already inverted)
struct WindowRect { int64_t offset; int32_t ih, iw, x, y, pitch, reserved; };    // offset: the rectangle's first pixel in the store
// A rectangle of one of several stores (af_window_rects_plan_stores_u8): the absolute device address of its first pixel instead
// of an offset, and its store's byte order - the launch has no store pointer of its own and the R/B choice is per item.
struct WindowStoreRect { const unsigned char* first; int32_t ih, iw, x, y, pitch, bgr; };
static_assert(sizeof(WindowStoreRect) == sizeof(WindowRect), "one table size for both rectangle forms");

// byte of pixel (row, col) of the work item's image, the one expression in which the two forms differ
__device__ __forceinline__ long long wb_byte(const af_align_frame& f, int row, int col) { return ((long long)row * f.iw + col) * 3; }
__device__ __forceinline__ long long wb_byte(const WindowRect& f, int row, int col) { return (long long)row * f.pitch + col * 3; }
__device__ __forceinline__ long long wb_byte(const WindowStoreRect& f, int row, int col) { return (long long)row * f.pitch + col * 3; }
// the work item's first byte, and whether its first and third byte are exchanged on the way out
__device__ __forceinline__ const unsigned char* wb_first(const unsigned char* pool, const af_align_frame& f) { return pool + f.offset; }
__device__ __forceinline__ const unsigned char* wb_first(const unsigned char* pool, const WindowRect& f) { return pool + f.offset; }
__device__ __forceinline__ const unsigned char* wb_first(const unsigned char*, const WindowStoreRect& f) { return f.first; }
template <bool kBgr> __device__ __forceinline__ bool wb_bgr(const af_align_frame&) { return kBgr; }
template <bool kBgr> __device__ __forceinline__ bool wb_bgr(const WindowRect&) { return kBgr; }
template <bool kBgr> __device__ __forceinline__ bool wb_bgr(const WindowStoreRect& f) { return f.bgr != 0; }
template <typename Item> struct WbKind;
template <> struct WbKind<af_align_frame> { static constexpr int32_t value = WB_KIND_POOL; };
template <> struct WbKind<WindowRect> { static constexpr int32_t value = WB_KIND_RECTS; };
template <> struct WbKind<WindowStoreRect> { static constexpr int32_t value = WB_KIND_STORES; };

static inline int64_t window_table_bytes(int n_windows, int clip_size, size_t item = sizeof(af_align_frame)) {
    return (int64_t)sizeof(WindowTableHeader) + (int64_t)n_windows * sizeof(WindowXform) + (int64_t)n_windows * clip_size * (int64_t)item;
}

template <typename Item, bool kBgr = false>
__global__ __launch_bounds__(WB_THREADS) void warp_affine_windows_kernel(const unsigned char* __restrict__ pool, const unsigned char* __restrict__ table,
                                                                         unsigned char* __restrict__ out, int n_windows, int clip_size, int size,
                                                                         int tiles) {
    __shared__ int s_ad[AF_WINDOW_MAX_SIZE], s_bd[AF_WINDOW_MAX_SIZE], s_x0[WB_ROWS], s_y0[WB_ROWS];
    const WindowTableHeader hd = *(const WindowTableHeader*)table;
    if (hd.n_windows != n_windows || hd.clip_size != clip_size || hd.size != size || hd.kind != WbKind<Item>::value) return;   // not this launch's table
    const int bid = blockIdx.x;                                   // work item k = window * clip_size + frame, window-major
    const int k = bid / tiles, tile = bid - k * tiles, y0 = tile * WB_ROWS;
    const WindowXform* xf = (const WindowXform*)(table + sizeof(WindowTableHeader));
    const Item f = ((const Item*)(xf + n_windows))[k];
    const int window = k / clip_size;
    const double m0 = xf[window].m[0], m1 = xf[window].m[1], m2 = xf[window].m[2];
    const double m3 = xf[window].m[3], m4 = xf[window].m[4], m5 = xf[window].m[5];
    for (int x = threadIdx.x; x < size; x += WB_THREADS) {
        s_ad[x] = cv_round_sat(__dmul_rn(__dmul_rn(m0, (double)x), 1024.0));
        s_bd[x] = cv_round_sat(__dmul_rn(__dmul_rn(m3, (double)x), 1024.0));
    }
    if (threadIdx.x < WB_ROWS) {
        const double y = (double)(y0 + (int)threadIdx.x);
        s_x0[threadIdx.x] = cv_round_sat(__dmul_rn(__dadd_rn(__dmul_rn(m1, y), m2), 1024.0)) + 16;
        s_y0[threadIdx.x] = cv_round_sat(__dmul_rn(__dadd_rn(__dmul_rn(m4, y), m5), 1024.0)) + 16;
    }
    __syncthreads();
    const int rows = size - y0 < WB_ROWS ? size - y0 : WB_ROWS, quads = size >> 2;
    const unsigned char* img = wb_first(pool, f);
    const bool bgr = wb_bgr<kBgr>(f);                             // a constant of the kernel, except for WindowStoreRect
    unsigned char* dst = out + ((long long)k * size + y0) * (long long)size * 3;
    for (int i = threadIdx.x; i < rows * quads; i += WB_THREADS) {
        const int r = i / quads, q = i - r * quads;
        const long long X0 = s_x0[r], Y0 = s_y0[r];
        unsigned px[4];
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            const int x = q * 4 + j;
            const long long X = (X0 + s_ad[x]) >> 5, Y = (Y0 + s_bd[x]) >> 5;
            const long long sxl = X >> 5, syl = Y >> 5;
            const int sx = (int)(sxl < -32768 ? -32768 : sxl > 32767 ? 32767 : sxl);      // saturate_cast<short>
            const int sy = (int)(syl < -32768 ? -32768 : syl > 32767 ? 32767 : syl);
            const int fx = (int)(X & 31), fy = (int)(Y & 31);
            const int ix = sx - f.x, iy = sy - f.y;                   // crop coordinates of the top-left tap (the crop lies inside the canvas)
            // the pair (A, B) is read at column clamp(ix): A is tap ix (or tap ix + 1 when ix = -1), B is tap ix + 1
            const bool in0 = (unsigned)ix < (unsigned)f.iw;
            const int wa = in0 ? 32 - fx : ix == -1 ? fx : 0;
            const int wb = in0 && ix + 1 < f.iw ? fx : 0;
            const int wy0 = (unsigned)iy < (unsigned)f.ih ? (32 - fy) * 32 : 0;
            const int wy1 = (unsigned)(iy + 1) < (unsigned)f.ih ? fy * 32 : 0;
            const int col = ix < 0 ? 0 : ix > f.iw - 1 ? f.iw - 1 : ix;
            const int ra = iy < 0 ? 0 : iy > f.ih - 1 ? f.ih - 1 : iy;
            const int rb = iy + 1 < 0 ? 0 : iy + 1 > f.ih - 1 ? f.ih - 1 : iy + 1;
            const unsigned char* pa = img + wb_byte(f, ra, col);
            const unsigned char* pb = img + wb_byte(f, rb, col);
            unsigned a4, b4; unsigned short a2, b2;
            __builtin_memcpy(&a4, pa, 4); __builtin_memcpy(&a2, pa + 4, 2);
            __builtin_memcpy(&b4, pb, 4); __builtin_memcpy(&b2, pb + 4, 2);
            const int w00 = wa * wy0, w01 = wb * wy0, w10 = wa * wy1, w11 = wb * wy1;     // = the four (32-fx)(32-fy)*32 ... weights, or 0
            const int c0 = w00 * (int)(a4 & 255) + w01 * (int)(a4 >> 24) + w10 * (int)(b4 & 255) + w11 * (int)(b4 >> 24);
            const int c1 = w00 * (int)((a4 >> 8) & 255) + w01 * (int)(a2 & 255) + w10 * (int)((b4 >> 8) & 255) + w11 * (int)(b2 & 255);
            const int c2 = w00 * (int)((a4 >> 16) & 255) + w01 * (int)(a2 >> 8) + w10 * (int)((b4 >> 16) & 255) + w11 * (int)(b2 >> 8);
            const int v0 = (c0 + (1 << 14)) >> 15, v1 = (c1 + (1 << 14)) >> 15, v2 = (c2 + (1 << 14)) >> 15;
            const int vr = bgr ? v2 : v0, vb = bgr ? v0 : v2;            // source byte 0 is B in a BGR frame; the store is R, G, B
            px[j] = (unsigned)(vr > 255 ? 255 : vr) | (unsigned)(v1 > 255 ? 255 : v1) << 8 | (unsigned)(vb > 255 ? 255 : vb) << 16;
        }
        uint3 o;                                                      // 4 x RGB = 3 dwords (size % 4 == 0: every quad is dword-aligned)
        o.x = px[0] | px[1] << 24;
        o.y = px[1] >> 8 | px[2] << 16;
        o.z = px[2] >> 16 | px[3] << 8;
        *(uint3*)(dst + ((long long)r * size + q * 4) * 3) = o;
    }
}

}  // namespace af

extern "C" int64_t af_window_batch_table_bytes(int n_windows, int clip_size) {
    if (n_windows <= 0 || n_windows > AF_WINDOW_MAX_BATCH || clip_size <= 0 || clip_size > AF_ALIGN_MAX_FRAMES) return 0;
    return af::window_table_bytes(n_windows, clip_size);
}

extern "C" int af_window_batch_plan_u8(const af_window_desc* windows, const af_align_frame* frames, int n_windows, int clip_size, int size,
                                       int64_t pool_bytes, void* table, int64_t table_bytes, int32_t* bad_window, int32_t* bad_frame) {
    using namespace af;
    if (bad_window) *bad_window = -1;
    if (bad_frame) *bad_frame = -1;
    AF_REQUIRE(windows && frames && table, "window_batch_plan: null argument");
    AF_REQUIRE(n_windows > 0 && n_windows <= AF_WINDOW_MAX_BATCH && clip_size > 0 && clip_size <= AF_ALIGN_MAX_FRAMES,
               "window_batch_plan: %d windows of %d frames (at most %d of %d)", n_windows, clip_size, AF_WINDOW_MAX_BATCH, AF_ALIGN_MAX_FRAMES);
    AF_REQUIRE(size > 0 && size <= AF_WINDOW_MAX_SIZE && size % 4 == 0, "window_batch_plan: size %d (a multiple of 4, at most %d)", size, AF_WINDOW_MAX_SIZE);
    AF_REQUIRE(pool_bytes > 0 && table_bytes >= window_table_bytes(n_windows, clip_size), "window_batch_plan: table of %lld bytes, %lld needed",
               (long long)table_bytes, (long long)window_table_bytes(n_windows, clip_size));
    WindowTableHeader* hd = (WindowTableHeader*)table;
    WindowXform* xf = (WindowXform*)(hd + 1);
    af_align_frame* out = (af_align_frame*)(xf + n_windows);
    for (int w = 0; w < n_windows; ++w) {
        const af_window_desc& d = windows[w];
        AF_REQUIRE(d.canvas_h > 0 && d.canvas_w > 0 && d.canvas_h <= 32767 && d.canvas_w <= 32767, "window_batch_plan: window %d: bad canvas %dx%d",
                   w, d.canvas_w, d.canvas_h);
        invert_affine_cv(d.tfm, xf[w].m);
        for (int t = 0; t < clip_size; ++t) {
            const af_align_frame& f = frames[w * clip_size + t];
            // the kernel reads the two taps of a row as 6 bytes: 3 readable bytes must follow every crop
            AF_REQUIRE(f.ih > 0 && f.iw > 0 && f.offset >= 0 && f.offset + (int64_t)f.ih * f.iw * 3 + 3 <= pool_bytes,
                       "window_batch_plan: window %d frame %d: crop %dx%d at byte %lld leaves the pool of %lld bytes", w, t, f.iw, f.ih,
                       (long long)f.offset, (long long)pool_bytes);
            // the reference pastes with new_image[y:y+ih, x:x+iw] = image, which numpy refuses unless the crop fits the canvas
            if (f.x < 0 || f.y < 0 || (long long)f.x + f.iw > d.canvas_w || (long long)f.y + f.ih > d.canvas_h) {
                if (bad_window) *bad_window = w;
                if (bad_frame) *bad_frame = t;
                return set_error(AF_ERR_ARG, "aligner: window %d frame %d (%dx%d at %d,%d) does not fit the %dx%d canvas", w, t, f.iw, f.ih, f.x, f.y,
                                 d.canvas_w, d.canvas_h);
            }
            out[w * clip_size + t] = f;
        }
    }
    hd->n_windows = n_windows; hd->clip_size = clip_size; hd->size = size; hd->kind = WB_KIND_POOL;
    return AF_OK;
}

namespace af {
template <typename Item, bool kBgr = false>
static int launch_window_warp(const char* what, const void* src, const void* table, int n_windows, int clip_size, int size, void* out, void* stream) {
    AF_REQUIRE(src && table && out, "%s: null argument", what);
    AF_REQUIRE(n_windows > 0 && n_windows <= AF_WINDOW_MAX_BATCH && clip_size > 0 && clip_size <= AF_ALIGN_MAX_FRAMES,
               "%s: %d windows of %d frames (at most %d of %d)", what, n_windows, clip_size, AF_WINDOW_MAX_BATCH, AF_ALIGN_MAX_FRAMES);
    AF_REQUIRE(size > 0 && size <= AF_WINDOW_MAX_SIZE && size % 4 == 0, "%s: size %d (a multiple of 4, at most %d)", what, size, AF_WINDOW_MAX_SIZE);
    AF_REQUIRE(((uintptr_t)out & 3) == 0 && ((uintptr_t)table & 7) == 0, "%s: out must be 4-byte, table 8-byte aligned", what);
    const int tiles = (size + WB_ROWS - 1) / WB_ROWS;
    const unsigned grid = (unsigned)(n_windows * clip_size * tiles);
    hipLaunchKernelGGL((warp_affine_windows_kernel<Item, kBgr>), dim3(grid), dim3(WB_THREADS), 0, (hipStream_t)stream, (const unsigned char*)src,
                       (const unsigned char*)table, (unsigned char*)out, n_windows, clip_size, size, tiles);
    AF_CHECK_LAUNCH("warp_affine_windows_kernel");
    return AF_OK;
}
}  // namespace af

extern "C" int af_warp_affine_windows_u8(const void* pool, const void* table, int n_windows, int clip_size, int size, void* out,
                                         void* stream) {
    return af::launch_window_warp<af_align_frame>("warp_affine_windows", pool, table, n_windows, clip_size, size, out, stream);
}

// ---- the same launch out of frames that are resident on the device (af_hip.h: af_frame_store / af_frame_rect) ----
extern "C" int64_t af_window_rects_table_bytes(int n_windows, int clip_size) {
    if (n_windows <= 0 || n_windows > AF_WINDOW_MAX_BATCH || clip_size <= 0 || clip_size > AF_ALIGN_MAX_FRAMES) return 0;
    return af::window_table_bytes(n_windows, clip_size, sizeof(af::WindowRect));
}

namespace af {
// what a checked rectangle becomes in the table: the one place the two rectangle forms differ on the host
static inline void window_item(WindowRect* out, const af_store_ref& st, int64_t offset, const af_frame_rect& r) {
    *out = WindowRect{offset, r.ih, r.iw, r.x, r.y, (int32_t)st.desc.row_pitch, 0};
}
static inline void window_item(WindowStoreRect* out, const af_store_ref& st, int64_t offset, const af_frame_rect& r) {
    *out = WindowStoreRect{(const unsigned char*)st.base + offset, r.ih, r.iw, r.x, r.y, (int32_t)st.desc.row_pitch, st.bgr ? 1 : 0};
}

// The planner of both rectangle forms.  WindowStoreRect: af_frame_rect.reserved names the rectangle's store in `stores`.
// WindowRect: one store, which every rectangle is of (reserved is not read) and whose base the launch is handed.
// A refusal of one (window, frame) sets *bad_window / *bad_frame, whatever its reason, and a refused table is no table.
template <typename Item>
static int plan_window_rects(const char* who, const af_window_desc* windows, const af_frame_rect* rects, int n_windows, int clip_size, int size,
                             const af_store_ref* stores, int n_stores, void* table, int64_t table_bytes, int32_t* bad_window, int32_t* bad_frame) {
    constexpr bool kListed = WbKind<Item>::value == WB_KIND_STORES;
    if (bad_window) *bad_window = -1;
    if (bad_frame) *bad_frame = -1;
    AF_REQUIRE(windows && rects && stores && table, "%s: null argument", who);
    AF_REQUIRE(n_windows > 0 && n_windows <= AF_WINDOW_MAX_BATCH && clip_size > 0 && clip_size <= AF_ALIGN_MAX_FRAMES,
               "%s: %d windows of %d frames (at most %d of %d)", who, n_windows, clip_size, AF_WINDOW_MAX_BATCH, AF_ALIGN_MAX_FRAMES);
    AF_REQUIRE(size > 0 && size <= AF_WINDOW_MAX_SIZE && size % 4 == 0, "%s: size %d (a multiple of 4, at most %d)", who, size, AF_WINDOW_MAX_SIZE);
    AF_REQUIRE(n_stores > 0 && n_stores <= AF_MAX_STORES, "%s: %d stores (1 to %d)", who, n_stores, AF_MAX_STORES);
    const int64_t need = window_table_bytes(n_windows, clip_size, sizeof(Item));
    AF_REQUIRE(table_bytes >= need, "%s: table of %lld bytes, %lld needed", who, (long long)table_bytes, (long long)need);
    for (int i = 0; i < n_stores; ++i) {
        AF_REQUIRE(!kListed || stores[i].base, "%s: store %d: null base pointer", who, i);
        const int rc = check_frame_store(who, kListed ? i : -1, stores[i].desc);
        if (rc != AF_OK) return rc;
    }
    WindowTableHeader* hd = (WindowTableHeader*)table;
    WindowXform* xf = (WindowXform*)(hd + 1);
    Item* out = (Item*)(xf + n_windows);
    hd->kind = -1;                                                  // a table that was refused half-way is no table
    for (int w = 0; w < n_windows; ++w) {
        const af_window_desc& d = windows[w];
        AF_REQUIRE(d.canvas_h > 0 && d.canvas_w > 0 && d.canvas_h <= 32767 && d.canvas_w <= 32767, "%s: window %d: bad canvas %dx%d", who, w,
                   d.canvas_w, d.canvas_h);
        invert_affine_cv(d.tfm, xf[w].m);
        for (int t = 0; t < clip_size; ++t) {
            const af_frame_rect& r = rects[w * clip_size + t];
            const int store = kListed ? r.reserved : 0;
            const bool listed = store >= 0 && store < n_stores;
            int64_t offset = 0;
            // the kernel reads the two taps of a row as 6 bytes: 3 readable bytes behind a rectangle that ends its store
            const int fault = listed ? frame_rect_fault(stores[store].desc, r, 3, &offset) : 0;
            // the reference pastes with new_image[y:y+ih, x:x+iw] = image, which numpy refuses unless the crop fits the canvas
            const bool misfit = r.x < 0 || r.y < 0 || (long long)r.x + r.iw > d.canvas_w || (long long)r.y + r.ih > d.canvas_h;
            if (!listed || fault || misfit) {
                if (bad_window) *bad_window = w;
                if (bad_frame) *bad_frame = t;
                char item[48];
                snprintf(item, sizeof item, "window %d frame %d", w, t);
                if (!listed) return set_error(AF_ERR_ARG, "%s: %s: the rectangle names store %d of %d", who, item, store, n_stores);
                if (fault) return refuse_frame_rect(who, item, kListed ? store : -1, stores[store].desc, r, fault);
                return set_error(AF_ERR_ARG, "aligner: %s (%dx%d at %d,%d) does not fit the %dx%d canvas", item, r.iw, r.ih, r.x, r.y, d.canvas_w,
                                 d.canvas_h);
            }
            window_item(&out[w * clip_size + t], stores[store], offset, r);
        }
    }
    hd->n_windows = n_windows; hd->clip_size = clip_size; hd->size = size; hd->kind = WbKind<Item>::value;
    return AF_OK;
}
}  // namespace af

extern "C" int af_window_rects_plan_u8(const af_window_desc* windows, const af_frame_rect* rects, int n_windows, int clip_size, int size,
                                       const af_frame_store* store, void* table, int64_t table_bytes, int32_t* bad_window, int32_t* bad_frame) {
    const af_store_ref one{nullptr, store ? *store : af_frame_store{}, 0, 0};      // the launch is handed the base; the items hold offsets
    return af::plan_window_rects<af::WindowRect>("window_rects_plan", windows, rects, n_windows, clip_size, size, store ? &one : nullptr, 1, table,
                                                 table_bytes, bad_window, bad_frame);
}

// ---- the same launch out of SEVERAL stores: af_frame_rect.reserved names the rectangle's store ----
extern "C" int af_window_rects_plan_stores_u8(const af_window_desc* windows, const af_frame_rect* rects, int n_windows, int clip_size, int size,
                                              const af_store_ref* stores, int n_stores, void* table, int64_t table_bytes, int32_t* bad_window,
                                              int32_t* bad_frame) {
    return af::plan_window_rects<af::WindowStoreRect>("window_rects_plan_stores", windows, rects, n_windows, clip_size, size, stores, n_stores, table,
                                                      table_bytes, bad_window, bad_frame);
}

extern "C" int af_warp_affine_window_stores_u8(const void* table, int n_windows, int clip_size, int size, void* out, void* stream) {
    // the items carry their own addresses: the launch's pool pointer is not read (the table stands in for the null check)
    return af::launch_window_warp<af::WindowStoreRect>("warp_affine_window_stores", table, table, n_windows, clip_size, size, out, stream);
}

extern "C" int af_warp_affine_window_rects_u8(const void* store, const void* table, int n_windows, int clip_size, int size, void* out,
                                              void* stream) {
    return af::launch_window_warp<af::WindowRect>("warp_affine_window_rects", store, table, n_windows, clip_size, size, out, stream);
}

extern "C" int af_warp_affine_window_rects_bgr_u8(const void* store, const void* table, int n_windows, int clip_size, int size, void* out,
                                                  void* stream) {
    return af::launch_window_warp<af::WindowRect, true>("warp_affine_window_rects_bgr", store, table, n_windows, clip_size, size, out, stream);
}

extern "C" int af_warp_affine_clip_u8(const void* crops, const af_align_frame* frames, int n_frames, int canvas_h, int canvas_w,
                                      const double* tfm, int size, void* out, void* stream) {
    using namespace af;
    AF_REQUIRE(crops && frames && tfm && out, "warp_affine_clip: null argument");
    AF_REQUIRE(n_frames >= 0 && n_frames <= AF_ALIGN_MAX_FRAMES, "warp_affine_clip: %d frames (at most %d per call)", n_frames, AF_ALIGN_MAX_FRAMES);
    AF_REQUIRE(size > 0 && size <= 4096 && canvas_h > 0 && canvas_w > 0 && canvas_h <= 32767 && canvas_w <= 32767,
               "warp_affine_clip: bad size %d / canvas %dx%d", size, canvas_h, canvas_w);
    if (n_frames == 0) return AF_OK;
    AlignArgs a;
    a.crops = (const unsigned char*)crops; a.out = (unsigned char*)out; a.size = size; a.n = n_frames;
    a.canvas_h = canvas_h; a.canvas_w = canvas_w;
    for (int i = 0; i < n_frames; ++i) {
        const af_align_frame& f = frames[i];
        // the reference pastes with new_image[y:y+ih, x:x+iw] = image, which numpy refuses unless the crop fits the canvas
        AF_REQUIRE(f.offset >= 0 && f.ih > 0 && f.iw > 0 && f.x >= 0 && f.y >= 0 && f.x + f.iw <= canvas_w && f.y + f.ih <= canvas_h,
                   "warp_affine_clip: frame %d (%dx%d at %d,%d) does not fit the %dx%d canvas", i, f.iw, f.ih, f.x, f.y, canvas_w, canvas_h);
        a.f[i] = f;
    }
    invert_affine_cv(tfm, a.m);
    const dim3 grid((unsigned)((size * size + 255) / 256), (unsigned)n_frames);
    hipLaunchKernelGGL(warp_affine_clip_kernel, grid, dim3(256), 0, (hipStream_t)stream, a);
    AF_CHECK_LAUNCH("warp_affine_clip_kernel");
    return AF_OK;
}

// Host helper of the aligner: copies n rectangles of uint8 rows into one (pinned) staging buffer - memcpy per row, no device work.
// The Python caller cut each crop to the rows / columns the warp can sample; numpy copies such a strided view with ~100 ns of
// iterator overhead per row (8 000 rows per clip: half of the aligner call).  ctypes releases the GIL for the call.
extern "C" int af_align_plan_u8(const af_align_crop* crops, int n, int canvas_h, int canvas_w, const double* tfm, int size,
                                af_stage_rect* rects, af_align_frame* frames, int64_t* total_bytes, int32_t* bad_frame) {
    using namespace af;
    AF_REQUIRE(crops && n >= 0 && tfm && size > 0 && rects && frames && total_bytes, "align_plan_u8: bad argument");
    if (bad_frame) *bad_frame = -1;
    // the rectangle of the canvas the destination square can sample: dst = M [x y 1]^T  ->  src = M^-1 (dst - t) at its four corners
    const double det = tfm[0] * tfm[4] - tfm[1] * tfm[3];
    bool cut = std::isfinite(det) && std::fabs(det) >= 1e-12;      // singular map: OpenCV's D = 0 path samples around one point; keep everything
    long long ylo = 0, yhi = 0;
    if (cut) {
        const double s = (double)(size - 1), cx[4] = {0.0, s, 0.0, s}, cy[4] = {0.0, 0.0, s, s};
        double ymin = 0.0, ymax = 0.0;
        for (int k = 0; k < 4; ++k) {
            const double dx = cx[k] - tfm[2], dy = cy[k] - tfm[5];
            const double xs = (tfm[4] * dx - tfm[1] * dy) / det, ys = (-tfm[3] * dx + tfm[0] * dy) / det;
            if (!std::isfinite(xs) || !std::isfinite(ys)) { cut = false; break; }
            if (k == 0 || ys < ymin) ymin = ys;
            if (k == 0 || ys > ymax) ymax = ys;
        }
        if (cut) { ylo = (long long)std::floor(ymin) - 3; yhi = (long long)std::ceil(ymax) + 4; }
    }
    int64_t total = 0;
    for (int i = 0; i < n; ++i) {
        const af_align_crop& c = crops[i];
        AF_REQUIRE(c.src && c.h > 0 && c.w > 0 && c.pitch >= (int64_t)c.w * 3, "align_plan_u8: bad crop %d", i);
        if (c.x < 0 || c.y < 0 || (long long)c.x + c.w > canvas_w || (long long)c.y + c.h > canvas_h) {
            if (bad_frame) *bad_frame = i;
            return set_error(AF_ERR_ARG, "aligner: frame %d (%dx%d at %d,%d) does not fit the %dx%d canvas", i, c.w, c.h, c.x, c.y, canvas_w, canvas_h);
        }
        long long r0 = 0, r1 = c.h;
        if (cut) {
            r0 = ylo - c.y > 0 ? ylo - c.y : 0;
            r1 = yhi - c.y < c.h ? yhi - c.y : c.h;
        }
        int iw = c.w;
        if (r1 <= r0) { r0 = 0; r1 = 1; iw = 1; }                   // the warp never reaches this crop: one pixel keeps the frame table valid
        rects[i].src = (const char*)c.src + r0 * c.pitch;
        rects[i].dst_offset = total;
        rects[i].src_pitch = c.pitch;
        rects[i].rows = (int32_t)(r1 - r0);
        rects[i].row_bytes = iw * 3;
        if (rects[i].rows == 1) rects[i].src_pitch = rects[i].row_bytes;
        frames[i].offset = total;
        frames[i].ih = (int32_t)(r1 - r0);
        frames[i].iw = iw;
        frames[i].x = c.x;
        frames[i].y = (int32_t)(c.y + r0);
        total += ((int64_t)(r1 - r0) * iw * 3 + 15) / 16 * 16;
    }
    *total_bytes = total;
    return AF_OK;
}

extern "C" int af_stage_rows_u8(void* dst, const af_stage_rect* rects, int n) {
    using namespace af;
    AF_REQUIRE(dst && rects && n >= 0, "stage_rows_u8: bad argument");
    for (int i = 0; i < n; ++i) {
        const af_stage_rect& r = rects[i];
        AF_REQUIRE(r.src && r.rows >= 0 && r.row_bytes >= 0 && r.src_pitch >= r.row_bytes && r.dst_offset >= 0, "stage_rows_u8: bad rectangle %d", i);
        char* d = (char*)dst + r.dst_offset;
        const char* s_ = (const char*)r.src;
        if (r.src_pitch == r.row_bytes) memcpy(d, s_, (size_t)r.rows * r.row_bytes);
        else for (int y = 0; y < r.rows; ++y) memcpy(d + (size_t)y * r.row_bytes, s_ + (size_t)y * r.src_pitch, (size_t)r.row_bytes);
    }
    return AF_OK;
}
