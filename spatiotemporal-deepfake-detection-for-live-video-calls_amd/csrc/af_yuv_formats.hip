// YUV frames of every layout a live call delivers -> packed B, G, R or R, G, B bytes, written straight into frame stores: packed 4:2:2
// (YUY2 / UYVY / YVYU, what a webcam hands over), planar and semi-planar 4:2:2 and 4:4:4 (MJPEG decoders), 10-bit 4:2:0 (P010 / I010)
// and the four 8-bit 4:2:0 layouts of af_yuv.hip, each at BT.601 or BT.709, limited or full range.  af_yuv.hip keeps the launch for
// batches of its four layouts at OpenCV's colour; any other batch goes through this one whole.
//
// Arithmetic: OpenCV's form (color_yuv.simd.hpp), the one af_yuv.hip states, with the offsets and the five coefficients taken from
// AF_YUV_COLOUR_TABLES (include/af_hip.h) by depth, range and matrix:
//     y = max(0, Y - Yoff) * CY;  u = U - Cmid;  v = V - Cmid
//     R = clamp((y + 2^19 + CVR v) >> 20)   G = clamp((y + 2^19 + CVG v + CUG u) >> 20)   B = clamp((y + 2^19 + CUB u) >> 20)
// in int32 (the largest magnitude over all tables is 5.8e8) with arithmetic shifts.  A 10-bit sample is v >> 6 (P010) or min(v, 1023)
// (I010); the output is 8-bit.  A (U, V) serves the 2 x 2, 2 x 1 or single pixel(s) it belongs to; nothing is interpolated.
// NV24 / NV42, packed 10-bit, 12-bit, BT.2020 and chroma siting are not built.
//
// Shape: af_yuv.hip's.  A lane owns a run of 8 pixels - of two rows where chroma is halved vertically, else of one; 256 runs make a
// tile, the tiles of all items form one flat list with a `first_tile` prefix per item, the table travels by value.  A tile lies in
// one item, so the layout switch is uniform over a workgroup.
//
// Alignment and stray accesses: as in af_yuv.hip.  Every row access picks the widest naturally aligned form its address shows
// (load_bytes / store_run of af_yuv_runs.h); uint16 planes have even addresses and pitches, which the planner and the launch check.
// A full run (8 j + 8 <= w) reads exactly its samples: bytes [8 j, 8 j + 8) of an 8-bit Y row, [16 j, 16 j + 16) of a 16-bit or
// packed one, and the chroma samples of pixel pairs 4 j .. 4 j + 3 (pixels 8 j .. 8 j + 7 at 4:4:4).  The last run of a row when w is
// no multiple of 8 moves its 1, 2 or 3 pixel pairs one by one with loads of exactly the pair's samples.  No load is rounded down to
// an aligned address or widened past its samples; no byte outside the h rows of 3 w destination bytes is written.
#include "af_common.h"
#include "af_yuv_runs.h"

namespace af {

constexpr int YUVX_SHIFT = 20, YUVX_HALF = 1 << 19;
constexpr int YUVX_TABLES[8][5] = AF_YUV_COLOUR_TABLES;

struct YuvExArgs {
    int32_t n, total_tiles;
    af_yuv_item_ex item[AF_YUV_MAX_FRAMES];
};
static_assert(sizeof(af_yuv_item_ex) == 56, "argument budget");
static_assert(sizeof(YuvExArgs) <= 4096, "kernel arguments");

template <int L>
struct YuvLayout {
    static constexpr bool vsub = L == AF_YUV_LAYOUT_420P || L == AF_YUV_LAYOUT_420SP || L == AF_YUV_LAYOUT_420SP16 || L == AF_YUV_LAYOUT_420P16;
    static constexpr bool wide = L == AF_YUV_LAYOUT_420SP16 || L == AF_YUV_LAYOUT_420P16;                  // uint16 samples
    static constexpr bool semi = L == AF_YUV_LAYOUT_420SP || L == AF_YUV_LAYOUT_422SP || L == AF_YUV_LAYOUT_420SP16;
    static constexpr bool packed = L == AF_YUV_LAYOUT_422PK;
    static constexpr bool each = L == AF_YUV_LAYOUT_444P;                                                  // a (U, V) per pixel
    static constexpr int bps = wide ? 2 : 1;                                                               // bytes per sample
    static constexpr int rows = vsub ? 2 : 1;
    static constexpr int nc = each ? 8 : 4;                                                                // (U, V)s of a full run
};

// what the host knows of a layout
struct YuvShape {
    bool vsub, wide, semi, packed, each;
};
static inline YuvShape yuv_shape(int layout) {
    switch (layout) {
#define AF_YUV_SHAPE(L) \
    case L: return YuvShape{YuvLayout<L>::vsub, YuvLayout<L>::wide, YuvLayout<L>::semi, YuvLayout<L>::packed, YuvLayout<L>::each};
        AF_YUV_SHAPE(AF_YUV_LAYOUT_420P) AF_YUV_SHAPE(AF_YUV_LAYOUT_420SP) AF_YUV_SHAPE(AF_YUV_LAYOUT_422P) AF_YUV_SHAPE(AF_YUV_LAYOUT_422SP)
        AF_YUV_SHAPE(AF_YUV_LAYOUT_444P) AF_YUV_SHAPE(AF_YUV_LAYOUT_422PK) AF_YUV_SHAPE(AF_YUV_LAYOUT_420SP16) AF_YUV_SHAPE(AF_YUV_LAYOUT_420P16)
#undef AF_YUV_SHAPE
    }
    return YuvShape{false, false, false, false, false};
}
static inline int yuv_y_row_bytes(const YuvShape& s, int w) { return s.packed ? 2 * w : (s.wide ? 2 * w : w); }
static inline int yuv_c_row_bytes(const YuvShape& s, int w) { return s.packed ? 0 : ((s.semi || s.each) ? w : w / 2) * (s.wide ? 2 : 1); }

static inline int64_t yuv_tiles_ex(int layout, int h, int w) {
    const int64_t runs = (int64_t)(yuv_shape(layout).vsub ? h / 2 : h) * ((w + YUV_RUN - 1) / YUV_RUN);
    return (runs + YUV_TILE - 1) / YUV_TILE;
}

struct YuvColour {
    int cy, cvr, cvg, cug, cub, yoff, cmid;
};
struct ChromaEx {
    int r, g, b;
};
__device__ __forceinline__ ChromaEx chroma_terms_ex(const YuvColour& k, int U, int V) {
    const int u = U - k.cmid, v = V - k.cmid;
    return ChromaEx{YUVX_HALF + k.cvr * v, YUVX_HALF + k.cvg * v + k.cug * u, YUVX_HALF + k.cub * u};
}
// one pixel's three bytes in the destination's order, as the low 24 bits
__device__ __forceinline__ unsigned pixel_bytes_ex(const YuvColour& k, int Y, const ChromaEx& c, int bgr) {
    const int y = max(0, Y - k.yoff) * k.cy;
    const unsigned R = clamp_u8((y + c.r) >> YUVX_SHIFT), G = clamp_u8((y + c.g) >> YUVX_SHIFT), B = clamp_u8((y + c.b) >> YUVX_SHIFT);
    return bgr ? (B | (G << 8) | (R << 16)) : (R | (G << 8) | (B << 16));
}

// the value of a sample as it lies in memory: 8-bit as it is, P010 in bits 15..6, I010 in the low bits
template <int L>
__device__ __forceinline__ int sample_value(unsigned raw) {
    if constexpr (L == AF_YUV_LAYOUT_420SP16) return (int)(raw >> 6);
    else if constexpr (L == AF_YUV_LAYOUT_420P16) return (int)min(raw, 1023u);
    else return (int)raw;
}
// sample i of little-endian dwords d
template <int L>
__device__ __forceinline__ int sample_of(const unsigned* d, int i) {
    if constexpr (YuvLayout<L>::wide) return sample_value<L>((d[i >> 1] >> (16 * (i & 1))) & 0xffffu);
    else return (int)((d[i >> 2] >> (8 * (i & 3))) & 255u);
}
// sample i behind p, by a load of exactly its bytes (a uint16 plane is even, so its halfword load is aligned)
template <int L>
__device__ __forceinline__ int sample_at(const unsigned char* p, int i) {
    if constexpr (YuvLayout<L>::wide) return sample_value<L>(((const unsigned short*)p)[i]);
    else return (int)p[i];
}
// the four bytes of a packed pixel pair -> Y0, Y1, U, V
__device__ __forceinline__ void unpack_pair(unsigned d, int order, int& y0, int& y1, int& u, int& v) {
    const int b0 = (int)(d & 255u), b1 = (int)((d >> 8) & 255u), b2 = (int)((d >> 16) & 255u), b3 = (int)(d >> 24);
    if (order == 1) { y0 = b1; y1 = b3; u = b0; v = b2; }           // U Y0 V Y1
    else { y0 = b0; y1 = b2; u = order == 2 ? b3 : b1; v = order == 2 ? b1 : b3; }     // Y0 U Y1 V, Y0 V Y1 U
}

// eight pixels' low-24-bit byte triples -> 24 bytes as six dwords
__device__ __forceinline__ void pack_run(const unsigned (&px)[8], unsigned (&out)[6]) {
#pragma unroll
    for (int q = 0; q < 2; ++q) {                                 // four pixels are three dwords
        out[3 * q + 0] = px[4 * q] | (px[4 * q + 1] << 24);
        out[3 * q + 1] = (px[4 * q + 1] >> 8) | (px[4 * q + 2] << 16);
        out[3 * q + 2] = (px[4 * q + 2] >> 16) | (px[4 * q + 3] << 8);
    }
}

template <int L>
__device__ __forceinline__ void convert_run_of(const af_yuv_item_ex& it, int run) {
    using T = YuvLayout<L>;
    const int w = it.w, h = it.h;
    const int runs_x = (w + YUV_RUN - 1) / YUV_RUN;
    if (run >= (T::vsub ? h / 2 : h) * runs_x) return;
    const int rg = run / runs_x, j = run - rg * runs_x;          // the row (or row pair) and the run in it
    const int x0 = j * YUV_RUN, row0 = T::vsub ? 2 * rg : rg;
    const int bgr = it.bgr, order = it.order;
    const int* tab = YUVX_TABLES[(T::wide ? 4 : 0) + (it.colour & 3)];
    const bool full = (it.colour & 2) != 0;
    const YuvColour k{tab[0], tab[1], tab[2], tab[3], tab[4], full ? 0 : (T::wide ? 64 : 16), T::wide ? 512 : 128};

    // row r of the run: its Y (or packed) samples at ys + r * y_pitch, its destination at ds + r * dst_pitch
    const unsigned char* ys = (const unsigned char*)it.y + (long long)row0 * it.y_pitch + (long long)x0 * (T::packed ? 2 : T::bps);
    unsigned char* ds = (unsigned char*)it.dst + (long long)row0 * it.dst_pitch + (long long)x0 * 3;
    // the chroma row is rg in every layout: row pair rg where chroma is halved vertically, else row rg itself
    const unsigned char* c0 = nullptr;
    const unsigned char* c1 = nullptr;
    if constexpr (!T::packed) {
        const long long at = (long long)rg * it.c_pitch + (long long)((T::semi || T::each) ? x0 : x0 / 2) * T::bps;
        c0 = (const unsigned char*)it.c0 + at;
        if constexpr (!T::semi) c1 = (const unsigned char*)it.c1 + at;
    }

    if (x0 + YUV_RUN <= w) {
        // A full run: x0 + 8 <= w, so every load below lies inside its plane's row (see the head of this file).
        int Y[T::rows][8];
        ChromaEx c[T::nc];
        if constexpr (T::packed) {
            unsigned d[4];
            load_bytes<16>(ys, d);
#pragma unroll
            for (int p = 0; p < 4; ++p) {
                int u, v;
                unpack_pair(d[p], order, Y[0][2 * p], Y[0][2 * p + 1], u, v);
                c[p] = chroma_terms_ex(k, u, v);
            }
        } else {
#pragma unroll
            for (int r = 0; r < T::rows; ++r) {
                unsigned d[2 * T::bps];
                load_bytes<8 * T::bps>(ys + (long long)r * it.y_pitch, d);
#pragma unroll
                for (int i = 0; i < 8; ++i) Y[r][i] = sample_of<L>(d, i);
            }
            if constexpr (T::semi) {
                unsigned d[2 * T::bps];                           // four (first, second) pairs
                load_bytes<8 * T::bps>(c0, d);
#pragma unroll
                for (int p = 0; p < 4; ++p) {
                    const int first = sample_of<L>(d, 2 * p), second = sample_of<L>(d, 2 * p + 1);
                    c[p] = order ? chroma_terms_ex(k, second, first) : chroma_terms_ex(k, first, second);
                }
            } else {
                unsigned da[T::nc * T::bps / 4], db[T::nc * T::bps / 4];
                load_bytes<T::nc * T::bps>(c0, da);
                load_bytes<T::nc * T::bps>(c1, db);
#pragma unroll
                for (int p = 0; p < T::nc; ++p) {
                    const int first = sample_of<L>(da, p), second = sample_of<L>(db, p);
                    c[p] = order ? chroma_terms_ex(k, second, first) : chroma_terms_ex(k, first, second);
                }
            }
        }
#pragma unroll
        for (int r = 0; r < T::rows; ++r) {
            unsigned px[8], out[6];
#pragma unroll
            for (int i = 0; i < 8; ++i) px[i] = pixel_bytes_ex(k, Y[r][i], c[T::each ? i : i >> 1], bgr);
            pack_run(px, out);
            store_run(ds + (long long)r * it.dst_pitch, out);
        }
    } else {
        // The tail of a row: (w - x0) / 2 = 1, 2 or 3 pixel pairs, each with loads of its own samples only.
        const int pairs = (w - x0) / 2;
        for (int p = 0; p < pairs; ++p) {
            if constexpr (T::packed) {
                const unsigned d = (unsigned)ys[4 * p] | ((unsigned)ys[4 * p + 1] << 8) | ((unsigned)ys[4 * p + 2] << 16) | ((unsigned)ys[4 * p + 3] << 24);
                int y0, y1, u, v;
                unpack_pair(d, order, y0, y1, u, v);
                const ChromaEx cc = chroma_terms_ex(k, u, v);
                store_pair(ds + 6 * p, pixel_bytes_ex(k, y0, cc, bgr), pixel_bytes_ex(k, y1, cc, bgr));
            } else {
                ChromaEx ca, cb;                                  // of the pair's first and second pixel
                if constexpr (T::each) {
                    const int f0 = sample_at<L>(c0, 2 * p), s0 = sample_at<L>(c1, 2 * p), f1 = sample_at<L>(c0, 2 * p + 1), s1 = sample_at<L>(c1, 2 * p + 1);
                    ca = order ? chroma_terms_ex(k, s0, f0) : chroma_terms_ex(k, f0, s0);
                    cb = order ? chroma_terms_ex(k, s1, f1) : chroma_terms_ex(k, f1, s1);
                } else {
                    const int first = T::semi ? sample_at<L>(c0, 2 * p) : sample_at<L>(c0, p);
                    const int second = T::semi ? sample_at<L>(c0, 2 * p + 1) : sample_at<L>(c1, p);
                    ca = cb = order ? chroma_terms_ex(k, second, first) : chroma_terms_ex(k, first, second);
                }
#pragma unroll
                for (int r = 0; r < T::rows; ++r) {
                    const unsigned char* yr = ys + (long long)r * it.y_pitch;
                    store_pair(ds + (long long)r * it.dst_pitch + 6 * p, pixel_bytes_ex(k, sample_at<L>(yr, 2 * p), ca, bgr),
                               pixel_bytes_ex(k, sample_at<L>(yr, 2 * p + 1), cb, bgr));
                }
            }
        }
    }
}

__global__ __launch_bounds__(YUV_TILE) void yuv_to_rgb_ex_kernel(const YuvExArgs a) {
    const int tile = blockIdx.x;
    if (tile >= a.total_tiles) return;
    int k = 0;
    while (k + 1 < a.n && a.item[k + 1].first_tile <= tile) ++k;  // tens of items: a scan
    const af_yuv_item_ex it = a.item[k];
    const int run = (tile - it.first_tile) * YUV_TILE + (int)threadIdx.x;      // at most 32767 * 4096 runs per item
    switch (it.layout) {                                          // uniform over the workgroup: a tile lies in one item
        case AF_YUV_LAYOUT_420P: convert_run_of<AF_YUV_LAYOUT_420P>(it, run); break;
        case AF_YUV_LAYOUT_420SP: convert_run_of<AF_YUV_LAYOUT_420SP>(it, run); break;
        case AF_YUV_LAYOUT_422P: convert_run_of<AF_YUV_LAYOUT_422P>(it, run); break;
        case AF_YUV_LAYOUT_422SP: convert_run_of<AF_YUV_LAYOUT_422SP>(it, run); break;
        case AF_YUV_LAYOUT_444P: convert_run_of<AF_YUV_LAYOUT_444P>(it, run); break;
        case AF_YUV_LAYOUT_422PK: convert_run_of<AF_YUV_LAYOUT_422PK>(it, run); break;
        case AF_YUV_LAYOUT_420SP16: convert_run_of<AF_YUV_LAYOUT_420SP16>(it, run); break;
        case AF_YUV_LAYOUT_420P16: convert_run_of<AF_YUV_LAYOUT_420P16>(it, run); break;
        default: break;                                           // the launch refuses other codes on the host
    }
}

// the checks the planner and the launch share: codes, size, planes, pitches
static int yuv_check_ex(const char* who, const char* what, int i, int layout, int order, int colour, int h, int w, const void* y, const void* c0,
                        const void* c1, int64_t y_pitch, int64_t c_pitch) {
    AF_REQUIRE(layout >= 0 && layout < AF_YUV_LAYOUTS, "%s: %s %d: layout %d is not one of the %d AF_YUV_LAYOUT_ codes", who, what, i, layout, AF_YUV_LAYOUTS);
    const YuvShape s = yuv_shape(layout);
    AF_REQUIRE(order >= 0 && order <= (s.packed ? 2 : 1), "%s: %s %d: component order %d of layout %d", who, what, i, order, layout);
    AF_REQUIRE(colour >= 0 && colour <= 3, "%s: %s %d: colour %d (2 * full_range + matrix, each 0 or 1)", who, what, i, colour);
    AF_REQUIRE(h > 0 && w > 0 && w % 2 == 0 && (!s.vsub || h % 2 == 0) && h <= 32767 && w <= 32766,
               "%s: %s %d: a frame of layout %d is positive, even in width%s (at most 32766 x 32767), not %dx%d", who, what, i, layout,
               s.vsub ? " and even in height" : "", w, h);
    AF_REQUIRE(y && (s.packed || c0) && (s.packed || s.semi || c1), "%s: %s %d: null plane", who, what, i);
    const int yrow = yuv_y_row_bytes(s, w), crow = yuv_c_row_bytes(s, w);
    AF_REQUIRE(y_pitch >= yrow && y_pitch <= 0x7fffffff, "%s: %s %d: Y pitch %lld is shorter than a row of %d bytes", who, what, i, (long long)y_pitch, yrow);
    AF_REQUIRE(s.packed || (c_pitch >= crow && c_pitch <= 0x7fffffff), "%s: %s %d: chroma pitch %lld is shorter than a row of %d bytes", who, what, i,
               (long long)c_pitch, crow);
    AF_REQUIRE(!s.wide || (((uintptr_t)y | (uintptr_t)c0 | (uintptr_t)c1 | (uintptr_t)y_pitch | (uintptr_t)c_pitch) & 1) == 0,
               "%s: %s %d: the planes and pitches of a 16-bit layout are even", who, what, i);
    return AF_OK;
}

}  // namespace af

extern "C" int af_yuv_plan_ex_u8(const af_yuv_frame_ex* frames, int n, const af_store_ref* stores, int n_stores, af_yuv_item_ex* items) {
    using namespace af;
    AF_REQUIRE(frames && stores && items, "yuv_plan_ex: null argument");
    AF_REQUIRE(n >= 0 && n <= AF_YUV_MAX_FRAMES, "yuv_plan_ex: %d frames (at most %d per launch)", n, AF_YUV_MAX_FRAMES);
    AF_REQUIRE(n_stores > 0 && n_stores <= AF_MAX_STORES, "yuv_plan_ex: %d stores (1 to %d per launch)", n_stores, AF_MAX_STORES);
    int64_t tiles = 0;
    for (int i = 0; i < n; ++i) {
        const af_yuv_frame_ex& f = frames[i];
        AF_REQUIRE((f.matrix == 0 || f.matrix == 1) && (f.full_range == 0 || f.full_range == 1), "yuv_plan_ex: frame %d: matrix %d, full_range %d (each 0 or 1)",
                   i, f.matrix, f.full_range);
        int rc = yuv_check_ex("yuv_plan_ex", "frame", i, f.layout, f.order, 2 * f.full_range + f.matrix, f.h, f.w, f.y, f.u, f.v, f.y_pitch, f.c_pitch);
        if (rc != AF_OK) return rc;
        const YuvShape sh = yuv_shape(f.layout);
        const af_store_ref* ref;
        unsigned char* dst;
        // one slot is written, so the store need not hold all its frames (whole = false): the slot's own bytes are checked below
        rc = store_frame("yuv_plan_ex", "frame", i, stores, n_stores, f.store, f.slot, true, false, &ref, &dst);
        if (rc != AF_OK) return rc;
        const af_store_ref& st = *ref;
        const af_frame_store& s = st.desc;
        AF_REQUIRE(s.height == f.h && s.width == f.w, "yuv_plan_ex: frame %d of %dx%d does not fit store %d of %d frames of %dx%d", i, f.w, f.h, f.store,
                   s.n_frames, s.width, s.height);
        AF_REQUIRE((int64_t)f.slot * s.frame_stride + frame_span(s) <= s.store_bytes, "yuv_plan_ex: frame %d: slot %d leaves store %d of %d frames, %lld bytes", i,
                   f.slot, f.store, s.n_frames, (long long)s.store_bytes);
        af_yuv_item_ex& it = items[i];
        it.y = f.y; it.c0 = sh.packed ? nullptr : f.u; it.c1 = (sh.packed || sh.semi) ? nullptr : f.v;
        it.dst = dst;
        it.y_pitch = (int32_t)f.y_pitch; it.c_pitch = sh.packed ? 0 : (int32_t)f.c_pitch; it.dst_pitch = (int32_t)s.row_pitch;
        it.first_tile = (int32_t)tiles;
        it.h = (uint16_t)f.h; it.w = (uint16_t)f.w;
        it.layout = (uint8_t)f.layout; it.order = (uint8_t)f.order; it.bgr = st.bgr ? 1 : 0; it.colour = (uint8_t)(2 * f.full_range + f.matrix);
        tiles += yuv_tiles_ex(f.layout, f.h, f.w);
        AF_REQUIRE(tiles <= 0x7fffffff, "yuv_plan_ex: too many pixels");
    }
    return AF_OK;
}

extern "C" int af_yuv_to_rgb_ex_u8(const af_yuv_item_ex* items, int n, void* stream) {
    using namespace af;
    AF_REQUIRE(items, "yuv_to_rgb_ex: null argument");
    AF_REQUIRE(n >= 0 && n <= AF_YUV_MAX_FRAMES, "yuv_to_rgb_ex: %d frames (at most %d per launch)", n, AF_YUV_MAX_FRAMES);
    if (n == 0) return AF_OK;
    YuvExArgs a;
    a.n = n;
    int64_t tiles = 0;
    for (int i = 0; i < n; ++i) {
        const af_yuv_item_ex& it = items[i];
        const int rc = yuv_check_ex("yuv_to_rgb_ex", "item", i, it.layout, it.order, it.colour, it.h, it.w, it.y, it.c0, it.c1, it.y_pitch, it.c_pitch);
        if (rc != AF_OK) return rc;
        AF_REQUIRE(it.dst, "yuv_to_rgb_ex: item %d: null destination", i);
        AF_REQUIRE(it.dst_pitch >= 3 * (int)it.w, "yuv_to_rgb_ex: item %d: destination pitch %d is shorter than a row of %d bytes", i, it.dst_pitch, 3 * (int)it.w);
        AF_REQUIRE(it.first_tile == tiles, "yuv_to_rgb_ex: item %d: first_tile %d, %lld by the sizes before it (hand in a table af_yuv_plan_ex_u8 filled)", i,
                   it.first_tile, (long long)tiles);
        a.item[i] = it;
        tiles += yuv_tiles_ex(it.layout, it.h, it.w);
        AF_REQUIRE(tiles <= 0x7fffffff, "yuv_to_rgb_ex: too many pixels");
    }
    a.total_tiles = (int32_t)tiles;
    hipLaunchKernelGGL(yuv_to_rgb_ex_kernel, dim3((unsigned)tiles), dim3(YUV_TILE), 0, (hipStream_t)stream, a);
    AF_CHECK_LAUNCH("yuv_to_rgb_ex_kernel");
    return AF_OK;
}
