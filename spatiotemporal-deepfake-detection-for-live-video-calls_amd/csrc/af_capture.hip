// Captured bitmaps into frame stores: what the reference's capture code does on the host before RealtimeAF.step sees a frame
// (test/win_capture.py:37, :110-115; test/capture_tile.py:190, :199-201) -
//     frame = cv2.cvtColor(bitmap, cv2.COLOR_BGRA2BGR)                                  the alpha byte is dropped
//     frame = frame[y0:y1, x0:x1]                                                        the window's client rectangle
//     frame = cv2.resize(frame, (max_w, new_h), interpolation=cv2.INTER_AREA)            down to max_w columns
// - in one launch for up to AF_CAPTURE_MAX_FRAMES frames, which may differ in size, format (B, G, R[, x] or R, G, B[, x]), mode,
// destination store and the store's byte order.  The rectangle is a pointer and a pitch, the alpha byte is never read into a
// result, and the reorder is a choice of which byte of a result goes where.
//
// Arithmetic: OpenCV 4.x resize.cpp for 8-bit images, per channel, applied after the alpha drop, restated (like the warp, the quality
// gate, the YUV conversion and the bilinear resize it cannot be pinned against cv2 itself where this is built, only against
// tests/capture_ref.py, its hand-worked anchors and its tie to tests/quality_ref.py's half_size):
//     COPY    dw == w and dh == h                      the three bytes
//     AREA2   w == 2 dw and h == 2 dh                  (a + b + c + d + 2) >> 2 over each 2 x 2 block (ResizeAreaFastVec)
//     BOX     w % dw == 0 and h % dh == 0, not those   kx = w / dw, ky = h / dh (either may be 1): the integer sum of the kx x ky box,
//                                                      converted to fp32, times fp32(1) / fp32(kx ky), rounded half to even, saturated
//                                                      (ResizeAreaFast_Invoker)
//     TABLE   everything else                          computeResizeAreaTab on BOTH axes, also when one of them is a whole ratio
//                                                      (ResizeArea_Invoker) - which does not give the BOX bytes:
//         scale = src / dst in fp64; destination cell d covers [d scale, d scale + scale); sx1 = ceil, sx2 = min(floor, src - 1),
//         sx1 = min(sx1, sx2); cell = min(scale, src - d scale); taps in this order: (sx1 - 1, (sx1 - fsx1) / cell) if sx1 - fsx1 >
//         1e-3; (sx, 1 / cell) for sx1 <= sx < sx2; (sx2, min(min(fsx2 - sx2, 1), cell) / cell) if fsx2 - sx2 > 1e-3; weights cast
//         to fp32.  The planner computes the tables on the host.
//         Per destination row the kernel visits its source rows in table order; for each it computes buf = buf + s * alpha over the x
//         taps in table order (an fp32 multiply, then an fp32 add, buf starting at 0); the first source row gives out = beta * buf,
//         later ones out = out + beta * buf; at the end out is rounded half to even and saturated.
// No contraction anywhere on that path: one fused multiply-add breaks byte equality with the statement (a sum that lands on .5
// exactly rounds the other way).  hipcc contracts by default, and its __fmul_rn / __fadd_rn are plain x * y and x + y that fuse
// with their neighbours once inlined, so every product and sum here is cp_mul / cp_add, written below a file-scope
// `#pragma clang fp contract(off)`; the build's ISA holds no fused multiply-add for this kernel.
//
// Shape: a memory stream; the runs, tiles and fixed grid of af_frame_runs.h, which also holds the argument for the writes.  A
// 4-channel pixel is one dword load when the rectangle's address and pitch are 4-byte aligned (four of them one 16-byte load where
// the address allows), byte loads otherwise.
//
// No stray access, reads: a pixel (row, col) with 0 <= row < h, 0 <= col < w is read as the 3 bytes row * pitch + col * channels +
// {0, 1, 2}, or - 4 channels, aligned - as the dword of its 4 bytes; nothing is rounded down or widened past a pixel, so reads stay
// inside [src, src + pitch * (h - 1) + w * channels).  COPY: row dy < h, columns x0 + i < dw = w.  AREA2: rows 2 dy + 1 < h, columns
// 2 (x0 + i) + 1 < w.  BOX: rows ky dy + j < h, columns kx (x0 + i) + k < w.  TABLE: the planner refuses a tap outside [0, size).
#include <cmath>

#include "af_frame_runs.h"

namespace af {

static_assert(sizeof(af_capture_header) % 8 == 0 && sizeof(af_capture_item) == 72 && sizeof(af_capture_tap) == 8 && sizeof(af_capture_frame) == 48,
              "table layout");

static inline int64_t pad8(int64_t v) { return (v + 7) & ~(int64_t)7; }

#pragma clang fp contract(off)                      // from here to the end of the file: a product and a sum stay two roundings
__device__ __forceinline__ float cp_mul(float a, float b) { return a * b; }
__device__ __forceinline__ float cp_add(float a, float b) { return a + b; }

// one pixel as B0 | B1 << 8 | B2 << 16 (memory order); reads its 3 bytes, or the dword of its 4
__device__ __forceinline__ unsigned cp_px(const unsigned char* row, int col, int ch, bool dword) {
    const unsigned char* p = row + col * ch;
    if (dword) return *(const unsigned*)p & 0xffffffu;
    return (unsigned)p[0] | ((unsigned)p[1] << 8) | ((unsigned)p[2] << 16);
}
// pixels col .. col + 3 of a row, all inside it
__device__ __forceinline__ void cp_px4(const unsigned char* row, int col, int ch, bool dword, unsigned* px) {
    const unsigned char* p = row + col * ch;
    if (dword && ((unsigned)(uintptr_t)p & 15) == 0) {
        const uint4 v = *(const uint4*)p;
        px[0] = v.x & 0xffffffu; px[1] = v.y & 0xffffffu; px[2] = v.z & 0xffffffu; px[3] = v.w & 0xffffffu;
    } else {
#pragma unroll
        for (int i = 0; i < 4; ++i) px[i] = cp_px(row, col + i, ch, dword);
    }
}
__device__ __forceinline__ unsigned cp_ch(unsigned px, int c) { return (px >> (8 * c)) & 255u; }
__device__ __forceinline__ unsigned cp_area2(unsigned a, unsigned b, unsigned c, unsigned d) {
    unsigned out = 0;
#pragma unroll
    for (int k = 0; k < 3; ++k) out |= area2(cp_ch(a, k), cp_ch(b, k), cp_ch(c, k), cp_ch(d, k)) << (8 * k);
    return out;
}
// cvRound and saturate_cast<uchar>: half to even, then clamped
__device__ __forceinline__ unsigned cp_round(float v) { return (unsigned)min(max(__float2int_rn(v), 0), 255); }

// TABLE mode of one run whose destination columns have at most K taps each: the x taps of the 4 pixels are read once, every source
// row then issues its 4 K pixel loads together.  A slot past a pixel's taps repeats the run's first tap (a valid column) with weight
// 0: buf + s * 0 = buf exactly (nothing here is negative), so the sums are those of the loop over the real taps, in their order.
template <int K>
__device__ __forceinline__ void cp_table_run(const unsigned char* src, int pitch, int ch, bool dword, const af_capture_tap* xtaps, const int (&xb)[5],
                                             const af_capture_tap* ytaps, int yb, int ye, float (&acc)[12]) {
    int idx[4][K];
    float wgt[4][K];
#pragma unroll
    for (int i = 0; i < 4; ++i)
#pragma unroll
        for (int k = 0; k < K; ++k) {
            const bool on = xb[i] + k < xb[i + 1];
            const af_capture_tap xt = xtaps[on ? xb[i] + k : xb[0]];               // xb[0] < xb[1]: the run has a first pixel
            idx[i][k] = xt.idx;
            wgt[i][k] = on ? xt.weight : 0.f;
        }
    for (int e = yb; e < ye; ++e) {
        const af_capture_tap yt = ytaps[e];                          // 0 <= idx < h by the planner
        const unsigned char* row = src + (long long)yt.idx * pitch;
        unsigned p[4][K];
#pragma unroll
        for (int i = 0; i < 4; ++i)
#pragma unroll
            for (int k = 0; k < K; ++k) p[i][k] = cp_px(row, idx[i][k], ch, dword);  // 0 <= idx < w by the planner
#pragma unroll
        for (int i = 0; i < 4; ++i)
#pragma unroll
            for (int c = 0; c < 3; ++c) {
                float buf = 0.f;
#pragma unroll
                for (int k = 0; k < K; ++k) buf = cp_add(buf, cp_mul((float)cp_ch(p[i][k], c), wgt[i][k]));
                acc[3 * i + c] = e == yb ? cp_mul(yt.weight, buf) : cp_add(acc[3 * i + c], cp_mul(yt.weight, buf));
            }
    }
}

__global__ __launch_bounds__(RUN_TILE) void capture_frames_kernel(const unsigned char* __restrict__ table, int n) {
    for (int tile = blockIdx.x, total = launch_tiles<AF_CAPTURE_KIND, af_capture_header>(table, n); tile < total; tile += gridDim.x) {
        const TileRun<af_capture_item> r = tile_run<af_capture_header, af_capture_item>(table, n, tile);
        if (!r.npx) continue;
        const af_capture_item& it = r.it;
        const int dy = r.dy, x0 = r.x0, npx = r.npx;
        const unsigned char* src = (const unsigned char*)it.src;
        const int ch = it.channels;
        const bool dword = it.dword != 0;
        unsigned px[4] = {0, 0, 0, 0}, out[3];
        if (it.mode == AF_CAPTURE_COPY) {
            const unsigned char* row = src + (long long)dy * it.src_pitch;
            if (npx == RUN_PX) {
                cp_px4(row, x0, ch, dword, px);                      // x0 + 4 <= dw = w
            } else {
                for (int i = 0; i < npx; ++i) px[i] = cp_px(row, x0 + i, ch, dword);
            }
        } else if (it.mode == AF_CAPTURE_AREA2) {
            const unsigned char* r0 = src + (long long)(2 * dy) * it.src_pitch;      // rows 2 dy, 2 dy + 1 < h = 2 dh
            const unsigned char* r1 = r0 + it.src_pitch;
            if (npx == RUN_PX) {
                unsigned a[8], b[8];                                 // source pixels 2 x0 .. 2 x0 + 7 <= 2 dw - 1 = w - 1
                cp_px4(r0, 2 * x0, ch, dword, a); cp_px4(r0, 2 * x0 + 4, ch, dword, a + 4);
                cp_px4(r1, 2 * x0, ch, dword, b); cp_px4(r1, 2 * x0 + 4, ch, dword, b + 4);
#pragma unroll
                for (int i = 0; i < 4; ++i) px[i] = cp_area2(a[2 * i], a[2 * i + 1], b[2 * i], b[2 * i + 1]);
            } else {
                for (int i = 0; i < npx; ++i) {
                    const int c0 = 2 * (x0 + i);
                    px[i] = cp_area2(cp_px(r0, c0, ch, dword), cp_px(r0, c0 + 1, ch, dword), cp_px(r1, c0, ch, dword), cp_px(r1, c0 + 1, ch, dword));
                }
            }
        } else if (it.mode == AF_CAPTURE_BOX) {
            for (int i = 0; i < npx; ++i) {
                unsigned long long sum[3] = {0, 0, 0};
                const int c0 = (x0 + i) * it.kx;                     // columns c0 .. c0 + kx - 1 <= dw kx - 1 = w - 1
                for (int jy = 0; jy < it.ky; ++jy) {                 // rows ky dy .. ky dy + ky - 1 <= h - 1
                    const unsigned char* row = src + (long long)(dy * it.ky + jy) * it.src_pitch;
                    unsigned rs[3] = {0, 0, 0};                      // at most 8192 * 255
                    for (int jx = 0; jx < it.kx; ++jx) {
                        const unsigned p = cp_px(row, c0 + jx, ch, dword);
                        rs[0] += cp_ch(p, 0); rs[1] += cp_ch(p, 1); rs[2] += cp_ch(p, 2);
                    }
                    sum[0] += rs[0]; sum[1] += rs[1]; sum[2] += rs[2];
                }
#pragma unroll
                for (int c = 0; c < 3; ++c) px[i] |= cp_round(cp_mul((float)sum[c], it.inv_area)) << (8 * c);
            }
        } else {
            const int* xfirst = (const int*)(table + it.xtab);
            const af_capture_tap* xtaps = (const af_capture_tap*)(table + it.xtab + (((it.dw + 1) * 4 + 7) & ~7));
            const int* yfirst = (const int*)(table + it.ytab);
            const af_capture_tap* ytaps = (const af_capture_tap*)(table + it.ytab + (((it.dh + 1) * 4 + 7) & ~7));
            int xb[5];
#pragma unroll
            for (int i = 0; i < 5; ++i) xb[i] = xfirst[x0 + min(i, npx)];           // x0 + npx <= dw: first[] has dw + 1 entries
            float acc[12];
#pragma unroll
            for (int q = 0; q < 12; ++q) acc[q] = 0.f;
            const int yb = yfirst[dy], ye = yfirst[dy + 1];
            if (it.xk <= 4) cp_table_run<4>(src, it.src_pitch, ch, dword, xtaps, xb, ytaps, yb, ye, acc);
            else for (int e = yb; e < ye; ++e) {                     // (an 8-tap form too took the kernel from 136 to 234 VGPRs)
                const af_capture_tap yt = ytaps[e];                  // 0 <= idx < h by the planner
                const unsigned char* row = src + (long long)yt.idx * it.src_pitch;
                float buf[12];
#pragma unroll
                for (int q = 0; q < 12; ++q) buf[q] = 0.f;
#pragma unroll
                for (int i = 0; i < 4; ++i) {
                    for (int t = xb[i]; t < xb[i + 1]; ++t) {        // empty for i >= npx
                        const af_capture_tap xt = xtaps[t];          // 0 <= idx < w by the planner
                        const unsigned p = cp_px(row, xt.idx, ch, dword);
#pragma unroll
                        for (int c = 0; c < 3; ++c) buf[3 * i + c] = cp_add(buf[3 * i + c], cp_mul((float)cp_ch(p, c), xt.weight));
                    }
                }
                if (e == yb) {
#pragma unroll
                    for (int q = 0; q < 12; ++q) acc[q] = cp_mul(yt.weight, buf[q]);
                } else {
#pragma unroll
                    for (int q = 0; q < 12; ++q) acc[q] = cp_add(acc[q], cp_mul(yt.weight, buf[q]));
                }
            }
#pragma unroll
            for (int i = 0; i < 4; ++i)
#pragma unroll
                for (int c = 0; c < 3; ++c) px[i] |= cp_round(acc[3 * i + c]) << (8 * c);
        }

        if (it.swap) {                                               // the store's byte order is the other one
#pragma unroll
            for (int i = 0; i < 4; ++i) px[i] = (px[i] & 0xff00u) | (px[i] >> 16) | ((px[i] & 0xffu) << 16);
        }
        pack_run(px, out);
        store_run12(run_dst(r), out, npx);
    }
}

static inline int capture_mode(int h, int w, int dh, int dw) {
    if (dw == w && dh == h) return AF_CAPTURE_COPY;
    if (w == 2 * dw && h == 2 * dh) return AF_CAPTURE_AREA2;
    if (w % dw == 0 && h % dh == 0) return AF_CAPTURE_BOX;
    return AF_CAPTURE_TABLE;
}

// computeResizeAreaTab of one axis, src -> dst pixels (dst <= src): first[d] .. first[d + 1] are destination d's taps
struct AreaTable {
    int src, dst;
    int32_t offset;
    std::vector<int32_t> first;
    std::vector<af_capture_tap> taps;
    int most_taps() const {
        int most = 0;
        for (size_t d = 0; d + 1 < first.size(); ++d) most = first[d + 1] - first[d] > most ? first[d + 1] - first[d] : most;
        return most;
    }
    int64_t prepare() {                                              // fills first and taps; the bytes they take in the table
#pragma clang fp contract(off)
        const double scale = (double)src / (double)dst;
        for (int dx = 0; dx < dst; ++dx) {
            first.push_back((int32_t)taps.size());
            const double fsx1 = dx * scale;
            const double fsx2 = fsx1 + scale;
            const double cell = std::fmin(scale, src - fsx1);
            int sx1 = (int)std::ceil(fsx1), sx2 = (int)std::floor(fsx2);
            sx2 = sx2 < src - 1 ? sx2 : src - 1;
            sx1 = sx1 < sx2 ? sx1 : sx2;
            if (sx1 - fsx1 > 1e-3) taps.push_back(af_capture_tap{sx1 - 1, (float)((sx1 - fsx1) / cell)});
            for (int sx = sx1; sx < sx2; ++sx) taps.push_back(af_capture_tap{sx, (float)(1.0 / cell)});
            if (fsx2 - sx2 > 1e-3) taps.push_back(af_capture_tap{sx2, (float)(std::fmin(std::fmin(fsx2 - sx2, 1.0), cell) / cell)});
        }
        first.push_back((int32_t)taps.size());
        return pad8((int64_t)first.size() * 4) + (int64_t)taps.size() * (int64_t)sizeof(af_capture_tap);
    }
};

static int check_area_table(const AreaTable& g) {
    for (int d = 0; d < g.dst; ++d)
        AF_REQUIRE(g.first[d + 1] > g.first[d], "capture_plan: the area table %d -> %d has no tap for %d", g.src, g.dst, d);
    for (const af_capture_tap& t : g.taps)
        AF_REQUIRE(t.idx >= 0 && t.idx < g.src, "capture_plan: the area table %d -> %d names %d", g.src, g.dst, t.idx);
    return AF_OK;
}

static inline bool capture_side(int v) { return v >= 1 && v <= AF_CAPTURE_MAX_SIDE; }

static int capture_plan(const af_capture_frame* frames, int n, const af_store_ref* stores, int n_stores, void* table, int64_t table_bytes,
                        int64_t* used_bytes) {
    RunPlan<af_capture_header, af_capture_item> plan;
    int rc = plan.begin("capture_plan", n, n_stores);
    if (rc != AF_OK) return rc;
    std::vector<AreaTable> xs, ys;
    for (int i = 0; i < n; ++i) {
        const af_capture_frame& f = frames[i];
        AF_REQUIRE(f.src, "capture_plan: frame %d: null source", i);
        AF_REQUIRE(f.channels == 3 || f.channels == 4, "capture_plan: frame %d: %d channels (3 or 4)", i, f.channels);
        AF_REQUIRE(capture_side(f.h) && capture_side(f.w) && capture_side(f.dh) && capture_side(f.dw),
                   "capture_plan: frame %d: %dx%d -> %dx%d (every side 1 to %d)", i, f.w, f.h, f.dw, f.dh, AF_CAPTURE_MAX_SIDE);
        AF_REQUIRE(f.dw <= f.w && f.dh <= f.h, "capture_plan: frame %d: %dx%d -> %dx%d is upscaling", i, f.w, f.h, f.dw, f.dh);
        AF_REQUIRE(f.pitch >= (int64_t)f.w * f.channels && f.pitch <= 0x7fffffff, "capture_plan: frame %d: pitch %lld is shorter than a row of %d bytes",
                   i, (long long)f.pitch, f.w * f.channels);
        const af_store_ref* st;
        unsigned char* dst;
        rc = store_frame("capture_plan", "frame", i, stores, n_stores, f.store, f.slot, true, true, &st, &dst);
        if (rc != AF_OK) return rc;
        const af_frame_store& s = st->desc;
        AF_REQUIRE(s.height == f.dh && s.width == f.dw, "capture_plan: frame %d: a destination of %dx%d does not fit store %d of %dx%d", i, f.dw, f.dh,
                   f.store, s.width, s.height);
        af_capture_item& it = plan.items[i];
        it.src = f.src;
        it.dst = dst;
        it.src_pitch = (int32_t)f.pitch; it.dst_pitch = (int32_t)s.row_pitch;
        it.h = f.h; it.w = f.w; it.dh = f.dh; it.dw = f.dw;
        it.runs_x = row_runs(f.dw);
        it.mode = capture_mode(f.h, f.w, f.dh, f.dw);
        it.kx = it.ky = 1; it.inv_area = 1.f;
        if (it.mode == AF_CAPTURE_BOX) {
            it.kx = f.w / f.dw; it.ky = f.h / f.dh;
            it.inv_area = 1.f / (float)(it.kx * it.ky);              // one fp32 division, as the statement's
        } else if (it.mode == AF_CAPTURE_TABLE) {
            const AreaTable& x = axis_table_at(xs, f.w, f.dw, &plan.used);
            it.xtab = x.offset;
            it.xk = (uint8_t)(x.most_taps() < 255 ? x.most_taps() : 255);
            it.ytab = axis_table_at(ys, f.h, f.dh, &plan.used).offset;
        }
        it.channels = (uint8_t)f.channels;
        it.swap = (uint8_t)((st->bgr != 0) != (f.src_bgr != 0));
        it.dword = (uint8_t)(f.channels == 4 && ((uintptr_t)f.src & 3) == 0 && (f.pitch & 3) == 0);
        plan.add_tiles(i, f.dh, f.dw);
    }
    for (const std::vector<AreaTable>* axis : {&xs, &ys})
        for (const AreaTable& g : *axis) {
            rc = check_area_table(g);
            if (rc != AF_OK) return rc;
        }
    rc = plan.finish("capture_plan", AF_CAPTURE_KIND, table, table_bytes, used_bytes);
    if (rc != AF_OK) return rc;
    unsigned char* t = (unsigned char*)table;
    for (const std::vector<AreaTable>* axis : {&xs, &ys})
        for (const AreaTable& g : *axis) {
            const int64_t head = pad8((int64_t)g.first.size() * 4);
            memset(t + g.offset, 0, (size_t)head);
            memcpy(t + g.offset, g.first.data(), g.first.size() * 4);
            memcpy(t + g.offset + head, g.taps.data(), g.taps.size() * sizeof(af_capture_tap));
        }
    return AF_OK;
}

}  // namespace af

extern "C" int64_t af_capture_table_bytes(const af_capture_frame* frames, int n) {
    using namespace af;
    if (!frames || n < 0 || n > AF_CAPTURE_MAX_FRAMES) return -1;
    int64_t bytes = (int64_t)sizeof(af_capture_header) + (int64_t)n * sizeof(af_capture_item);
    for (int i = 0; i < n; ++i) {
        const af_capture_frame& f = frames[i];
        if (!capture_side(f.h) || !capture_side(f.w) || !capture_side(f.dh) || !capture_side(f.dw) || f.dw > f.w || f.dh > f.h) return -1;
        if (capture_mode(f.h, f.w, f.dh, f.dw) != AF_CAPTURE_TABLE) continue;
        // a source pixel lies in at most two cells (a cell is at least one pixel wide); one more tap per cell for the 1e-3 rules
        bytes += pad8(((int64_t)f.dw + 1) * 4) + pad8(((int64_t)f.dh + 1) * 4) +
                 (2 * (int64_t)f.w + f.dw + 2 * (int64_t)f.h + f.dh) * (int64_t)sizeof(af_capture_tap);
    }
    return bytes;
}

extern "C" int af_capture_plan_u8(const af_capture_frame* frames, int n, const af_store_ref* stores, int n_stores, void* table, int64_t table_bytes,
                                  int64_t* used_bytes) {
    using namespace af;
    return plan_into<af_capture_header>("capture_plan", table, table_bytes, used_bytes, [&] {      // null frames or stores: stamped too
        return frames && stores ? capture_plan(frames, n, stores, n_stores, table, table_bytes, used_bytes) : set_error(AF_ERR_ARG, "capture_plan: null argument");
    });
}

extern "C" int af_capture_to_stores_u8(const void* table_dev, int n, void* stream) {
    return af::launch_runs("capture_to_stores", "capture_frames_kernel", af::capture_frames_kernel, table_dev, n, AF_CAPTURE_MAX_FRAMES, stream);
}
