// The quality gate's pixel part for every face of a frame in one launch: the reference's _frame_quality_weight (test/af_realtime.py
// :265-267) with variance_of_laplacian (:191-192),
//     small = cv2.resize(crop_rgb, (max(1, w // 2), max(1, h // 2)), interpolation=cv2.INTER_AREA)
//     lap   = cv2.Laplacian(cv2.cvtColor(small, cv2.COLOR_RGB2GRAY), cv2.CV_64F).var()
// over rectangles of frames that are resident on the device (af_hip.h: af_frame_store / af_frame_rect), so no crop is cut on the host.
//
// Arithmetic (a restatement of OpenCV 4.x - resize.cpp, color_rgb, deriv.cpp; like the warp of af_align.hip it cannot be pinned
// against cv2 itself where this is built, only against tests/quality_ref.py and the hand-worked cases of tests/test_realtime_host.py):
//   sizes      dw = max(1, w / 2), dh = max(1, h / 2)
//   half size  per channel, to uint8:  w == 2 dw and h == 2 dh: (a + b + c + d + 2) >> 2;  both w / dw and h / dh whole: the integer
//              box sum times fp32 1 / area, rounded half to even;  otherwise OpenCV's area table: cell bounds in fp64 (scale = w / dw;
//              the first and last partial source pixel weigh overlap / cellWidth and count when the overlap exceeds 1e-3, whole
//              pixels weigh 1 / cellWidth), weights cast to fp32, fp32 accumulation along x in table order, then over the rows with
//              their weights, rounded half to even and saturated.  No contraction: __dmul_rn / __dadd_rn / __fmul_rn / __fadd_rn.
//   grey       (R * 9798 + G * 19235 + B * 3735 + 16384) >> 15 on the resized bytes
//   Laplacian  up + down + left + right - 4 * centre with BORDER_REFLECT_101 (-1 -> 1, n -> n - 2; a dimension of 1 -> 0): an integer in
//              [-1020, 1020]
//   sums       S1 = sum L, S2 = sum L^2 (64-bit), n_px = dw * dh; the host forms lap = (n_px * S2 - S1^2) / n_px^2.
//
// Shape: a workgroup of 256 threads takes one 8 x 32 tile of one rectangle's half-size image, builds the tile's grey bytes with a
// halo of one (reflected) pixel in LDS, applies the stencil, reduces in the wave and adds the tile's two totals to the rectangle's
// 64-bit accumulators with global integer atomics - integer addition commutes, so the sums do not depend on the order the tiles
// finish in.  The accumulators are cleared by a hipMemsetAsync in front of the launch, on the same stream.  Rectangles are tens:
// they and the prefix table of their tiles travel as kernel arguments.  Byte work on a few hundred KB; nothing here is tuned.
#include "af_common.h"

namespace af {

constexpr int Q_TH = 8, Q_TW = 32;                  // the tile of half-size pixels one workgroup takes
constexpr int Q_GH = Q_TH + 2, Q_GW = Q_TW + 2;     // with its halo

// A rectangle carries the absolute address of its first pixel, its store's row pitch and byte order, so the launch needs no table of
// stores - one (af_face_quality_u8) or several (af_face_quality_stores_u8); 64 x 32 bytes + the header stay far under the 4 KB of
// arguments.
struct QualityStoreRect {
    const unsigned char* first;
    int32_t pitch, w, h;
    int32_t first_tile, grey_offset;
    int32_t bgr;
};
static_assert(sizeof(QualityStoreRect) == 32, "argument budget");

struct QualityStoresArgs {
    af_quality_sums* sums;
    unsigned char* grey;
    int n, total_tiles;
    QualityStoreRect r[AF_QUALITY_MAX_RECTS];
};
static_assert(sizeof(QualityStoresArgs) <= 4096, "kernel arguments");

__device__ __forceinline__ int reflect101(int i, int n) { return n == 1 ? 0 : (i < 0 ? -i : (i >= n ? 2 * n - 2 - i : i)); }

__device__ __forceinline__ int round_sat_u8(float v) {          // saturate_cast<uchar>(float): cvRound (half to even), then clamp
    const int r = (int)rintf(v);
    return r < 0 ? 0 : (r > 255 ? 255 : r);
}

// One destination index of computeResizeAreaTab: the whole source pixels [s1, s2) at weight `mid`, the partial one s1 - 1 in front
// at `first` and the partial one s2 behind at `last` (each only if `has_*`).
struct AreaCell {
    int s1, s2;
    float first, mid, last;
    bool has_first, has_last;
};

__device__ __forceinline__ AreaCell area_cell(int d, int ssize, int dsize) {
    const double scale = (double)ssize / (double)dsize;
    const double f1 = __dmul_rn((double)d, scale), f2 = __dadd_rn(f1, scale);
    const double cell = fmin(scale, __dadd_rn((double)ssize, -f1));
    int s1 = (int)ceil(f1), s2 = (int)floor(f2);
    s2 = min(s2, ssize - 1);
    s1 = min(s1, s2);
    AreaCell c;
    c.s1 = s1; c.s2 = s2;
    const double lead = __dadd_rn((double)s1, -f1), tail = __dadd_rn(f2, -(double)s2);
    c.has_first = lead > 1e-3;
    c.has_last = tail > 1e-3;
    c.first = (float)(lead / cell);
    c.mid = (float)(1.0 / cell);
    c.last = (float)(fmin(fmin(tail, 1.0), cell) / cell);
    return c;
}

// the grey byte at (gx, gy) of the rectangle's half-size image - FULL: of the rectangle as it is, no resize stage -; `src` is the
// rectangle's first byte
template <bool FULL>
__device__ int grey_at(const unsigned char* src, long long pitch, int w, int h, int dw, int dh, int gx, int gy, int bgr) {
    int ch[3];
    if (FULL) {
        const unsigned char* p = src + (long long)gy * pitch + (long long)gx * 3;
#pragma unroll
        for (int c = 0; c < 3; ++c) ch[c] = p[c];
    } else if (w == 2 * dw && h == 2 * dh) {
        const unsigned char* p = src + (long long)(2 * gy) * pitch + (long long)(2 * gx) * 3;
#pragma unroll
        for (int c = 0; c < 3; ++c) ch[c] = (p[c] + p[3 + c] + p[pitch + c] + p[pitch + 3 + c] + 2) >> 2;
    } else if (w % dw == 0 && h % dh == 0) {
        const int kx = w / dw, ky = h / dh;
        const float inv = (float)(1.0 / (double)(kx * ky));       // == 1.f / area: 53 bits round twice harmlessly for a quotient of small integers
        int sum[3] = {0, 0, 0};
        for (int y = 0; y < ky; ++y) {
            const unsigned char* p = src + (long long)(gy * ky + y) * pitch + (long long)(gx * kx) * 3;
            for (int x = 0; x < kx; ++x)
#pragma unroll
                for (int c = 0; c < 3; ++c) sum[c] += p[x * 3 + c];
        }
#pragma unroll
        for (int c = 0; c < 3; ++c) ch[c] = round_sat_u8(__fmul_rn((float)sum[c], inv));
    } else {
        const AreaCell cx = area_cell(gx, w, dw), cy = area_cell(gy, h, dh);
        float acc[3] = {0.f, 0.f, 0.f};
        bool started = false;
        for (int sy = cy.has_first ? cy.s1 - 1 : cy.s1; sy <= (cy.has_last ? cy.s2 : cy.s2 - 1); ++sy) {
            const float beta = sy < cy.s1 ? cy.first : (sy < cy.s2 ? cy.mid : cy.last);
            const unsigned char* p = src + (long long)sy * pitch;
            float buf[3] = {0.f, 0.f, 0.f};
            for (int sx = cx.has_first ? cx.s1 - 1 : cx.s1; sx <= (cx.has_last ? cx.s2 : cx.s2 - 1); ++sx) {
                const float alpha = sx < cx.s1 ? cx.first : (sx < cx.s2 ? cx.mid : cx.last);
#pragma unroll
                for (int c = 0; c < 3; ++c) buf[c] = __fadd_rn(buf[c], __fmul_rn((float)p[sx * 3 + c], alpha));
            }
#pragma unroll
            for (int c = 0; c < 3; ++c) acc[c] = started ? __fadd_rn(acc[c], __fmul_rn(beta, buf[c])) : __fmul_rn(beta, buf[c]);
            started = true;
        }
#pragma unroll
        for (int c = 0; c < 3; ++c) ch[c] = round_sat_u8(acc[c]);
    }
    const int r = bgr ? ch[2] : ch[0], b = bgr ? ch[0] : ch[2];
    return (r * 9798 + ch[1] * 19235 + b * 3735 + 16384) >> 15;
}

// One tile of one rectangle: `src` the rectangle's first byte, rows `pitch` bytes apart, w x h pixels, tile `local` of it; the
// tile's totals go to `out`, its grey bytes (tests) to `grey` (the rectangle's own image, or null).  FULL: the measured image is
// the rectangle itself (dw = w, dh = h), the reference's second, full-size variance_of_laplacian (TEST2.py:296-299).
template <bool FULL>
__device__ __forceinline__ void quality_tile(const unsigned char* src, long long pitch, int w, int h, int local, int bgr, af_quality_sums* out,
                                             unsigned char* grey) {
    __shared__ unsigned char g[Q_GH][Q_GW + 2];
    __shared__ long long part[2][4];
    const int dw = FULL ? w : max(1, w / 2), dh = FULL ? h : max(1, h / 2);
    const int tiles_x = (dw + Q_TW - 1) / Q_TW;
    const int ty0 = (local / tiles_x) * Q_TH, tx0 = (local % tiles_x) * Q_TW;

    for (int i = threadIdx.x; i < Q_GH * Q_GW; i += 256) {
        const int gr = i / Q_GW, gc = i - gr * Q_GW;
        const int y = ty0 - 1 + gr, x = tx0 - 1 + gc;             // half-size coordinates before the border rule
        int v = 0;
        if (y <= dh && x <= dw) {                                 // beyond n nothing reads the cell
            const int yy = reflect101(y, dh), xx = reflect101(x, dw);
            v = grey_at<FULL>(src, pitch, w, h, dw, dh, xx, yy, bgr);
            if (grey && gr >= 1 && gr <= Q_TH && gc >= 1 && gc <= Q_TW && y < dh && x < dw)
                grey[(long long)y * dw + x] = (unsigned char)v;
        }
        g[gr][gc] = (unsigned char)v;
    }
    __syncthreads();

    const int ly = threadIdx.x / Q_TW, lx = threadIdx.x % Q_TW;
    long long s1 = 0, s2 = 0;
    if (ty0 + ly < dh && tx0 + lx < dw) {
        const int L = (int)g[ly][lx + 1] + (int)g[ly + 2][lx + 1] + (int)g[ly + 1][lx] + (int)g[ly + 1][lx + 2] - 4 * (int)g[ly + 1][lx + 1];
        s1 = L;
        s2 = (long long)L * L;
    }
    for (int off = 32; off > 0; off >>= 1) {                      // wave64
        s1 += __shfl_down(s1, off, 64);
        s2 += __shfl_down(s2, off, 64);
    }
    const int wave = threadIdx.x >> 6;
    if ((threadIdx.x & 63) == 0) { part[0][wave] = s1; part[1][wave] = s2; }
    __syncthreads();
    if (threadIdx.x == 0) {
        const long long t1 = part[0][0] + part[0][1] + part[0][2] + part[0][3];
        const long long t2 = part[1][0] + part[1][1] + part[1][2] + part[1][3];
        atomicAdd((unsigned long long*)&out->s1, (unsigned long long)t1);      // two's complement: the signed sum of the parts
        atomicAdd((unsigned long long*)&out->s2, (unsigned long long)t2);
        if (local == 0) out->n_px = dw * dh;
    }
}

template <bool FULL>
__global__ __launch_bounds__(256) void face_quality_stores_kernel(const QualityStoresArgs a) {
    const int tile = blockIdx.x;
    if (tile >= a.total_tiles) return;
    int k = 0;
    while (k + 1 < a.n && a.r[k + 1].first_tile <= tile) ++k;     // tens of rectangles: a scan
    const QualityStoreRect r = a.r[k];
    quality_tile<FULL>(r.first, r.pitch, r.w, r.h, tile - r.first_tile, r.bgr, a.sums + k, a.grey ? a.grey + r.grey_offset : nullptr);
}

// ---- the launch whose rectangles lie in a chunk record in device memory (af_hip.h, "chunk stage") ----
// A fixed grid: workgroup b takes tiles b, b + gridDim.x, ... below the record's tile total, which it reads itself.  A tile finds
// its candidate by bisection of the tile prefixes; the candidate is checked against the store before a byte of it is read.
struct QualityTableArgs {
    const unsigned char* base;
    int64_t store_bytes, frame_stride, row_pitch;
    int32_t n_frames, height, width, bgr;
    af_runner_header* head;
    af_runner_cand* cands;
    af_quality_sums* sums;
    unsigned char* grey;
    int64_t grey_stride;
    int32_t capacity, max_tiles;
};
constexpr int Q_TABLE_GRID = 1024;

template <bool FULL>
__global__ __launch_bounds__(256) void face_quality_table_kernel(const QualityTableArgs a) {
    int n = a.head->n_cands;
    n = n < 0 ? 0 : (n > a.capacity ? a.capacity : n);
    int total = FULL ? a.head->tiles_full : a.head->tiles_half;
    total = total < 0 ? 0 : (total > a.max_tiles ? a.max_tiles : total);
    if (n == 0) return;
    for (int tile = blockIdx.x; tile < total; tile += gridDim.x) {     // uniform in the workgroup
        int lo = 0, hi = n - 1;                                        // the last candidate whose first tile is <= tile
        while (lo < hi) {
            const int mid = (lo + hi + 1) >> 1;
            const int first = FULL ? a.cands[mid].tile_full : a.cands[mid].tile_half;
            if (first <= tile) lo = mid; else hi = mid - 1;
        }
        af_runner_cand* c = a.cands + lo;
        const int x1 = c->box[0], y1 = c->box[1], x2 = c->box[2], y2 = c->box[3], slot = c->slot;
        const int local = tile - (FULL ? c->tile_full : c->tile_half);
        const long long w = (long long)x2 - x1, h = (long long)y2 - y1;
        bool ok = slot >= 0 && slot < a.n_frames && x1 >= 0 && y1 >= 0 && w > 0 && h > 0 && x2 <= a.width && y2 <= a.height;
        long long offset = 0;
        if (ok) {
            offset = (long long)slot * a.frame_stride + (long long)y1 * a.row_pitch + (long long)x1 * 3;
            ok = offset + (h - 1) * a.row_pitch + w * 3 <= a.store_bytes;
        }
        if (ok) {
            const int dw = FULL ? (int)w : max(1, (int)w / 2), dh = FULL ? (int)h : max(1, (int)h / 2);
            ok = local >= 0 && local < ((dw + Q_TW - 1) / Q_TW) * ((dh + Q_TH - 1) / Q_TH);
            if (ok) {
                unsigned char* g = (a.grey && (long long)dw * dh <= a.grey_stride) ? a.grey + (long long)lo * a.grey_stride : nullptr;
                quality_tile<FULL>(a.base + offset, a.row_pitch, (int)w, (int)h, local, a.bgr, a.sums + lo, g);
            }
        }
        if (!ok && threadIdx.x == 0) {
            atomicOr(&c->flags, AF_RUNNER_CAND_BAD);
            atomicOr(&a.head->bad, 1);
        }
        __syncthreads();                                               // quality_tile's LDS is the next tile's too
    }
}

// ---- the launch whose rectangles lie in the candidate records of live calls in device memory (af_hip.h, "a live tick's face stage") ----
// Up to 64 jobs - a record, its frame's slot and its store, packed to 56 bytes each - travel in the arguments.  A fixed grid: every
// workgroup reads the jobs' tile totals (cut at what the job's frame can hold), forms their prefix in LDS and takes tiles b,
// b + gridDim.x, ...; a tile finds its job, then its entry in the job's record, by bisection of ascending tile prefixes.  The entry
// is checked against the job's store before a byte of it is read.
struct QualityRecordJob {
    const unsigned char* base;
    int64_t store_bytes, frame_stride;
    af_live_record* rec;
    int32_t row_pitch, n_frames, slot, max_tiles;
    int16_t height, width;
    int32_t bgr;
};
static_assert(sizeof(QualityRecordJob) == 56, "argument budget");
struct QualityRecordsArgs {
    af_quality_sums* sums;
    unsigned char* grey;
    int64_t grey_stride;
    int32_t n, reserved;
    QualityRecordJob j[AF_QUALITY_MAX_RECTS];
};
static_assert(sizeof(QualityRecordsArgs) <= 4096, "kernel arguments");

__global__ __launch_bounds__(256) void face_quality_records_kernel(const QualityRecordsArgs a) {
    __shared__ int first[AF_QUALITY_MAX_RECTS + 1];                    // first[j]: the first tile of job j; first[n]: the total
    __shared__ int tiles[AF_QUALITY_MAX_RECTS];
    if ((int)threadIdx.x < a.n) {
        const int t = a.j[threadIdx.x].rec->tiles;
        tiles[threadIdx.x] = t < 0 ? 0 : (t > a.j[threadIdx.x].max_tiles ? a.j[threadIdx.x].max_tiles : t);
    }
    __syncthreads();
    if (threadIdx.x == 0) {
        int total = 0;                                                 // the sum of the jobs' max_tiles is <= 0x7fffffff: checked on the host
        for (int j = 0; j < a.n; ++j) {
            first[j] = total;
            total += tiles[j];
        }
        first[a.n] = total;
    }
    __syncthreads();
    const int total = first[a.n];
    for (int tile = blockIdx.x; tile < total; tile += gridDim.x) {     // uniform in the workgroup
        int lo = 0, hi = a.n - 1;                                      // the last job whose first tile is <= tile
        while (lo < hi) {
            const int mid = (lo + hi + 1) >> 1;
            if (first[mid] <= tile) lo = mid; else hi = mid - 1;
        }
        const int job = lo, in_job = tile - first[job];
        const QualityRecordJob& q = a.j[job];
        int n = q.rec->n_online;
        n = n < 0 ? 0 : (n > AF_TRACK_MAX_TRACKS ? AF_TRACK_MAX_TRACKS : n);
        bool ok = n > 0;
        af_live_entry* e = q.rec->online;
        if (ok) {
            lo = 0; hi = n - 1;                                        // the last entry whose first tile is <= in_job
            while (lo < hi) {
                const int mid = (lo + hi + 1) >> 1;
                if (q.rec->online[mid].first_tile <= in_job) lo = mid; else hi = mid - 1;
            }
            e = q.rec->online + lo;
        }
        const int x1 = e->box[0], y1 = e->box[1], x2 = e->box[2], y2 = e->box[3], k = e->cand;
        const int local = in_job - e->first_tile;
        const long long w = (long long)x2 - x1, h = (long long)y2 - y1;
        ok = ok && (e->flags & AF_LIVE_CANDIDATE) && k >= 0 && k < AF_TRACK_MAX_TRACKS;
        ok = ok && q.slot >= 0 && q.slot < q.n_frames && x1 >= 0 && y1 >= 0 && w > 0 && h > 0 && x2 <= q.width && y2 <= q.height;
        long long offset = 0;
        if (ok) {
            offset = (long long)q.slot * q.frame_stride + (long long)y1 * q.row_pitch + (long long)x1 * 3;
            ok = offset + (h - 1) * q.row_pitch + w * 3 <= q.store_bytes;
        }
        if (ok) {
            const int dw = max(1, (int)w / 2), dh = max(1, (int)h / 2);
            ok = local >= 0 && local < ((dw + Q_TW - 1) / Q_TW) * ((dh + Q_TH - 1) / Q_TH);
            if (ok) {
                const long long at = (long long)job * AF_TRACK_MAX_TRACKS + k;
                unsigned char* g = (a.grey && (long long)dw * dh <= a.grey_stride) ? a.grey + at * a.grey_stride : nullptr;
                quality_tile<false>(q.base + offset, q.row_pitch, (int)w, (int)h, local, q.bgr, a.sums + at, g);
            }
        }
        if (!ok && threadIdx.x == 0) {
            atomicOr(&e->flags, AF_LIVE_BAD);
            atomicOr(&q.rec->bad, 1);
        }
        __syncthreads();                                               // quality_tile's LDS is the next tile's too
    }
}

// The host side of both entry points: the stores and the rectangles checked, one memset and one launch.  `listed`: a rectangle
// names its store in af_frame_rect.reserved; otherwise every rectangle is of the one store and reserved is not read.  `full`: the
// kernel's full-size mode.
static int face_quality(const char* who, const af_store_ref* stores, int n_stores, bool listed, bool full, const af_frame_rect* rects, int n,
                        af_quality_sums* sums, void* grey, int64_t grey_bytes, void* stream) {
    AF_REQUIRE(stores && rects && sums, "%s: null argument", who);
    AF_REQUIRE(n >= 0 && n <= AF_QUALITY_MAX_RECTS, "%s: %d rectangles (at most %d per launch)", who, n, AF_QUALITY_MAX_RECTS);
    AF_REQUIRE(n_stores > 0 && n_stores <= AF_MAX_STORES, "%s: %d stores (1 to %d per launch)", who, n_stores, AF_MAX_STORES);
    if (n == 0) return AF_OK;
    for (int i = 0; i < n_stores; ++i) {
        AF_REQUIRE(stores[i].base, "%s: store %d: null base pointer", who, i);
        const int rc = check_frame_store(who, listed ? i : -1, stores[i].desc);
        if (rc != AF_OK) return rc;
    }
    QualityStoresArgs a;
    a.sums = sums; a.grey = (unsigned char*)grey; a.n = n;
    int64_t tiles = 0, grey_total = 0;
    for (int i = 0; i < n; ++i) {
        const af_frame_rect& r = rects[i];
        const int store = listed ? r.reserved : 0;
        AF_REQUIRE(store >= 0 && store < n_stores, "%s: rectangle %d names store %d of %d", who, i, store, n_stores);
        const af_store_ref& st = stores[store];
        int64_t offset = 0;
        if (const int fault = frame_rect_fault(st.desc, r, 0, &offset)) {
            char item[32];
            snprintf(item, sizeof item, "rectangle %d", i);
            return refuse_frame_rect(who, item, listed ? store : -1, st.desc, r, fault);
        }
        const int dw = full ? r.iw : (r.iw / 2 > 1 ? r.iw / 2 : 1), dh = full ? r.ih : (r.ih / 2 > 1 ? r.ih / 2 : 1);
        a.r[i] = QualityStoreRect{(const unsigned char*)st.base + offset, (int32_t)st.desc.row_pitch, r.iw, r.ih, (int32_t)tiles, (int32_t)grey_total,
                                  st.bgr ? 1 : 0};
        tiles += (int64_t)((dw + Q_TW - 1) / Q_TW) * ((dh + Q_TH - 1) / Q_TH);
        grey_total += (int64_t)dw * dh;
        AF_REQUIRE(tiles <= 0x7fffffff && grey_total <= 0x7fffffff, "%s: too many pixels", who);
    }
    AF_REQUIRE(!grey || grey_bytes >= grey_total, "%s: grey image buffer of %lld bytes, %lld needed", who, (long long)grey_bytes, (long long)grey_total);
    a.total_tiles = (int)tiles;
    hipError_t e = hipMemsetAsync(sums, 0, sizeof(af_quality_sums) * (size_t)n, (hipStream_t)stream);
    if (e != hipSuccess) return set_error(AF_ERR_LAUNCH, "%s: hipMemsetAsync: %s", who, hipGetErrorString(e));
    if (full)
        hipLaunchKernelGGL(face_quality_stores_kernel<true>, dim3((unsigned)tiles), dim3(256), 0, (hipStream_t)stream, a);
    else
        hipLaunchKernelGGL(face_quality_stores_kernel<false>, dim3((unsigned)tiles), dim3(256), 0, (hipStream_t)stream, a);
    AF_CHECK_LAUNCH("face_quality_stores_kernel");
    return AF_OK;
}

}  // namespace af

extern "C" int af_face_quality_u8(const void* store, const af_frame_store* desc, const af_frame_rect* rects, int n, int bgr,
                                  af_quality_sums* sums, void* grey, int64_t grey_bytes, void* stream) {
    const af_store_ref one{store, desc ? *desc : af_frame_store{}, bgr, 0};
    return af::face_quality("face_quality", store && desc ? &one : nullptr, 1, false, false, rects, n, sums, grey, grey_bytes, stream);
}

extern "C" int af_face_quality_stores_u8(const af_store_ref* stores, int n_stores, const af_frame_rect* rects, int n, af_quality_sums* sums,
                                         void* grey, int64_t grey_bytes, void* stream) {
    return af::face_quality("face_quality_stores", stores, n_stores, true, false, rects, n, sums, grey, grey_bytes, stream);
}

extern "C" int af_face_laplacian_stores_u8(const af_store_ref* stores, int n_stores, const af_frame_rect* rects, int n, af_quality_sums* sums,
                                           void* grey, int64_t grey_bytes, void* stream) {
    return af::face_quality("face_laplacian_stores", stores, n_stores, true, true, rects, n, sums, grey, grey_bytes, stream);
}

extern "C" int af_face_quality_table_u8(const af_store_ref* store, void* record, int capacity, int full, af_quality_sums* sums, void* grey,
                                        int64_t grey_stride, void* stream) {
    using namespace af;
    const char* who = "face_quality_table";
    AF_REQUIRE(store && record && sums && store->base, "%s: null argument", who);
    AF_REQUIRE(((uintptr_t)record & 7) == 0, "%s: the record is not 8-byte aligned", who);
    AF_REQUIRE(capacity >= 0 && capacity <= AF_RUNNER_MAX_FRAMES * AF_TRACK_MAX_TRACKS, "%s: %d candidates (at most %d)", who, capacity,
               AF_RUNNER_MAX_FRAMES * AF_TRACK_MAX_TRACKS);
    AF_REQUIRE(!grey || grey_stride >= 1, "%s: a grey stride of %lld bytes", who, (long long)grey_stride);
    const int rc = check_frame_store(who, -1, store->desc);
    if (rc != AF_OK) return rc;
    if (capacity == 0) return AF_OK;
    const af_frame_store& d = store->desc;
    const int64_t per_frame = (int64_t)((d.width + Q_TW - 1) / Q_TW) * ((d.height + Q_TH - 1) / Q_TH);
    AF_REQUIRE(per_frame * capacity <= 0x7fffffff, "%s: too many pixels", who);
    QualityTableArgs a;
    a.base = (const unsigned char*)store->base;
    a.store_bytes = d.store_bytes; a.frame_stride = d.frame_stride; a.row_pitch = d.row_pitch;
    a.n_frames = d.n_frames; a.height = d.height; a.width = d.width; a.bgr = store->bgr ? 1 : 0;
    a.head = (af_runner_header*)record;
    a.cands = (af_runner_cand*)((char*)record + sizeof(af_runner_header) + AF_RUNNER_MAX_FRAMES * sizeof(af_runner_frame));
    a.sums = sums; a.grey = (unsigned char*)grey; a.grey_stride = grey_stride;
    a.capacity = capacity; a.max_tiles = (int32_t)(per_frame * capacity);
    hipError_t e = hipMemsetAsync(sums, 0, sizeof(af_quality_sums) * (size_t)capacity, (hipStream_t)stream);
    if (e != hipSuccess) return set_error(AF_ERR_LAUNCH, "%s: hipMemsetAsync: %s", who, hipGetErrorString(e));
    const unsigned grid = (unsigned)(a.max_tiles < Q_TABLE_GRID ? a.max_tiles : Q_TABLE_GRID);
    if (full)
        hipLaunchKernelGGL(face_quality_table_kernel<true>, dim3(grid), dim3(256), 0, (hipStream_t)stream, a);
    else
        hipLaunchKernelGGL(face_quality_table_kernel<false>, dim3(grid), dim3(256), 0, (hipStream_t)stream, a);
    AF_CHECK_LAUNCH("face_quality_table_kernel");
    return AF_OK;
}

extern "C" int af_face_quality_records_u8(const af_store_ref* stores, int n_stores, const af_live_quality_job* jobs, int n_jobs, af_quality_sums* sums,
                                          void* grey, int64_t grey_stride, void* stream) {
    using namespace af;
    const char* who = "face_quality_records";
    AF_REQUIRE(stores && jobs && sums, "%s: null argument", who);
    AF_REQUIRE(((uintptr_t)sums & 7) == 0, "%s: the sums are not 8-byte aligned", who);
    AF_REQUIRE(n_jobs >= 0 && n_jobs <= AF_QUALITY_MAX_RECTS, "%s: %d jobs (at most %d per launch)", who, n_jobs, AF_QUALITY_MAX_RECTS);
    AF_REQUIRE(n_stores > 0 && n_stores <= AF_MAX_STORES, "%s: %d stores (1 to %d per launch)", who, n_stores, AF_MAX_STORES);
    AF_REQUIRE(!grey || grey_stride >= 1, "%s: a grey stride of %lld bytes", who, (long long)grey_stride);
    if (n_jobs == 0) return AF_OK;
    for (int i = 0; i < n_stores; ++i) {
        AF_REQUIRE(stores[i].base, "%s: store %d: null base pointer", who, i);
        const int rc = check_frame_store(who, i, stores[i].desc);
        if (rc != AF_OK) return rc;
    }
    QualityRecordsArgs a;
    a.sums = sums; a.grey = (unsigned char*)grey; a.grey_stride = grey_stride; a.n = n_jobs; a.reserved = 0;
    int64_t max_total = 0;
    for (int j = 0; j < n_jobs; ++j) {
        const af_live_quality_job& in = jobs[j];
        AF_REQUIRE(in.record && ((uintptr_t)in.record & 7) == 0, "%s: job %d: the record is null or not 8-byte aligned", who, j);
        AF_REQUIRE(in.store >= 0 && in.store < n_stores, "%s: job %d names store %d of %d", who, j, in.store, n_stores);
        const af_store_ref& st = stores[in.store];
        const af_frame_store& d = st.desc;
        const int64_t per_frame = (int64_t)((d.width + Q_TW - 1) / Q_TW) * ((d.height + Q_TH - 1) / Q_TH);   // no half-size image has more tiles
        max_total += per_frame * AF_TRACK_MAX_TRACKS;
        a.j[j] = QualityRecordJob{(const unsigned char*)st.base, d.store_bytes, d.frame_stride, (af_live_record*)in.record, (int32_t)d.row_pitch, d.n_frames,
                                  in.slot, (int32_t)(per_frame * AF_TRACK_MAX_TRACKS), (int16_t)d.height, (int16_t)d.width, st.bgr ? 1 : 0};
    }
    AF_REQUIRE(max_total <= 0x7fffffff, "%s: too many pixels", who);
    hipError_t e = hipMemsetAsync(sums, 0, sizeof(af_quality_sums) * (size_t)n_jobs * AF_TRACK_MAX_TRACKS, (hipStream_t)stream);
    if (e != hipSuccess) return set_error(AF_ERR_LAUNCH, "%s: hipMemsetAsync: %s", who, hipGetErrorString(e));
    const unsigned grid = (unsigned)(max_total < Q_TABLE_GRID ? max_total : Q_TABLE_GRID);
    hipLaunchKernelGGL(face_quality_records_kernel, dim3(grid), dim3(256), 0, (hipStream_t)stream, a);
    AF_CHECK_LAUNCH("face_quality_records_kernel");
    return AF_OK;
}
