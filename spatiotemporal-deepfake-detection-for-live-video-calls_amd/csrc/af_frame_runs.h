// What af_resize.hip and af_capture.hip share: a launch that writes 3-byte pixels into many destinations as runs of 4 pixels, and
// the planner of the table such a launch reads.  Integer code only: af_capture.hip's fp-contraction pragma has nothing to cover here.
//
// Shape.  A lane owns a run of 4 adjacent pixels of one destination row (12 bytes, three dwords); the runs of an item are numbered
// row by row, a workgroup of 256 lanes takes 256 consecutive runs (a tile), and the tiles of all items form one flat list with a
// first_tile prefix in the table's header.  The table lies in device memory (it holds the items' coefficient tables), so the launch
// cannot know the tile count: a fixed grid strides over the tiles.  Header and Item are af_resize_* or af_capture_*: the headers
// have the same fields, and the items share dh, dw, runs_x, dst and dst_pitch by name.
//
// No stray access, writes.  A lane whose run lies behind its item's dh * runs_x runs writes nothing.  A full run writes the 12 bytes
// [12 j, 12 j + 12) of its destination row, as three dwords when the address is 4-byte aligned and as bytes otherwise; the last run
// of a row with dw % 4 != 0 writes its 3, 6 or 9 bytes as bytes.  Exactly dh rows of 3 dw bytes: nothing goes into the pitch
// padding, between frames or behind the last row.  A table whose kind or n is not the launch's (a refused one) writes nothing.
#pragma once
#include <cstring>
#include <vector>

#include "af_common.h"

namespace af {

constexpr int RUN_PX = 4;                           // pixels of a row one lane produces
constexpr int RUN_TILE = 256;                       // runs per workgroup
constexpr int RUN_GRID = 2048;                      // workgroups of a launch: 8 per CU, each strides over the tiles

static inline int row_runs(int dw) { return (dw + RUN_PX - 1) / RUN_PX; }
static inline int64_t run_tiles(int dh, int dw) { return ((int64_t)dh * row_runs(dw) + RUN_TILE - 1) / RUN_TILE; }

// four pixels (24 bits each) -> the 12 bytes of a run
__device__ __forceinline__ void pack_run(const unsigned (&px)[4], unsigned (&out)[3]) {
    out[0] = px[0] | (px[1] << 24);
    out[1] = (px[1] >> 8) | (px[2] << 16);
    out[2] = (px[2] >> 16) | (px[3] << 8);
}

// the first npx pixels of a packed run -> d
__device__ __forceinline__ void store_run12(unsigned char* d, const unsigned (&out)[3], int npx) {
    if (npx == RUN_PX && ((unsigned)(uintptr_t)d & 3) == 0) {
        ((unsigned*)d)[0] = out[0]; ((unsigned*)d)[1] = out[1]; ((unsigned*)d)[2] = out[2];
    } else {
        for (int i = 0; i < 3 * npx; ++i) d[i] = (unsigned char)(out[i >> 2] >> (8 * (i & 3)));
    }
}

// one channel of OpenCV's 2 x 2 fast area path: the mean, half up
__device__ __forceinline__ unsigned area2(unsigned a, unsigned b, unsigned c, unsigned d) { return (a + b + c + d + 2u) >> 2; }

// A kernel strides the fixed grid over launch_tiles() tiles; tile_run() gives the lane's run in one of them: pixels x0 .. x0 + npx - 1
// of row dy of item `it`, to be packed and handed to store_run12(run_dst(r), out, r.npx).  npx == 0: the lane has no run in this tile.
template <int KIND, class Header>
__device__ __forceinline__ int launch_tiles(const unsigned char* table, int n) {
    const Header* hd = (const Header*)table;
    if (hd->kind != KIND || hd->n != n) return 0;                   // not this launch's table (or a refused one): write nothing
    return hd->total_tiles;
}
template <class Item>
struct TileRun { Item it; int dy, x0, npx; };
template <class Header, class Item>
__device__ __forceinline__ TileRun<Item> tile_run(const unsigned char* table, int n, int tile) {
    const Header* hd = (const Header*)table;
    int k = 0, hi = n - 1;                                           // the last item whose first tile is <= tile
    while (k < hi) {
        const int mid = (k + hi + 1) >> 1;
        if (hd->first_tile[mid] <= tile) k = mid; else hi = mid - 1;
    }
    TileRun<Item> r;
    r.it = ((const Item*)(table + sizeof(Header)))[k];
    const int run = (tile - hd->first_tile[k]) * RUN_TILE + (int)threadIdx.x;
    r.dy = r.x0 = r.npx = 0;
    if (run >= r.it.dh * r.it.runs_x) return r;
    r.dy = run / r.it.runs_x;
    r.x0 = (run - r.dy * r.it.runs_x) * RUN_PX;
    r.npx = min(RUN_PX, r.it.dw - r.x0);
    return r;
}
template <class Item>
__device__ __forceinline__ unsigned char* run_dst(const TileRun<Item>& r) { return (unsigned char*)r.it.dst + (long long)r.dy * r.it.dst_pitch + 3 * r.x0; }

// ---- the planner's side (host) ----
// The table of (src -> dst) among `known`, or a new one at *used.  An Entry has src, dst, offset and prepare(), which makes
// whatever the entry keeps on the host and returns the bytes it takes in the table.
template <class Entry>
static Entry& axis_table_at(std::vector<Entry>& known, int src, int dst, int64_t* used) {
    for (Entry& g : known)
        if (g.src == src && g.dst == dst) return g;
    known.emplace_back();
    Entry& g = known.back();
    g.src = src; g.dst = dst; g.offset = (int32_t)*used;
    *used += g.prepare();
    return g;
}

// A table in the making: begin(), then per item its checks, items[i] and add_tiles(i, ...), then finish() and the axis tables.
template <class Header, class Item>
struct RunPlan {
    static constexpr int MAX = (int)(sizeof(Header::first_tile) / sizeof(int32_t)) - 1;
    Header hd = {};
    std::vector<Item> items;                                        // zeroed, padding included
    int64_t used = 0, tiles = 0;

    int begin(const char* who, int n, int n_stores) {
        AF_REQUIRE(n >= 0 && n <= MAX, "%s: %d frames (at most %d per launch)", who, n, MAX);
        AF_REQUIRE(n_stores > 0 && n_stores <= AF_MAX_STORES, "%s: %d stores (1 to %d per launch)", who, n_stores, AF_MAX_STORES);
        items.resize((size_t)n);
        used = (int64_t)sizeof(Header) + (int64_t)n * sizeof(Item);
        return AF_OK;
    }
    void add_tiles(int i, int dh, int dw) { hd.first_tile[i] = (int32_t)tiles; tiles += run_tiles(dh, dw); }
    // header and items into `table`; the caller writes its axis tables behind them
    int finish(const char* who, int kind, void* table, int64_t table_bytes, int64_t* used_bytes) {
        const int n = (int)items.size();
        for (int i = n; i <= MAX; ++i) hd.first_tile[i] = (int32_t)tiles;
        AF_REQUIRE(table_bytes >= used, "%s: the table needs %lld bytes, the buffer has %lld", who, (long long)used, (long long)table_bytes);
        AF_REQUIRE(used <= 0x7fffffff && tiles <= 0x7fffffff, "%s: a table of %lld bytes and %lld tiles", who, (long long)used, (long long)tiles);
        hd.kind = kind; hd.n = n; hd.total_tiles = (int32_t)tiles; hd.used_bytes = (int32_t)used;
        memcpy(table, &hd, sizeof hd);
        if (n) memcpy((unsigned char*)table + sizeof hd, items.data(), (size_t)n * sizeof(Item));
        *used_bytes = used;
        return AF_OK;
    }
};

// An extern planner around plan(): a table buffer that can at least be stamped, and the stamp when plan() refuses - a refused
// table is no table, no launch takes it.
template <class Header, class Plan>
static int plan_into(const char* who, void* table, int64_t table_bytes, int64_t* used_bytes, Plan plan) {
    AF_REQUIRE(table && used_bytes, "%s: null argument", who);
    AF_REQUIRE(((uintptr_t)table & 7) == 0, "%s: the table buffer must be 8-byte aligned", who);
    AF_REQUIRE(table_bytes >= (int64_t)sizeof(Header), "%s: the table needs %lld bytes for its header alone, the buffer has %lld", who,
               (long long)sizeof(Header), (long long)table_bytes);
    *used_bytes = 0;
    const int rc = plan();
    if (rc != AF_OK) ((Header*)table)->kind = -1;
    return rc;
}

// the launch over a device copy of a table of at most max_n items
static inline int launch_runs(const char* who, const char* kernel_name, void (*kernel)(const unsigned char*, int), const void* table_dev, int n, int max_n,
                              void* stream) {
    AF_REQUIRE(table_dev, "%s: null table", who);
    AF_REQUIRE(((uintptr_t)table_dev & 7) == 0, "%s: the table must be 8-byte aligned", who);
    AF_REQUIRE(n >= 0 && n <= max_n, "%s: %d frames (at most %d per launch)", who, n, max_n);
    if (n == 0) return AF_OK;
    hipLaunchKernelGGL(kernel, dim3(RUN_GRID), dim3(RUN_TILE), 0, (hipStream_t)stream, (const unsigned char*)table_dev, n);
    AF_CHECK_LAUNCH(kernel_name);
    return AF_OK;
}

}  // namespace af
