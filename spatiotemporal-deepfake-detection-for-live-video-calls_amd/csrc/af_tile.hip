// The speaker tile of a captured call grid: LargestTilePicker's pixel work (test/capture_tile.py:55-95) on a frame that is resident
// on the device, so that the one step of the capture path that would pull a whole frame back to the host per frame stays where the
// frame is.  The host keeps what is a few integers: the variance test on exact sums, the sort, the 16:9 fit, the smoothing.
//
// Arithmetic (a restatement of OpenCV 4.x's plain C++ path; it equals tests/tile_ref.py byte for byte and, like the other OpenCV
// statements here, is unpinned against cv2 itself, absent where this is built):
//   grey       (R * 9798 + G * 19235 + B * 3735 + 16384) >> 15
//   blur       GaussianBlur (5, 5), sigma 0, 8-bit: the tabulated [1, 4, 6, 4, 1] / 16 in 8.8 fixed point on both axes, exact, so
//              g = (S + 128) >> 8 with S = sum k_i k_j p; BORDER_REFLECT_101
//   Sobel      3 x 3 dx, dy of g with BORDER_REPLICATE; m = |dx| + |dy|; m outside the image is 0
//   NMS        m > 50 and, with TG22 = 13573, x = |dx|, y = |dy| << 15:  y < x TG22: m > left && m >= right;
//              y > x TG22 + (x << 16): m > up && m >= down;  else along the gradient's diagonal, both strict.  Strong: m > 150.
//   edges      the candidates 8-connected, through candidates, to a strong one - a set, so OpenCV's stack order is immaterial
//   dilate     3 x 3 once: the maximum over the neighbours inside the image
//   contours   RETR_EXTERNAL + boundingRect: 8-connected components of the mask; kept when it touches the image border or is
//              4-adjacent to background that is 4-connected to the border (a tile's frame is a closed loop: the faces inside it
//              must not become candidates)
//   motion     unblurred grey, |diff| > 16, medianBlur 5 of a binary image (>= 13 of the 25 BORDER_REPLICATE neighbours), two 5 x 5
//              dilations = a 9 x 9 maximum inside the image, the union of the boxes with w h >= area_min.  Nested components lie
//              inside their parent's box, so the union over all components is the union over the external ones.
//
// Shape.  Two front kernels, one pass each: a workgroup of 256 threads takes an 8 x 32 tile, stages the grey bytes with the halo the
// chain needs in LDS (candidates: blur 2 + Sobel 1 + NMS 1 = 4; motion: median 2 + maximum 4 = 6) and writes the tile's bytes.
// One labelling core, label equivalence by union-find with 32-bit atomicMin on the parent array, used three ways:
//   (a) the candidates, 8-connected, with a per-root "holds a strong pixel" byte: the hysteresis, no host loop, no "changed" flag
//   (b) the mask's set pixels, 8-connected, with per-root boxes by atomicMin / atomicMax (only pixels that can be an extreme add)
//   (c) the mask's clear pixels, 4-connected, with a per-root "reaches the border" byte
// (b) and (c) share one parent array and one pass: the two pixel sets are disjoint.  A link always points to a smaller index, so
// after compression a root is the smallest pixel index of its component and labels do not depend on the schedule.  The unions run
// per tile in LDS first (label_tiles_kernel), then across the tile seams on the global parent array (label_seams_kernel).
// Loops: a find walks strictly decreasing indices and a union's retry strictly lowers its larger root, so both end within n =
// h w steps; each is cut at n and sets a bit of the result's error word, which the caller reads - a defect fails, it does not spin.
// A find reads parents with agent-scope relaxed atomic loads: another CU's atomicMin is otherwise not seen through this CU's L1.
// A stale parent would still be an ancestor (links only ever move towards the root), so only speed depends on it.
// Nothing here is tuned: byte work on a megabyte, a dozen short launches on one stream, no host wait.
#include "af_common.h"

namespace af {

constexpr int T_TH = 8, T_TW = 32;                       // the pixels one workgroup takes, one per thread
constexpr int T_TG22 = 13573;                            // int(tan(22.5 deg) * 2^15 + 0.5)
constexpr int T_ERR_FIND = 1, T_ERR_UNION = 2;
constexpr int64_t T_HEADER = 4096;                       // the result and the survivors' list at the workspace's start

struct TileHeader {
    af_tile_result res;
    int32_t listed;                                      // survivors seen (may exceed AF_TILE_MAX_BOXES)
    int32_t list[AF_TILE_MAX_BOXES];                     // their roots, in arrival order
};
static_assert(sizeof(TileHeader) <= T_HEADER, "header");
static_assert(sizeof(af_tile_box) == 40 && sizeof(af_tile_result) == 48 + 40 * AF_TILE_MAX_BOXES, "ABI");

struct TileWorkspace {
    TileHeader* hdr;
    int* parent;                                         // n
    int* box;                                            // 4 n
    unsigned char *fa, *fb;                              // per-root bytes: (a) strong / (c) reaches the border; (b) external
    unsigned char *g, *cls, *edges, *mask;               // n each
};

static inline int64_t align256(int64_t v) { return (v + 255) & ~(int64_t)255; }
static inline int64_t tile_workspace_bytes(int h, int w) {
    const int64_t n = (int64_t)h * w;
    return T_HEADER + align256(4 * n) + align256(16 * n) + 6 * align256(n);
}
static inline TileWorkspace carve(void* base, int h, int w) {
    const int64_t n = (int64_t)h * w;
    unsigned char* p = (unsigned char*)base;
    TileWorkspace ws;
    ws.hdr = (TileHeader*)p; p += T_HEADER;
    ws.parent = (int*)p; p += align256(4 * n);
    ws.box = (int*)p; p += align256(16 * n);
    unsigned char** bytes[6] = {&ws.fa, &ws.fb, &ws.g, &ws.cls, &ws.edges, &ws.mask};
    for (auto b : bytes) { *b = p; p += align256(n); }
    return ws;
}

__device__ __forceinline__ int t_reflect101(int i, int n) { return i < 0 ? -i : (i >= n ? 2 * n - 2 - i : i); }
__device__ __forceinline__ int t_clamp(int i, int n) { return i < 0 ? 0 : (i >= n ? n - 1 : i); }
__device__ __forceinline__ int t_grey(const unsigned char* src, long long pitch, int y, int x, int bgr) {
    const unsigned char* p = src + (long long)y * pitch + (long long)x * 3;
    const int c0 = p[0], c1 = p[1], c2 = p[2];
    return ((bgr ? c2 : c0) * 9798 + c1 * 19235 + (bgr ? c0 : c2) * 3735 + 16384) >> 15;
}

// ---- front, candidates: source -> g (blurred grey) and cls (0 none, 1 candidate, 2 strong candidate)
__global__ __launch_bounds__(256) void tile_front_kernel(const unsigned char* src, long long pitch, int h, int w, int bgr, unsigned char* g_out,
                                                         unsigned char* cls_out) {
    __shared__ unsigned char grey[T_TH + 8][T_TW + 8];   // position p -> grey[reflect101(p)]
    __shared__ unsigned char blur[T_TH + 4][T_TW + 4];   // position p -> g[clamp(p)]: the Sobel's BORDER_REPLICATE
    __shared__ short mag[T_TH + 2][T_TW + 2];            // position p -> m, 0 outside the image
    const int y0 = blockIdx.y * T_TH, x0 = blockIdx.x * T_TW;

    for (int i = threadIdx.x; i < (T_TH + 8) * (T_TW + 8); i += 256) {
        const int r = i / (T_TW + 8), c = i - r * (T_TW + 8);
        const int y = y0 - 4 + r, x = x0 - 4 + c;
        int v = 0;
        if (y < h + 4 && x < w + 4) v = t_grey(src, pitch, t_reflect101(y, h), t_reflect101(x, w), bgr);   // h, w >= 8: one reflection
        grey[r][c] = (unsigned char)v;
    }
    __syncthreads();
    for (int i = threadIdx.x; i < (T_TH + 4) * (T_TW + 4); i += 256) {
        const int r = i / (T_TW + 4), c = i - r * (T_TW + 4);
        const int yc = t_clamp(y0 - 2 + r, h), xc = t_clamp(x0 - 2 + c, w);
        const int gr = yc - y0 + 4, gc = xc - x0 + 4;    // the centre's cell of `grey`; rows gr - 2 .. gr + 2 lie in [0, T_TH + 8)
        int s = 0;
#pragma unroll
        for (int dy = 0; dy < 5; ++dy) {
            const int ky = dy == 0 || dy == 4 ? 1 : (dy == 2 ? 6 : 4);
            const unsigned char* row = &grey[gr - 2 + dy][gc - 2];
            s += ky * (row[0] + 4 * row[1] + 6 * row[2] + 4 * row[3] + row[4]);
        }
        blur[r][c] = (unsigned char)((s + 128) >> 8);
    }
    __syncthreads();
    for (int i = threadIdx.x; i < (T_TH + 2) * (T_TW + 2); i += 256) {
        const int r = i / (T_TW + 2), c = i - r * (T_TW + 2);
        const int y = y0 - 1 + r, x = x0 - 1 + c;
        int m = 0;
        if (y >= 0 && y < h && x >= 0 && x < w) {
            const unsigned char (*b)[T_TW + 4] = blur;   // position (y, x) is cell (r + 1, c + 1)
            const int dx = (b[r][c + 2] + 2 * b[r + 1][c + 2] + b[r + 2][c + 2]) - (b[r][c] + 2 * b[r + 1][c] + b[r + 2][c]);
            const int dy = (b[r + 2][c] + 2 * b[r + 2][c + 1] + b[r + 2][c + 2]) - (b[r][c] + 2 * b[r][c + 1] + b[r][c + 2]);
            m = abs(dx) + abs(dy);
        }
        mag[r][c] = (short)m;
    }
    __syncthreads();
    const int ty = threadIdx.x / T_TW, tx = threadIdx.x % T_TW;
    const int y = y0 + ty, x = x0 + tx;
    if (y >= h || x >= w) return;
    const unsigned char (*b)[T_TW + 4] = blur;
    const int r = ty + 1, c = tx + 1;                    // the pixel's cell of `mag`; its cell of `blur` is (r + 1, c + 1)
    const int dx = (b[r][c + 2] + 2 * b[r + 1][c + 2] + b[r + 2][c + 2]) - (b[r][c] + 2 * b[r + 1][c] + b[r + 2][c]);
    const int dy = (b[r + 2][c] + 2 * b[r + 2][c + 1] + b[r + 2][c + 2]) - (b[r][c] + 2 * b[r][c + 1] + b[r][c + 2]);
    const int m = mag[r][c];
    int cls = 0;
    if (m > 50) {
        const int ax = abs(dx), ay = abs(dy) << 15, tg = ax * T_TG22;
        bool keep;
        if (ay < tg) keep = m > mag[r][c - 1] && m >= mag[r][c + 1];
        else if (ay > tg + (ax << 16)) keep = m > mag[r - 1][c] && m >= mag[r + 1][c];
        else {
            const int s = (dx ^ dy) < 0 ? -1 : 1;
            keep = m > mag[r - 1][c - s] && m > mag[r + 1][c + s];
        }
        if (keep) cls = m > 150 ? 2 : 1;
    }
    const long long at = (long long)y * w + x;
    g_out[at] = blur[ty + 2][tx + 2];
    cls_out[at] = (unsigned char)cls;
}

// ---- front, motion: source -> grey, th = |grey - prev| > 16, med = medianBlur 5 of th, mask = 9 x 9 maximum of med (0 / 255).
// prev null: grey only.  prev and grey_out are different buffers: other workgroups read prev under this one's halo.
__global__ __launch_bounds__(256) void tile_motion_kernel(const unsigned char* src, long long pitch, int h, int w, int bgr, const unsigned char* prev,
                                                          unsigned char* grey_out, unsigned char* th_out, unsigned char* med_out,
                                                          unsigned char* mask_out) {
    __shared__ unsigned char th[T_TH + 12][T_TW + 12];   // position p -> th[clamp(p)]: the median's BORDER_REPLICATE
    __shared__ unsigned char med[T_TH + 8][T_TW + 8];    // position p -> med, 0 outside the image
    const int y0 = blockIdx.y * T_TH, x0 = blockIdx.x * T_TW;
    const int ty = threadIdx.x / T_TW, tx = threadIdx.x % T_TW;
    const int y = y0 + ty, x = x0 + tx;
    const bool inside = y < h && x < w;
    if (!prev) {
        if (inside) grey_out[(long long)y * w + x] = (unsigned char)t_grey(src, pitch, y, x, bgr);
        return;
    }
    for (int i = threadIdx.x; i < (T_TH + 12) * (T_TW + 12); i += 256) {
        const int r = i / (T_TW + 12), c = i - r * (T_TW + 12);
        const int yc = t_clamp(y0 - 6 + r, h), xc = t_clamp(x0 - 6 + c, w);
        const int v = t_grey(src, pitch, yc, xc, bgr);
        const int d = v - (int)prev[(long long)yc * w + xc];
        const int t = abs(d) > 16 ? 1 : 0;
        th[r][c] = (unsigned char)t;
        if (r >= 6 && r < 6 + T_TH && c >= 6 && c < 6 + T_TW && y0 - 6 + r < h && x0 - 6 + c < w) {
            grey_out[(long long)yc * w + xc] = (unsigned char)v;
            th_out[(long long)yc * w + xc] = (unsigned char)t;
        }
    }
    __syncthreads();
    for (int i = threadIdx.x; i < (T_TH + 8) * (T_TW + 8); i += 256) {
        const int r = i / (T_TW + 8), c = i - r * (T_TW + 8);
        const int yy = y0 - 4 + r, xx = x0 - 4 + c;
        int v = 0;
        if (yy >= 0 && yy < h && xx >= 0 && xx < w) {
            int cnt = 0;                                 // position (yy, xx) is cell (r + 2, c + 2) of `th`
#pragma unroll
            for (int dy = 0; dy < 5; ++dy)
#pragma unroll
                for (int dx = 0; dx < 5; ++dx) cnt += th[r + dy][c + dx];
            v = cnt >= 13;
        }
        med[r][c] = (unsigned char)v;
    }
    __syncthreads();
    if (!inside) return;
    int any = 0;
    for (int dy = 0; dy < 9; ++dy)
#pragma unroll
        for (int dx = 0; dx < 9; ++dx) any |= med[ty + dy][tx + dx];
    const long long at = (long long)y * w + x;
    med_out[at] = med[ty + 4][tx + 4];
    mask_out[at] = any ? 255 : 0;
}

// ---- the labelling core
__device__ __forceinline__ int uf_find(int* parent, int i, int bound, int* err) {
    for (int s = 0; s <= bound; ++s) {
        const int p = __hip_atomic_load(parent + i, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        if (p == i) return i;
        i = p;
    }
    atomicOr(err, T_ERR_FIND);
    return -1;
}
__device__ __forceinline__ void uf_union(int* parent, int a, int b, int bound, int* err) {
    for (int s = 0; s <= bound; ++s) {
        a = uf_find(parent, a, bound, err);
        b = uf_find(parent, b, bound, err);
        if (a < 0 || b < 0 || a == b) return;
        if (a < b) { const int t = a; a = b; b = t; }
        const int old = atomicMin(parent + a, b);        // a > b: links point to smaller indices
        if (old == a) return;                            // a was a root and now hangs under b
        a = old;                                         // it was not: its former parent and b are still to be joined
    }
    atomicOr(err, T_ERR_UNION);
}

enum { LABEL_CANDIDATES = 0, LABEL_MASK = 1 };
// CANDIDATES: member = cls != 0, 8-connected; the rest is unlabelled (-1).  MASK: set pixels 8-connected, clear pixels 4-connected.
// First per tile, in LDS: a workgroup labels its 8 x 32 pixels among themselves (the same union-find on a parent array of 256 local
// indices, which are ordered as the global ones, so the local root is the tile's smallest member) and writes every pixel's parent
// as the GLOBAL index of that root; it also clears the per-root bytes and boxes.  What is left for the global array is the seams.
template <int MODE>
__global__ __launch_bounds__(256) void label_tiles_kernel(const unsigned char* member, int h, int w, TileWorkspace ws) {
    __shared__ int local[T_TH * T_TW];
    __shared__ unsigned char cell[T_TH][T_TW];           // 0 clear, 1 set, 2 outside the image
    const int t = threadIdx.x, ty = t / T_TW, tx = t % T_TW;
    const int y0 = blockIdx.y * T_TH, x0 = blockIdx.x * T_TW, y = y0 + ty, x = x0 + tx;
    const bool inside = y < h && x < w;
    const int i = y * w + x;
    const int v = inside ? (member[i] ? 1 : 0) : 2;
    cell[ty][tx] = (unsigned char)v;
    local[t] = t;
    __syncthreads();
    int* err = &ws.hdr->res.error;
    const bool labelled = inside && (MODE == LABEL_MASK || v == 1);
    if (labelled) {
        if (v == 1) {
            if (tx > 0 && cell[ty][tx - 1] == 1) uf_union(local, t, t - 1, T_TH * T_TW, err);
            if (ty > 0) {
                if (cell[ty - 1][tx] == 1) uf_union(local, t, t - T_TW, T_TH * T_TW, err);
                if (tx > 0 && cell[ty - 1][tx - 1] == 1) uf_union(local, t, t - T_TW - 1, T_TH * T_TW, err);
                if (tx + 1 < T_TW && cell[ty - 1][tx + 1] == 1) uf_union(local, t, t - T_TW + 1, T_TH * T_TW, err);
            }
        } else {
            if (tx > 0 && cell[ty][tx - 1] == 0) uf_union(local, t, t - 1, T_TH * T_TW, err);
            if (ty > 0 && cell[ty - 1][tx] == 0) uf_union(local, t, t - T_TW, T_TH * T_TW, err);
        }
    }
    __syncthreads();
    if (!inside) return;
    int r = labelled ? uf_find(local, t, T_TH * T_TW, err) : -1;
    if (labelled && r < 0) r = t;                        // a tripped bound is reported; the pixel stays a valid root of its own
    ws.parent[i] = labelled ? (y0 + r / T_TW) * w + x0 + r % T_TW : -1;
    ws.fa[i] = 0;
    if (MODE == LABEL_MASK) {
        ws.fb[i] = 0;
        reinterpret_cast<int4*>(ws.box)[i] = make_int4(w, h, -1, -1);
        if (i == 0) { ws.hdr->res.x1 = w; ws.hdr->res.y1 = h; }
    }
}
// ... then across the tile seams, on the global array: only a neighbour in another tile is still to be joined
template <int MODE>
__global__ __launch_bounds__(256) void label_seams_kernel(const unsigned char* member, int h, int w, TileWorkspace ws) {
    const int n = h * w, i = blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    const int y = i / w, x = i - y * w;
    const bool top = y % T_TH == 0, left = x % T_TW == 0, right = x % T_TW == T_TW - 1;
    if (!top && !left && !right) return;
    const bool set = member[i] != 0;
    if (MODE == LABEL_CANDIDATES && !set) return;
    int* err = &ws.hdr->res.error;
    if (set) {
        if (left && x > 0 && member[i - 1]) uf_union(ws.parent, i, i - 1, n, err);
        if (y > 0) {
            if (top && member[i - w]) uf_union(ws.parent, i, i - w, n, err);
            if ((top || left) && x > 0 && member[i - w - 1]) uf_union(ws.parent, i, i - w - 1, n, err);
            if ((top || right) && x + 1 < w && member[i - w + 1]) uf_union(ws.parent, i, i - w + 1, n, err);
        }
    } else {
        if (left && x > 0 && !member[i - 1]) uf_union(ws.parent, i, i - 1, n, err);
        if (top && y > 0 && !member[i - w]) uf_union(ws.parent, i, i - w, n, err);
    }
}
// every member's parent becomes its root; (a): a strong pixel marks its root; (c): a clear pixel on the border marks its root
template <int MODE>
__global__ __launch_bounds__(256) void label_flatten_kernel(const unsigned char* member, int h, int w, TileWorkspace ws) {
    const int n = h * w, i = blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    const int v = member[i];
    if (MODE == LABEL_CANDIDATES && !v) return;
    const int r = uf_find(ws.parent, i, n, &ws.hdr->res.error);
    if (r < 0) return;
    ws.parent[i] = r;
    if (MODE == LABEL_CANDIDATES) {
        if (v == 2) ws.fa[r] = 1;
    } else {
        const int y = i / w, x = i - y * w;
        if (!v && (y == 0 || x == 0 || y == h - 1 || x == w - 1)) ws.fa[r] = 1;
    }
}
// (a) ends: edges = candidates whose root holds a strong pixel; mask = their 3 x 3 dilation inside the image
__global__ __launch_bounds__(256) void edges_dilate_kernel(int h, int w, TileWorkspace ws) {
    const int n = h * w, i = blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    const int y = i / w, x = i - y * w;
    int self = 0, any = 0;
    for (int dy = -1; dy <= 1; ++dy)
        for (int dx = -1; dx <= 1; ++dx) {
            const int yy = y + dy, xx = x + dx;
            if (yy < 0 || yy >= h || xx < 0 || xx >= w) continue;
            const int j = yy * w + xx;
            const int e = ws.cls[j] && ws.fa[ws.parent[j]];
            any |= e;
            if (dy == 0 && dx == 0) self = e;
        }
    ws.edges[i] = self ? 255 : 0;
    ws.mask[i] = any ? 255 : 0;
}
// (b) ends: boxes, external bytes, the count of components and - for tests - the labels as the header states them
__global__ __launch_bounds__(256) void component_boxes_kernel(int h, int w, TileWorkspace ws, int* labels_out) {
    const int n = h * w, i = blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    const unsigned char* m = ws.mask;
    if (!m[i]) {
        if (labels_out) labels_out[i] = -1;
        return;
    }
    const int y = i / w, x = i - y * w, r = ws.parent[i];
    if (labels_out) labels_out[i] = r;
    if (r == i) atomicAdd(&ws.hdr->res.components, 1);
    int* box = ws.box + 4 * (long long)r;
    // a set neighbour on an axis is of the same component and lies further out: only the others can hold an extreme
    const bool left = x == 0 || !m[i - 1], right = x == w - 1 || !m[i + 1], up = y == 0 || !m[i - w], down = y == h - 1 || !m[i + w];
    if (left) atomicMin(box + 0, x);
    if (up) atomicMin(box + 1, y);
    if (right) atomicMax(box + 2, x);
    if (down) atomicMax(box + 3, y);
    bool ext = x == 0 || y == 0 || x == w - 1 || y == h - 1;
    if (!ext) ext = (!m[i - 1] && ws.fa[ws.parent[i - 1]]) || (!m[i + 1] && ws.fa[ws.parent[i + 1]]) || (!m[i - w] && ws.fa[ws.parent[i - w]]) ||
                    (!m[i + w] && ws.fa[ws.parent[i + w]]);
    if (ext) ws.fb[r] = 1;
}
// _valid on every external root, in fp64 as Python computes it
__global__ __launch_bounds__(256) void select_kernel(int h, int w, TileWorkspace ws, af_tile_params p) {
    const int n = h * w, i = blockIdx.x * 256 + threadIdx.x;
    if (i >= n || !ws.mask[i] || ws.parent[i] != i || !ws.fb[i]) return;
    const int4 b = reinterpret_cast<const int4*>(ws.box)[i];
    const int ww = b.z - b.x + 1, hh = b.w - b.y + 1;
    if (ww < p.min_w || hh < p.min_h) return;
    const double ar = (double)ww / (double)hh;
    if (!(p.ar_lo <= ar && ar <= p.ar_hi && (double)((long long)ww * hh) >= p.area_min)) return;
    const int slot = atomicAdd(&ws.hdr->listed, 1);
    if (slot < AF_TILE_MAX_BOXES) ws.hdr->list[slot] = i;
    else ws.hdr->res.overflow = 1;
}
// one workgroup per survivor: its rank by root (the record order does not depend on arrival) and the sums of g over the inset roi
__global__ __launch_bounds__(256) void survivor_sums_kernel(int w, TileWorkspace ws, const unsigned char* g) {
    __shared__ long long part[2][4];
    TileHeader* hdr = ws.hdr;
    const int count = min(hdr->listed, AF_TILE_MAX_BOXES);
    if (blockIdx.x == 0 && threadIdx.x == 0) hdr->res.count = count;
    if ((int)blockIdx.x >= count) return;
    const int root = hdr->list[blockIdx.x];
    int rank = 0;
    for (int j = 0; j < count; ++j) rank += hdr->list[j] < root;
    const int4 b = reinterpret_cast<const int4*>(ws.box)[root];
    const int bw = b.z - b.x + 1, bh = b.w - b.y + 1;
    const int rw = bw > 8 && bh > 8 ? bw - 8 : 0, rh = rw ? bh - 8 : 0;
    long long s1 = 0, s2 = 0;
    if (g)
        for (long long k = threadIdx.x; k < (long long)rw * rh; k += 256) {
            const int yy = (int)(k / rw), xx = (int)(k - (long long)yy * rw);
            const long long v = g[(long long)(b.y + 4 + yy) * w + b.x + 4 + xx];
            s1 += v;
            s2 += v * v;
        }
    for (int off = 32; off > 0; off >>= 1) {              // wave64
        s1 += __shfl_down(s1, off, 64);
        s2 += __shfl_down(s2, off, 64);
    }
    if ((threadIdx.x & 63) == 0) { part[0][threadIdx.x >> 6] = s1; part[1][threadIdx.x >> 6] = s2; }
    __syncthreads();
    if (threadIdx.x == 0) {
        af_tile_box& o = hdr->res.box[rank];
        o.root = root; o.x = b.x; o.y = b.y; o.w = bw; o.h = bh; o.n_px = rw * rh;
        o.s1 = part[0][0] + part[0][1] + part[0][2] + part[0][3];
        o.s2 = part[1][0] + part[1][1] + part[1][2] + part[1][3];
    }
}
// motion ends: the union of the boxes with w h >= area_min (x2, y2 exclusive, as the reference's x + w)
__global__ __launch_bounds__(256) void motion_union_kernel(int h, int w, TileWorkspace ws, double area_min) {
    const int n = h * w, i = blockIdx.x * 256 + threadIdx.x;
    if (i >= n || !ws.mask[i] || ws.parent[i] != i) return;
    const int4 b = reinterpret_cast<const int4*>(ws.box)[i];
    const int ww = b.z - b.x + 1, hh = b.w - b.y + 1;
    if ((double)((long long)ww * hh) < area_min) return;
    af_tile_result* res = &ws.hdr->res;
    atomicMin(&res->x1, b.x);
    atomicMin(&res->y1, b.y);
    atomicMax(&res->x2, b.x + ww);
    atomicMax(&res->y2, b.y + hh);
    atomicAdd(&res->union_count, 1);
}

#define TILE_LAUNCH(kernel, grid, ...)                                        \
    do {                                                                      \
        hipLaunchKernelGGL(kernel, grid, dim3(256), 0, s, __VA_ARGS__);       \
        AF_CHECK_LAUNCH(#kernel);                                             \
    } while (0)

static int tile_check(const char* who, int h, int w, void* workspace, int64_t workspace_bytes) {
    AF_REQUIRE(h >= AF_TILE_MIN_SIDE && w >= AF_TILE_MIN_SIDE && h <= AF_TILE_MAX_SIDE && w <= AF_TILE_MAX_SIDE,
               "%s: a frame of %dx%d (both sides %d to %d)", who, w, h, AF_TILE_MIN_SIDE, AF_TILE_MAX_SIDE);
    AF_REQUIRE(workspace && ((uintptr_t)workspace & 255) == 0, "%s: the workspace is null or not 256-byte aligned", who);
    AF_REQUIRE(workspace_bytes >= tile_workspace_bytes(h, w), "%s: workspace of %lld bytes, %lld needed", who, (long long)workspace_bytes,
               (long long)tile_workspace_bytes(h, w));
    return AF_OK;
}
static int tile_source_check(const char* who, const af_tile_source* src) {
    AF_REQUIRE(src && src->pixels, "%s: null source", who);
    AF_REQUIRE(src->h > 0 && src->w > 0 && src->pitch >= (int64_t)src->w * 3 && src->pitch <= 0x7fffffff, "%s: row pitch %lld for rows of %d pixels", who,
               (long long)src->pitch, src->w);
    return AF_OK;
}
static int tile_clear(const char* who, const TileWorkspace& ws, hipStream_t s) {
    const hipError_t e = hipMemsetAsync(ws.hdr, 0, T_HEADER, s);
    if (e != hipSuccess) return set_error(AF_ERR_LAUNCH, "%s: hipMemsetAsync: %s", who, hipGetErrorString(e));
    return AF_OK;
}
static int tile_copy(const char* who, void* dst, const void* from, int64_t bytes, hipStream_t s) {
    if (!dst) return AF_OK;
    const hipError_t e = hipMemcpyAsync(dst, from, (size_t)bytes, hipMemcpyDeviceToDevice, s);
    if (e != hipSuccess) return set_error(AF_ERR_LAUNCH, "%s: hipMemcpyAsync: %s", who, hipGetErrorString(e));
    return AF_OK;
}

// the stage every sequence ends in, on ws.mask: labels, boxes, external bytes; `params`: selection and sums over g; `area_min` >= 0:
// the motion union
static int tile_components(const char* who, int h, int w, const TileWorkspace& ws, const unsigned char* g, const af_tile_params* params, double area_min,
                           const af_tile_outputs* out, hipStream_t s) {
    const int64_t n = (int64_t)h * w;
    const dim3 grid((unsigned)((n + 255) / 256));
    const dim3 tiles((w + T_TW - 1) / T_TW, (h + T_TH - 1) / T_TH);
    TILE_LAUNCH(label_tiles_kernel<LABEL_MASK>, tiles, ws.mask, h, w, ws);
    TILE_LAUNCH(label_seams_kernel<LABEL_MASK>, grid, ws.mask, h, w, ws);
    TILE_LAUNCH(label_flatten_kernel<LABEL_MASK>, grid, ws.mask, h, w, ws);
    TILE_LAUNCH(component_boxes_kernel, grid, h, w, ws, out ? (int*)out->labels : nullptr);
    if (params) {
        TILE_LAUNCH(select_kernel, grid, h, w, ws, *params);
        TILE_LAUNCH(survivor_sums_kernel, dim3(AF_TILE_MAX_BOXES), w, ws, g);
    }
    if (area_min >= 0) TILE_LAUNCH(motion_union_kernel, grid, h, w, ws, area_min);
    if (out) {
        int rc = tile_copy(who, out->mask, ws.mask, n, s);
        if (rc == AF_OK) rc = tile_copy(who, out->boxes, ws.box, 16 * n, s);
        if (rc == AF_OK) rc = tile_copy(who, out->external, ws.fb, n, s);
        if (rc != AF_OK) return rc;
    }
    return AF_OK;
}

}  // namespace af

extern "C" int64_t af_tile_workspace_bytes(int h, int w) {
    if (h < AF_TILE_MIN_SIDE || w < AF_TILE_MIN_SIDE || h > AF_TILE_MAX_SIDE || w > AF_TILE_MAX_SIDE) return -1;
    return af::tile_workspace_bytes(h, w);
}

extern "C" int af_tile_candidates_u8(const af_tile_source* src, const af_tile_params* params, void* workspace, int64_t workspace_bytes,
                                     const af_tile_outputs* out, void* stream) {
    using namespace af;
    const char* who = "tile_candidates";
    int rc = tile_source_check(who, src);
    if (rc != AF_OK) return rc;
    AF_REQUIRE(params, "%s: null params", who);
    const int h = src->h, w = src->w;
    if ((rc = tile_check(who, h, w, workspace, workspace_bytes)) != AF_OK) return rc;
    const TileWorkspace ws = carve(workspace, h, w);
    hipStream_t s = (hipStream_t)stream;
    if ((rc = tile_clear(who, ws, s)) != AF_OK) return rc;
    const int64_t n = (int64_t)h * w;
    const dim3 grid((unsigned)((n + 255) / 256)), tiles((w + T_TW - 1) / T_TW, (h + T_TH - 1) / T_TH);
    TILE_LAUNCH(tile_front_kernel, tiles, (const unsigned char*)src->pixels, (long long)src->pitch, h, w, src->bgr, ws.g, ws.cls);
    TILE_LAUNCH(label_tiles_kernel<LABEL_CANDIDATES>, tiles, ws.cls, h, w, ws);
    TILE_LAUNCH(label_seams_kernel<LABEL_CANDIDATES>, grid, ws.cls, h, w, ws);
    TILE_LAUNCH(label_flatten_kernel<LABEL_CANDIDATES>, grid, ws.cls, h, w, ws);
    TILE_LAUNCH(edges_dilate_kernel, grid, h, w, ws);
    if (out) {
        rc = tile_copy(who, out->g, ws.g, n, s);
        if (rc == AF_OK) rc = tile_copy(who, out->cls, ws.cls, n, s);
        if (rc == AF_OK) rc = tile_copy(who, out->edges, ws.edges, n, s);
        if (rc != AF_OK) return rc;
    }
    return tile_components(who, h, w, ws, ws.g, params, -1.0, out, s);
}

extern "C" int af_tile_motion_u8(const af_tile_source* src, const void* prev_grey, void* grey, double area_min, void* workspace,
                                 int64_t workspace_bytes, const af_tile_outputs* out, void* stream) {
    using namespace af;
    const char* who = "tile_motion";
    int rc = tile_source_check(who, src);
    if (rc != AF_OK) return rc;
    AF_REQUIRE(grey && grey != prev_grey, "%s: the grey image is null or is the previous one", who);
    AF_REQUIRE(area_min >= 0, "%s: area_min %g", who, area_min);
    const int h = src->h, w = src->w;
    if ((rc = tile_check(who, h, w, workspace, workspace_bytes)) != AF_OK) return rc;
    const TileWorkspace ws = carve(workspace, h, w);
    hipStream_t s = (hipStream_t)stream;
    if ((rc = tile_clear(who, ws, s)) != AF_OK) return rc;
    const int64_t n = (int64_t)h * w;
    const dim3 tiles((w + T_TW - 1) / T_TW, (h + T_TH - 1) / T_TH);
    TILE_LAUNCH(tile_motion_kernel, tiles, (const unsigned char*)src->pixels, (long long)src->pitch, h, w, src->bgr, (const unsigned char*)prev_grey,
                (unsigned char*)grey, ws.cls, ws.edges, ws.mask);
    if (out && (rc = tile_copy(who, out->g, grey, n, s)) != AF_OK) return rc;
    if (!prev_grey) return AF_OK;
    if (out) {
        rc = tile_copy(who, out->cls, ws.cls, n, s);
        if (rc == AF_OK) rc = tile_copy(who, out->edges, ws.edges, n, s);
        if (rc != AF_OK) return rc;
    }
    return tile_components(who, h, w, ws, nullptr, nullptr, area_min, out, s);
}

extern "C" int af_tile_components_u8(const void* mask, int64_t pitch, int h, int w, const void* g, const af_tile_params* params, void* workspace,
                                     int64_t workspace_bytes, const af_tile_outputs* out, void* stream) {
    using namespace af;
    const char* who = "tile_components";
    AF_REQUIRE(mask, "%s: null mask", who);
    int rc = tile_check(who, h, w, workspace, workspace_bytes);
    if (rc != AF_OK) return rc;
    AF_REQUIRE(pitch >= w, "%s: row pitch %lld for rows of %d bytes", who, (long long)pitch, w);
    const TileWorkspace ws = carve(workspace, h, w);
    hipStream_t s = (hipStream_t)stream;
    if ((rc = tile_clear(who, ws, s)) != AF_OK) return rc;
    const hipError_t e = hipMemcpy2DAsync(ws.mask, (size_t)w, mask, (size_t)pitch, (size_t)w, (size_t)h, hipMemcpyDeviceToDevice, s);
    if (e != hipSuccess) return set_error(AF_ERR_LAUNCH, "%s: hipMemcpy2DAsync: %s", who, hipGetErrorString(e));
    return tile_components(who, h, w, ws, (const unsigned char*)g, params, -1.0, out, s);
}
