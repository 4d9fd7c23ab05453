// The stratified-bootstrap index rows of numpy's own PCG64 stream, drawn on the device (include/af_hip.h, "bootstrap rows"; DESIGN 26;
// the numpy statement is tests/pcg64_ref.py).  Integer arithmetic only: a 128-bit LCG with an XSL-RR output, a 32-bit word stream and
// Lemire's rejection rule.  Which bound applies to word k depends on how many words before k were rejected, so a call is three launches
// on one stream and no workgroup waits on another:
//   scan     over the first T + ceil(max_rejects / 2) words (T: the words a call accepts): a thread jumps to its chunk of DR_SCAN words
//            and appends those that either bound would reject to a list (atomic append);
//   resolve  ONE workgroup sorts the list and one thread walks it in word order with the running count s of true rejections: word k
//            has accepted-index k - s, which says which bound applies there; -> the sorted true rejections, consumed = T + s and the
//            half-word numpy would hold buffered;
//   emit     a thread owns DR_EMIT consecutive ACCEPTED words: its first word is x + #{i : rej[i] - i <= x} (a binary search), it jumps
//            there, walks on, skips the listed words, and the workgroup stores its tile through LDS in numpy's order.
// Every loop is bounded by a constant or by an argument the host checked (rows, counts, max_rejects); none runs on the stream's data.
#include <algorithm>

#include "af_common.h"

namespace af {

typedef unsigned __int128 u128;
typedef unsigned long long u64;

constexpr int DR_T = 256;                    // threads of every phase
constexpr int DR_SCAN = 32;                  // words a scan thread walks: 16 outputs behind one jump
constexpr int DR_EMIT = 16;                  // accepted words an emit thread owns
constexpr int DR_TILE = DR_T * DR_EMIT;
constexpr int DR_JUMPS = 32;                 // s -> A s + C over 2^i outputs, i < 32: a call stays below 2^31 outputs
constexpr int DR_HEAD = 64;                  // bytes of the workspace in front of the lists
static_assert((AF_DRAW_MAX_REJECTS & (AF_DRAW_MAX_REJECTS - 1)) == 0, "draw: the sort wants a power of two");
static_assert(AF_DRAW_MAX_REJECTS * 8 + 1024 <= kLdsBudget, "draw: the list does not fit the LDS");

struct DrawJump { u64 a_lo, a_hi, c_lo, c_hi; };
struct DrawArgs {
    DrawJump jump[DR_JUMPS];
    u64 s_lo, s_hi, inc_lo, inc_hi;
    unsigned has, uinteger;
    unsigned m_a, m_b, thr_a, thr_b;
    int c_a, c_b, ca_eff, cb_eff;            // eff: 0 where the bound is 1 - such a segment takes no word
    int rows, max_rejects;
    long long T, K;                          // accepted words of the call; words the scan covers, T + ceil(max_rejects / 2)
    const int *items_a, *items_b;
    int* idx;
    long long* row_off;
    long long row_base;
    af_draw_result* res;
    unsigned* n_list;                        // workspace: the append counter,
    u64* list;                               //   max_rejects entries (word index << 2 | rejected under b << 1 | rejected under a),
    unsigned* rej;                           //   max_rejects word indices of the true rejections, ascending
};

__host__ __device__ static inline u128 dr_u128(u64 hi, u64 lo) { return ((u128)hi << 64) | lo; }
__host__ __device__ static inline u128 dr_mult() { return dr_u128(0x2360ED051FC65DA4ull, 0x4385DF649FCCF645ull); }

__device__ static inline u64 dr_output(u128 s) {                                  // XSL-RR 128/64
    const u64 hi = (u64)(s >> 64), lo = (u64)s, x = hi ^ lo;
    const unsigned r = (unsigned)(hi >> 58);
    return (x >> r) | (x << ((64 - r) & 63));
}

__device__ static inline u128 dr_jump(const DrawArgs& a, u128 s, unsigned outputs) {
    for (int i = 0; i < DR_JUMPS; ++i)
        if ((outputs >> i) & 1u) s = dr_u128(a.jump[i].a_hi, a.jump[i].a_lo) * s + dr_u128(a.jump[i].c_hi, a.jump[i].c_lo);
    return s;
}

// the 32-bit word stream: w[0] is the buffered half where there is one; output j (j >= 1) gives its low half, then its high half
struct DrawCursor {
    u128 s;
    u64 out;
    unsigned k;
    __device__ unsigned seek(const DrawArgs& a, unsigned k0) {
        k = k0;
        s = dr_u128(a.s_hi, a.s_lo);
        out = 0;
        if (a.has && k0 == 0) return a.uinteger;
        const unsigned q = k0 - a.has;
        s = dr_jump(a, s, q / 2 + 1);
        out = dr_output(s);
        return (q & 1u) ? (unsigned)(out >> 32) : (unsigned)out;
    }
    __device__ unsigned next(const DrawArgs& a) {
        ++k;
        if ((k - a.has) & 1u) return (unsigned)(out >> 32);
        s = s * dr_mult() + dr_u128(a.inc_hi, a.inc_lo);
        out = dr_output(s);
        return (unsigned)out;
    }
};

__global__ __launch_bounds__(DR_T) void draw_scan_kernel(DrawArgs a) {
    const u64 k0 = ((u64)blockIdx.x * DR_T + threadIdx.x) * DR_SCAN;
    if ((long long)k0 >= a.K) return;
    const int n = (int)min((long long)DR_SCAN, a.K - (long long)k0);
    DrawCursor c;
    unsigned w = c.seek(a, (unsigned)k0);
    for (int i = 0; i < n; ++i) {
        if (i) w = c.next(a);
        const unsigned flags = (a.ca_eff && w * a.m_a < a.thr_a ? 1u : 0u) | (a.cb_eff && w * a.m_b < a.thr_b ? 2u : 0u);
        if (flags) {
            const unsigned at = atomicAdd(a.n_list, 1u);
            if (at < (unsigned)a.max_rejects) a.list[at] = ((k0 + (u64)i) << 2) | flags;
        }
    }
}

__global__ __launch_bounds__(DR_T) void draw_resolve_kernel(DrawArgs a) {
    extern __shared__ __attribute__((aligned(16))) unsigned char dr_lds[];
    u64* key = reinterpret_cast<u64*>(dr_lds);
    const int t = threadIdx.x;
    const unsigned listed = *a.n_list;
    int overflow = listed > (unsigned)a.max_rejects;                               // the list is incomplete: nothing below reads it
    const int n = overflow ? 0 : (int)listed;
    int p2 = 1;
    for (int i = 0; i < 14 && p2 < n; ++i) p2 <<= 1;                                // n <= max_rejects <= 2^13
    for (int i = t; i < p2; i += DR_T) key[i] = i < n ? a.list[i] : ~0ull;
    __syncthreads();
    for (int size = 2; size <= p2; size <<= 1)                                     // bitonic, ascending; the keys are distinct
        for (int stride = size >> 1; stride > 0; stride >>= 1) {
            for (int i = t; i < p2 / 2; i += DR_T) {
                const int lo = 2 * i - (i & (stride - 1)), hi = lo + stride;
                const u64 x = key[lo], y = key[hi];
                if ((x > y) == ((lo & size) == 0)) {
                    key[lo] = y;
                    key[hi] = x;
                }
            }
            __syncthreads();
        }
    if (t != 0) return;
    unsigned s = 0;
    const unsigned L = (unsigned)(a.ca_eff + a.cb_eff), tail = (unsigned)(a.K - a.T);
    for (int i = 0; i < n && L > 0; ++i) {
        const u64 e = key[i], k = e >> 2;
        const long long acc = (long long)k - (long long)s;
        if (acc >= a.T) break;                                                     // behind the last accepted word: not consumed
        const bool in_a = (unsigned)acc % L < (unsigned)a.ca_eff;
        if (e & (in_a ? 1u : 2u)) {
            if (s == tail) {                                                       // the draw would run past the words that were scanned
                overflow = 1;
                break;
            }
            a.rej[s++] = (unsigned)k;
        }
    }
    af_draw_result r = {};
    r.consumed = overflow ? -1 : a.T + (long long)s;
    r.has_uint32 = (int)a.has;
    r.uinteger = a.uinteger;
    if (r.consumed > 0) {                                                          // numpy's buffer after the last word
        const long long made = r.consumed - (long long)a.has;                      // words that came out of 64-bit outputs
        r.outputs = (made + 1) / 2;
        r.has_uint32 = (int)(made & 1);
        if (r.outputs > 0) r.uinteger = (unsigned)(dr_output(dr_jump(a, dr_u128(a.s_hi, a.s_lo), (unsigned)r.outputs)) >> 32);
    }
    r.rejected = overflow ? 0 : (int)s;
    r.listed = listed > 0x7fffffffu ? 0x7fffffff : (int)listed;
    r.error = overflow;
    *a.res = r;
}

__global__ __launch_bounds__(DR_T) void draw_emit_kernel(DrawArgs a) {
    __shared__ unsigned val[DR_T * (DR_EMIT + 1)];
    const int t = threadIdx.x;
    const long long gid = (long long)blockIdx.x * DR_T + t, nthreads = (long long)gridDim.x * DR_T;
    const long long row_len = (long long)a.c_a + a.c_b;
    for (long long r = gid; r <= a.rows; r += nthreads) a.row_off[r] = a.row_base + r * row_len;
    int bad = 0;
    if (a.ca_eff != a.c_a) {                                                       // bound 1: `count` copies of the one item, no word
        const int fill = a.items_a ? a.items_a[0] : 0;
        for (long long i = gid; i < (long long)a.rows * a.c_a; i += nthreads) a.idx[i / a.c_a * row_len + i % a.c_a] = fill;
    }
    if (a.cb_eff != a.c_b) {
        const int fill = a.items_b ? a.items_b[0] : 0;
        for (long long i = gid; i < (long long)a.rows * a.c_b; i += nthreads) a.idx[i / a.c_b * row_len + a.c_a + i % a.c_b] = fill;
    }
    const long long X0 = (long long)blockIdx.x * DR_TILE;
    if (a.res->error != 0 || X0 >= a.T) return;                                    // the same answer for the whole workgroup
    const unsigned L = (unsigned)(a.ca_eff + a.cb_eff), n_rej = (unsigned)a.res->rejected;
    const long long x = X0 + (long long)t * DR_EMIT;
    const int cnt = (int)max(0ll, min((long long)DR_EMIT, a.T - x));
    if (cnt > 0) {
        unsigned lo = 0, hi = n_rej;
        for (int it = 0; it < 14 && lo < hi; ++it) {                                // n_rej <= max_rejects <= 2^13
            const unsigned mid = (lo + hi) / 2;
            if ((long long)a.rej[mid] - (long long)mid <= x) lo = mid + 1; else hi = mid;
        }
        unsigned ri = lo, next_rej = ri < n_rej ? a.rej[ri] : ~0u;
        unsigned pos = (unsigned)x % L;
        DrawCursor c;
        unsigned w = c.seek(a, (unsigned)x + ri);
        int e = 0;
        for (int step = 0; step < DR_EMIT + a.max_rejects; ++step) {
            if (step) w = c.next(a);
            if (c.k == next_rej) {
                ++ri;
                next_rej = ri < n_rej ? a.rej[ri] : ~0u;
                continue;
            }
            val[t * (DR_EMIT + 1) + e] = __umulhi(w, pos < (unsigned)a.ca_eff ? a.m_a : a.m_b);
            if (++pos == L) pos = 0;
            if (++e == cnt) break;
        }
    }
    __syncthreads();
    for (int e = 0; e < DR_EMIT; ++e) {
        const int i = e * DR_T + t;
        const long long xx = X0 + i;
        if (xx >= a.T) break;
        const unsigned v = val[i / DR_EMIT * (DR_EMIT + 1) + i % DR_EMIT];
        const unsigned row = (unsigned)xx / L, pos = (unsigned)xx % L;
        const bool in_a = pos < (unsigned)a.ca_eff;
        const long long o = row * row_len + (in_a ? (long long)pos : (long long)a.c_a + (pos - (unsigned)a.ca_eff));
        const int* items = in_a ? a.items_a : a.items_b;
        if (!items) a.idx[o] = (int)v;                                             // value mode: the uint32 draw itself
        else if (v < (in_a ? a.m_a : a.m_b)) a.idx[o] = items[v];
        else ++bad;                                                                // hi32(w m) < m: cannot happen
    }
    if (bad) atomicAdd(&a.res->error, bad);
}

static int64_t draw_workspace(int max_rejects) { return DR_HEAD + (int64_t)max_rejects * 12; }

}  // namespace af

extern "C" int64_t af_pcg64_draw_workspace_bytes(int max_rejects) {
    if (max_rejects < 1 || max_rejects > AF_DRAW_MAX_REJECTS) return 0;
    return af::draw_workspace(max_rejects);
}

extern "C" int af_pcg64_draw_rows(const af_pcg64_state* start, int64_t bound_a, int count_a, int64_t bound_b, int count_b, int rows,
                                  const int32_t* items_a, const int32_t* items_b, int max_rejects, int32_t* idx, int64_t* row_off,
                                  int64_t row_base, af_draw_result* result, void* workspace, int64_t workspace_bytes, void* stream) {
    using namespace af;
    const char* who = "pcg64_draw_rows";
    AF_REQUIRE(start && row_off && result && workspace, "%s: null state, row table, result or workspace pointer", who);
    AF_REQUIRE(bound_a >= 1 && bound_a <= 0xffffffffll && bound_b >= 1 && bound_b <= 0xffffffffll,
               "%s: bounds %lld and %lld (1 to 2^32 - 1: numpy draws the bound 2^32 another way)", who, (long long)bound_a, (long long)bound_b);
    AF_REQUIRE(count_a >= 0 && count_b >= 0 && rows >= 0, "%s: counts %d and %d, %d rows", who, count_a, count_b, rows);
    AF_REQUIRE((int64_t)rows * ((int64_t)count_a + count_b) < 0x80000000ll, "%s: %d rows of %d + %d draws (below 2^31 in all)", who, rows, count_a,
               count_b);
    AF_REQUIRE(idx || (int64_t)rows * ((int64_t)count_a + count_b) == 0, "%s: null index buffer", who);
    AF_REQUIRE(!items_a || bound_a == count_a, "%s: items_a: a bound of %lld over %d items", who, (long long)bound_a, count_a);
    AF_REQUIRE(!items_b || bound_b == count_b, "%s: items_b: a bound of %lld over %d items", who, (long long)bound_b, count_b);
    AF_REQUIRE(max_rejects >= 1 && max_rejects <= AF_DRAW_MAX_REJECTS, "%s: a rejection list of %d entries (1 to %d)", who, max_rejects,
               AF_DRAW_MAX_REJECTS);
    AF_REQUIRE(workspace_bytes >= draw_workspace(max_rejects), "%s: a workspace of %lld bytes, %lld needed", who, (long long)workspace_bytes,
               (long long)draw_workspace(max_rejects));
    AF_REQUIRE((start->has_uint32 == 0 || start->has_uint32 == 1) && (start->inc_lo & 1), "%s: has_uint32 %d, increment %s", who,
               start->has_uint32, (start->inc_lo & 1) ? "odd" : "even");
    AF_REQUIRE(row_base >= 0, "%s: row base %lld", who, (long long)row_base);
    AF_REQUIRE(((uintptr_t)workspace & 7) == 0 && ((uintptr_t)row_off & 7) == 0 && ((uintptr_t)result & 7) == 0,
               "%s: workspace, row table and result are 8-byte aligned", who);
    hipStream_t s = (hipStream_t)stream;
    DrawArgs a = {};
    u128 A = dr_mult(), Cc = dr_u128(start->inc_hi, start->inc_lo);
    for (int i = 0; i < DR_JUMPS; ++i) {                                           // f o f: s -> A A s + (A + 1) C
        a.jump[i] = {(u64)A, (u64)(A >> 64), (u64)Cc, (u64)(Cc >> 64)};
        Cc = (A + 1) * Cc;
        A = A * A;
    }
    a.s_lo = start->state_lo; a.s_hi = start->state_hi; a.inc_lo = start->inc_lo; a.inc_hi = start->inc_hi;
    a.has = (unsigned)start->has_uint32; a.uinteger = start->uinteger;
    a.m_a = (unsigned)bound_a; a.m_b = (unsigned)bound_b;
    a.thr_a = (unsigned)(0x100000000ull % (u64)bound_a); a.thr_b = (unsigned)(0x100000000ull % (u64)bound_b);
    a.c_a = count_a; a.c_b = count_b;
    a.ca_eff = bound_a == 1 ? 0 : count_a; a.cb_eff = bound_b == 1 ? 0 : count_b;
    a.rows = rows; a.max_rejects = max_rejects;
    a.T = (long long)rows * ((long long)a.ca_eff + a.cb_eff);
    a.K = a.T + (max_rejects + 1) / 2;
    a.items_a = items_a; a.items_b = items_b; a.idx = idx; a.row_off = (long long*)row_off; a.row_base = row_base; a.res = result;
    unsigned char* ws = (unsigned char*)workspace;
    a.n_list = (unsigned*)ws;
    a.list = (u64*)(ws + DR_HEAD);
    a.rej = (unsigned*)(ws + DR_HEAD + (size_t)max_rejects * 8);
    hipError_t e = hipMemsetAsync(ws, 0, DR_HEAD, s);
    if (e != hipSuccess) return set_error(AF_ERR_LAUNCH, "%s: hipMemsetAsync: %s", who, hipGetErrorString(e));
    if (a.T > 0) {
        const long long per = (long long)DR_T * DR_SCAN;
        hipLaunchKernelGGL(draw_scan_kernel, dim3((unsigned)((a.K + per - 1) / per)), dim3(DR_T), 0, s, a);
        AF_CHECK_LAUNCH(who);
    }
    int p2 = 1;
    while (p2 < max_rejects) p2 <<= 1;
    AF_SET_MAX_LDS(draw_resolve_kernel, AF_DRAW_MAX_REJECTS * 8, who);
    hipLaunchKernelGGL(draw_resolve_kernel, dim3(1), dim3(DR_T), (size_t)p2 * 8, s, a);
    AF_CHECK_LAUNCH(who);
    const long long fill = (long long)rows * std::max(a.ca_eff != count_a ? count_a : 0, a.cb_eff != count_b ? count_b : 0);
    const long long blocks = std::max(1ll, std::max((a.T + DR_TILE - 1) / DR_TILE, (fill + DR_TILE - 1) / DR_TILE));
    hipLaunchKernelGGL(draw_emit_kernel, dim3((unsigned)blocks), dim3(DR_T), 0, s, a);
    AF_CHECK_LAUNCH(who);
    return AF_OK;
}
