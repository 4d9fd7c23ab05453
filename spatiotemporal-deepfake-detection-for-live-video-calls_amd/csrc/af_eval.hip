// AUROC / average precision of many index rows over one scored pool, on integers (include/af_hip.h, "rank metrics"; the
// numpy statement is tests/evalsuite_ref.py).  One workgroup of AF_RANK_THREADS threads per row:
//   1  the draws of every rank are counted in LDS with integer atomics (any order gives the same counts);
//   2  a thread owns the contiguous ranks [t chunk, (t + 1) chunk), chunk = ceil(n / threads): it sums its positives and negatives and
//      notes what lies in front of the LAST tie group that starts in its chunk; a scan over the threads turns both into prefixes;
//   3  it walks its chunk again with the running prefix (tp, fp).  A group's term is formed at the group's last rank; the prefix at the
//      group's first rank - the carry across chunk and wave seams - is its own when the group starts in the chunk, and else that of
//      the nearest earlier thread in whose chunk a group starts;
//   4  u2 is an int64 sum (order-free); ap_sum is the thread's terms in rank order, then the tree p[i] += p[i + h].
// fp64 products, quotients and sums are rounded once each: nothing in this file is contracted.
#include "af_common.h"

#pragma clang fp contract(off)

namespace af {

constexpr int RK_T = AF_RANK_THREADS;

struct RankScratch {
    int2 scan[2][RK_T];                      // (pos, neg) per thread, double-buffered
    int sp_tp[RK_T], sp_fp[RK_T], has[RK_T]; // the prefix in front of the last group that starts in thread t's chunk, and whether one does
    double ap[RK_T];
    unsigned long long u2;
    int tp_cut, fp_cut, err, reserved;
};
constexpr int RK_SCRATCH = (int)((sizeof(RankScratch) + 15) & ~(size_t)15);
static_assert(RK_SCRATCH + AF_RANK_MAX_POOL * 4 <= kLdsBudget, "rank metrics: the counts do not fit the LDS");
static_assert((RK_T & (RK_T - 1)) == 0, "rank metrics: the tree wants a power of two");

struct RankArgs {
    const int* rank_of_item;
    const int* group_of_rank;
    const unsigned char* label_of_rank;
    const int* idx;
    const long long* row_off;                // null: one row, idx[0 .. n_idx)
    long long n_idx;
    int n, cut;
    af_rank_row* out;                        // rows
    int *tps, *fps, *n_groups;               // the curve form
    int* error;
};

template <bool CURVE>
__global__ __launch_bounds__(RK_T) void rank_rows_kernel(RankArgs a) {
#pragma clang fp contract(off)
    extern __shared__ __attribute__((aligned(16))) unsigned char rk_lds[];
    RankScratch& sc = *reinterpret_cast<RankScratch*>(rk_lds);
    int* cnt = reinterpret_cast<int*>(rk_lds + RK_SCRATCH);
    const int t = threadIdx.x, n = a.n;
    int bad = 0;
    long long lo = 0, hi = a.n_idx;
    if (!CURVE) {
        lo = a.row_off[blockIdx.x];
        hi = a.row_off[blockIdx.x + 1];
        if (lo < 0 || hi < lo || hi > a.n_idx) {             // a row that leaves the index buffer: read nothing
            bad = t == 0;
            lo = hi = 0;
        }
    }
    for (int r = t; r < n; r += RK_T) cnt[r] = 0;
    if (t == 0) {
        sc.u2 = 0;
        sc.tp_cut = sc.fp_cut = sc.err = 0;
    }
    __syncthreads();
    // 1: the counts
    for (long long i = lo + t; i < hi; i += RK_T) {
        const int item = a.idx[i];
        int r = -1;
        if ((unsigned)item < (unsigned)n) r = a.rank_of_item[item];
        if ((unsigned)r < (unsigned)n) atomicAdd(&cnt[r], 1);
        else ++bad;
    }
    __syncthreads();
    // 2: a thread's sums
    const int chunk = (n + RK_T - 1) / RK_T;
    const int r0 = min(t * chunk, n), r1 = min(r0 + chunk, n);
    int pos = 0, neg = 0, rel_pos = 0, rel_neg = 0, tpc = 0, fpc = 0, has = 0;
    {
        int gprev = r0 > 0 && r0 < r1 ? a.group_of_rank[r0 - 1] : 0;
        for (int r = r0; r < r1; ++r) {
            const int g = a.group_of_rank[r], c = cnt[r];
            const bool lab = a.label_of_rank[r] != 0;
            if (r == 0 || g != gprev) {
                has = 1;
                rel_pos = pos;
                rel_neg = neg;
            }
            gprev = g;
            if (lab) pos += c; else neg += c;
            if (r < a.cut) { if (lab) tpc += c; else fpc += c; }
        }
    }
    int src = 0;
    sc.scan[0][t] = make_int2(pos, neg);
    __syncthreads();
    for (int d = 1; d < RK_T; d <<= 1) {
        int2 v = sc.scan[src][t];
        if (t >= d) {
            const int2 w = sc.scan[src][t - d];
            v.x += w.x;
            v.y += w.y;
        }
        sc.scan[src ^ 1][t] = v;
        __syncthreads();
        src ^= 1;
    }
    const int2 incl = sc.scan[src][t], total = sc.scan[src][RK_T - 1];
    const int ex_pos = incl.x - pos, ex_neg = incl.y - neg, P = total.x, N = total.y;
    sc.has[t] = has;
    sc.sp_tp[t] = ex_pos + rel_pos;
    sc.sp_fp[t] = ex_neg + rel_neg;
    if (tpc) atomicAdd(&sc.tp_cut, tpc);
    if (fpc) atomicAdd(&sc.fp_cut, fpc);
    if (bad) atomicAdd(&sc.err, bad);
    __syncthreads();
    // 3: the groups that end in this chunk
    int tp = ex_pos, fp = ex_neg, gs_tp = ex_pos, gs_fp = ex_neg;
    if (r0 > 0 && r0 < r1 && a.group_of_rank[r0] == a.group_of_rank[r0 - 1]) {     // the group came in over the seam
        int u = t - 1;
        while (u > 0 && !sc.has[u]) --u;                                         // thread 0 owns rank 0, where a group starts
        gs_tp = sc.sp_tp[u];
        gs_fp = sc.sp_fp[u];
    }
    long long u2 = 0;
    double ap = 0.0;
    int bad_group = 0;
    for (int r = r0; r < r1; ++r) {
        const int c = cnt[r], g = a.group_of_rank[r];
        if (a.label_of_rank[r] != 0) tp += c; else fp += c;
        if (r == n - 1 || a.group_of_rank[r + 1] != g) {
            const int pos_g = tp - gs_tp, neg_g = fp - gs_fp;
            if (pos_g > 0) {
                u2 += (long long)pos_g * (2ll * (N - fp) + neg_g);
                const double precision = (double)tp / (double)(tp + fp);
                const double term = (double)pos_g * precision;
                ap = ap + term;
            }
            if (CURVE) {
                if ((unsigned)g < (unsigned)n) {
                    a.tps[g] = tp;
                    a.fps[g] = fp;
                } else {
                    ++bad_group;
                }
            }
            gs_tp = tp;
            gs_fp = fp;
        }
    }
    // 4: the sums
    sc.ap[t] = ap;
    if (u2) atomicAdd(&sc.u2, (unsigned long long)u2);
    if (bad_group) atomicAdd(&sc.err, bad_group);
    __syncthreads();
    for (int h = RK_T / 2; h >= 1; h >>= 1) {
        if (t < h) sc.ap[t] = sc.ap[t] + sc.ap[t + h];
        __syncthreads();
    }
    if (t == 0) {
        int err = sc.err;
        if (CURVE) {
            const int groups = a.group_of_rank[n - 1] + 1;
            if (groups < 1 || groups > n) ++err;
            *a.n_groups = groups;
        } else {
            af_rank_row o;
            o.u2 = (long long)sc.u2;
            o.ap_sum = sc.ap[0];
            o.P = P;
            o.N = N;
            o.tp_cut = sc.tp_cut;
            o.fp_cut = sc.fp_cut;
            a.out[blockIdx.x] = o;
        }
        if (err) atomicAdd(a.error, err);
    }
}

template <bool CURVE>
static int rank_launch(const char* who, const RankArgs& a, int rows, hipStream_t s) {
    hipError_t e = hipMemsetAsync(a.error, 0, sizeof(int), s);
    if (e != hipSuccess) return set_error(AF_ERR_LAUNCH, "%s: hipMemsetAsync: %s", who, hipGetErrorString(e));
    if (rows == 0) return AF_OK;
    AF_SET_MAX_LDS(rank_rows_kernel<CURVE>, RK_SCRATCH + AF_RANK_MAX_POOL * 4, who);
    hipLaunchKernelGGL(rank_rows_kernel<CURVE>, dim3((unsigned)rows), dim3(RK_T), (size_t)(RK_SCRATCH + a.n * 4), s, a);
    AF_CHECK_LAUNCH(who);
    return AF_OK;
}

static int rank_check(const char* who, const void* rank_of_item, const void* group_of_rank, const void* label_of_rank, int n, const void* idx,
                      int64_t n_idx, const void* error) {
    AF_REQUIRE(rank_of_item && group_of_rank && label_of_rank && error, "%s: null pool or error pointer", who);
    AF_REQUIRE(n >= 1 && n <= AF_RANK_MAX_POOL, "%s: a pool of %d items (1 to %d: the counts live in LDS)", who, n, AF_RANK_MAX_POOL);
    AF_REQUIRE(n_idx >= 0 && n_idx <= 0x7fffffffll, "%s: %lld indices", who, (long long)n_idx);
    AF_REQUIRE(idx || n_idx == 0, "%s: null index buffer", who);
    return AF_OK;
}

}  // namespace af

extern "C" int af_rank_metrics_rows(const int32_t* rank_of_item, const int32_t* group_of_rank, const uint8_t* label_of_rank, int n,
                                    const int32_t* idx, int64_t n_idx, const int64_t* row_off, int rows, int cut, af_rank_row* out,
                                    int32_t* error, void* stream) {
    using namespace af;
    const char* who = "rank_metrics_rows";
    const int rc = rank_check(who, rank_of_item, group_of_rank, label_of_rank, n, idx, n_idx, error);
    if (rc != AF_OK) return rc;
    AF_REQUIRE(rows >= 0 && (rows == 0 || (row_off && out)), "%s: %d rows, null row table or output", who, rows);
    AF_REQUIRE(cut >= 0 && cut <= n, "%s: cut %d of a pool of %d", who, cut, n);
    RankArgs a = {};
    a.rank_of_item = rank_of_item; a.group_of_rank = group_of_rank; a.label_of_rank = label_of_rank; a.idx = idx;
    a.row_off = (const long long*)row_off; a.n_idx = n_idx; a.n = n; a.cut = cut; a.out = out; a.error = error;
    return rank_launch<false>(who, a, rows, (hipStream_t)stream);
}

extern "C" int af_rank_curve(const int32_t* rank_of_item, const int32_t* group_of_rank, const uint8_t* label_of_rank, int n, const int32_t* idx,
                             int64_t n_idx, int32_t* tps, int32_t* fps, int32_t* n_groups, int32_t* error, void* stream) {
    using namespace af;
    const char* who = "rank_curve";
    const int rc = rank_check(who, rank_of_item, group_of_rank, label_of_rank, n, idx, n_idx, error);
    if (rc != AF_OK) return rc;
    AF_REQUIRE(tps && fps && n_groups, "%s: null output", who);
    RankArgs a = {};
    a.rank_of_item = rank_of_item; a.group_of_rank = group_of_rank; a.label_of_rank = label_of_rank; a.idx = idx;
    a.n_idx = n_idx; a.n = n; a.cut = 0; a.tps = tps; a.fps = fps; a.n_groups = n_groups; a.error = error;
    return rank_launch<true>(who, a, 1, (hipStream_t)stream);
}
