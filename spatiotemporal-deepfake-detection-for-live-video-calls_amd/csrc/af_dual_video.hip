// dualrun at video level: what the reference does around DualEncoderAU_LMK.forward in numpy / torch host code.
//
// af_dual_clip_features - one workgroup per clip, per clip in the reference's order:
//   landmarks  dualrun/data/make_lmk_features.py:39-52, 152-187: the 66 KEY_LANDMARKS_IDXS points (the last three are the nose tip 1
//              and the mouth corners 78, 308) minus the nose; scale = ||ml - mr||; a frame whose scale is not finite or < 1e-8 is
//              dropped and the survivors compacted in order; divided by scale + 1e-6.  rot_invariant (:145-150, 173-176), collate_pad's
//              zero rows (data/vox_ds.py:19-26) and landmarks without AUs: af_dual_clip_features_ex, statement tests/lmkdisc_ref.py.
//   AUs        dualrun/data/make_au_features.py:41-53: X | diff(X, prepend=X[:1]) | the same of that, along the feature axis.
//   fixT       dualrun/rgb/fusion.py:331-336, per modality on its own row count: more rows than T keep the centred T, fewer repeat
//              the last row.
//   normalize_features  fusion.py:79-114 as written: clip = mean and unbiased std over the T rows, clamp_min(1e-6); global = the
//              given mean, std floored at 1e-6 twice (load_norm_stats, then clamp_min); nan_to_num on BOTH modalities in both
//              modes, also on the one `apply` leaves out; none = untouched, NaN included.
// Arithmetic is the statement tests/dualvideo_ref.py bit for bit: fp32 throughout; scale = sqrt(fl(dx dx) + fl(dy dy)); the mean is
// the sequential sum over t = 0..T-1 starting from +0, divided by T; the std is two-pass: deviations from that mean, sequential sum
// of their squares, / (T - 1), sqrt.  Lanes run over features and the T-loop runs inside a lane, so the order is fixed.  A fused
// multiply-add would change the sums of squares, so the file sits below `#pragma clang fp contract(off)` (DESIGN 19 has the
// reason hipcc's __fmul_rn does not do); divides and square roots are IEEE correctly rounded, which is hipcc's default
// (-fhip-fp32-correctly-rounded-divide-sqrt) and what build.py's flags leave on; fp32 denormals are kept (gfx9 default).
//
// af_dual_video_reduce - one workgroup per video: fusion.track_reduce / agg_video (fusion.py:118-130) on logits, or
// cli/best.py:518-591 aggregate_video_predictions on sigmoid(logit).  Medians by rank count (exact, order-free), means sequential
// in input order.  af_lmk_video_reduce - the same kernel on cli/test.py's rule: fp64 scores, np.median, noisy-OR.  No atomics anywhere.
//
// No stray access.  features: a clip record is used only if 0 <= track < n_tracks, 1 <= len <= 16, first >= 0, first + len <= n,
// lmk_pitch >= 934, au_pitch >= K; reads are then rows first..first+len-1 of the track, floats < 934 (landmark index <= 466) and
// < K of a row.  Writes: the clip's T * F_au and T * 132 floats and its one nvalid.  reduce: clip numbers outside [0, clips) are
// skipped; writes go to the video's own tracks and its own video slot.
#include <cmath>

#include "af_common.h"

namespace af {

#pragma clang fp contract(off)                      // to the end of the file: every product and sum is its own rounding

#define DV_THREADS 256
#define DV_PTS 66
#define DV_LMK (2 * DV_PTS)

__constant__ int DV_KEY_IDX[DV_PTS] = {
    33, 7, 163, 144, 145, 153, 154, 155, 133, 173, 157, 158, 159, 160, 161, 246, 70, 63, 105, 66, 107, 55, 65, 52, 53, 46,
    263, 249, 390, 373, 374, 380, 381, 382, 362, 398, 384, 385, 386, 387, 388, 466, 300, 293, 334, 296, 336, 285, 295, 282, 283, 276,
    61, 146, 91, 181, 84, 17, 314, 405, 321, 375, 291,
    1, 78, 308};
#define DV_NOSE 63
#define DV_ML 64
#define DV_MR 65

__device__ __forceinline__ float dv_nan_to_num(float v) {
    if (v != v) return 0.f;
    if (v == INFINITY) return 3.4028234663852886e38f;
    if (v == -INFINITY) return -3.4028234663852886e38f;
    return v;
}

__device__ __forceinline__ float dv_floor_std(float s) { return s < 1e-6f ? 1e-6f : s; }      // keeps NaN like clamp_min / np.maximum

// source row of output row t when `rows` rows are fixed to T (rows >= 1)
__device__ __forceinline__ int dv_fixt_row(int t, int rows, int T) {
    if (rows > T) return (rows - T) / 2 + t;
    return t < rows ? t : rows - 1;
}

// v[0..T) of one column -> normalised in place
__device__ __forceinline__ void dv_normalize(float* v, int T, int mode, bool apply, float gmean, float gstd) {
    if (mode == AF_DUALV_ZSCORE_NONE) return;
    if (apply) {
        float mu, sd;
        if (mode == AF_DUALV_ZSCORE_CLIP) {
            float s = 0.f;
#pragma unroll
            for (int t = 0; t < AF_DUALV_MAX_T; ++t) if (t < T) s = s + v[t];
            mu = s / (float)T;
            float ss = 0.f;
#pragma unroll
            for (int t = 0; t < AF_DUALV_MAX_T; ++t) if (t < T) { const float d = v[t] - mu; ss = ss + d * d; }
            sd = dv_floor_std(sqrtf(ss / (float)(T - 1)));
        } else {
            mu = gmean;
            sd = dv_floor_std(dv_floor_std(gstd));
        }
#pragma unroll
        for (int t = 0; t < AF_DUALV_MAX_T; ++t) if (t < T) v[t] = (v[t] - mu) / sd;
    }
#pragma unroll
    for (int t = 0; t < AF_DUALV_MAX_T; ++t) if (t < T) v[t] = dv_nan_to_num(v[t]);
}

// the mouth-line rotation of one surviving frame (make_lmk_features._rotate_to_mouth): c = cos(-theta), s = sin(-theta) with theta the
// angle of mr_c - ml_c, stated as dx / h and -dy / h, h = sqrt(dx dx + dy dy), in fp64 (products exact, one rounding each for the sum, the
// root and the quotients) and rounded to fp32 once; dx = dy = 0 is theta = 0
__device__ __forceinline__ void dv_mouth_rotation(const float* p, float div, float* c, float* s) {
    const float nx = p[2 * DV_NOSE], ny = p[2 * DV_NOSE + 1];
    const float mlx = (p[2 * DV_ML] - nx) / div, mly = (p[2 * DV_ML + 1] - ny) / div;
    const float mrx = (p[2 * DV_MR] - nx) / div, mry = (p[2 * DV_MR + 1] - ny) / div;
    const float dx = mrx - mlx, dy = mry - mly;
    if (dx == 0.f && dy == 0.f) { *c = 1.f; *s = 0.f; return; }
    const double h = sqrt((double)dx * (double)dx + (double)dy * (double)dy);
    *c = (float)((double)dx / h);
    *s = (float)(-(double)dy / h);
}

// EXT = false is af_dual_clip_features as it always was (rot and pad_zero are not read).  EXT = true adds what cli/test.py's path needs:
// A == nullptr (landmarks alone, the tracks' au pointers are not read), the mouth-line rotation, and collate_pad's zero rows.
template <bool EXT>
__global__ __launch_bounds__(DV_THREADS) void dual_clip_features_kernel(const af_dualv_track* tracks, int n_tracks, const af_dualv_clip* clips,
                                                                        af_dualv_opts o, float* A, float* L, int32_t* nvalid, int rot, int pad_zero) {
    extern __shared__ float sm[];                      // pts [16][132] raw key points | au [16][K] raw action units
    __shared__ float scale[AF_DUALV_MAX_T];            // scale + 1e-6 per frame
    __shared__ float rot_c[AF_DUALV_MAX_T], rot_s[AF_DUALV_MAX_T];   // EXT: the rotation of each surviving frame
    __shared__ int order[AF_DUALV_MAX_T];              // surviving frames, compacted
    __shared__ int nv_s;
    float* pts = sm;
    float* au = sm + AF_DUALV_MAX_T * DV_LMK;
    const int tid = threadIdx.x, clip = blockIdx.x;
    const bool has_au = !EXT || A != nullptr;
    const bool rotate = EXT && rot != 0, zero_rows = EXT && pad_zero != 0;
    const int T = o.frames, K = has_au ? o.au_k : 0;
    const int f_au = K * (1 + (o.use_delta ? 1 : 0) + (o.use_delta2 ? 1 : 0));
    float* Aout = A + (long long)clip * T * f_au;
    float* Lout = L + (long long)clip * T * DV_LMK;

    const af_dualv_clip c = clips[clip];
    bool ok = c.track >= 0 && c.track < n_tracks && c.len >= 1 && c.len <= AF_DUALV_MAX_T && c.first >= 0;
    af_dualv_track tr = {nullptr, nullptr, 0, 0, 0};
    if (ok) {
        tr = tracks[c.track];
        ok = tr.lmk && (long long)c.first + c.len <= tr.n && tr.lmk_pitch >= 2 * AF_DUALV_MIN_POINTS;
        if (has_au) ok = ok && tr.au && tr.au_pitch >= K;
        if (zero_rows) ok = ok && c.len <= T;          // collate_pad never shortens a clip: a longer one is a bad record
    }
    const int len = ok ? c.len : 0;

    for (int i = tid; i < len * DV_LMK; i += DV_THREADS) {
        const int l = i / DV_LMK, j = i - l * DV_LMK;
        pts[i] = tr.lmk[(long long)(c.first + l) * tr.lmk_pitch + 2 * DV_KEY_IDX[j >> 1] + (j & 1)];
    }
    for (int i = tid; i < len * K; i += DV_THREADS) {
        const int l = i / K, k = i - l * K;
        au[i] = tr.au[(long long)(c.first + l) * tr.au_pitch + k];
    }
    __syncthreads();
    if (tid == 0) {
        int nv = 0;
        for (int l = 0; l < len; ++l) {
            const float* p = pts + l * DV_LMK;
            const float dx = p[2 * DV_ML] - p[2 * DV_MR], dy = p[2 * DV_ML + 1] - p[2 * DV_MR + 1];
            const float s = sqrtf(dx * dx + dy * dy);
            if (s - s == 0.f && !(s < 1e-8f)) {        // finite and >= 1e-8
                order[nv] = l;
                scale[nv] = s + 1e-6f;
                if (rotate) dv_mouth_rotation(p, s + 1e-6f, &rot_c[nv], &rot_s[nv]);
                ++nv;
            }
        }
        nv_s = nv;
        nvalid[clip] = nv;
    }
    __syncthreads();
    const int nv = nv_s;
    if (nv == 0) {                                      // nothing survived (or a bad record): zeros, excluded downstream
        if (has_au)
            for (int i = tid; i < T * f_au; i += DV_THREADS) Aout[i] = 0.f;
        for (int i = tid; i < T * DV_LMK; i += DV_THREADS) Lout[i] = 0.f;
        return;
    }
    const bool global = o.zscore_mode == AF_DUALV_ZSCORE_GLOBAL;
    float v[AF_DUALV_MAX_T];

    if (tid < DV_LMK) {
        const int j = tid;
#pragma unroll
        for (int t = 0; t < AF_DUALV_MAX_T; ++t) {
            v[t] = 0.f;
            if (t < T && !(zero_rows && t >= nv)) {    // collate_pad: rows nv .. T-1 stay +0
                const int r = zero_rows ? t : dv_fixt_row(t, nv, T), l = order[r];
                if (rotate) {
                    const float* q = pts + l * DV_LMK;
                    const float x = (q[j & ~1] - q[2 * DV_NOSE]) / scale[r], y = (q[j | 1] - q[2 * DV_NOSE + 1]) / scale[r];
                    const float cc = rot_c[r], ss = rot_s[r];
                    v[t] = (j & 1) ? x * ss + y * cc : x * cc + y * (-ss);            // points @ R.T, R = [[c, -s], [s, c]]
                } else
                    v[t] = (pts[l * DV_LMK + j] - pts[l * DV_LMK + 2 * DV_NOSE + (j & 1)]) / scale[r];
            }
        }
        dv_normalize(v, T, o.zscore_mode, o.zscore_apply != AF_DUALV_APPLY_AU, global ? o.lmk_mean[j] : 0.f, global ? o.lmk_std[j] : 1.f);
#pragma unroll
        for (int t = 0; t < AF_DUALV_MAX_T; ++t) if (t < T) Lout[t * DV_LMK + j] = v[t];
    }

    if (!has_au) return;
    for (int f = tid; f < f_au; f += DV_THREADS) {
        const int blk = f / K, k = f - blk * K;
        const int kind = blk == 0 ? 0 : (blk == 1 && o.use_delta ? 1 : 2);          // X, first difference, second difference
#pragma unroll
        for (int t = 0; t < AF_DUALV_MAX_T; ++t) {
            v[t] = 0.f;
            if (t < T) {
                const int r = dv_fixt_row(t, len, T);
                const float x0 = au[r * K + k];
                if (kind == 0) v[t] = x0;
                else {
                    const float x1 = au[(r > 0 ? r - 1 : 0) * K + k];
                    const float d1 = x0 - x1;                                          // row 0: X[0] - X[0] (np.diff with prepend)
                    if (kind == 1) v[t] = d1;
                    else {
                        // d1 of the row before: row 0's own d1 for rows 0 and 1 (d1[0] is prepended)
                        const float x2 = au[(r > 1 ? r - 2 : 0) * K + k];
                        const float d0 = r > 0 ? x1 - x2 : d1;
                        v[t] = d1 - d0;
                    }
                }
            }
        }
        dv_normalize(v, T, o.zscore_mode, o.zscore_apply != AF_DUALV_APPLY_LMK, global ? o.au_mean[f] : 0.f, global ? o.au_std[f] : 1.f);
#pragma unroll
        for (int t = 0; t < AF_DUALV_MAX_T; ++t) if (t < T) Aout[t * f_au + f] = v[t];
    }
}

// fp32 sigmoid through fp64: 1 / (1 + exp(-x)) in double, rounded to float once
__device__ __forceinline__ float dv_sigmoid(float x) { return (float)(1.0 / (1.0 + exp(-(double)x))); }

// does a sort before b?  (value, then index)
__device__ __forceinline__ bool dv_before(double a, int ia, double b, int ib) { return a < b || (a == b && ia < ib); }

struct DvReduceArgs {
    const float* logits; const int32_t* nvalid; int clips;
    const int32_t* video_tracks; const int32_t* track_clips; int tracks; const int32_t* clip_index;
    int family, track_mode, video_mode; double thresh;
    float* track_logit; float* track_prob; float* video_logit; float* video_prob;
    float* clip_prob; double* track_score; int32_t* track_pred; double* video_score; int32_t* video_pred; int32_t* track_count;
    int invert; double* clip_score; int32_t* video_count;           // the lmk family (cli/test.py)
};

// the lmk family lives behind af_lmk_video_reduce alone: cli/test.py:86-94, 205-256.  clip_score = sigmoid(logit) or 1 - it, in fp64;
// track = np.median; video = noisy-OR, 1 - exp(sum log1p(-clip(p, 1e-6, 1 - 1e-6))), summed in CSR order.
#define DV_FAMILY_LMK 2

// the value clip entry e of a track contributes (its logit, or in the best family its probability, which phase 0 stored), and
// whether it takes part
__device__ __forceinline__ bool dv_entry(const DvReduceArgs& a, int e, double* val) {
    const int ci = a.clip_index[e];
    if (ci < 0 || ci >= a.clips || a.nvalid[ci] <= 0) return false;
    *val = a.family == DV_FAMILY_LMK ? a.clip_score[ci] : a.family == AF_DUALV_FAMILY_BEST ? (double)a.clip_prob[ci] : (double)a.logits[ci];
    return true;
}

__global__ __launch_bounds__(DV_THREADS) void dual_video_reduce_kernel(DvReduceArgs a) {
    __shared__ double sval[DV_THREADS];                // one chunk of a track's entries, for the sequential sums
    __shared__ int sok[DV_THREADS];
    __shared__ double pick[2];
    __shared__ int has_nan, count_s;
    const int tid = threadIdx.x, video = blockIdx.x;
    int t0 = a.video_tracks[video], t1 = a.video_tracks[video + 1];
    t0 = t0 < 0 ? 0 : t0;
    t1 = t1 > a.tracks ? a.tracks : t1;
    const bool lmk = a.family == DV_FAMILY_LMK;
    const bool best = a.family == AF_DUALV_FAMILY_BEST || lmk;                         // fp64 scores, np.median, preds at thresh
    const bool median = best ? a.track_mode == AF_DUALV_BEST_TRACK_MEDIAN : a.track_mode == AF_DUALV_TRACK_MEDIAN;

    // phase 0 (best family): the clip probabilities, best.py's y_score_clip, once per clip
    if (best && t0 < t1) {
        for (int e = a.track_clips[t0] + tid; e < a.track_clips[t1]; e += DV_THREADS) {
            const int ci = a.clip_index[e];
            if (ci < 0 || ci >= a.clips) continue;
            const float s = dv_sigmoid(a.logits[ci]);
            if (lmk) a.clip_score[ci] = a.invert ? 1.0 - (double)s : (double)s;
            else a.clip_prob[ci] = s;
        }
        __syncthreads();
    }

    // phases 1 and 2, the workgroup per track
    for (int t = t0; t < t1; ++t) {
        const int e0 = a.track_clips[t], e1 = a.track_clips[t + 1];
        // 1: count, sequential mean in input order, majority.  The lanes fetch a chunk, lane 0 adds it up in order.
        int m = 0, fake = 0;
        float s32 = 0.f;
        double s64 = 0.0;
        for (int c0 = e0; c0 < e1; c0 += DV_THREADS) {
            double val = 0.0;
            sok[tid] = c0 + tid < e1 && dv_entry(a, c0 + tid, &val) ? 1 : 0;
            sval[tid] = val;
            __syncthreads();
            if (tid == 0) {
                const int n = e1 - c0 < DV_THREADS ? e1 - c0 : DV_THREADS;
#pragma unroll 8
                for (int i = 0; i < n; ++i) {                                          // selects, not branches: only the adds are serial
                    const bool ok = sok[i] != 0;
                    const double x = sval[i];
                    m += ok ? 1 : 0;
                    if (best) { s64 = ok ? s64 + x : s64; fake += (ok & (x >= a.thresh)) ? 1 : 0; }
                    else s32 = ok ? s32 + (float)x : s32;
                }
            }
            __syncthreads();
        }
        if (tid == 0) {
            count_s = m;
            has_nan = 0;
            a.track_count[t] = m;
            if (best) {
                const double mean = m ? s64 / (double)m : 0.0;
                a.track_score[t] = mean;                                               // the median mode overwrites it below
                a.track_pred[t] = a.track_mode == AF_DUALV_BEST_TRACK_MAJORITY ? (m && (double)fake / (double)m >= 0.5 ? 1 : 0)
                                                                               : (m && mean >= a.thresh ? 1 : 0);
            } else {
                const float mean = m ? s32 / (float)m : NAN;
                a.track_logit[t] = mean;
                a.track_prob[t] = dv_sigmoid(mean);
            }
        }
        __syncthreads();
        m = count_s;
        __syncthreads();                                                               // count_s is read before the next track's is written
        if (!median || m == 0) continue;                                               // uniform over the workgroup
        // 2: the median by rank count - a value is the k-th if exactly k values sort before it (ties by position)
        const int klo = (m - 1) / 2, khi = best ? m / 2 : klo;                         // torch.median: the lower; np.median: both
        // a lane owns one entry per round of 256; the track passes through LDS a chunk at a time and every owner counts along
        for (int o0 = e0; o0 < e1; o0 += DV_THREADS) {
            const int e = o0 + tid;
            double val = 0.0;
            bool mine = e < e1 && dv_entry(a, e, &val);
            if (mine && val != val) { has_nan = 1; mine = false; }
            int rank = 0;
            for (int c0 = e0; c0 < e1; c0 += DV_THREADS) {
                double w = 0.0;
                sok[tid] = c0 + tid < e1 && dv_entry(a, c0 + tid, &w) ? 1 : 0;
                sval[tid] = w;
                __syncthreads();
                if (mine) {
                    const int n = e1 - c0 < DV_THREADS ? e1 - c0 : DV_THREADS;
#pragma unroll 8
                    for (int i = 0; i < n; ++i) {                                      // no branch: the LDS reads of a group go out together
                        const double w = sval[i];
                        const int g = c0 + i;
                        rank += ((sok[i] != 0) & (g != e) & ((w < val) | ((w == val) & (g < e)))) ? 1 : 0;
                    }
                }
                __syncthreads();
            }
            if (mine && rank == klo) pick[0] = val;
            if (mine && rank == khi) pick[1] = val;
        }
        __syncthreads();
        if (tid == 0) {
            if (best) {
                const double med = has_nan ? (double)NAN : (klo == khi ? pick[0] : (pick[0] + pick[1]) / 2.0);
                a.track_score[t] = med;
                a.track_pred[t] = med >= a.thresh ? 1 : 0;
            } else {
                const float med = has_nan ? NAN : (float)pick[0];
                a.track_logit[t] = med;
                a.track_prob[t] = dv_sigmoid(med);
            }
        }
        __syncthreads();
    }
    __syncthreads();

    // phase 3: the video over its tracks that kept a clip
    if (lmk) {
        if (tid == 0) {
            int n = 0;
            double acc = 0.0;
            for (int t = t0; t < t1; ++t) {
                if (a.track_count[t] == 0) continue;
                double p = a.track_score[t];
                p = p < 1e-6 ? 1e-6 : (p > 1.0 - 1e-6 ? 1.0 - 1e-6 : p);               // np.clip: a NaN stays
                acc = acc + log1p(-p);
                ++n;
            }
            const double score = n ? 1.0 - exp(acc) : 0.0;                             // noisy_or([]) = 0
            a.video_score[video] = score;
            a.video_pred[video] = score >= a.thresh ? 1 : 0;
            a.video_count[video] = n;
        }
        return;
    }
    if (best) {
        if (tid == 0) {
            bool any = false, fake = false;
            double top = 0.0;
            for (int t = t0; t < t1; ++t) {
                if (a.track_count[t] == 0) continue;
                const double s = a.track_score[t];
                if (!any || s > top) top = s;                                          // Python's max(): the first, then every greater
                any = true;
                fake = fake || a.track_pred[t] == 1;
            }
            a.video_score[video] = any ? top : 0.0;
            a.video_pred[video] = fake ? 1 : 0;
        }
        return;
    }
    if (a.video_mode == AF_DUALV_VIDEO_MEDIAN) {
        if (tid == 0) { has_nan = 0; pick[0] = (double)NAN; }
        __syncthreads();
        int m = 0;
        for (int t = t0; t < t1; ++t) m += a.track_count[t] > 0 ? 1 : 0;
        const int klo = (m - 1) / 2;
        for (int t = t0 + tid; t < t1; t += DV_THREADS) {
            if (a.track_count[t] == 0) continue;
            const float val = a.track_logit[t];
            if (val != val) { has_nan = 1; continue; }
            int rank = 0;
            for (int g = t0; g < t1; ++g)
                if (g != t && a.track_count[g] > 0 && dv_before((double)a.track_logit[g], g, (double)val, t)) ++rank;
            if (rank == klo) pick[0] = (double)val;
        }
        __syncthreads();
        if (tid == 0) {
            const float z = has_nan ? NAN : (float)pick[0];
            a.video_logit[video] = z;
            a.video_prob[video] = dv_sigmoid(z);
        }
        return;
    }
    if (tid == 0) {
        int m = 0;
        float acc = 0.f;
        for (int t = t0; t < t1; ++t) {
            if (a.track_count[t] == 0) continue;
            const float z = a.track_logit[t];
            if (a.video_mode == AF_DUALV_VIDEO_MEAN) acc = acc + z;
            else if (m == 0) acc = z;
            else if (acc == acc && (z > acc || z != z)) acc = z;                       // a max that keeps a NaN, like torch.max
            ++m;
        }
        const float z = m == 0 ? NAN : (a.video_mode == AF_DUALV_VIDEO_MEAN ? acc / (float)m : acc);
        a.video_logit[video] = z;
        a.video_prob[video] = dv_sigmoid(z);
    }
}

}  // namespace af

extern "C" int af_dual_clip_features(const af_dualv_track* tracks, int n_tracks, const af_dualv_clip* clips, int n_clips,
                                     const af_dualv_opts* opts, float* A, float* L, int32_t* nvalid, void* stream) {
    using namespace af;
    AF_REQUIRE(opts, "dual_clip_features: null options");
    const af_dualv_opts o = *opts;
    AF_REQUIRE(n_clips >= 0 && n_tracks >= 0, "dual_clip_features: negative count");
    AF_REQUIRE(o.frames >= 1 && o.frames <= AF_DUALV_MAX_T, "dual_clip_features: 1..%d frames per clip (got %d)", AF_DUALV_MAX_T, o.frames);
    const int mult = 1 + (o.use_delta ? 1 : 0) + (o.use_delta2 ? 1 : 0);
    AF_REQUIRE(o.au_k >= 1 && (long long)o.au_k * mult <= 256, "dual_clip_features: 1..256 AU features (got %d x %d)", o.au_k, mult);
    AF_REQUIRE(o.zscore_mode >= AF_DUALV_ZSCORE_NONE && o.zscore_mode <= AF_DUALV_ZSCORE_GLOBAL, "dual_clip_features: zscore_mode %d", o.zscore_mode);
    AF_REQUIRE(o.zscore_apply >= AF_DUALV_APPLY_BOTH && o.zscore_apply <= AF_DUALV_APPLY_LMK, "dual_clip_features: zscore_apply %d", o.zscore_apply);
    AF_REQUIRE(o.zscore_mode != AF_DUALV_ZSCORE_GLOBAL || (o.au_mean && o.au_std && o.lmk_mean && o.lmk_std),
               "dual_clip_features: global z-score needs its four stat vectors");
    if (n_clips == 0) return AF_OK;
    AF_REQUIRE(tracks && clips && A && L && nvalid && n_tracks >= 1, "dual_clip_features: null argument");
    const size_t lds = (size_t)AF_DUALV_MAX_T * (DV_LMK + o.au_k) * sizeof(float);
    hipLaunchKernelGGL(dual_clip_features_kernel<false>, dim3(n_clips), dim3(DV_THREADS), lds, (hipStream_t)stream, tracks, n_tracks, clips, o, A,
                       L, nvalid, 0, 0);
    AF_CHECK_LAUNCH("dual_clip_features_kernel");
    return AF_OK;
}

extern "C" int af_dual_clip_features_ex(const af_dualv_track* tracks, int n_tracks, const af_dualv_clip* clips, int n_clips,
                                        const af_dualv_opts* opts, int rot_invariant, int pad_mode, float* A, float* L, int32_t* nvalid,
                                        void* stream) {
    using namespace af;
    AF_REQUIRE(opts, "dual_clip_features_ex: null options");
    af_dualv_opts o = *opts;
    AF_REQUIRE(n_clips >= 0 && n_tracks >= 0, "dual_clip_features_ex: negative count");
    AF_REQUIRE(o.frames >= 1 && o.frames <= AF_DUALV_MAX_T, "dual_clip_features_ex: 1..%d frames per clip (got %d)", AF_DUALV_MAX_T, o.frames);
    AF_REQUIRE(pad_mode == AF_DUALV_PAD_FIXT || pad_mode == AF_DUALV_PAD_ZERO, "dual_clip_features_ex: pad_mode %d", pad_mode);
    AF_REQUIRE(rot_invariant == 0 || rot_invariant == 1, "dual_clip_features_ex: rot_invariant %d", rot_invariant);
    AF_REQUIRE(o.zscore_mode >= AF_DUALV_ZSCORE_NONE && o.zscore_mode <= AF_DUALV_ZSCORE_GLOBAL, "dual_clip_features_ex: zscore_mode %d", o.zscore_mode);
    AF_REQUIRE(o.zscore_apply >= AF_DUALV_APPLY_BOTH && o.zscore_apply <= AF_DUALV_APPLY_LMK, "dual_clip_features_ex: zscore_apply %d", o.zscore_apply);
    if (A) {
        const int mult = 1 + (o.use_delta ? 1 : 0) + (o.use_delta2 ? 1 : 0);
        AF_REQUIRE(o.au_k >= 1 && (long long)o.au_k * mult <= 256, "dual_clip_features_ex: 1..256 AU features (got %d x %d)", o.au_k, mult);
    } else {
        o.au_k = 0;                                     // landmarks alone: no AU row is read, no A is written
    }
    AF_REQUIRE(pad_mode == AF_DUALV_PAD_FIXT || (!A && o.zscore_mode == AF_DUALV_ZSCORE_NONE),
               "dual_clip_features_ex: zero padding is cli/test.py's form: landmarks alone (A null) and no z-score");
    AF_REQUIRE(o.zscore_mode != AF_DUALV_ZSCORE_GLOBAL || (o.lmk_mean && o.lmk_std && (!A || (o.au_mean && o.au_std))),
               "dual_clip_features_ex: global z-score needs its stat vectors");
    if (n_clips == 0) return AF_OK;
    AF_REQUIRE(tracks && clips && L && nvalid && n_tracks >= 1, "dual_clip_features_ex: null argument");
    const size_t lds = (size_t)AF_DUALV_MAX_T * (DV_LMK + o.au_k) * sizeof(float);
    hipLaunchKernelGGL(dual_clip_features_kernel<true>, dim3(n_clips), dim3(DV_THREADS), lds, (hipStream_t)stream, tracks, n_tracks, clips, o, A,
                       L, nvalid, rot_invariant, pad_mode == AF_DUALV_PAD_ZERO ? 1 : 0);
    AF_CHECK_LAUNCH("dual_clip_features_kernel<ext>");
    return AF_OK;
}

extern "C" int af_dual_video_reduce(const float* logits, const int32_t* nvalid, int clips, const int32_t* video_tracks, int videos,
                                    const int32_t* track_clips, int tracks, const int32_t* clip_index, int family, int track_mode,
                                    int video_mode, double prob_thresh, float* track_logit, float* track_prob, float* video_logit,
                                    float* video_prob, float* clip_prob, double* track_score, int32_t* track_pred,
                                    double* video_score, int32_t* video_pred, int32_t* track_count, void* stream) {
    using namespace af;
    AF_REQUIRE(videos >= 0 && tracks >= 0 && clips >= 0, "dual_video_reduce: negative count");
    AF_REQUIRE(family == AF_DUALV_FAMILY_FUSION || family == AF_DUALV_FAMILY_BEST, "dual_video_reduce: family %d", family);
    if (family == AF_DUALV_FAMILY_FUSION) {
        AF_REQUIRE(track_mode == AF_DUALV_TRACK_MEDIAN || track_mode == AF_DUALV_TRACK_MEAN, "dual_video_reduce: track mode %d", track_mode);
        AF_REQUIRE(video_mode >= AF_DUALV_VIDEO_MAX && video_mode <= AF_DUALV_VIDEO_MEAN, "dual_video_reduce: video mode %d", video_mode);
    } else {
        AF_REQUIRE(track_mode >= AF_DUALV_BEST_TRACK_MEAN && track_mode <= AF_DUALV_BEST_TRACK_MAJORITY, "dual_video_reduce: track mode %d", track_mode);
    }
    if (videos == 0) return AF_OK;
    AF_REQUIRE(video_tracks && track_clips && track_count && (clips == 0 || (logits && nvalid && clip_index)), "dual_video_reduce: null argument");
    if (family == AF_DUALV_FAMILY_FUSION)
        AF_REQUIRE(track_logit && track_prob && video_logit && video_prob, "dual_video_reduce: null fusion output");
    else
        AF_REQUIRE(clip_prob && track_score && track_pred && video_score && video_pred, "dual_video_reduce: null best output");
    DvReduceArgs a = {logits, nvalid, clips, video_tracks, track_clips, tracks, clip_index, family, track_mode, video_mode, prob_thresh,
                      track_logit, track_prob, video_logit, video_prob, clip_prob, track_score, track_pred, video_score, video_pred, track_count,
                      0, nullptr, nullptr};
    hipLaunchKernelGGL(dual_video_reduce_kernel, dim3(videos), dim3(DV_THREADS), 0, (hipStream_t)stream, a);
    AF_CHECK_LAUNCH("dual_video_reduce_kernel");
    return AF_OK;
}

extern "C" int af_lmk_video_reduce(const float* logits, const int32_t* nvalid, int clips, const int32_t* video_tracks, int videos,
                                   const int32_t* track_clips, int tracks, const int32_t* clip_index, int invert, double thresh,
                                   double* clip_score, double* track_score, int32_t* track_pred, int32_t* track_count,
                                   double* video_score, int32_t* video_pred, int32_t* video_count, void* stream) {
    using namespace af;
    AF_REQUIRE(videos >= 0 && tracks >= 0 && clips >= 0, "lmk_video_reduce: negative count");
    AF_REQUIRE(invert == 0 || invert == 1, "lmk_video_reduce: invert %d", invert);
    if (videos == 0) return AF_OK;
    AF_REQUIRE(video_tracks && track_clips && track_count && (clips == 0 || (logits && nvalid && clip_index && clip_score)),
               "lmk_video_reduce: null argument");
    AF_REQUIRE(track_score && track_pred && video_score && video_pred && video_count, "lmk_video_reduce: null output");
    DvReduceArgs a = {logits, nvalid, clips, video_tracks, track_clips, tracks, clip_index, DV_FAMILY_LMK, AF_DUALV_BEST_TRACK_MEDIAN, 0, thresh,
                      nullptr, nullptr, nullptr, nullptr, nullptr, track_score, track_pred, video_score, video_pred, track_count,
                      invert, clip_score, video_count};
    hipLaunchKernelGGL(dual_video_reduce_kernel, dim3(videos), dim3(DV_THREADS), 0, (hipStream_t)stream, a);
    AF_CHECK_LAUNCH("dual_video_reduce_kernel<lmk>");
    return AF_OK;
}
