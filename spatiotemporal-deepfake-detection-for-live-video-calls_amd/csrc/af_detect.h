// Shared by the face detectors (af_yunet.hip, af_retinaface.hip): the per-frame LDS sort of the candidate keys and the
// frame checks of their descriptors.
#pragma once
#include "af_common.h"

namespace af {
namespace detect {

constexpr int kSortThreads = 1024;
constexpr int kSortLdsBytes = 128 * 1024;
constexpr int kSortLdsKeys = kSortLdsBytes / 8;
constexpr int kSortHalf = kSortLdsKeys / 2;

// ascending bitonic sort of buf[0, n2) (n2 a power of two) by the whole block
__device__ __forceinline__ void bitonic_sort(unsigned long long* buf, int n2) {
    for (int k = 2; k <= n2; k <<= 1)
        for (int j = k >> 1; j > 0; j >>= 1) {
            for (int i = threadIdx.x; i < n2; i += kSortThreads) {
                const int l = i ^ j;
                if (l > i) {
                    const unsigned long long x = buf[i], y = buf[l];
                    if ((x > y) == ((i & k) == 0)) {
                        buf[i] = y;
                        buf[l] = x;
                    }
                }
            }
            __syncthreads();
        }
}

// One frame per block of kSortThreads: leaves the smallest min(n, kSortHalf) of the n keys gk[0, n) in ascending order
// at lds[0, ...) (kSortLdsBytes of dynamic LDS).  Up to kSortLdsKeys keys are sorted whole.  Above that only the kSortHalf
// smallest can matter to a caller whose top_k fits kSortHalf, so the block keeps them as a running set in the lower half
// and sorts it together with each next chunk of kSortHalf keys: n / kSortHalf LDS sorts of kSortLdsKeys keys instead of
// one sort of n in memory.
__device__ __forceinline__ void sort_keys(const unsigned long long* gk, int n, unsigned long long* lds) {
    const int tid = threadIdx.x;
    if (n <= kSortLdsKeys) {
        int n2 = 2;
        while (n2 < n) n2 <<= 1;
        for (int i = tid; i < n2; i += kSortThreads) lds[i] = i < n ? gk[i] : ~0ull;
        __syncthreads();
        bitonic_sort(lds, n2);
    } else {
        for (int i = tid; i < kSortHalf; i += kSortThreads) lds[i] = gk[i];
        for (int base = kSortHalf; base < n; base += kSortHalf) {
            for (int i = tid; i < kSortHalf; i += kSortThreads) lds[kSortHalf + i] = base + i < n ? gk[base + i] : ~0ull;
            __syncthreads();
            bitonic_sort(lds, kSortLdsKeys);
        }
    }
}

// The checks both detectors' descriptors share: batch and frame size, and unless `layout` is false (a caller that reads
// no frames) the row pitch and frame stride of the packed uint8 HWC frames.  `who` prefixes every message.
template <class Desc>
static int check_frames(const Desc* d, const char* who, int max_side, bool layout = true) {
    AF_REQUIRE(d, "%s: null descriptor", who);
    AF_REQUIRE(d->batch >= 1 && d->batch <= 65535, "%s: batch %d out of [1, 65535]", who, d->batch);
    AF_REQUIRE(d->height >= 1 && d->width >= 1 && d->height <= max_side && d->width <= max_side,
               "%s: frame %dx%d out of [1, %d]", who, d->width, d->height, max_side);
    if (layout) {
        AF_REQUIRE(d->row_pitch >= 3LL * d->width, "%s: row pitch %lld < 3 * width", who, (long long)d->row_pitch);
        AF_REQUIRE(d->batch == 1 || d->frame_stride >= d->row_pitch * d->height, "%s: frame stride %lld < pitch * height", who,
                   (long long)d->frame_stride);
    }
    return AF_OK;
}

}  // namespace detect
}  // namespace af
