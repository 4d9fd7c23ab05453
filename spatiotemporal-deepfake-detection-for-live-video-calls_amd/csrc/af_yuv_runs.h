// What the YUV launches (af_yuv.hip, af_yuv_formats.hip) share: the run and tile sizes, and the loads and stores that pick, per
// address, the widest naturally aligned form and touch exactly the bytes they are asked for.
#pragma once
#include "af_common.h"

namespace af {

constexpr int YUV_RUN = 8;                          // pixels of a row one lane converts
constexpr int YUV_TILE = 256;                       // runs per workgroup

__device__ __forceinline__ unsigned clamp_u8(int v) { return (unsigned)min(max(v, 0), 255); }

// N bytes (4, 8 or 16) from p as little-endian dwords, by the widest naturally aligned loads p allows.  Reads [p, p + N) and no more.
template <int N>
__device__ __forceinline__ void load_bytes(const unsigned char* p, unsigned (&d)[N / 4]) {
    const unsigned a = (unsigned)(uintptr_t)p;
    if ((a & 3) == 0) {
#pragma unroll
        for (int i = 0; i < N / 4; ++i) d[i] = ((const unsigned*)p)[i];
    } else if ((a & 1) == 0) {
#pragma unroll
        for (int i = 0; i < N / 4; ++i) d[i] = (unsigned)((const unsigned short*)p)[2 * i] | ((unsigned)((const unsigned short*)p)[2 * i + 1] << 16);
    } else {
#pragma unroll
        for (int i = 0; i < N / 4; ++i)
            d[i] = (unsigned)p[4 * i] | ((unsigned)p[4 * i + 1] << 8) | ((unsigned)p[4 * i + 2] << 16) | ((unsigned)p[4 * i + 3] << 24);
    }
}

// 24 bytes (six little-endian dwords) to p.  Writes [p, p + 24) and no more.
__device__ __forceinline__ void store_run(unsigned char* p, const unsigned (&d)[6]) {
    const unsigned a = (unsigned)(uintptr_t)p;
    if ((a & 3) == 0) {
#pragma unroll
        for (int i = 0; i < 6; ++i) ((unsigned*)p)[i] = d[i];
    } else if ((a & 3) == 2) {
        *(unsigned short*)p = (unsigned short)d[0];
#pragma unroll
        for (int i = 0; i < 5; ++i) ((unsigned*)(p + 2))[i] = (d[i] >> 16) | (d[i + 1] << 16);
        *(unsigned short*)(p + 22) = (unsigned short)(d[5] >> 16);
    } else {
#pragma unroll
        for (int i = 0; i < 24; ++i) p[i] = (unsigned char)(d[i >> 2] >> (8 * (i & 3)));
    }
}

// two pixels (6 bytes) to p, which need not be aligned at all
__device__ __forceinline__ void store_pair(unsigned char* p, unsigned p0, unsigned p1) {
    if (((unsigned)(uintptr_t)p & 1) == 0) {
        ((unsigned short*)p)[0] = (unsigned short)p0;
        ((unsigned short*)p)[1] = (unsigned short)((p0 >> 16) | (p1 << 8));
        ((unsigned short*)p)[2] = (unsigned short)(p1 >> 8);
    } else {
        p[0] = (unsigned char)p0; p[1] = (unsigned char)(p0 >> 8); p[2] = (unsigned char)(p0 >> 16);
        p[3] = (unsigned char)p1; p[4] = (unsigned char)(p1 >> 8); p[5] = (unsigned char)(p1 >> 16);
    }
}

}  // namespace af
