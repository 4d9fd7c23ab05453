// 1x3x3 / stride 1 / pad (0,1,1) convolution, 64 -> 64 channels, 16-bit operands: the `b` conv of the three
// s2 bottlenecks (reference altfreezing/slowfast/models/resnet_helper.py:283-297), + BN + ReLU.
//
// The generic implicit GEMM streams every activation row through LDS once PER TAP (9x) and re-reads the
// weight tile from LDS for every 32 positions; at Cin = Cout = 64 that makes the layer ingest / LDS bound
// (~0.37 PFLOP/s).  This kernel is shaped around what is small here:
//   * the weights stay with the waves for the life of the workgroup: EIGHT waves, two per SIMD, wave = (channel half,
//     m-tile group), 32 output channels x 4 m-tiles each; the MFMA A-fragments of taps 0-6 (7 taps x 2 k-halves x 2 channel
//     tiles = 112 registers) live in REGISTERS and those of the last two taps wait in LDS in fragment order (all nine taps in
//     registers spilled); a B fragment feeds 2 MFMAs and is read a whole (tap, k-half) step ahead of its use;
//   * a workgroup walks a contiguous run of image strips (R = 4 output rows); each strip's input patch
//     ((R+2) rows, zero halo columns included) is brought in ONCE by LDS-DMA (buffer loads; out-of-range lanes = zeros), double-buffered under the MFMAs
//     of the previous strip, and all 9 taps read it: with the rows stored at a padded pitch WP = W + 2 a tap
//     (dh,dw) is the constant row offset dh*WP + dw, so every B fragment is a plain swizzled ds_read_b128;
//   * positions are the padded strip (R x WP, two halo columns per row computed and discarded: 3.4 % waste).
// Persistent: one workgroup per CU, two barriers per strip.  Results leave through an LDS output tile ([position][64
// channels], swizzled like the patches): the workgroup stores whole 128-byte rows, and does so under the MFMAs of the
// NEXT strip.
#include "af_conv_paths.h"

namespace af {

struct C133Args {
    const char* in;
    const char* w;       // packed [64][9][64]
    const float* scale;
    const float* shift;
    char* out;
    int H, W, frames;
    int strips_per_frame, total_strips;
    int rows_alloc;      // LDS rows per patch buffer (multiple of 8)
#ifdef AF_STAMPS
    unsigned long long* stamps;   // diagnostic build only (tools/stamps_lib.sh): [workgroup][wave][8] shader-clock cycles per phase
    int dbg;                      // timing-only ablations (AF_C64_DBG; outputs are then garbage): 1 no tile stores, 2 no epilogue, 4 no patch DMA
#endif
};

// Diagnostic build (-DAF_STAMPS; never the shipped library): cycles of a wave's life by phase, summed over its strips.
// (s_memtime waits with lgkmcnt(0): the stamps sit where no LDS read is meant to stay in flight.)
#ifdef AF_STAMPS
#define C64_ACC_DECL unsigned long long st_acc[8] = {0, 0, 0, 0, 0, 0, 0, 0}, st_prev = __builtin_amdgcn_s_memtime()
#define C64_ACC(slot) do { const unsigned long long t_ = __builtin_amdgcn_s_memtime(); st_acc[slot] += t_ - st_prev; st_prev = t_; } while (0)
#ifdef C64_CT_DBG
#define C64_DBG(bit) ((C64_CT_DBG) & (bit))       // compile-time ablations: no branch left in the loop
#else
#define C64_DBG(bit) (a.dbg & (bit))
#endif
#define C64_FLUSH do { if (a.stamps && lane < 8) a.stamps[((long long)blockIdx.x * 8 + wave) * 8 + lane] = \
    lane == 0 ? st_acc[0] : lane == 1 ? st_acc[1] : lane == 2 ? st_acc[2] : lane == 3 ? st_acc[3] : lane == 4 ? st_acc[4] : lane == 5 ? st_acc[5] : lane == 6 ? st_acc[6] : st_acc[7]; } while (0)
#else
#define C64_ACC_DECL do {} while (0)
#define C64_ACC(slot) do {} while (0)
#define C64_DBG(bit) false
#define C64_FLUSH do {} while (0)
#endif

// The strip walk on EIGHT waves, two per SIMD: wave = (channel half ng = wave >> 2, m-tile group mg = wave & 3), 32 output
// channels x 4 m-tiles each.  Rounds 1-2 ran FOUR waves, one per SIMD, each with all 64 channels (288 weight registers, VGPRs +
// AGPRs): every non-MFMA instruction of the strip (patch DMA issue: 26 us per launch, tile stores: 16, epilogue: 14, of 145)
// sat in the MFMA stream's way; with two waves per SIMD, one wave's DMA issue /
// epilogue / stores run under the other's MFMAs.  The price: every B fragment is read by both channel halves (2x the LDS
// fragment reads: ~125 B/clk of the CU's 256) and feeds 2 MFMAs instead of 4 - which is why the fragments of step s + 1 are read
// a whole step (8 MFMAs) ahead of their use (round 1's 8-wave form read them right in front: a chain of LDS latencies, 58 %).
template <int DT, int R>
__global__ __launch_bounds__(512, 2) void conv133_c64x2_kernel(const C133Args a) {
    typedef Elem<DT> E;
    static_assert(E::EPC == 8, "16-bit operands only");
    constexpr int MT = 4, NT2 = 2;
    constexpr int OTROWS = 16 * 16;

    extern __shared__ uint4 smem[];
    const unsigned lds0 = (unsigned)(uintptr_t)(__attribute__((address_space(3))) char*)smem;
    const int tid = threadIdx.x, lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int mg = wave & 3, ng = wave >> 2;
    const int frow = lane & 15, fg = lane >> 4;
    const int WP = a.W + 2;
    const int NP = a.rows_alloc >> 3;
    const int buf_bytes = a.rows_alloc * 128;
    char* otile = reinterpret_cast<char*>(smem) + 2 * buf_bytes;
    C64_ACC_DECL;

    // ---- this wave's 32 output channels of the weights -> registers
    // (taps 0-6 in registers: 112; the last two taps' fragments wait in LDS in fragment order - 144 + accumulators + fragments +
    //  the store / DMA temporaries spilled 22 registers, and a scratch reload's vmcnt(0) also waits for the patch DMA in flight)
    constexpr int RT = 7;                                        // taps whose weights live in registers
    // Round 4: the weights come in through LDS.  As 28 global loads per wave in fragment order (a wave instruction = 16 rows x 64
    // bytes, every wave of every workgroup asking for the same 73 KB at the same moment) the prologue took 16-22 k cycles of a
    // workgroup's ~240 k (in-kernel stamps) - ~14 bytes per clock and CU.  Now the [64][9][64] tensor is ONE coalesced LDS-DMA image
    // per workgroup (72 pieces of 8 x 128 bytes, rows swizzled like the patches, in the patch buffers' space), every wave takes its
    // fragments from there, and the first patch is issued once everyone has.
    u32x4 wreg[RT][2][NT2];
    float* bn_lds = reinterpret_cast<float*>(otile + OTROWS * 128);
    uint4* w8 = reinterpret_cast<uint4*>(bn_lds + 128);          // taps RT .. 8: [tap][k-half][channel tile 0..3][64 lanes]
    {
        const i32x4 wdesc = make_desc(a.w);
        const int wrow = lane >> 3, wchunk = (lane & 7) ^ wrow;
#pragma unroll
        for (int j = 0; j < 9; ++j) {
            const int g = wave + 8 * j;                          // rows 8 g .. 8 g + 7 of the 576 (channel, tap) rows
            blds16((unsigned)((g * 8 + wrow) * 128 + wchunk * 16), wdesc, 0, __builtin_amdgcn_readfirstlane(lds0 + g * 1024));
        }
        if (tid < 64) { bn_lds[tid] = a.scale[tid]; bn_lds[64 + tid] = a.shift[tid]; }
        wait_vmcnt<0>();
        __syncthreads();
        const uint4* wimg = smem;
        auto frag = [&](int ch, int tap, int kk) {               // 8 input channels kk * 32 + fg * 8 .. of (output channel ch, tap)
            const int row = ch * 9 + tap;
            return wimg[row * 8 + ((kk * 4 + fg) ^ (row & 7))];
        };
#pragma unroll
        for (int tap = 0; tap < RT; ++tap)
#pragma unroll
            for (int kk = 0; kk < 2; ++kk)
#pragma unroll
                for (int i = 0; i < NT2; ++i) wreg[tap][kk][i] = __builtin_bit_cast(u32x4, frag(ng * 32 + i * 16 + frow, tap, kk));
        for (int idx = tid; idx < (9 - RT) * 512; idx += 512) {
            const int f = idx >> 6, tap = RT + (f >> 3), kk = (f >> 2) & 1, ct = f & 3;
            w8[idx] = frag(ct * 16 + frow, tap, kk);
        }
#pragma unroll
        for (int tap = 0; tap < RT; ++tap)
#pragma unroll
            for (int kk = 0; kk < 2; ++kk)
#pragma unroll
                for (int i = 0; i < NT2; ++i) asm volatile("" : "+v"(wreg[tap][kk][i]));    // (registers for good: no re-reads inside the loop)
    }

    unsigned* dma_tab = reinterpret_cast<unsigned*>(w8 + (9 - RT) * 512);
    const int dma_row = lane >> 3, dma_chunk = (lane & 7) ^ dma_row;
    for (int g = wave; g < NP; g += 8) {
        const int q = g * 8 + dma_row - 1;
        const int r = q / WP, c = q - r * WP;
        const bool ok = q >= 0 && r < R + 2 && c >= 1 && c <= a.W;
        dma_tab[g * 64 + lane] = ok ? ((unsigned)r << 24) | (unsigned)((r * a.W + (c - 1)) * 128 + dma_chunk * 16) : 0xffffffffu;
    }
    __syncthreads();
    auto issue_patch = [&](int strip, int buf) {
        const int frame = strip / a.strips_per_frame;
        const int h0 = (strip - frame * a.strips_per_frame) * R;
        const i32x4 desc = make_desc(a.in + ((long long)frame * a.H + h0 - 1) * a.W * 128);
        for (int g = wave; g < NP; g += 8) {
            const unsigned e = dma_tab[g * 64 + lane];
            const bool ok = e != 0xffffffffu && (unsigned)(h0 - 1 + (int)(e >> 24)) < (unsigned)a.H;
            blds16(ok ? (e & 0xffffffu) : kOutOfRange, desc, 0, __builtin_amdgcn_readfirstlane(lds0 + buf * buf_bytes + g * 1024));
        }
    };
    const int G = gridDim.x, b = blockIdx.x;
    const int s0 = (int)((long long)a.total_strips * b / G), s1 = (int)((long long)a.total_strips * (b + 1) / G);
    if (s0 < s1) issue_patch(s0, 0);
    C64_ACC(0);                                                      // 0: prologue (weights, tables, first patch issue)
    auto store_tile = [&](int sp) {
        const int frame = sp / a.strips_per_frame;
        const int h0 = (sp - frame * a.strips_per_frame) * R;
        char* obase = a.out + ((long long)frame * a.H + h0) * a.W * 128;
        if (C64_DBG(1)) return;
#pragma unroll
        for (int j = 0; j < OTROWS * 8 / 512; ++j) {
            const int row = (tid + 512 * j) >> 3, chunk = tid & 7, r = row / WP, c = row - r * WP;
            if (r < R && c >= 1 && c <= a.W && h0 + r < a.H) {            // halo columns / rows beyond the strip are not stored
                const u32x4 o = *reinterpret_cast<const u32x4*>(otile + row * 128 + ((chunk ^ (row & 7)) << 4));
                __builtin_nontemporal_store(o, reinterpret_cast<u32x4*>(obase + (r * a.W + (c - 1)) * 128 + chunk * 16));
            }
        }
    };

    for (int s = s0; s < s1; ++s) {
        const int buf = (s - s0) & 1;
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
        C64_ACC(1);                                                  // 1: wait for the patch DMA (and the tile stores)
        __builtin_amdgcn_s_barrier();
        C64_ACC(2);                                                  // 2: barrier
        if (s + 1 < s1 && !C64_DBG(4)) issue_patch(s + 1, buf ^ 1);
        C64_ACC(3);                                                  // 3: next patch issue

        const char* xb = reinterpret_cast<const char*>(smem) + buf * buf_bytes;
        f32x4 acc[NT2][MT];
#pragma unroll
        for (int i = 0; i < NT2; ++i)
#pragma unroll
            for (int k = 0; k < MT; ++k) acc[i][k] = f32x4{0.f, 0.f, 0.f, 0.f};
        // ONE fragment set, refilled in place: m-tile k's fragment of step s + 1 is read right behind the two MFMAs that consumed
        // its fragment of step s - still a whole step (8 MFMAs of this wave) ahead of its use, with half the registers of two
        // sets (two sets + 144 weight registers spilled)
        uint4 bf[MT];
        uint4 aw[2][NT2];                                            // LDS-resident weight fragments of the step / the next step (taps 7, 8)
        auto read_frag = [&](int step, int k) {
            const int tap = step >> 1, kk = step & 1;
            const int row = frow + (tap / 3) * WP + (tap % 3);
            return *reinterpret_cast<const uint4*>(xb + row * 128 + (((kk * 4 + fg) ^ (row & 7)) << 4) + (mg + 4 * k) * (16 * 128));
        };
#pragma unroll
        for (int k = 0; k < MT; ++k) bf[k] = read_frag(0, k);
#pragma unroll
        for (int step = 0; step < 18; ++step) {
            if (step == 6 && s > s0) store_tile(s - 1);
            // (round 4: the LDS-resident weight fragments of the last two taps are read ONCE per step, in front of its four m-tiles;
            //  read per use - hipcc does not merge loads across the sched_barriers - every MFMA pair of those four steps waited
            //  for an LDS round trip of its own: `rr [lgkmcnt(1)] M` in the ISA)
            //  ... and a whole step ahead of its use (two fragment sets, alternating by step parity)
            if (step + 1 >= 2 * RT && step + 1 < 18) {
#pragma unroll
                for (int i = 0; i < NT2; ++i) aw[(step + 1) & 1][i] = w8[((((step + 1) >> 1) - RT) * 8 + ((step + 1) & 1) * 4 + ng * 2 + i) * 64 + lane];
            }
#pragma unroll
            for (int k = 0; k < MT; ++k) {
#pragma unroll
                for (int i = 0; i < NT2; ++i)
                    Mma<DT>::run(step < 2 * RT ? __builtin_bit_cast(uint4, wreg[step < 2 * RT ? step >> 1 : 0][step & 1][i]) : aw[step & 1][i],
                                 bf[k], acc[i][k]);
                if (step + 1 < 18) bf[k] = read_frag(step + 1, k);
                __builtin_amdgcn_sched_barrier(0);
            }
        }
        f32x4 sc[NT2], sf[NT2];
#pragma unroll
        for (int i = 0; i < NT2; ++i) {
            sc[i] = *reinterpret_cast<const f32x4*>(bn_lds + ng * 32 + i * 16 + fg * 4);
            sf[i] = *reinterpret_cast<const f32x4*>(bn_lds + 64 + ng * 32 + i * 16 + fg * 4);
        }
        asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
        C64_ACC(4);                                                  // 4: the 144 MFMAs (+ the previous tile's stores at step 6)
        __builtin_amdgcn_s_barrier();
        C64_ACC(5);                                                  // 5: barrier (everyone has read the previous tile out)
        if (!C64_DBG(2)) {
#pragma unroll
        for (int k = 0; k < MT; ++k) {
            const int row = (mg + 4 * k) * 16 + frow;
#pragma unroll
            for (int i = 0; i < NT2; ++i) {
                f32x4 v = acc[i][k] * sc[i] + sf[i];
                v[0] = relu_f(v[0]); v[1] = relu_f(v[1]); v[2] = relu_f(v[2]); v[3] = relu_f(v[3]);
                const int ch = ng * 32 + i * 16 + fg * 4;
                Vec4<DT>::store(otile + row * 128 + (((ch >> 3) ^ (row & 7)) << 4) + (ch & 4) * 2, v);
            }
        }
        }
        C64_ACC(6);                                                  // 6: epilogue
    }
    if (s0 < s1) {
        asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
        __builtin_amdgcn_s_barrier();
        store_tile(s1 - 1);
    }
    C64_ACC(7);
    C64_FLUSH;
}

// Round 4, tried and NOT kept (DESIGN 3.1b has the stamp tables): a "skewed" form of this kernel - waves 4-7 taking the strip's one
// barrier in the middle of their strip (three patch slots), DMA pieces issued one per tap-step with computed offsets, no output tile
// (register epilogue: permlane16 swaps + four counted 16-byte buffer stores per wave and strip).  Parity green, 129-135 us against
// 120-128 for this form; with the skew switched off 122-127: a tie.  What the stamps showed instead is where this form's time is:
// the MFMA phase of the two waves of a SIMD is MFMA-bound while both multiply (5.0-5.4 k cycles per strip for 288 MFMAs), the older
// wave of the two wins the issue arbitration and the younger one starves until it is alone, and alone a wave with one tap-step of
// LDS look-ahead runs at ~25 cycles per MFMA - so putting one wave's epilogue under the other's MFMAs buys what the lone stretches lose.
// How a layer runs on this path: strips of kStripRows rows of a frame at the padded pitch W + 2 (ok == false: not this path)
constexpr int kStripRows = 4;
struct Geom133 { bool ok; int strips_per_frame, total_strips, rows_alloc, lds; };
static Geom133 geom133(const af_conv_desc* d) {
    Geom133 g = {};
    const int positions = kStripRows * (d->w + 2);           // of the 256 every workgroup multiplies
    if (d->dtype == AF_F32 || d->cin != 64 || d->cout != 64 || !kernel_is(d, 1, 3, 3) || !unit_stride(d) || !pad_is(d, 0, 1, 1) ||
        !d->relu || d->tpool || positions > 256) return g;
    // narrow frames (SlowFast's Fast pathway in s5: 7 x 7) would run at 14 % and took 2.4x the generic kernel's time
    if (positions < 112) return g;
    g.ok = true; g.strips_per_frame = (d->h + kStripRows - 1) / kStripRows;
    g.total_strips = d->n * d->t * g.strips_per_frame;
    g.rows_alloc = (((kStripRows + 2) * (d->w + 2) + 2 + 16) + 7) & ~7;
    g.lds = 2 * g.rows_alloc * 128 + 16 * 16 * 128 + 128 * 4 + 2 * 512 * 16 + (g.rows_alloc / 8) * 64 * 4;   // (2 * 512 * 16: the last two taps' fragments)
    return g;
}

// true iff this layer takes the register-resident-weights path
static bool c133_applies(const ConvCall& c) {
    return !c.d2 && c.residual == nullptr && (c.out_ld == 0 || c.out_ld == 64) && geom133(c.d).ok;
}

// persistent grid: each workgroup a contiguous range of strips
static void c133_work(const ConvCall& c, long long* units, int* workgroups) {
    const Geom133 g = geom133(c.d);
    *units = g.total_strips; *workgroups = persistent_grid(g.total_strips);
}

static int c133_run(const ConvCall& c) {
    const af_conv_desc* d = c.d;
    C133Args a;
    a.in = (const char*)c.in; a.w = (const char*)c.w; a.scale = c.scale; a.shift = c.shift; a.out = (char*)c.out;
    const Geom133 g = geom133(d);
    a.H = d->h; a.W = d->w; a.frames = d->n * d->t;
    a.strips_per_frame = g.strips_per_frame; a.total_strips = g.total_strips; a.rows_alloc = g.rows_alloc;
    fill_stamps(a, "AF_C64_DBG");
    return with_dtype16(d->dtype, [&](auto dt) {
        return launch_lds<&conv133_c64x2_kernel<dt, kStripRows>>("conv133", persistent_grid(a.total_strips), g.lds, c.stream, a);
    });
}

const ConvPath& conv133_path() {
    static const ConvPath path = {VAR_C133, c133_applies, c133_work, c133_run, true};
    return path;
}

}  // namespace af
