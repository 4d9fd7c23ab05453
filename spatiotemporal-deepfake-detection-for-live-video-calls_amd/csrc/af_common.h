// Internal helpers shared by the gfx950 kernels of libafhip.so.  CDNA4 only: wave64, MFMA.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <stdio.h>
#include <stdarg.h>
#include <stdlib.h>

#include <vector>

#include "../../include/af_hip.h"

namespace af {

int set_error(int code, const char* fmt, ...);

// An integer knob from the environment; `dflt` when it is not set.  The shipped library reads exactly three names, all in host-side
// selection code and all flipped in-process by tests: AF_FORCE_VAR and AF_IGEMM_224 (af_conv.hip, pick_variant) and AF_ABC_INNER32
// (af_block_abc.hip); tests/test_host_cpu.py pins that set.  They are read per call on purpose: a cached value would not see the
// tests' changes, and a setter in the C ABI would be more machinery than three knobs deserve.  A kernel FORM is not chosen here: two
// forms are compared as two libraries (tools/ab_lib.sh).  The diagnostic build's knobs are all below, under AF_STAMPS.
inline int env_int(const char* name, int dflt) {
    const char* e = getenv(name);
    return e ? atoi(e) : dflt;
}

// Diagnostic build (-DAF_STAMPS; never the shipped library) only - every environment name it reads is read here.
// fill_dbg: a kernel's timing-ablation knob (AF_G_DBG, AF_C64_DBG, AF_CA_DBG) into its arguments; fill_stamps: that and the stamp
// buffer of AF_STAMP_PTR; stamps_unit_per_workgroup: should conv133g give every unit a workgroup of its own instead of persisting?
template <class Args>
inline void fill_dbg(Args& a, const char* dbg_knob) {
#ifdef AF_STAMPS
    a.dbg = env_int(dbg_knob, 0);
#endif
}
template <class Args>
inline void fill_stamps(Args& a, const char* dbg_knob) {
#ifdef AF_STAMPS
    const char* ep = getenv("AF_STAMP_PTR");
    a.stamps = ep ? (unsigned long long*)strtoull(ep, nullptr, 0) : nullptr;
#endif
    fill_dbg(a, dbg_knob);
}
inline bool stamps_unit_per_workgroup() {
#ifdef AF_STAMPS
    static const int persist = env_int("AF_G_PERSIST", 1);   // 0: the stamp slots are per unit (tools/r04_collect.sh)
    return !persist;
#else
    return false;
#endif
}
// ... and its device side: shader-clock stamps around the phases of a tile / unit, kept in registers and written behind the last
// output store to a buffer nothing else reads (tools/stamps_lib.sh; never the shipped library).  `block` is the kernel's workgroup index.
#ifdef AF_STAMPS
#define AF_STAMP_DECL unsigned long long stamp_v[8] = {0, 0, 0, 0, 0, 0, 0, 0}
#define AF_DBG(bit) (a.dbg & (bit))
#define AF_STAMP(slot) stamp_v[slot] = (slot) >= 6 ? __builtin_amdgcn_s_memrealtime() : __builtin_amdgcn_s_memtime()
#define AF_STAMP_FLUSH(block) do { if (a.stamps && lane < 8) a.stamps[((long long)(block) * 8 + wave) * 8 + lane] = \
    lane == 0 ? stamp_v[0] : lane == 1 ? stamp_v[1] : lane == 2 ? stamp_v[2] : lane == 3 ? stamp_v[3] : lane == 4 ? stamp_v[4] : lane == 5 ? stamp_v[5] : lane == 6 ? stamp_v[6] : stamp_v[7]; } while (0)
#else
#define AF_STAMP_DECL do {} while (0)
#define AF_DBG(bit) false
#define AF_STAMP(slot) do {} while (0)
#define AF_STAMP_FLUSH(block) do {} while (0)
#endif

// ---- LDS-DMA helpers shared by the convolution kernels
typedef unsigned int u32x4 __attribute__((ext_vector_type(4)));
// one 16-byte-per-lane LDS-DMA: LDS[lds_base + lane*16 .. +16) <- desc.base[voff + soff .. +16); a lane whose
// voff is outside the descriptor's 2 GiB window (kOutOfRange) gets zeros - that is how padding taps, rows beyond M
// and channel tails are filled.  hipcc does not count this load: every wait on it is an explicit s_waitcnt vmcnt(N).
typedef int i32x4 __attribute__((ext_vector_type(4)));
typedef float f32x4 __attribute__((ext_vector_type(4)));
constexpr unsigned kOutOfRange = 0x80000000u;
__device__ __forceinline__ void blds16(unsigned voff, const i32x4& desc, int soff, unsigned lds_base) {
    unsigned keep;
    asm volatile("s_mov_b32 %0, m0\n\ts_mov_b32 m0, %3\n\ts_nop 0\n\tbuffer_load_dwordx4 %1, %2, %4 offen lds\n\ts_mov_b32 m0, %0"
                 : "=&s"(keep) : "v"(voff), "s"(desc), "s"(lds_base), "s"(soff) : "memory");
}
// the same without saving m0 around the load (2 scalar instructions per piece instead of 4; hipcc is told that m0 is clobbered):
// for the streaming kernels, which are bound by instruction issue at 2 waves per SIMD
__device__ __forceinline__ void blds16_m0(unsigned voff, const i32x4& desc, int soff, unsigned lds_base) {
    asm volatile("s_mov_b32 m0, %2\n\ts_nop 0\n\tbuffer_load_dwordx4 %0, %1, %3 offen lds"
                 : : "v"(voff), "s"(desc), "s"(lds_base), "s"(soff) : "memory", "m0");
}
__device__ __forceinline__ void blds16_nt_m0(unsigned voff, const i32x4& desc, int soff, unsigned lds_base) {
    asm volatile("s_mov_b32 m0, %2\n\ts_nop 0\n\tbuffer_load_dwordx4 %0, %1, %3 offen nt lds"
                 : : "v"(voff), "s"(desc), "s"(lds_base), "s"(soff) : "memory", "m0");
}
// the same with the non-temporal cache policy: for bytes one CU reads once (a residual stream)
__device__ __forceinline__ void blds16_nt(unsigned voff, const i32x4& desc, int soff, unsigned lds_base) {
    unsigned keep;
    asm volatile("s_mov_b32 %0, m0\n\ts_mov_b32 m0, %3\n\ts_nop 0\n\tbuffer_load_dwordx4 %1, %2, %4 offen nt lds\n\ts_mov_b32 m0, %0"
                 : "=&s"(keep) : "v"(voff), "s"(desc), "s"(lds_base), "s"(soff) : "memory");
}
// A plain 16-byte buffer load that hipcc does NOT count: for register prefetch several tiles ahead.  (For a counted load the
// compiler must assume that nothing younger is in the queue when the value is finally used - the stores and loads issued since
// are conditional for it - and emits s_waitcnt vmcnt(0..3), which drains the LDS-DMA issued behind it as well.)  The caller
// waits with its own counted s_waitcnt vmcnt and passes the registers through an empty asm ("+v") before the first use.
__device__ __forceinline__ u32x4 bload16_nt_uncounted(unsigned voff, const i32x4& desc, int soff) {
    u32x4 r;
    asm volatile("buffer_load_dwordx4 %0, %1, %2, %3 offen nt" : "=v"(r) : "v"(voff), "s"(desc), "s"(soff) : "memory");
    return r;
}
// (the same for a 64-bit address)
__device__ __forceinline__ uint4 gload16_uncounted(const void* p) {
    u32x4 r;
    asm volatile("global_load_dwordx4 %0, %1, off" : "=v"(r) : "v"(p) : "memory");
    return __builtin_bit_cast(uint4, r);
}
// raw buffer descriptor over [base, base + 2 GiB): stride 0, no swizzle, 32-bit data format
__device__ __forceinline__ i32x4 make_desc(const char* base) {
    const unsigned long long b = (unsigned long long)base;
    i32x4 d;
    d[0] = __builtin_amdgcn_readfirstlane((int)(b & 0xffffffffu));
    d[1] = __builtin_amdgcn_readfirstlane((int)((b >> 32) & 0xffffu));
    d[2] = (int)kOutOfRange;
    d[3] = 0x00020000;
    return d;
}

// ReLU and pooling max with torch's NaN behaviour: a NaN activation stays NaN through clamp_min / max_pool, so a clip
// with a non-finite pixel yields a NaN logit (as in the reference) instead of a plausible score
// (gfx950 has the IEEE-754-2019 maximum / minimum - v_maximum3_f32 / v_minimum3_f32 - which return NaN when an operand is NaN:
//  one instruction each, where a compare + select took two to four and the v_max3 / v_min3 forms needed separate NaN flags)
__device__ __forceinline__ float relu_f(float v) { return __builtin_elementwise_maximum(v, 0.f); }
__device__ __forceinline__ float max_nan(float m, float x) { return __builtin_elementwise_maximum(m, x); }
__device__ __forceinline__ float min_nan(float m, float x) { return __builtin_elementwise_minimum(m, x); }

template <int N> __device__ __forceinline__ void wait_vmcnt() { asm volatile("s_waitcnt vmcnt(%0)" ::"n"(N) : "memory"); }

// s_waitcnt vmcnt(n) for a wave-uniform run-time n in [0, MAXN] (the immediate is a compile-time constant: a scalar branch chain)
template <int MAXN, int K = 0> __device__ __forceinline__ void wait_vmcnt_dyn(int n) {
    if constexpr (K >= MAXN) wait_vmcnt<MAXN>();
    else { if (n == K) wait_vmcnt<K>(); else wait_vmcnt_dyn<MAXN, K + 1>(n); }
}

// LDS fragment reads hipcc does NOT count (round 4).  A software-pipelined K loop reads the fragments of half-step h + 1 while
// half-step h multiplies; when the reads of h were issued in the previous loop iteration and the body has control flow in it
// (conditional DMA issue), hipcc's wait insertion gives up counting across the back edge and puts s_waitcnt lgkmcnt(0) in front
// of the first MFMA - behind the reads just issued, i.e. the whole LDS round trip of 8 waves x 11 reads is exposed once per
// K-step (conv133g, ISA dump of tools/isa_schedule.py).  With the reads as inline asm the kernel waits itself: lgkmcnt counts LDS
// operations in issue order, so wait_lgkmcnt<N>() = "all but my N youngest reads are back"; the registers then pass through
// pin_frag (an empty asm with a "+v" operand) so that no consumer can be scheduled above the wait.
template <int OFF> __device__ __forceinline__ u32x4 lds_read16_uncounted(unsigned addr) {
    u32x4 r;
    asm volatile("ds_read_b128 %0, %1 offset:%2" : "=v"(r) : "v"(addr), "n"(OFF) : "memory");
    return r;
}
template <int OFF> __device__ __forceinline__ unsigned lds_read4_uncounted(unsigned addr) {
    unsigned r;
    asm volatile("ds_read_b32 %0, %1 offset:%2" : "=v"(r) : "v"(addr), "n"(OFF) : "memory");
    return r;
}
template <int N> __device__ __forceinline__ void wait_lgkmcnt() { asm volatile("s_waitcnt lgkmcnt(%0)" ::"n"(N) : "memory"); }
__device__ __forceinline__ void pin_frag(u32x4& v) { asm volatile("" : "+v"(v)); }
// An MFMA as an asm statement, accumulating IN PLACE ("+v"): hipcc's three-address form of the builtin gave every unrolled K-step
// body its own accumulator registers (an unrolled 9-tap loop of 28 accumulator tiles then spilled ~300 registers), and an asm
// statement is issued exactly where it is written.  Hazards are the caller's: an accumulate chain on the same tile needs no
// wait state; anything ELSE that reads or writes the tile behind the last MFMA does (mfma_drain() in front of the epilogue).
template <int DT> struct MmaAsm;
template <> struct MmaAsm<AF_BF16> {
    static __device__ __forceinline__ void run(const u32x4& a, const u32x4& b, f32x4& c) {
        asm volatile("v_mfma_f32_16x16x32_bf16 %0, %1, %2, %0" : "+v"(c) : "v"(a), "v"(b));
    }
};
template <> struct MmaAsm<AF_F16> {
    static __device__ __forceinline__ void run(const u32x4& a, const u32x4& b, f32x4& c) {
        asm volatile("v_mfma_f32_16x16x32_f16 %0, %1, %2, %0" : "+v"(c) : "v"(a), "v"(b));
    }
};
// The accumulators of an asm-MFMA loop must be ordinary live registers BEFORE the loop: left to itself hipcc sinks "acc = 0" to the
// first use (a peeled first iteration: v_mov zero, zero, MFMA, v_mov ...), i.e. it writes an MFMA's C operand with vector moves
// one or two instructions in front of the asm MFMA that reads it - and reuses a fragment register the previous MFMA is still
// reading for the next tile's zeros - without the wait states its hazard recogniser would give its own MFMAs (whole-network f16
// logits moved by 2e-3, differently from run to run).  acc_live() makes the zeroed tile opaque (no rematerialisation, one register
// set for the whole loop); mfma_operands_settled() = the wait states between the last vector write of an operand and the first MFMA.
__device__ __forceinline__ void acc_live(f32x4& c) { asm volatile("" : "+v"(c)); }
__device__ __forceinline__ void mfma_operands_settled() { asm volatile("s_nop 3" ::: "memory"); }
__device__ __forceinline__ void mfma_drain() { asm volatile("s_nop 15\n\ts_nop 7" ::: "memory"); }   // > the 8-pass MFMA's 12 wait states
// What rides behind MFMA t of a K-step's second MFMA group: NP DMA pieces and NR fragment reads dealt out one per MFMA in the
// pattern piece, read, read, piece, ... (a piece first: the DMA of the stage two ahead wants all the lead it can get; the reads
// only have to be back by the next group) until one kind runs out.  group2_slot(t): >= 0: piece index; < 0: read index -1 - r;
// kNoSlot: nothing.
constexpr int kNoSlot = 1 << 20;
constexpr int group2_slot(int t, int NP, int NR) {
    int p = 0, r = 0;
    for (int i = 0;; ++i) {
        int what = kNoSlot;
        if (p < NP && (i % 3 == 0 || r >= NR)) what = p++;
        else if (r < NR) what = -1 - r++;
        if (i == t) return what;
        if (what == kNoSlot) return kNoSlot;
    }
}
// compile-time loop: f(std::integral_constant<int, 0>{}) ... f(std::integral_constant<int, N - 1>{}) (asm immediates need constants)
template <int I> struct IC { static constexpr int value = I; constexpr operator int() const { return I; } };
template <int N, int I = 0, class F> __device__ __forceinline__ void static_for(F&& f) {
    if constexpr (I < N) { f(IC<I>{}); static_for<N, I + 1>(f); }
}
// run-time dtype -> template argument: f(IC<AF_BF16>{}) or f(IC<AF_F16>{}) for the 16-bit kernels (`f` is a generic lambda that
// launches kernel<dt, ...>); with_dtype adds fp32 where a kernel has that form
template <class F> inline auto with_dtype16(int dtype, F&& f) { return dtype == AF_BF16 ? f(IC<AF_BF16>{}) : f(IC<AF_F16>{}); }
template <class F> inline auto with_dtype(int dtype, F&& f) { return dtype == AF_F32 ? f(IC<AF_F32>{}) : with_dtype16(dtype, f); }

// One-time PER-DEVICE setup.  hipFuncSetAttribute and the CU count belong to a device, and one process may drive several
// (one engine per device): every "done once" flag is therefore indexed by the current device ordinal.
constexpr int kMaxDevices = 64;
constexpr int kLdsBudget = 160 * 1024;   // LDS of a CU: what one workgroup may ask for
static inline int current_device() {
    int d = 0;
    return (hipGetDevice(&d) == hipSuccess && d >= 0 && d < kMaxDevices) ? d : -1;
}
struct DeviceOnce { bool done[kMaxDevices] = {}; };
// compute units of the current device (cached per device; af_api.hip)
int device_cus();
// How the fused stems (af_stem_pool.hip, af_stem3.hip) cut `frames` frames of `hq` pooled rows into work units (frame, band of
// pooled rows) and how many persistent workgroups walk them: both launchers run from this and af_stem_work_units answers from it
// (af_api.hip)
struct StemUnits { int bands, band_rows, units, workgroups; };
StemUnits stem_units(int frames, int hq);

// raise a kernel's dynamic-LDS limit once per (kernel instantiation, device)
#define AF_SET_MAX_LDS(kernel_ptr, bytes, what)                                                                        \
    do {                                                                                                               \
        static af::DeviceOnce once__;                                                                                  \
        const int dev__ = af::current_device();                                                                        \
        if (dev__ < 0 || !once__.done[dev__]) {                                                                        \
            hipError_t e__ = hipFuncSetAttribute(reinterpret_cast<const void*>(kernel_ptr),                            \
                                                 hipFuncAttributeMaxDynamicSharedMemorySize, (bytes));                 \
            if (e__ != hipSuccess)                                                                                     \
                return af::set_error(AF_ERR_LAUNCH, "%s: hipFuncSetAttribute: %s", what, hipGetErrorString(e__));      \
            if (dev__ >= 0) once__.done[dev__] = true;                                                                 \
        }                                                                                                              \
    } while (0)

#define AF_REQUIRE(cond, ...)                                    \
    do {                                                         \
        if (!(cond)) return af::set_error(AF_ERR_ARG, __VA_ARGS__); \
    } while (0)

#define AF_CHECK_LAUNCH(what)                                                        \
    do {                                                                             \
        hipError_t e__ = hipGetLastError();                                          \
        if (e__ != hipSuccess)                                                       \
            return af::set_error(AF_ERR_LAUNCH, "%s: %s", what, hipGetErrorString(e__)); \
    } while (0)

// ---- frame stores (af_hip.h: af_frame_store / af_frame_rect): the host checks of every entry point that is handed one ----
static inline int64_t frame_span(const af_frame_store& s) { return (int64_t)(s.height - 1) * s.row_pitch + (int64_t)s.width * 3; }   // first to last byte of one frame
struct StoreName {                                                // "store 3", or "the store" for index -1; made only for a message
    char text[24];
    explicit StoreName(int index) { index < 0 ? snprintf(text, sizeof text, "the store") : snprintf(text, sizeof text, "store %d", index); }
};
// Is this store sane?  `who`: the entry point, for the message.  `whole`: all n_frames frames must lie inside store_bytes (every
// reader of rectangles); the YUV planner writes one slot, checks that slot's bytes itself and passes false.
static inline int check_frame_store(const char* who, int index, const af_frame_store& s, bool whole = true) {
    AF_REQUIRE(s.n_frames > 0 && s.height > 0 && s.width > 0 && s.height <= 32767 && s.width <= 32767, "%s: %s of %d frames %dx%d", who,
               StoreName(index).text, s.n_frames, s.width, s.height);
    AF_REQUIRE(s.row_pitch >= (int64_t)s.width * 3 && s.row_pitch <= 0x7fffffff && s.frame_stride >= frame_span(s),
               "%s: %s: row pitch %lld, frame stride %lld for frames of %dx%d", who, StoreName(index).text, (long long)s.row_pitch,
               (long long)s.frame_stride, s.width, s.height);
    AF_REQUIRE(!whole || s.store_bytes >= (int64_t)(s.n_frames - 1) * s.frame_stride + frame_span(s), "%s: %s: %d frames do not fit a store of %lld bytes",
               who, StoreName(index).text, s.n_frames, (long long)s.store_bytes);
    return AF_OK;
}
// Frame k of stores[index], for item i of a planner (`item`: its word for one, "job" or "frame"): the index in range, a base
// pointer, a sane store, k in range - said as a slot that is written (`slot`) or a frame that is read.  Yields the store and the
// frame's first byte.
static inline int store_frame(const char* who, const char* item, int i, const af_store_ref* stores, int n_stores, int index, int k, bool slot, bool whole,
                              const af_store_ref** store, unsigned char** frame) {
    AF_REQUIRE(index >= 0 && index < n_stores, "%s: %s %d names store %d of %d", who, item, i, index, n_stores);
    const af_store_ref& st = stores[index];
    AF_REQUIRE(st.base, "%s: store %d: null base pointer", who, index);
    const int rc = check_frame_store(who, index, st.desc, whole);
    if (rc != AF_OK) return rc;
    AF_REQUIRE(k >= 0 && k < st.desc.n_frames, slot ? "%s: %s %d: slot %d leaves store %d of %d frames" : "%s: %s %d names frame %d of store %d of %d frames",
               who, item, i, k, index, st.desc.n_frames);
    *store = &st;
    *frame = (unsigned char*)st.base + (int64_t)k * st.desc.frame_stride;
    return AF_OK;
}
// Is this rectangle inside its frame, and the frame in the (checked) store?  Yields the byte offset of its first pixel and returns
// 0, or what is wrong with it for refuse_frame_rect.  `slack`: readable bytes wanted behind the rectangle's last pixel (3 for the
// warp's 6-byte tap reads).  Inside a frame those are the frame's next pixels: only a rectangle that ends the store can lack them.
static inline int frame_rect_fault(const af_frame_store& s, const af_frame_rect& r, int slack, int64_t* offset) {
    if (!(r.frame >= 0 && r.frame < s.n_frames && r.ih > 0 && r.iw > 0 && r.rx >= 0 && r.ry >= 0 && (int64_t)r.rx + r.iw <= s.width &&
          (int64_t)r.ry + r.ih <= s.height))
        return 1;
    *offset = (int64_t)r.frame * s.frame_stride + (int64_t)r.ry * s.row_pitch + (int64_t)r.rx * 3;
    return *offset + (int64_t)(r.ih - 1) * s.row_pitch + (int64_t)r.iw * 3 + slack > s.store_bytes ? 2 : 0;
}
// ... and the refusal in words; `item` is the caller's name for the rectangle ("window 1 frame 2", "rectangle 3")
static inline int refuse_frame_rect(const char* who, const char* item, int index, const af_frame_store& s, const af_frame_rect& r, int fault) {
    const StoreName name(index);
    if (fault == 1)
        return set_error(AF_ERR_ARG, "%s: %s: %dx%d at (%d,%d) of frame %d leaves the %d frames of %dx%d of %s", who, item, r.iw, r.ih, r.rx, r.ry,
                         r.frame, s.n_frames, s.width, s.height, name.text);
    return set_error(AF_ERR_ARG, "%s: %s: 3 readable bytes must follow the rectangle that ends %s of %lld bytes", who, item, name.text,
                     (long long)s.store_bytes);
}

// the event marks of a launch sequence: the i-th call records ev[i] on s, so mark() before launch 0 and after every
// launch gives launch i the span between ev[i] and ev[i + 1].  Does nothing when ev is null (an untimed run).
struct Marks {
    hipStream_t s;
    hipEvent_t* ev;
    int k;
    void operator()() { if (ev) (void)hipEventRecord(ev[k++], s); }
};

// The *_timed entry points: runs fn(ev) with n + 1 fresh events (fn marks its n launches with a Marks on ev), waits for
// the stream and writes the n device times in ms.  `who` prefixes the error messages.
template <class F>
int timed(const char* who, hipStream_t s, int n, float* ms, F fn) {
    AF_REQUIRE(ms, "%s: null ms", who);
    std::vector<hipEvent_t> ev;
    for (int i = 0; i <= n; ++i) {
        hipEvent_t e;
        if (hipEventCreate(&e) != hipSuccess) {
            for (auto& e_ : ev) (void)hipEventDestroy(e_);
            return set_error(AF_ERR_LAUNCH, "%s: cannot create event %d", who, i);
        }
        ev.push_back(e);
    }
    int rc = fn(ev.data());
    hipError_t e = hipStreamSynchronize(s);
    if (rc == AF_OK && e != hipSuccess) rc = set_error(AF_ERR_LAUNCH, "%s: %s", who, hipGetErrorString(e));
    if (rc == AF_OK)
        for (int i = 0; i < n; ++i) (void)hipEventElapsedTime(&ms[i], ev[i], ev[i + 1]);
    for (auto& e_ : ev) (void)hipEventDestroy(e_);
    return rc;
}

static inline bool aligned16(const void* p) { return (reinterpret_cast<uintptr_t>(p) & 15u) == 0; }
static inline int dtype_size(int dt) { return dt == AF_F32 ? 4 : 2; }
static inline bool dtype_ok(int dt) { return dt == AF_F32 || dt == AF_BF16 || dt == AF_F16; }
// bytes of one row of the rgb3 stem input: (w + halo) pixels of 3 x 16 bit, rounded up to 16 (af_stem3.hip reads it, af_pack*.hip write it)
static inline int rgb3_row_bytes(int w) { return ((w + AF_STEM_PAD_W_TOTAL) * 6 + 15) & ~15; }

typedef __bf16 bf16x8 __attribute__((ext_vector_type(8)));
typedef _Float16 f16x8 __attribute__((ext_vector_type(8)));

// One 16-byte operand chunk per lane -> MFMA(s) on a 16x16 fp32 accumulator tile.
//   16-bit: one v_mfma_f32_16x16x32 (8 k-values per lane, k = 8*(lane>>4)+j)
//   fp32  : four v_mfma_f32_16x16x4_f32; instruction j takes element j of the chunk, so it
//           reduces over k = {4*(lane>>4)+j}: both operands use the same k order, which is all
//           a dot product needs (exact fp32 fma chain per output element).
template <int DT> struct Mma;
template <> struct Mma<AF_BF16> {
    static __device__ __forceinline__ void run(const uint4& a, const uint4& b, f32x4& c) {
        c = __builtin_amdgcn_mfma_f32_16x16x32_bf16(__builtin_bit_cast(bf16x8, a), __builtin_bit_cast(bf16x8, b), c, 0, 0, 0);
    }
};
template <> struct Mma<AF_F16> {
    static __device__ __forceinline__ void run(const uint4& a, const uint4& b, f32x4& c) {
        c = __builtin_amdgcn_mfma_f32_16x16x32_f16(__builtin_bit_cast(f16x8, a), __builtin_bit_cast(f16x8, b), c, 0, 0, 0);
    }
};
template <> struct Mma<AF_F32> {
    static __device__ __forceinline__ void run(const uint4& a, const uint4& b, f32x4& c) {
        f32x4 af = __builtin_bit_cast(f32x4, a), bf = __builtin_bit_cast(f32x4, b);
        c = __builtin_amdgcn_mfma_f32_16x16x4f32(af[0], bf[0], c, 0, 0, 0);
        c = __builtin_amdgcn_mfma_f32_16x16x4f32(af[1], bf[1], c, 0, 0, 0);
        c = __builtin_amdgcn_mfma_f32_16x16x4f32(af[2], bf[2], c, 0, 0, 0);
        c = __builtin_amdgcn_mfma_f32_16x16x4f32(af[3], bf[3], c, 0, 0, 0);
    }
};

// element conversions (fp32 <-> storage type)
template <int DT> struct Elem;
template <> struct Elem<AF_F32> {
    typedef float type;
    static constexpr int EPC = 4;  // elements per 16-byte chunk
    static __device__ __forceinline__ float to_f32(float v) { return v; }
    static __device__ __forceinline__ float from_f32(float v) { return v; }
};
template <> struct Elem<AF_BF16> {
    typedef __bf16 type;
    static constexpr int EPC = 8;
    static __device__ __forceinline__ float to_f32(__bf16 v) { return (float)v; }
    static __device__ __forceinline__ __bf16 from_f32(float v) { return (__bf16)v; }
};
template <> struct Elem<AF_F16> {
    typedef _Float16 type;
    static constexpr int EPC = 8;
    static __device__ __forceinline__ float to_f32(_Float16 v) { return (float)v; }
    static __device__ __forceinline__ _Float16 from_f32(float v) { return (_Float16)v; }
};

// 4 consecutive channels <-> one vector store/load (16 B fp32, 8 B 16-bit)
template <int DT> struct Vec4;
template <> struct Vec4<AF_F32> {
    static __device__ __forceinline__ void store(void* p, f32x4 v) { *reinterpret_cast<f32x4*>(p) = v; }
    static __device__ __forceinline__ f32x4 load(const void* p) { return *reinterpret_cast<const f32x4*>(p); }
};
// the 16-bit types (T = __bf16 / _Float16).  store_relu: ReLU (NaN kept, like torch's clamp_min) + the one rounding + store
template <class T> struct Vec4x16 {
    typedef T t4 __attribute__((ext_vector_type(4)));
    static __device__ __forceinline__ void store(void* p, f32x4 v) {
        t4 o; o[0] = (T)v[0]; o[1] = (T)v[1]; o[2] = (T)v[2]; o[3] = (T)v[3];
        *reinterpret_cast<t4*>(p) = o;
    }
    static __device__ __forceinline__ void store_relu(void* p, f32x4 v) {
        v[0] = relu_f(v[0]); v[1] = relu_f(v[1]); v[2] = relu_f(v[2]); v[3] = relu_f(v[3]);
        store(p, v);
    }
    static __device__ __forceinline__ unsigned __attribute__((ext_vector_type(2))) pack_relu(f32x4 v) {
        t4 o; o[0] = (T)relu_f(v[0]); o[1] = (T)relu_f(v[1]); o[2] = (T)relu_f(v[2]); o[3] = (T)relu_f(v[3]);
        return __builtin_bit_cast(unsigned __attribute__((ext_vector_type(2))), o);
    }
    static __device__ __forceinline__ f32x4 load(const void* p) {
        t4 i = *reinterpret_cast<const t4*>(p);
        f32x4 o; o[0] = (float)i[0]; o[1] = (float)i[1]; o[2] = (float)i[2]; o[3] = (float)i[3];
        return o;
    }
    static __device__ __forceinline__ f32x4 unpack(unsigned __attribute__((ext_vector_type(2))) raw) {   // 8 bytes read earlier
        t4 i = __builtin_bit_cast(t4, raw);
        f32x4 o; o[0] = (float)i[0]; o[1] = (float)i[1]; o[2] = (float)i[2]; o[3] = (float)i[3];
        return o;
    }
};
template <> struct Vec4<AF_BF16> : Vec4x16<__bf16> {};
template <> struct Vec4<AF_F16> : Vec4x16<_Float16> {};
// Two MFMA accumulator tiles (lane = 4 consecutive channels of position frow, k-group fg) -> 16 contiguous bytes per lane
// without LDS: v_permlane16_swap_b32 (gfx950) exchanges the odd 16-lane rows of its first operand with the even rows of the second,
// so after swapping the packed halves of tile A and tile B a lane holds 8 consecutive channels: fg = 0 / 2: A's channels
// 0..7 / 8..15, fg = 1 / 3: B's.  (8-byte stores of 32-byte row segments cost the texture path ~3x their share)
typedef unsigned u32x2 __attribute__((ext_vector_type(2)));
__device__ __forceinline__ u32x4 swap_pair16(u32x2 a, u32x2 b) {
    const u32x2 r0 = __builtin_amdgcn_permlane16_swap(a[0], b[0], false, false);
    const u32x2 r1 = __builtin_amdgcn_permlane16_swap(a[1], b[1], false, false);
    return u32x4{r0[0], r1[0], r0[1], r1[1]};
}
}  // namespace af
