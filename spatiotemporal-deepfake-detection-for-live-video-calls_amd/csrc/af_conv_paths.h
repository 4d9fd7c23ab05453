// Host side shared by the specialised convolution paths (af_conv_small / 133 / 133g / 311 / 111, the fused pairs af_conv_ca / cpa and
// af_block_abc) and by af_conv.hip, which chooses among them: the words their shape tests are written in, the one launcher of a
// 512-thread kernel with dynamic LDS, the two grid rules of the persistent kernels, and the record a layer path is entered in
// af_conv.hip's table with.  Host code only.  Adding a path: DESIGN.md 22.
#pragma once
#include "af_common.h"

namespace af {

// ---- shape vocabulary over af_conv_desc
static inline bool kernel_is(const af_conv_desc* d, int kt, int kh, int kw) { return d->kt == kt && d->kh == kh && d->kw == kw; }
static inline bool unit_stride(const af_conv_desc* d) { return d->st == 1 && d->sh == 1 && d->sw == 1; }
static inline bool pad_is(const af_conv_desc* d, int pt, int ph, int pw) { return d->pt == pt && d->ph == ph && d->pw == pw; }
// 1x1x1, stride 1, no padding
static inline bool pointwise(const af_conv_desc* d) { return kernel_is(d, 1, 1, 1) && unit_stride(d) && pad_is(d, 0, 0, 0); }
// 3x1x1, stride 1, padding (1,0,0): the `a` convs
static inline bool temporal3(const af_conv_desc* d) { return kernel_is(d, 3, 1, 1) && unit_stride(d) && pad_is(d, 1, 0, 0); }
// the same t, h, w of the input; same_input: and the same n
static inline bool same_frames(const af_conv_desc* a, const af_conv_desc* b) { return a->t == b->t && a->h == b->h && a->w == b->w; }
static inline bool same_input(const af_conv_desc* a, const af_conv_desc* b) { return a->n == b->n && same_frames(a, b); }
static inline bool keeps_size(const af_conv_desc* d) { return d->to == d->t && d->ho == d->h && d->wo == d->w; }

// ---- argument lists of the entry points
template <class... P> static inline bool none_null(P... p) { return (... && (p != nullptr)); }
template <class... P> static inline bool all_aligned16(P... p) { return (... && aligned16(p)); }

// ---- grids of the persistent kernels: one workgroup per CU (at most one per unit), workgroup b walks units b, b + grid, ...
static inline int persistent_grid(long long units) {
    const int cus = device_cus();
    return units < cus ? (int)units : cus;
}
// a persistent stream only pays with several tiles per workgroup (small batches stay on the generic path / keep their two launches)
static inline bool fills_chip(long long tiles) { return tiles >= 4LL * device_cus(); }

// ---- the launch of a 512-thread kernel with `lds` bytes of dynamic LDS: refuses more than a CU has, raises the kernel's limit once
// per (instantiation, device), launches, checks.  `what`: the path's name in the messages ("conv_ca"; its kernel: "conv_ca_kernel").
template <auto Kernel, class Args>
static int launch_lds(const char* what, int grid, int lds, hipStream_t stream, const Args& a) {
    if (lds > kLdsBudget) return set_error(AF_ERR_ARG, "%s: %d bytes of LDS needed", what, lds);
    AF_SET_MAX_LDS(Kernel, kLdsBudget, what);
    hipLaunchKernelGGL(Kernel, dim3(grid), dim3(512), lds, stream, a);
    hipError_t e = hipGetLastError();
    if (e != hipSuccess) return set_error(AF_ERR_LAUNCH, "%s_kernel: %s", what, hipGetErrorString(e));
    return AF_OK;
}

// ---- layer paths.  The ids af_conv_variant reports (names: variant_info in af_conv.hip): conv_igemm tiles and specialised paths
enum { VAR_128x256 = 0, VAR_64x256 = 1, VAR_128x128 = 2, VAR_64x128 = 3, VAR_C133 = 4, VAR_128x128_R2 = 5, VAR_256x256 = 6,
       VAR_128x512 = 7, VAR_C311 = 8, VAR_SMALL = 9, VAR_C111 = 10, VAR_C133G = 11, VAR_256x224 = 12, VAR_C311G = 13, VAR_COUNT = 14 };

// One call of af_conv3d_bn_act / af_conv3d_dual_bn_act as a path sees it (d2, in2, w2: the second K segment, or null).  The
// questions af_conv_variant and af_conv_work_units ask carry the two descriptors only.
struct ConvCall {
    const af_conv_desc* d;
    const af_conv_desc* d2;
    const void* in;
    const void* w;
    const void* in2;
    const void* w2;
    const float* scale;
    const float* shift;
    const void* residual;
    void* out;
    int out_ld;          // 0 in a question; in a run: the row stride in elements, never 0
    hipStream_t stream;
};
// A specialised path: a row of conv_path's table (af_conv.hip), which is tried in order.  `applies`: does the layer take it; `work`: the
// units it is cut into and the workgroups `run` launches (null: not cut into units); `run`: the launch, for a call that `applies`
// accepted and conv_common checked.  before_segment_checks: the path takes neither a second segment nor a residual and runs in
// front of conv_common's checks of those.  A path file exports its row through an accessor: the row holds pointers to host functions,
// and a namespace-scope constant would be emitted into the device code as well.
struct ConvPath {
    int variant;
    bool (*applies)(const ConvCall&);
    void (*work)(const ConvCall&, long long* units, int* workgroups);
    int (*run)(const ConvCall&);
    bool before_segment_checks;
};
const ConvPath& conv_small_path();    // af_conv_small.hip: direct-gather MFMA path for narrow layers (SlowFast's Fast pathway)
const ConvPath& conv133_path();      // af_conv133.hip: register-resident-weights 1x3x3 64 -> 64 (s2 `b` convs)
const ConvPath& conv133g_path();     // af_conv133g.hip: frame / band resident 1x3x3 into 128 / 256 channels (s3 / s4 `b` convs)
const ConvPath& conv311g_path();     // ... and its temporal mode: 3x1x1 into 128 / 256 channels (s3 / s4 `a` convs)
const ConvPath& conv311_path();      // af_conv311.hip: time-tiled 3x1x1 -> 64 channels (s2 `a` convs)
const ConvPath& conv111_path();      // af_conv111.hip: persistent weights-in-registers 1x1x1 stream (short-K `c` convs of s2 / s3)

// ---- fused pairs: not layer paths; af_conv.hip's pair entry points call them
// af_conv133g.hip: b (1x3x3) + c (1x1x1, + residual, + ReLU) of a bottleneck as one launch
bool conv133g_fused_applies(const af_conv_desc* db, const af_conv_desc* dc, int out_ld);
int conv133g_fused_run(const af_conv_desc* db, const void* in, const void* wb, const float* scale_b, const float* shift_b,
                       const af_conv_desc* dc, const void* wc, const float* scale_c, const float* shift_c, const void* residual,
                       void* out, int out_ld, hipStream_t stream);
// af_conv_ca.hip: c(i) -> a(i+1) across a block boundary of s2 in the time-tiled layout (the trunk slab is produced in LDS)
bool conv_ca_applies(const af_conv_desc* dc, const af_conv_desc* d1, const af_conv_desc* da);
int conv_ca_run(const af_conv_desc* dc, const void* inb, const void* wc, const void* in1, const void* w1, const float* scale_c,
                const float* shift_c, const void* residual, void* outx, const af_conv_desc* da, const void* wa, const float* scale_a,
                const float* shift_a, void* outa, hipStream_t stream);
// af_conv_ca_work_units: the tiles of the pair and the grid conv_ca_run launches; false: not fused
bool conv_ca_work(const af_conv_desc* dc, const af_conv_desc* d1, const af_conv_desc* da, long long* tiles, int* workgroups, int* form,
                  int* pixels);

}  // namespace af
