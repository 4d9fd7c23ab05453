// The device tracker's launch and its host twin (include/af_hip.h, "device tracker"): one wave per tracker runs
// af_track_core.h's update on the tracker's state block in device memory, cost matrices and lists in LDS; a grid of up to
// AF_TRACK_MAX_CALLS trackers.  The calls travel in the launch arguments, packed to 56 bytes each.
#include <string.h>

#include "af_common.h"

#pragma clang fp contract(off)                      // to the end of the file: every product and sum is its own rounding
#include "af_track_launch.h"

namespace af {

struct TrkArgs {
    trk::Record* records;
    int32_t n, reserved;
    TrkPacked c[AF_TRACK_MAX_CALLS];
};
static_assert(sizeof(TrkArgs) <= 4096, "kernel arguments");
static_assert(sizeof(trk::Scratch) <= 48 * 1024, "tracker: the scratch does not fit the LDS");
static_assert(sizeof(trk::State) % 8 == 0 && sizeof(trk::Record) % 8 == 0, "tracker: blocks of whole doubles");

__global__ __launch_bounds__(64) void bytetrack_kernel(TrkArgs a) {
    __shared__ trk::Scratch sc;
    const int b = blockIdx.x;
    if (b >= a.n) return;
    const trk::Call c = trk_unpacked(a.c[b]);
    trk::update(c, a.records + b, &sc);
}

__global__ __launch_bounds__(256) void track_probe_kernel(const double* x, const double* y, double* q, double* r, int n) {
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    q[i] = x[i] / y[i];
    r[i] = sqrt(x[i]);
}

}  // namespace af

extern "C" int64_t af_bytetrack_state_bytes(void) { return (int64_t)sizeof(af::trk::State); }
extern "C" int64_t af_bytetrack_record_bytes(void) { return (int64_t)sizeof(af::trk::Record); }

extern "C" int af_bytetrack_reset(void* state, double track_thresh, double match_thresh, int buffer_size) {
    using namespace af;
    AF_REQUIRE(state && ((uintptr_t)state & 7) == 0, "bytetrack_reset: the state block is null or not 8-byte aligned");
    AF_REQUIRE(buffer_size >= 0, "bytetrack_reset: a buffer of %d frames", buffer_size);
    memset(state, 0, sizeof(trk::State));
    trk::State* st = (trk::State*)state;
    st->magic = trk::TRK_MAGIC;
    st->max_time_lost = buffer_size;
    st->track_thresh = track_thresh;
    st->match_thresh = match_thresh;
    st->det_thresh = track_thresh + 0.1;
    return AF_OK;
}

extern "C" int af_bytetrack_update_host(const af_track_call* call, void* record) {
    using namespace af;
    const char* who = "bytetrack_update_host";
    AF_REQUIRE(call && record && ((uintptr_t)record & 7) == 0, "%s: null call or record, or a misaligned record", who);
    trk::Call c;
    const int rc = pack_call(*call, &c, who, 0);
    if (rc != AF_OK) return rc;
    static thread_local trk::Scratch sc;
    trk::update(c, (trk::Record*)record, &sc);
    return AF_OK;
}

extern "C" int af_bytetrack_update_calls(const af_track_call* calls, int n_calls, void* records, void* stream) {
    using namespace af;
    const char* who = "bytetrack_update_calls";
    AF_REQUIRE(calls && records && ((uintptr_t)records & 7) == 0, "%s: null calls or records, or misaligned records", who);
    AF_REQUIRE(n_calls >= 1 && n_calls <= AF_TRACK_MAX_CALLS, "%s: %d calls (1 to %d)", who, n_calls, AF_TRACK_MAX_CALLS);
    TrkArgs a = {};
    a.records = (trk::Record*)records;
    a.n = n_calls;
    for (int i = 0; i < n_calls; ++i) {
        trk::Call c;
        const int rc = pack_call(calls[i], &c, who, i);
        if (rc != AF_OK) return rc;
        for (int j = 0; j < i; ++j) AF_REQUIRE(a.c[j].state != (void*)c.state, "%s: calls %d and %d share a state block", who, j, i);
        a.c[i] = trk_packed(c);
    }
    hipLaunchKernelGGL(bytetrack_kernel, dim3((unsigned)n_calls), dim3(64), 0, (hipStream_t)stream, a);
    AF_CHECK_LAUNCH(who);
    return AF_OK;
}

extern "C" int af_track_probe_f64(const double* x, const double* y, double* q, double* r, int n, void* stream) {
    using namespace af;
    const char* who = "track_probe_f64";
    AF_REQUIRE(x && y && q && r && n >= 1, "%s: null pointer or %d values", who, n);
    hipLaunchKernelGGL(track_probe_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, (hipStream_t)stream, x, y, q, r, n);
    AF_CHECK_LAUNCH(who);
    return AF_OK;
}
