// A live tick's face stage as a launch, and its host twin (include/af_hip.h, "a live tick's face stage"): one wave per
// call runs af_live_core.h's update - the tracker, then track_candidates - on the call's state block and the detector's rows in
// device memory, the tracker's matrices and the picked rows in LDS.  The calls travel in the launch arguments, the tracker's part
// packed as af_track.hip packs it; as many launches as the argument space asks for.
#include <string.h>

#include "af_common.h"

#pragma clang fp contract(off)                      // to the end of the file: every product and sum is its own rounding
#include "af_track_launch.h"
#include "af_live_core.h"

namespace af {

struct LivePacked {
    TrkPacked t;
    live::Job j;
};
struct LiveArgsHead {
    trk::Record* track_records;
    af_live_record* records;
    int32_t n, reserved;
};
constexpr int LIVE_ARG_BYTES = 4096;                // what a launch may carry in its arguments
constexpr int LIVE_PER_LAUNCH = (LIVE_ARG_BYTES - (int)sizeof(LiveArgsHead)) / (int)sizeof(LivePacked);
struct LiveArgs {
    LiveArgsHead h;
    LivePacked c[LIVE_PER_LAUNCH];
};
static_assert(LIVE_PER_LAUNCH >= 1 && sizeof(LiveArgs) <= LIVE_ARG_BYTES, "kernel arguments");
static_assert(sizeof(LivePacked) % 8 == 0, "live: packed calls of whole doubles");
static_assert(sizeof(live::Scratch) <= 48 * 1024, "live: the scratch does not fit the LDS");
static_assert(sizeof(live::State) % 8 == 0 && sizeof(af_live_record) % 8 == 0 && sizeof(af_live_entry) % 8 == 0, "live: blocks of whole doubles");
static_assert(sizeof(af_live_record) == 32 + AF_TRACK_MAX_TRACKS * sizeof(af_live_entry), "live: the record is packed");

__global__ __launch_bounds__(64) void live_update_kernel(const LiveArgs a) {
    __shared__ live::Scratch sc;
    const int b = blockIdx.x;
    if (b >= a.h.n) return;
    const trk::Call c = trk_unpacked(a.c[b].t);
    live::update(c, a.c[b].j, a.h.track_records + b, a.h.records + b, &sc);
}

// the tracker's call as af_track.hip checks it, then what the candidate stage reads beyond it
static int pack_live(const af_live_call& in, trk::Call* c, live::Job* j, const char* who, int i) {
    const int rc = pack_call(in.track, c, who, i);
    if (rc != AF_OK) return rc;
    AF_REQUIRE(in.frame_idx >= 0 && in.slot >= 0 && in.mesh_every >= 1, "%s: call %d: frame %d, slot %d, mesh_every %d", who, i, in.frame_idx, in.slot,
               in.mesh_every);
    AF_REQUIRE(in.frame_h >= 1 && in.frame_w >= 1 && in.frame_h <= 32767 && in.frame_w <= 32767, "%s: call %d: frames of %dx%d", who, i, in.frame_w, in.frame_h);
    AF_REQUIRE(in.n_purged >= 0 && in.n_purged <= AF_TRACK_MAX_TRACKS, "%s: call %d: %d purged tids (at most %d)", who, i, in.n_purged, AF_TRACK_MAX_TRACKS);
    AF_REQUIRE((int64_t)run::tiles_of(in.frame_w, in.frame_h) * AF_TRACK_MAX_TRACKS <= 0x7fffffff, "%s: call %d: too many tiles", who, i);
    if (c->form == AF_TRACK_FORM_LIST && c->limit > 0) {   // the candidate stage reads the five points of every row
        AF_REQUIRE(c->stride >= 15 && c->stride < (1 << 10) && c->limit < (1 << 20), "%s: call %d: %d rows of %d floats (15 or more)", who, i, c->limit, c->stride);
        AF_REQUIRE((int64_t)c->limit * c->stride <= in.rows_floats, "%s: call %d: %d rows of %d floats, %lld floats of rows", who, i, c->limit, c->stride,
                   (long long)in.rows_floats);
    }
    j->crop_scale = in.crop_scale;
    for (int k = 0; k < 4; ++k) j->exclude[k] = in.exclude[k];
    j->frame_idx = in.frame_idx; j->slot = in.slot; j->mesh_every = in.mesh_every;
    j->frame_h = in.frame_h; j->frame_w = in.frame_w; j->n_purged = in.n_purged;
    for (int k = 0; k < AF_TRACK_MAX_TRACKS; ++k) j->purged[k] = k < in.n_purged ? in.purged[k] : 0;
    return AF_OK;
}

}  // namespace af

extern "C" int64_t af_live_state_bytes(void) { return (int64_t)sizeof(af::live::State); }
extern "C" int64_t af_live_record_bytes(void) { return (int64_t)sizeof(af_live_record); }
extern "C" int af_live_calls_per_launch(void) { return af::LIVE_PER_LAUNCH; }

extern "C" int af_live_reset(void* host_state, double track_thresh, double match_thresh, int buffer_size) {
    using namespace af;
    AF_REQUIRE(host_state && ((uintptr_t)host_state & 7) == 0, "live_reset: the state block is null or not 8-byte aligned");
    memset(host_state, 0, sizeof(live::State));
    live::State* ls = (live::State*)host_state;
    const int rc = af_bytetrack_reset(&ls->trk, track_thresh, match_thresh, buffer_size);
    if (rc != AF_OK) return rc;
    ls->trk.reserved = live::LIVE_MAGIC;
    return AF_OK;
}

extern "C" int af_live_update_host(const af_live_call* call, void* track_record, void* record) {
    using namespace af;
    const char* who = "live_update_host";
    AF_REQUIRE(call && track_record && record && ((uintptr_t)track_record & 7) == 0 && ((uintptr_t)record & 7) == 0,
               "%s: null call or records, or a misaligned record", who);
    trk::Call c;
    live::Job j;
    const int rc = pack_live(*call, &c, &j, who, 0);
    if (rc != AF_OK) return rc;
    static thread_local live::Scratch sc;
    live::update(c, j, (trk::Record*)track_record, (af_live_record*)record, &sc);
    return AF_OK;
}

extern "C" int af_live_update_calls(const af_live_call* calls, int n_calls, void* track_records, void* records, void* stream) {
    using namespace af;
    const char* who = "live_update_calls";
    AF_REQUIRE(calls && track_records && records && ((uintptr_t)track_records & 7) == 0 && ((uintptr_t)records & 7) == 0,
               "%s: null calls or records, or misaligned records", who);
    AF_REQUIRE(n_calls >= 1 && n_calls <= AF_TRACK_MAX_CALLS, "%s: %d calls (1 to %d)", who, n_calls, AF_TRACK_MAX_CALLS);
    static thread_local LiveArgs launches[(AF_TRACK_MAX_CALLS + LIVE_PER_LAUNCH - 1) / LIVE_PER_LAUNCH];
    for (int i = 0; i < n_calls; ++i) {                 // every call is checked before the first launch
        trk::Call c;
        LiveArgs& a = launches[i / LIVE_PER_LAUNCH];
        const int rc = pack_live(calls[i], &c, &a.c[i % LIVE_PER_LAUNCH].j, who, i);
        if (rc != AF_OK) return rc;
        for (int k = 0; k < i; ++k) AF_REQUIRE(calls[k].track.state != calls[i].track.state, "%s: calls %d and %d share a state block", who, k, i);
        a.c[i % LIVE_PER_LAUNCH].t = trk_packed(c);
    }
    for (int lo = 0; lo < n_calls; lo += LIVE_PER_LAUNCH) {
        LiveArgs& a = launches[lo / LIVE_PER_LAUNCH];
        const int n = n_calls - lo < LIVE_PER_LAUNCH ? n_calls - lo : LIVE_PER_LAUNCH;
        a.h.track_records = (trk::Record*)track_records + lo;
        a.h.records = (af_live_record*)records + lo;
        a.h.n = n;
        a.h.reserved = 0;
        hipLaunchKernelGGL(live_update_kernel, dim3((unsigned)n), dim3(64), 0, (hipStream_t)stream, a);
        AF_CHECK_LAUNCH(who);
    }
    return AF_OK;
}
