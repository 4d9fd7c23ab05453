// The evaluator's chunk stage as one launch, and its host twin (include/af_hip.h, "chunk stage"): one workgroup of one
// wave runs af_runner_core.h's chunk on the run's state block and the detector's rows in device memory, the tracker's matrices and
// the frame's lists in LDS.  The chunk - frame indices and parameters - travels in the launch arguments.
#include <stddef.h>
#include <string.h>

#include "af_common.h"

#pragma clang fp contract(off)                      // to the end of the file: every product and sum is its own rounding
#include "af_runner_core.h"

namespace af {

static_assert(sizeof(af_runner_chunk) <= 4096, "kernel arguments");
static_assert(sizeof(run::Scratch) <= 60 * 1024, "runner: the scratch does not fit the LDS");
static_assert(sizeof(run::State) % 8 == 0 && sizeof(af_runner_cand) % 8 == 0 && sizeof(af_runner_frame) % 8 == 0 && sizeof(af_runner_header) % 8 == 0,
              "runner: blocks of whole doubles");
static_assert(offsetof(run::Record, cands) == sizeof(af_runner_header) + AF_RUNNER_MAX_FRAMES * sizeof(af_runner_frame), "runner: the record is packed");

__global__ __launch_bounds__(64) void runner_chunk_kernel(const af_runner_chunk c) {
    __shared__ run::Scratch sc;
    run::chunk(c, &sc);
}

static int check_chunk(const af_runner_chunk* c, const char* who) {
    AF_REQUIRE(c, "%s: null chunk", who);
    AF_REQUIRE(c->state && c->record && ((uintptr_t)c->state & 7) == 0 && ((uintptr_t)c->record & 7) == 0, "%s: the state or the record is null or not 8-byte aligned", who);
    AF_REQUIRE(c->n_frames >= 1 && c->n_frames <= AF_RUNNER_MAX_FRAMES, "%s: %d frames (1 to %d)", who, c->n_frames, AF_RUNNER_MAX_FRAMES);
    AF_REQUIRE(c->rows && c->counts && ((uintptr_t)c->rows & 3) == 0 && ((uintptr_t)c->counts & 3) == 0, "%s: rows or counts null or misaligned", who);
    AF_REQUIRE(c->max_rows >= 1 && c->max_rows < (1 << 20) && c->row_stride >= 15 && c->row_stride < (1 << 10), "%s: %d rows of %d floats (15 or more)", who,
               c->max_rows, c->row_stride);
    AF_REQUIRE((int64_t)c->n_frames * c->max_rows * c->row_stride <= c->rows_floats, "%s: %d frames of %d rows of %d floats, %lld floats of rows", who,
               c->n_frames, c->max_rows, c->row_stride, (long long)c->rows_floats);
    AF_REQUIRE(c->frame_h >= 1 && c->frame_w >= 1 && c->frame_h <= 32767 && c->frame_w <= 32767, "%s: frames of %dx%d", who, c->frame_w, c->frame_h);
    AF_REQUIRE((int64_t)run::tiles_of(c->frame_w, c->frame_h) * c->n_frames * AF_TRACK_MAX_TRACKS <= 0x7fffffff, "%s: too many tiles", who);
    AF_REQUIRE(c->detect_every >= 1 && c->mesh_every >= 1 && c->budget_frames >= 0 && c->first_slot >= 0, "%s: detect_every %d, mesh_every %d, budget %d, slot %d",
               who, c->detect_every, c->mesh_every, c->budget_frames, c->first_slot);
    for (int j = 0; j < c->n_frames; ++j) AF_REQUIRE(c->frame_idx[j] >= 0, "%s: frame %d has index %d", who, j, c->frame_idx[j]);
    return AF_OK;
}

}  // namespace af

extern "C" int64_t af_runner_state_bytes(void) { return (int64_t)sizeof(af::run::State); }

extern "C" int64_t af_runner_record_bytes(int n_frames) {
    if (n_frames < 1 || n_frames > AF_RUNNER_MAX_FRAMES) return 0;
    return (int64_t)offsetof(af::run::Record, cands) + (int64_t)n_frames * AF_TRACK_MAX_TRACKS * (int64_t)sizeof(af_runner_cand);
}

extern "C" int af_runner_reset(void* host_state, double track_thresh, double match_thresh, int buffer_size, int started) {
    using namespace af;
    AF_REQUIRE(host_state && ((uintptr_t)host_state & 7) == 0, "runner_reset: the state block is null or not 8-byte aligned");
    memset(host_state, 0, sizeof(run::State));
    run::State* rs = (run::State*)host_state;
    const int rc = af_bytetrack_reset(&rs->trk, track_thresh, match_thresh, buffer_size);
    if (rc != AF_OK) return rc;
    rs->magic = run::RUN_MAGIC;
    rs->started = started ? 1 : 0;
    return AF_OK;
}

extern "C" int af_runner_track_chunk_host(const af_runner_chunk* chunk) {
    using namespace af;
    const int rc = check_chunk(chunk, "runner_track_chunk_host");
    if (rc != AF_OK) return rc;
    static thread_local run::Scratch sc;
    run::chunk(*chunk, &sc);
    return AF_OK;
}

extern "C" int af_runner_track_chunk(const af_runner_chunk* chunk, void* stream) {
    using namespace af;
    const int rc = check_chunk(chunk, "runner_track_chunk");
    if (rc != AF_OK) return rc;
    hipLaunchKernelGGL(runner_chunk_kernel, dim3(1), dim3(64), 0, (hipStream_t)stream, *chunk);
    AF_CHECK_LAUNCH("runner_track_chunk");
    return AF_OK;
}
