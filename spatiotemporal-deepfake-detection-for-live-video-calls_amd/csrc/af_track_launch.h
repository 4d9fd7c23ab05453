// What the launches that run af_track_core.h's update share (csrc/af_track.hip, csrc/af_live.hip): an af_track_call checked on the
// host, packed to 56 bytes of launch arguments and unpacked on the device.
#pragma once
#include "af_common.h"
#include "af_track_core.h"

namespace af {

struct TrkPacked {
    void* state;
    const void* rows;
    const int32_t* count_ptr;
    int32_t limit, form_stride;                     // form in the low 2 bits, the row stride above them
    float start_conf, start_min_size;
    double sx, sy;
};
static_assert(sizeof(TrkPacked) == 56, "argument budget");

__host__ __device__ static inline TrkPacked trk_packed(const trk::Call& c) {
    return {c.state, c.rows, c.count_ptr, c.limit, (c.stride << 2) | c.form, c.start_conf, c.start_min_size, c.sx, c.sy};
}

__host__ __device__ static inline trk::Call trk_unpacked(const TrkPacked& p) {
    trk::Call c;
    c.state = (trk::State*)p.state;
    c.rows = p.rows;
    c.count_ptr = p.count_ptr;
    c.limit = p.limit;
    c.form = p.form_stride & 3;
    c.stride = p.form_stride >> 2;
    c.start_conf = p.start_conf;
    c.start_min_size = p.start_min_size;
    c.sx = p.sx;
    c.sy = p.sy;
    c.pick = nullptr;
    return c;
}

static inline int pack_call(const af_track_call& in, trk::Call* c, const char* who, int i) {
    AF_REQUIRE(in.state && ((uintptr_t)in.state & 7) == 0, "%s: call %d: the state block is null or not 8-byte aligned", who, i);
    AF_REQUIRE(in.form >= AF_TRACK_FORM_EMPTY && in.form <= AF_TRACK_FORM_LIST64, "%s: call %d: form %d", who, i, in.form);
    c->state = (trk::State*)in.state;
    c->rows = in.rows;
    c->count_ptr = in.count_ptr;
    c->form = in.form;
    c->stride = in.row_stride;
    c->limit = in.count_ptr ? in.max_rows : in.count;
    c->start_conf = in.start_conf;
    c->start_min_size = in.start_min_size;
    c->sx = in.scale_x;
    c->sy = in.scale_y;
    c->pick = nullptr;
    if (in.form == AF_TRACK_FORM_EMPTY) {
        c->rows = nullptr;
        c->count_ptr = nullptr;
        c->limit = 0;
        return AF_OK;
    }
    AF_REQUIRE(c->limit >= 0, "%s: call %d: %d rows", who, i, c->limit);
    AF_REQUIRE(in.rows || (c->limit == 0 && !in.count_ptr), "%s: call %d: null rows", who, i);
    AF_REQUIRE(in.row_stride >= 5 && in.row_stride < (1 << 20), "%s: call %d: a row stride of %d (5 or more)", who, i, in.row_stride);
    const int el = in.form == AF_TRACK_FORM_LIST ? 4 : 8;
    AF_REQUIRE(((uintptr_t)in.rows & (el - 1)) == 0 && ((uintptr_t)in.count_ptr & 3) == 0, "%s: call %d: rows or count misaligned", who, i);
    if (in.form == AF_TRACK_FORM_ARRAY) {
        AF_REQUIRE(in.img_info[0] > 0 && in.img_info[1] > 0 && in.img_size[0] > 0 && in.img_size[1] > 0, "%s: call %d: img_info %dx%d, img_size %dx%d",
                   who, i, in.img_info[0], in.img_info[1], in.img_size[0], in.img_size[1]);
        const double a = in.img_size[0] / (double)in.img_info[1], b = in.img_size[1] / (double)in.img_info[0];
        c->sx = a < b ? a : b;
        c->sy = 0.0;
    }
    return AF_OK;
}

}  // namespace af
