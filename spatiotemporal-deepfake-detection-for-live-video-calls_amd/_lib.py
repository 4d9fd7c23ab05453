"""ctypes binding of libafhip.so (include/af_hip.h).  There is NO fallback: if the HIP library is
missing or does not export the ABI this file declares, importing fails loudly."""
import ctypes as C
import os

HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.environ.get("AF_HIP_LIB") or os.path.join(HERE, "libafhip.so")   # override: kernel experiments

AF_F32, AF_BF16, AF_F16 = 0, 1, 2
(AF_OP_STEM, AF_OP_CONV, AF_OP_MAXPOOL, AF_OP_HEAD, AF_OP_PACK_F32, AF_OP_PACK_U8, AF_OP_CONV_DUAL, AF_OP_STEM_POOL, AF_OP_AVGPOOL,
 AF_OP_LINEAR, AF_OP_TSTEM, AF_OP_TOKENS, AF_OP_LAYERNORM, AF_OP_ATTENTION, AF_OP_GELU, AF_OP_CONV_BC, AF_OP_PACK3_F32,
 AF_OP_PACK3_U8, AF_OP_STEM3_POOL, AF_OP_CONV_CA, AF_OP_BLOCK_ABC, AF_OP_TSTEM_POOL3, AF_OP_CONV_CPA, AF_OP_PACK_PATHWAYS_U8,
 AF_OP_NOP) = range(25)
AF_PACK_C4, AF_PACK_RGB3 = 0, 1
AF_ABI_VERSION = 6
STEM_PAD_T, STEM_PAD_H, STEM_PAD_W_LEFT, STEM_PAD_W_TOTAL, STEM_CPAD = 2, 3, 3, 8, 4

DTYPE_CODES = {"f32": AF_F32, "bf16": AF_BF16, "f16": AF_F16}


class ConvDesc(C.Structure):
    _fields_ = [(n, C.c_int32) for n in (
        "n", "t", "h", "w", "cin", "cout", "kt", "kh", "kw", "st", "sh", "sw", "pt", "ph", "pw",
        "to", "ho", "wo", "relu", "dtype", "tpool")]


class StageRect(C.Structure):
    _fields_ = [("src", C.c_void_p), ("dst_offset", C.c_int64), ("src_pitch", C.c_int64), ("rows", C.c_int32), ("row_bytes", C.c_int32)]


class AlignFrame(C.Structure):
    _fields_ = [("offset", C.c_int64), ("ih", C.c_int32), ("iw", C.c_int32), ("x", C.c_int32), ("y", C.c_int32)]


class AlignCrop(C.Structure):
    _fields_ = [("src", C.c_void_p), ("pitch", C.c_int64), ("h", C.c_int32), ("w", C.c_int32), ("x", C.c_int32), ("y", C.c_int32)]


ALIGN_MAX_FRAMES = 64


class WindowDesc(C.Structure):
    _fields_ = [("tfm", C.c_double * 6), ("canvas_h", C.c_int32), ("canvas_w", C.c_int32)]


WINDOW_MAX_BATCH, WINDOW_MAX_SIZE, WINDOW_TABLE_HEADER = 64, 1024, 16


class FrameStore(C.Structure):
    _fields_ = [("store_bytes", C.c_int64), ("frame_stride", C.c_int64), ("row_pitch", C.c_int64), ("n_frames", C.c_int32),
                ("height", C.c_int32), ("width", C.c_int32), ("reserved", C.c_int32)]


class FrameRect(C.Structure):
    _fields_ = [(n, C.c_int32) for n in ("frame", "rx", "ry", "ih", "iw", "x", "y", "reserved")]


class TrackCall(C.Structure):
    """af_track_call (include/af_hip.h, "device tracker")"""
    _fields_ = [("state", C.c_void_p), ("rows", C.c_void_p), ("count_ptr", C.c_void_p), ("count", C.c_int32), ("max_rows", C.c_int32),
                ("form", C.c_int32), ("row_stride", C.c_int32), ("img_info", C.c_int32 * 2), ("img_size", C.c_int32 * 2),
                ("start_conf", C.c_float), ("start_min_size", C.c_float), ("scale_x", C.c_double), ("scale_y", C.c_double)]


AF_TRACK_MAX_TRACKS, AF_TRACK_MAX_DETS, AF_TRACK_MAX_CALLS = 32, 32, 64
AF_TRACK_FORM_EMPTY, AF_TRACK_FORM_LIST, AF_TRACK_FORM_ARRAY, AF_TRACK_FORM_LIST64 = 0, 1, 2, 3
AF_TRACK_OVERFLOW_DETS, AF_TRACK_OVERFLOW_TRACKS, AF_TRACK_NOT_RESET = 1, 2, 3


class LiveCall(C.Structure):
    """af_live_call (include/af_hip.h, "a live tick's face stage")"""
    _fields_ = [("track", TrackCall), ("rows_floats", C.c_int64), ("frame_idx", C.c_int32), ("slot", C.c_int32), ("mesh_every", C.c_int32),
                ("frame_h", C.c_int32), ("frame_w", C.c_int32), ("n_purged", C.c_int32), ("crop_scale", C.c_double), ("exclude", C.c_double * 4),
                ("purged", C.c_int32 * AF_TRACK_MAX_TRACKS)]


class LiveQualityJob(C.Structure):
    """af_live_quality_job: a candidate record in device memory, the index of its store in the launch and its frame's slot"""
    _fields_ = [("record", C.c_void_p), ("store", C.c_int32), ("slot", C.c_int32)]


AF_LIVE_EXCLUDED, AF_LIVE_NO_POINTS, AF_LIVE_EMPTY_BOX, AF_LIVE_CANDIDATE, AF_LIVE_REFRESHED, AF_LIVE_BAD = 1, 2, 4, 8, 16, 32


AF_RUNNER_MAX_FRAMES = 64
AF_RUNNER_NEED_DETECT, AF_RUNNER_DROPPED, AF_RUNNER_PROCESSED, AF_RUNNER_NOT_REACHED, AF_RUNNER_REFUSED = 1, 2, 4, 8, 16
AF_RUNNER_CAND_BAD = 1


class RunnerChunk(C.Structure):
    """af_runner_chunk (include/af_hip.h, "chunk stage")"""
    _fields_ = [("state", C.c_void_p), ("rows", C.c_void_p), ("counts", C.c_void_p), ("record", C.c_void_p), ("rows_floats", C.c_int64),
                ("n_frames", C.c_int32), ("max_rows", C.c_int32), ("row_stride", C.c_int32), ("first_slot", C.c_int32),
                ("frame_h", C.c_int32), ("frame_w", C.c_int32), ("detect_every", C.c_int32), ("start_after_n", C.c_int32),
                ("mesh_every", C.c_int32), ("budget_frames", C.c_int32),
                ("start_conf", C.c_float), ("start_min_size", C.c_float), ("min_det_side", C.c_float), ("min_det_area", C.c_float),
                ("bottom_limit", C.c_float), ("reserved", C.c_float), ("min_track_side", C.c_double), ("crop_scale", C.c_double),
                ("frame_idx", C.c_int32 * AF_RUNNER_MAX_FRAMES)]


class QualitySums(C.Structure):
    _fields_ = [("s1", C.c_int64), ("s2", C.c_int64), ("n_px", C.c_int32), ("reserved", C.c_int32)]


QUALITY_MAX_RECTS = 64


class StoreRef(C.Structure):
    """a frame store named for the several-stores launches: device base pointer, description, byte order"""
    _fields_ = [("base", C.c_void_p), ("desc", FrameStore), ("bgr", C.c_int32), ("reserved", C.c_int32)]


MAX_STORES = 64


class YuvFrameDesc(C.Structure):
    """af_yuv_frame: one 4:2:0 frame on the device and the store slot it is converted into"""
    _fields_ = [("y", C.c_void_p), ("u", C.c_void_p), ("v", C.c_void_p), ("y_pitch", C.c_int64), ("c_pitch", C.c_int64),
                ("h", C.c_int32), ("w", C.c_int32), ("interleaved", C.c_int32), ("swap_uv", C.c_int32), ("store", C.c_int32),
                ("slot", C.c_int32)]


class YuvItem(C.Structure):
    """af_yuv_item: what af_yuv420_plan_u8 fills and af_yuv420_to_rgb_u8 launches over"""
    _fields_ = [("y", C.c_void_p), ("c0", C.c_void_p), ("c1", C.c_void_p), ("dst", C.c_void_p), ("y_pitch", C.c_int32),
                ("c_pitch", C.c_int32), ("dst_pitch", C.c_int32), ("first_tile", C.c_int32), ("h", C.c_uint16), ("w", C.c_uint16),
                ("interleaved", C.c_uint8), ("swap_uv", C.c_uint8), ("bgr", C.c_uint8), ("reserved", C.c_uint8)]


YUV_MAX_FRAMES, YUV_RUN, YUV_TILE = 64, 8, 256


class YuvFrameEx(C.Structure):
    """af_yuv_frame_ex: one YUV frame of any built layout, depth and colour on the device and the store slot it is converted into"""
    _fields_ = [("y", C.c_void_p), ("u", C.c_void_p), ("v", C.c_void_p), ("y_pitch", C.c_int64), ("c_pitch", C.c_int64),
                ("h", C.c_int32), ("w", C.c_int32), ("layout", C.c_int32), ("order", C.c_int32), ("matrix", C.c_int32),
                ("full_range", C.c_int32), ("store", C.c_int32), ("slot", C.c_int32)]


class YuvItemEx(C.Structure):
    """af_yuv_item_ex: what af_yuv_plan_ex_u8 fills and af_yuv_to_rgb_ex_u8 launches over"""
    _fields_ = [("y", C.c_void_p), ("c0", C.c_void_p), ("c1", C.c_void_p), ("dst", C.c_void_p), ("y_pitch", C.c_int32),
                ("c_pitch", C.c_int32), ("dst_pitch", C.c_int32), ("first_tile", C.c_int32), ("h", C.c_uint16), ("w", C.c_uint16),
                ("layout", C.c_uint8), ("order", C.c_uint8), ("bgr", C.c_uint8), ("colour", C.c_uint8)]


# AF_YUV_LAYOUT_*
YUV_420P, YUV_420SP, YUV_422P, YUV_422SP, YUV_444P, YUV_422PK, YUV_420SP16, YUV_420P16 = range(8)


class ResizeJob(C.Structure):
    """af_resize_job: frame `frame` of store `store` -> dh rows of dw pixels at the device pointer dst"""
    _fields_ = [("store", C.c_int32), ("frame", C.c_int32), ("dst", C.c_void_p), ("dst_pitch", C.c_int64), ("dh", C.c_int32), ("dw", C.c_int32)]


RESIZE_MAX_FRAMES, RESIZE_MAX_SIDE, RESIZE_KIND = 64, 8192, 0x315a5352
RESIZE_COPY, RESIZE_AREA2, RESIZE_LINEAR = 0, 1, 2


class ResizeHeader(C.Structure):
    """af_resize_header: the first bytes of the table af_resize_plan_u8 fills"""
    _fields_ = [("kind", C.c_int32), ("n", C.c_int32), ("total_tiles", C.c_int32), ("used_bytes", C.c_int32),
                ("first_tile", C.c_int32 * (RESIZE_MAX_FRAMES + 1)), ("reserved", C.c_int32 * 3)]


class ResizeItem(C.Structure):
    """af_resize_item: one job as the kernel reads it"""
    _fields_ = [("src", C.c_void_p), ("dst", C.c_void_p), ("src_pitch", C.c_int32), ("dst_pitch", C.c_int32), ("h", C.c_int32), ("w", C.c_int32),
                ("dh", C.c_int32), ("dw", C.c_int32), ("mode", C.c_int32), ("runs_x", C.c_int32), ("xtab", C.c_int32), ("ytab", C.c_int32)]


class ResizeCoef(C.Structure):
    """af_resize_coef: first tap and the two 11-bit weights of one destination column or row"""
    _fields_ = [("idx", C.c_int32), ("a0", C.c_int16), ("a1", C.c_int16)]


class CaptureFrame(C.Structure):
    """af_capture_frame: the rectangle of one captured bitmap on the device and the store slot it goes into"""
    _fields_ = [("src", C.c_void_p), ("pitch", C.c_int64), ("h", C.c_int32), ("w", C.c_int32), ("channels", C.c_int32), ("src_bgr", C.c_int32),
                ("store", C.c_int32), ("slot", C.c_int32), ("dh", C.c_int32), ("dw", C.c_int32)]


CAPTURE_MAX_FRAMES, CAPTURE_MAX_SIDE, CAPTURE_KIND = 64, 8192, 0x31504143
CAPTURE_COPY, CAPTURE_AREA2, CAPTURE_BOX, CAPTURE_TABLE = 0, 1, 2, 3
CAPTURE_RUN, CAPTURE_TILE = 4, 256


class CaptureHeader(C.Structure):
    """af_capture_header: the first bytes of the table af_capture_plan_u8 fills"""
    _fields_ = [("kind", C.c_int32), ("n", C.c_int32), ("total_tiles", C.c_int32), ("used_bytes", C.c_int32),
                ("first_tile", C.c_int32 * (CAPTURE_MAX_FRAMES + 1)), ("reserved", C.c_int32 * 3)]


class CaptureItem(C.Structure):
    """af_capture_item: one frame as the kernel reads it"""
    _fields_ = [("src", C.c_void_p), ("dst", C.c_void_p), ("src_pitch", C.c_int32), ("dst_pitch", C.c_int32), ("h", C.c_int32), ("w", C.c_int32),
                ("dh", C.c_int32), ("dw", C.c_int32), ("mode", C.c_int32), ("runs_x", C.c_int32), ("xtab", C.c_int32), ("ytab", C.c_int32),
                ("kx", C.c_int32), ("ky", C.c_int32), ("inv_area", C.c_float), ("channels", C.c_uint8), ("swap", C.c_uint8),
                ("dword", C.c_uint8), ("xk", C.c_uint8)]


class CaptureTap(C.Structure):
    """af_capture_tap: one entry of an area table: source index and fp32 weight"""
    _fields_ = [("idx", C.c_int32), ("weight", C.c_float)]


class TileSource(C.Structure):
    """af_tile_source: h rows of w packed 3-byte pixels on the device"""
    _fields_ = [("pixels", C.c_void_p), ("pitch", C.c_int64), ("h", C.c_int32), ("w", C.c_int32), ("bgr", C.c_int32), ("reserved", C.c_int32)]


class TileParams(C.Structure):
    """af_tile_params: LargestTilePicker._valid's constants; area_min is the host's own 0.10 * W * H"""
    _fields_ = [("min_w", C.c_int32), ("min_h", C.c_int32), ("ar_lo", C.c_double), ("ar_hi", C.c_double), ("area_min", C.c_double)]


TILE_MAX_BOXES, TILE_MIN_SIDE, TILE_MAX_SIDE = 64, 8, 8192


class TileBox(C.Structure):
    _fields_ = [(n, C.c_int32) for n in ("root", "x", "y", "w", "h", "n_px")] + [("s1", C.c_int64), ("s2", C.c_int64)]


class TileResult(C.Structure):
    """af_tile_result: the first bytes of the workspace after a call"""
    _fields_ = [(n, C.c_int32) for n in ("error", "count", "overflow", "components", "x1", "y1", "x2", "y2", "union_count")] + [
        ("reserved", C.c_int32 * 3), ("box", TileBox * TILE_MAX_BOXES)]


class TileOutputs(C.Structure):
    """af_tile_outputs: optional tight copies of the stages"""
    _fields_ = [(n, C.c_void_p) for n in ("g", "cls", "edges", "mask", "labels", "boxes", "external")]


class RankRow(C.Structure):
    """af_rank_row: what af_rank_metrics_rows writes per index row"""
    _fields_ = [("u2", C.c_int64), ("ap_sum", C.c_double), ("P", C.c_int32), ("N", C.c_int32), ("tp_cut", C.c_int32), ("fp_cut", C.c_int32)]


RANK_MAX_POOL, RANK_THREADS = 16384, 256


class Pcg64State(C.Structure):
    """af_pcg64_state: numpy's PCG64 bit_generator.state, the 128-bit words in 64-bit halves"""
    _fields_ = [("state_hi", C.c_uint64), ("state_lo", C.c_uint64), ("inc_hi", C.c_uint64), ("inc_lo", C.c_uint64),
                ("has_uint32", C.c_int32), ("uinteger", C.c_uint32)]


class DrawResult(C.Structure):
    """af_draw_result: what af_pcg64_draw_rows leaves on the device beside the rows"""
    _fields_ = [("consumed", C.c_int64), ("outputs", C.c_int64), ("has_uint32", C.c_int32), ("uinteger", C.c_uint32),
                ("rejected", C.c_int32), ("listed", C.c_int32), ("error", C.c_int32), ("reserved", C.c_int32)]


DRAW_MAX_REJECTS = 8192


class DualvTrack(C.Structure):
    """af_dualv_track: one face track's raw landmark and AU rows on the device"""
    _fields_ = [("lmk", C.c_void_p), ("au", C.c_void_p), ("lmk_pitch", C.c_int64), ("au_pitch", C.c_int32), ("n", C.c_int32)]


class DualvClip(C.Structure):
    """af_dualv_clip: frames first .. first + len - 1 of a track"""
    _fields_ = [("track", C.c_int32), ("first", C.c_int32), ("len", C.c_int32), ("reserved", C.c_int32)]


class DualvOpts(C.Structure):
    """af_dualv_opts"""
    _fields_ = [("frames", C.c_int32), ("au_k", C.c_int32), ("zscore_mode", C.c_int32), ("zscore_apply", C.c_int32),
                ("use_delta", C.c_int32), ("use_delta2", C.c_int32), ("au_mean", C.c_void_p), ("au_std", C.c_void_p),
                ("lmk_mean", C.c_void_p), ("lmk_std", C.c_void_p)]


DUALV_MAX_T, DUALV_LMK_DIM, DUALV_MIN_POINTS = 16, 132, 467
DUALV_ZSCORE = {"none": 0, "clip": 1, "global": 2}
DUALV_APPLY = {"both": 0, "au": 1, "lmk": 2}
DUALV_FAMILY_FUSION, DUALV_FAMILY_BEST = 0, 1
DUALV_TRACK = {"median": 0, "mean": 1}
DUALV_VIDEO = {"max": 0, "median": 1, "mean": 2}
DUALV_BEST = {"track_mean": 0, "track_median": 1, "track_majority": 2}
DUALV_PAD_FIXT, DUALV_PAD_ZERO = 0, 1


class PoolDesc(C.Structure):
    _fields_ = [(n, C.c_int32) for n in (
        "n", "t", "h", "w", "c", "kt", "kh", "kw", "st", "sh", "sw", "pt", "ph", "pw", "to", "ho", "wo", "dtype",
        "out_ld")]


def _out_dims(dims, kernel, stride, pad):
    return tuple((d + 2 * p - k) // s + 1 for d, k, s, p in zip(dims, kernel, stride, pad))


def conv_desc(n, dims, cin, cout, kernel, stride, pad, relu, code, dout=None, tpool=0) -> ConvDesc:
    """The one place a ConvDesc is filled.  dims / kernel / stride / pad / dout are (t, h, w) triples; ``dout`` None = the
    usual (d + 2 p - k) // s + 1."""
    dout = _out_dims(dims, kernel, stride, pad) if dout is None else dout
    return ConvDesc(n, *dims, cin, cout, *kernel, *stride, *pad, *dout, int(relu), code, int(tpool))


def pool_desc(n, dims, c, kernel, stride, pad, code, dout=None, out_ld=0) -> PoolDesc:
    dout = _out_dims(dims, kernel, stride, pad) if dout is None else dout
    return PoolDesc(n, *dims, c, *kernel, *stride, *pad, *dout, code, out_ld)


class Op(C.Structure):
    _fields_ = [
        ("kind", C.c_int32), ("out_ld", C.c_int32),
        ("conv", ConvDesc), ("pool", PoolDesc),
        ("in_", C.c_void_p), ("weight", C.c_void_p), ("scale", C.c_void_p), ("shift", C.c_void_p),
        ("residual", C.c_void_p), ("out", C.c_void_p), ("aux", C.c_void_p),
        ("num_classes", C.c_int32), ("tag", C.c_int32),
        ("conv2", ConvDesc), ("in2", C.c_void_p), ("weight2", C.c_void_p),
        ("in_strides", C.c_int64 * 5),
        ("mean", C.c_float * 3), ("std_", C.c_float * 3),
        ("workspace", C.c_void_p), ("workspace_bytes", C.c_int64),
        ("scores", C.c_void_p),
        ("scale2", C.c_void_p), ("shift2", C.c_void_p),
        ("conv3", ConvDesc), ("in3", C.c_void_p), ("weight3", C.c_void_p),
        ("scale3", C.c_void_p), ("shift3", C.c_void_p),
        ("conv4", ConvDesc), ("weight4", C.c_void_p),
        ("x_sub", C.c_int32), ("pack_rgb3", C.c_int32),
    ]


class YunetDesc(C.Structure):
    _fields_ = [("batch", C.c_int32), ("height", C.c_int32), ("width", C.c_int32), ("top_k", C.c_int32),
                ("frame_stride", C.c_int64), ("row_pitch", C.c_int64), ("conf_threshold", C.c_float), ("nms_threshold", C.c_float)]


YUNET_MAX_TOPK, YUNET_MAX_SIDE, YUNET_LAUNCHES, YUNET_MAX_LIST = 8192, 8192, 18, 64


class RetinafaceDesc(C.Structure):
    _fields_ = [("batch", C.c_int32), ("height", C.c_int32), ("width", C.c_int32), ("keep_top_k", C.c_int32),
                ("frame_stride", C.c_int64), ("row_pitch", C.c_int64), ("max_count", C.c_int32), ("reserved", C.c_int32),
                ("min_score", C.c_double)]


RETINAFACE_MAX_SIDE, RETINAFACE_TOP_K, RETINAFACE_MAX_KEEP = 8192, 5000, 5000
RETINAFACE_LAUNCHES, RETINAFACE_POST_LAUNCHES = 54, 5

# name -> (restype, argtypes); tests/test_host_cpu.py::test_c_abi_exports_every_declared_symbol checks this table against
# include/af_hip.h and the built library
ABI = {
    "af_version": (C.c_int, []),
    "af_last_error": (C.c_char_p, []),
    "af_device_count": (C.c_int, []),
    "af_fold_bn": (C.c_int, [C.c_void_p] * 4 + [C.c_float, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p]),
    "af_packed_conv_weight_bytes": (C.c_int64, [C.c_int] * 6),
    "af_padded_channels": (C.c_int, [C.c_int]),
    "af_pack_conv_weight": (C.c_int, [C.c_void_p] + [C.c_int] * 6 + [C.c_void_p, C.c_void_p]),
    "af_pack_conv_weight_scaled": (C.c_int, [C.c_void_p, C.c_void_p] + [C.c_int] * 6 + [C.c_void_p, C.c_void_p]),
    "af_packed_stem_weight_bytes": (C.c_int64, [C.c_int] * 4),
    "af_pack_stem_weight": (C.c_int, [C.c_void_p] + [C.c_int] * 5 + [C.c_void_p, C.c_void_p]),
    "af_stem_input_bytes": (C.c_int64, [C.c_int] * 5),
    "af_pack_input_f32": (C.c_int, [C.c_void_p] + [C.c_int] * 4 + [C.c_int64] * 5 + [C.c_int, C.c_void_p, C.c_void_p]),
    "af_pack_input_u8": (C.c_int, [C.c_void_p] + [C.c_int] * 4 + [C.POINTER(C.c_float), C.POINTER(C.c_float),
                                                                  C.c_int, C.c_void_p, C.c_void_p]),
    "af_stem_conv_bn_relu": (C.c_int, [C.POINTER(ConvDesc)] + [C.c_void_p] * 6),
    "af_stem_conv_bn_relu_maxpool": (C.c_int, [C.POINTER(ConvDesc)] + [C.c_void_p] * 6),
    "af_stem_input_bytes_rgb3": (C.c_int64, [C.c_int] * 5),
    "af_pack_input_f32_rgb3": (C.c_int, [C.c_void_p] + [C.c_int] * 4 + [C.c_int64] * 5 + [C.c_int, C.c_void_p, C.c_void_p]),
    "af_pack_input_u8_rgb3": (C.c_int, [C.c_void_p] + [C.c_int] * 4 + [C.POINTER(C.c_float), C.POINTER(C.c_float),
                                                                       C.c_int, C.c_void_p, C.c_void_p]),
    "af_pack_input_u8_pathways": (C.c_int, [C.c_void_p] + [C.c_int] * 4 + [C.POINTER(C.c_float), C.POINTER(C.c_float), C.c_int, C.c_int,
                                            C.c_void_p, C.c_int, C.c_void_p, C.c_int, C.c_void_p]),
    "af_packed_stem_weight_bytes_rgb3": (C.c_int64, [C.c_int] * 2),
    "af_pack_stem_weight_rgb3": (C.c_int, [C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_void_p]),
    "af_stem_conv_bn_relu_maxpool_rgb3": (C.c_int, [C.POINTER(ConvDesc)] + [C.c_void_p] * 6),
    "af_stem_conv_bn_relu_maxpool_rgb3_ld": (C.c_int, [C.POINTER(ConvDesc)] + [C.c_void_p] * 5 + [C.c_int, C.c_void_p]),
    "af_conv_workspace_bytes": (C.c_int64, [C.POINTER(ConvDesc)]),
    "af_conv3d_bn_act": (C.c_int, [C.POINTER(ConvDesc)] + [C.c_void_p] * 6 + [C.c_int, C.c_void_p, C.c_int64, C.c_void_p]),
    "af_conv3d_dual_bn_act": (C.c_int, [C.POINTER(ConvDesc), C.c_void_p, C.c_void_p, C.POINTER(ConvDesc)] + [C.c_void_p] * 5
                              + [C.c_int, C.c_void_p]),
    "af_conv_ca_fusable": (C.c_int, [C.POINTER(ConvDesc)] * 3),
    "af_stage_rows_u8": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int]),
    "af_align_plan_u8": (C.c_int, [C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]),
    "af_window_batch_table_bytes": (C.c_int64, [C.c_int, C.c_int]),
    "af_window_batch_plan_u8": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_int64, C.c_void_p, C.c_int64,
                                          C.c_void_p, C.c_void_p]),
    "af_warp_affine_windows_u8": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_void_p]),
    "af_window_rects_table_bytes": (C.c_int64, [C.c_int, C.c_int]),
    "af_window_rects_plan_u8": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_int, C.POINTER(FrameStore), C.c_void_p, C.c_int64,
                                          C.c_void_p, C.c_void_p]),
    "af_warp_affine_window_rects_u8": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_void_p]),
    "af_warp_affine_window_rects_bgr_u8": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_void_p]),
    "af_face_quality_u8": (C.c_int, [C.c_void_p, C.POINTER(FrameStore), C.c_void_p, C.c_int, C.c_int, C.c_void_p, C.c_void_p, C.c_int64,
                                     C.c_void_p]),
    "af_window_rects_plan_stores_u8": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_int, C.c_void_p, C.c_int64,
                                                 C.c_void_p, C.c_void_p]),
    "af_warp_affine_window_stores_u8": (C.c_int, [C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_void_p]),
    "af_face_quality_stores_u8": (C.c_int, [C.c_void_p, C.c_int, C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.c_int64, C.c_void_p]),
    "af_face_laplacian_stores_u8": (C.c_int, [C.c_void_p, C.c_int, C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.c_int64, C.c_void_p]),
    "af_yuv420_plan_u8":(C.c_int, [C.c_void_p, C.c_int, C.c_void_p, C.c_int, C.c_void_p]),
    "af_yuv420_to_rgb_u8": (C.c_int, [C.c_void_p, C.c_int, C.c_void_p]),
    "af_yuv_plan_ex_u8":(C.c_int, [C.c_void_p, C.c_int, C.c_void_p, C.c_int, C.c_void_p]),
    "af_yuv_to_rgb_ex_u8": (C.c_int, [C.c_void_p, C.c_int, C.c_void_p]),
    "af_resize_table_bytes": (C.c_int64, [C.c_void_p, C.c_int]),
    "af_resize_plan_u8": (C.c_int, [C.c_void_p, C.c_int, C.c_void_p, C.c_int, C.c_void_p, C.c_int64, C.POINTER(C.c_int64)]),
    "af_resize_frames_u8": (C.c_int, [C.c_void_p, C.c_int, C.c_void_p]),
    "af_capture_table_bytes": (C.c_int64, [C.c_void_p, C.c_int]),
    "af_capture_plan_u8": (C.c_int, [C.c_void_p, C.c_int, C.c_void_p, C.c_int, C.c_void_p, C.c_int64, C.POINTER(C.c_int64)]),
    "af_capture_to_stores_u8": (C.c_int, [C.c_void_p, C.c_int, C.c_void_p]),
    "af_tile_workspace_bytes": (C.c_int64, [C.c_int, C.c_int]),
    "af_tile_candidates_u8": (C.c_int, [C.POINTER(TileSource), C.POINTER(TileParams), C.c_void_p, C.c_int64, C.POINTER(TileOutputs), C.c_void_p]),
    "af_tile_motion_u8": (C.c_int, [C.POINTER(TileSource), C.c_void_p, C.c_void_p, C.c_double, C.c_void_p, C.c_int64, C.POINTER(TileOutputs),
                                    C.c_void_p]),
    "af_tile_components_u8": (C.c_int, [C.c_void_p, C.c_int64, C.c_int, C.c_int, C.c_void_p, C.POINTER(TileParams), C.c_void_p, C.c_int64,
                                        C.POINTER(TileOutputs), C.c_void_p]),
    "af_rank_metrics_rows": (C.c_int, [C.c_void_p] * 3 + [C.c_int, C.c_void_p, C.c_int64, C.c_void_p, C.c_int, C.c_int, C.c_void_p, C.c_void_p,
                                       C.c_void_p]),
    "af_rank_curve": (C.c_int, [C.c_void_p] * 3 + [C.c_int, C.c_void_p, C.c_int64] + [C.c_void_p] * 5),
    "af_pcg64_draw_workspace_bytes": (C.c_int64, [C.c_int]),
    "af_pcg64_draw_rows": (C.c_int, [C.POINTER(Pcg64State), C.c_int64, C.c_int, C.c_int64, C.c_int, C.c_int, C.c_void_p, C.c_void_p, C.c_int,
                                     C.c_void_p, C.c_void_p, C.c_int64, C.c_void_p, C.c_void_p, C.c_int64, C.c_void_p]),
    "af_conv_cpa_fusable": (C.c_int, [C.POINTER(ConvDesc)] * 2 + [C.c_int]),
    "af_conv3d_cpa_bn_act": (C.c_int, [C.POINTER(ConvDesc)] + [C.c_void_p] * 6 + [C.c_int, C.POINTER(ConvDesc)] + [C.c_void_p] * 5),
    "af_conv3d_ca_bn_act": (C.c_int, [C.POINTER(ConvDesc), C.c_void_p, C.c_void_p, C.POINTER(ConvDesc)] + [C.c_void_p] * 6
                            + [C.POINTER(ConvDesc)] + [C.c_void_p] * 5),
    "af_conv_bc_fusable": (C.c_int, [C.POINTER(ConvDesc), C.POINTER(ConvDesc)]),
    "af_conv3d_bc_bn_act": (C.c_int, [C.POINTER(ConvDesc)] + [C.c_void_p] * 4 + [C.POINTER(ConvDesc)] + [C.c_void_p] * 5
                            + [C.c_int, C.c_void_p]),
    "af_block_abc_fusable": (C.c_int, [C.POINTER(ConvDesc)] * 4),
    "af_block_abc_bn_act": (C.c_int, ([C.POINTER(ConvDesc)] + [C.c_void_p] * 4) + ([C.POINTER(ConvDesc)] + [C.c_void_p] * 3) * 2
                            + [C.POINTER(ConvDesc), C.c_void_p] + [C.c_void_p, C.c_int, C.c_void_p]),
    "af_conv_variant": (C.c_int, [C.POINTER(ConvDesc), C.POINTER(ConvDesc)]),
    "af_conv_variant_name": (C.c_char_p, [C.c_int]),
    "af_conv_work_units": (C.c_int, [C.POINTER(ConvDesc), C.POINTER(ConvDesc), C.POINTER(C.c_int64), C.POINTER(C.c_int)]),
    "af_conv_ca_work_units": (C.c_int, [C.POINTER(ConvDesc)] * 3 + [C.POINTER(C.c_int64)] + [C.POINTER(C.c_int)] * 3),
    "af_conv_cpa_work_units": (C.c_int, [C.POINTER(ConvDesc)] * 2 + [C.c_int, C.POINTER(C.c_int64), C.POINTER(C.c_int)]),
    "af_block_abc_work_units": (C.c_int, [C.POINTER(ConvDesc)] * 4 + [C.POINTER(C.c_int)] * 2 + [C.POINTER(C.c_int64)]),
    "af_stem_work_units": (C.c_int, [C.POINTER(ConvDesc), C.c_int, C.POINTER(C.c_int64), C.POINTER(C.c_int), C.POINTER(C.c_int)]),
    "af_maxpool3d": (C.c_int, [C.POINTER(PoolDesc), C.c_void_p, C.c_void_p, C.c_void_p]),
    "af_avgpool_fc": (C.c_int, [C.POINTER(PoolDesc)] + [C.c_void_p] * 3 + [C.c_int] + [C.c_void_p] * 3),
    "af_avgpool_fc_scores": (C.c_int, [C.POINTER(PoolDesc)] + [C.c_void_p] * 3 + [C.c_int] + [C.c_void_p] * 4),
    "af_linear_scores": (C.c_int, [C.c_void_p] * 3 + [C.c_int] * 3 + [C.c_void_p, C.c_void_p, C.c_void_p]),
    "af_masked_mean_proj": (C.c_int, [C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_int, C.c_void_p, C.c_int, C.c_void_p,
                                      C.c_int, C.c_void_p]),
    "af_mlp_head": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p]),
    "af_avgpool": (C.c_int, [C.POINTER(PoolDesc), C.c_void_p, C.c_void_p, C.c_int, C.c_void_p]),
    "af_linear": (C.c_int, [C.c_void_p] * 3 + [C.c_int] * 3 + [C.c_void_p, C.c_void_p]),
    "af_pack_tstem_weight": (C.c_int, [C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_void_p]),
    "af_packed_tstem_weight_bytes": (C.c_longlong, [C.c_int]),
    "af_tstem_conv_bn_pool_relu": (C.c_int, [C.POINTER(ConvDesc)] + [C.c_void_p] * 6),
    "af_tstem_conv_bn_pool_relu_maxpool": (C.c_int, [C.POINTER(ConvDesc)] + [C.c_void_p] * 6),
    "af_tokens_assemble": (C.c_int, [C.c_void_p] * 3 + [C.c_int] * 3 + [C.c_void_p, C.c_void_p]),
    "af_layernorm": (C.c_int, [C.c_void_p, C.c_longlong, C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_float, C.c_void_p,
                               C.c_longlong, C.c_void_p]),
    "af_attention": (C.c_int, [C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_void_p]),
    "af_gelu": (C.c_int, [C.c_void_p, C.c_longlong, C.c_void_p]),
    "af_dual_branch_weight_floats": (C.c_longlong, [C.c_int] * 4),
    "af_transpose_f32": (C.c_int, [C.c_void_p, C.c_int, C.c_int, C.c_void_p, C.c_void_p]),
    "af_dual_branch_encoders": (C.c_int, [C.c_int, C.POINTER(C.c_void_p), C.POINTER(C.c_void_p), C.POINTER(C.c_int), C.c_void_p,
                                           C.c_void_p] + [C.c_int] * 6 + [C.c_float, C.c_void_p, C.c_int, C.c_void_p]),
    "af_gated_moe": (C.c_int, [C.c_void_p] * 3 + [C.c_int, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p]),
    "af_dual_clip_features": (C.c_int, [C.c_void_p, C.c_int, C.c_void_p, C.c_int, C.POINTER(DualvOpts)] + [C.c_void_p] * 4),
    "af_dual_video_reduce": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int, C.c_void_p, C.c_int, C.c_void_p, C.c_int, C.c_void_p,
                                       C.c_int, C.c_int, C.c_int, C.c_double] + [C.c_void_p] * 11),
    "af_dual_clip_features_ex": (C.c_int, [C.c_void_p, C.c_int, C.c_void_p, C.c_int, C.POINTER(DualvOpts), C.c_int, C.c_int] + [C.c_void_p] * 4),
    "af_lmk_video_reduce": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int, C.c_void_p, C.c_int, C.c_void_p, C.c_int, C.c_void_p,
                                      C.c_int, C.c_double] + [C.c_void_p] * 8),
    "af_warp_affine_clip_u8": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_int, C.POINTER(C.c_double), C.c_int,
                                         C.c_void_p, C.c_void_p]),
    "af_dual_head": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_void_p, C.c_void_p]),
    "af_run_ops": (C.c_int, [C.POINTER(Op), C.c_int, C.c_void_p]),
    "af_run_ops_timed": (C.c_int, [C.POINTER(Op), C.c_int, C.c_void_p, C.POINTER(C.c_float)]),
    "af_yunet_weight_floats": (C.c_int64, []),
    "af_yunet_workspace_bytes": (C.c_int64, [C.POINTER(YunetDesc)]),
    "af_yunet_detect": (C.c_int, [C.POINTER(YunetDesc)] + [C.c_void_p] * 3 + [C.c_int64] + [C.c_void_p] * 4),
    "af_yunet_detect_frames": (C.c_int, [C.POINTER(YunetDesc), C.c_void_p, C.POINTER(C.c_void_p), C.c_void_p, C.c_int64] + [C.c_void_p] * 4),
    "af_yunet_detect_timed": (C.c_int, [C.POINTER(YunetDesc)] + [C.c_void_p] * 3 + [C.c_int64] + [C.c_void_p] * 4
                              + [C.POINTER(C.c_float)]),
    "af_retinaface_weight_floats": (C.c_int64, []),
    "af_retinaface_anchors": (C.c_int64, [C.POINTER(RetinafaceDesc)]),
    "af_retinaface_max_rows": (C.c_int32, [C.POINTER(RetinafaceDesc)]),
    "af_retinaface_workspace_bytes": (C.c_int64, [C.POINTER(RetinafaceDesc)]),
    "af_retinaface_detect": (C.c_int, [C.POINTER(RetinafaceDesc)] + [C.c_void_p] * 3 + [C.c_int64] + [C.c_void_p] * 4),
    "af_retinaface_detect_timed": (C.c_int, [C.POINTER(RetinafaceDesc)] + [C.c_void_p] * 3 + [C.c_int64] + [C.c_void_p] * 4
                                   + [C.POINTER(C.c_float)]),
    "af_retinaface_postprocess": (C.c_int, [C.POINTER(RetinafaceDesc)] + [C.c_void_p] * 4 + [C.c_int64] + [C.c_void_p] * 3),
    "af_retinaface_postprocess_timed": (C.c_int, [C.POINTER(RetinafaceDesc)] + [C.c_void_p] * 4 + [C.c_int64] + [C.c_void_p] * 3
                                        + [C.POINTER(C.c_float)]),
    "af_bytetrack_state_bytes": (C.c_int64, []),
    "af_bytetrack_record_bytes": (C.c_int64, []),
    "af_bytetrack_reset": (C.c_int, [C.c_void_p, C.c_double, C.c_double, C.c_int]),
    "af_bytetrack_update_calls": (C.c_int, [C.POINTER(TrackCall), C.c_int, C.c_void_p, C.c_void_p]),
    "af_bytetrack_update_host": (C.c_int, [C.POINTER(TrackCall), C.c_void_p]),
    "af_track_probe_f64": (C.c_int, [C.c_void_p] * 4 + [C.c_int, C.c_void_p]),
    "af_runner_state_bytes": (C.c_int64, []),
    "af_runner_record_bytes": (C.c_int64, [C.c_int]),
    "af_runner_reset": (C.c_int, [C.c_void_p, C.c_double, C.c_double, C.c_int, C.c_int]),
    "af_runner_track_chunk": (C.c_int, [C.POINTER(RunnerChunk), C.c_void_p]),
    "af_runner_track_chunk_host": (C.c_int, [C.POINTER(RunnerChunk)]),
    "af_face_quality_table_u8": (C.c_int, [C.POINTER(StoreRef), C.c_void_p, C.c_int, C.c_int, C.c_void_p, C.c_void_p, C.c_int64, C.c_void_p]),
    "af_live_state_bytes": (C.c_int64, []),
    "af_live_record_bytes": (C.c_int64, []),
    "af_live_calls_per_launch": (C.c_int, []),
    "af_live_reset": (C.c_int, [C.c_void_p, C.c_double, C.c_double, C.c_int]),
    "af_live_update_calls": (C.c_int, [C.POINTER(LiveCall), C.c_int, C.c_void_p, C.c_void_p, C.c_void_p]),
    "af_live_update_host": (C.c_int, [C.POINTER(LiveCall), C.c_void_p, C.c_void_p]),
    "af_face_quality_records_u8": (C.c_int, [C.POINTER(StoreRef), C.c_int, C.POINTER(LiveQualityJob), C.c_int, C.c_void_p, C.c_void_p, C.c_int64,
                                             C.c_void_p]),
}


class AfError(RuntimeError):
    pass


def _load():
    if not os.path.exists(LIB_PATH):
        raise ImportError(
            "libafhip.so not found at %s - build it with `python -c 'import __graft_entry__ as g; g.build()'` "
            "(hipcc --offload-arch=gfx950); there is no CPU fallback for the HIP path" % LIB_PATH)
    lib = C.CDLL(LIB_PATH)
    for name, (res, args) in ABI.items():
        fn = getattr(lib, name)          # AttributeError if the symbol is missing: fail loudly
        fn.restype = res
        fn.argtypes = args
    if lib.af_version() != AF_ABI_VERSION:
        raise ImportError("libafhip.so ABI version %d, binding expects %d" % (lib.af_version(), AF_ABI_VERSION))
    return lib


lib = _load()


def check(rc: int, what: str = ""):
    if rc != 0:
        raise AfError("%s failed (%d): %s" % (what or "libafhip call", rc, lib.af_last_error().decode()))
