"""CPU: the YuNet detector's host side - the minimal ONNX reader, the plan matcher and its refusals, the padding
arithmetic, the numpy restatement of OpenCV's decode + NMS on hand-made head outputs, and the drop-in signature."""
import ctypes as C
import hashlib
import inspect
import json
import os
from collections import Counter

import numpy as np
import pytest

from conftest import GOLDEN, ROOT
import yunet_ref

MODEL = os.path.join(GOLDEN, "yunet_2023mar.onnx")


@pytest.fixture()
def graph():
    from af_mi355x import onnx_min
    return onnx_min.load(MODEL)


def test_fixture_provenance():
    meta = json.load(open(os.path.join(GOLDEN, "yunet_2023mar.json")))
    assert hashlib.sha256(open(MODEL, "rb").read()).hexdigest() == meta["sha256"]
    assert os.path.getsize(MODEL) == meta["bytes"]


def test_reader_counts(graph):
    ops = Counter(n.op_type for n in graph.nodes)
    assert ops == {"Conv": 53, "Relu": 15, "MaxPool": 4, "Resize": 2, "Add": 2, "Sigmoid": 6, "Transpose": 12, "Reshape": 12}
    assert len(graph.initializers) == 112
    assert sum(t.array.size for t in graph.initializers.values()) == 53121
    assert graph.opset == 11
    assert [o.name for o in graph.outputs] == ["cls_8", "cls_16", "cls_32", "obj_8", "obj_16", "obj_32",
                                               "bbox_8", "bbox_16", "bbox_32", "kps_8", "kps_16", "kps_32"]
    assert graph.inputs[0].name == "input" and graph.inputs[0].shape == (1, 3, 640, 640)
    assert graph.outputs[9].shape == (1, 6400, 10)
    w = graph.initializers["420"]
    assert w.dims == (16, 3, 3, 3) and w.array.dtype == np.float32


def test_plan(graph):
    from af_mi355x import detector, _lib
    p = detector.build_plan(graph)
    assert [(u.cin, u.cout) for u in p.units] == [(16, 16), (16, 16), (16, 32), (32, 32), (32, 64)] + [(64, 64)] * 9
    assert [u.out for u in p.units if u.pool] == ["188", "205", "214", "223"]
    assert [u.neck for u in p.units if u.neck] == [("223", "236"), ("214", "246")]
    assert p.head_inputs == ["256", "246", "236"]
    assert p.resize_scales == (1.0, 1.0, 2.0, 2.0)
    assert p.num_params == 53121
    assert detector.pack_weights(p).size == _lib.lib.af_yunet_weight_floats() == 53104   # + 17 resize / reshape constants


def _expect_refusal(graph, needle):
    from af_mi355x import detector
    with pytest.raises(ValueError) as e:
        detector.build_plan(graph)
    assert needle in str(e.value), str(e.value)


def test_plan_refuses_a_dropped_node(graph):
    del graph.nodes[5]                                     # the first MaxPool
    _expect_refusal(graph, "expected MaxPool")


def test_plan_refuses_a_changed_kernel_shape(graph):
    graph.nodes[3].attrs["kernel_shape"] = (5, 5)          # unit 0's depthwise conv
    _expect_refusal(graph, "node 3 Conv")


def test_plan_refuses_reordered_outputs(graph):
    graph.outputs[0], graph.outputs[3] = graph.outputs[3], graph.outputs[0]
    _expect_refusal(graph, "outputs")


def test_plan_refuses_other_resize_scales(graph):
    from af_mi355x import onnx_min
    t = graph.initializers["464"]
    graph.initializers["464"] = onnx_min.Tensor(t.name, t.dims, np.array([1, 1, 3, 3], np.float32))
    _expect_refusal(graph, "Resize scales")


@pytest.mark.parametrize("w,h,pw,ph", [(320, 320, 320, 320), (641, 359, 672, 384), (1920, 1080, 1920, 1088)])
def test_pad_to_32(w, h, pw, ph):
    from af_mi355x import detector
    assert detector.padded_size(w, h) == (pw, ph)
    assert yunet_ref.preprocess(np.zeros((h, w, 3), np.uint8)).shape == (1, 3, ph, pw)
    assert detector.num_anchors(w, h) == sum((pw // s) * (ph // s) for s in (8, 16, 32))


def _outs(w, h):
    """all-background head outputs (score 0) for a w x h input"""
    pw, ph = (w - 1) // 32 * 32 + 32, (h - 1) // 32 * 32 + 32
    o = {}
    for s in (8, 16, 32):
        n = (pw // s) * (ph // s)
        o["cls_%d" % s] = np.zeros((n, 1), np.float32)
        o["obj_%d" % s] = np.zeros((n, 1), np.float32)
        o["bbox_%d" % s] = np.zeros((n, 4), np.float32)
        o["kps_%d" % s] = np.zeros((n, 10), np.float32)
    return o


def test_restatement_known_box():
    o = _outs(64, 64)                                       # stride 8: 8 x 8 anchors
    idx = 2 * 8 + 3                                         # r = 2, c = 3
    o["cls_8"][idx] = 0.81
    o["obj_8"][idx] = 1.0
    o["bbox_8"][idx] = [0.5, 0.25, np.log(2.0), 0.0]
    o["kps_8"][idx] = np.arange(10) / 10.0
    out = yunet_ref.decode_nms(o, 64, 64, 0.6, 0.3, 5000)
    assert out.shape == (1, 15)                             # single candidate: returned as is
    cx, cy, bw, bh = 3.5 * 8, 2.25 * 8, 16.0, 8.0
    np.testing.assert_allclose(out[0, :4], [cx - bw / 2, cy - bh / 2, bw, bh], rtol=1e-6)
    np.testing.assert_allclose(out[0, 4:6], [(0.0 + 3) * 8, (0.1 + 2) * 8], rtol=1e-6)
    np.testing.assert_allclose(out[0, 14], 0.9, rtol=1e-6)


def test_restatement_tie_order_topk_and_strict_threshold():
    o = _outs(64, 64)
    for idx in (0, 9, 18, 27, 36):                          # diagonal, far apart: no overlap
        o["cls_8"][idx] = o["obj_8"][idx] = 0.7
    o["cls_8"][36] = o["obj_8"][36] = 0.8                   # highest score: first
    faces = yunet_ref.decode(o, 64, 64, 0.6)
    assert faces.shape[0] == 5
    out = yunet_ref.nms(faces, 0.6, 0.3, 5000)
    # equal scores keep anchor order (stable sort)
    assert [int(round(r[4] / 8)) for r in out] == [4, 0, 1, 2, 3]
    assert yunet_ref.nms(faces, 0.6, 0.3, 2).shape[0] == 2  # top_k cut before NMS
    # scores equal to the threshold pass the decode (>=) but not NMSBoxes (>)
    assert yunet_ref.nms(faces, np.float32(0.7), 0.3, 5000).shape[0] == 1


def test_restatement_overlap_and_rect2i_truncation():
    assert int(np.float32(-3.7)) == -3                      # Rect2i(int(x), ...) truncates toward zero
    o = _outs(64, 64)
    o["cls_8"][0] = o["obj_8"][0] = 0.9
    o["cls_8"][1] = o["obj_8"][1] = 0.8                      # next anchor, same box size: IoU 1/3 at stride 8 w = 16
    o["bbox_8"][0] = o["bbox_8"][1] = [0.0, 0.0, np.log(2.0), np.log(2.0)]
    faces = yunet_ref.decode(o, 64, 64, 0.6)
    assert faces[0, 0] == -8.0 and faces[0, 1] == -8.0
    # boxes (-8, -8, 16, 16) and (0, -8, 16, 16): intersection 8 * 16 = 128, union 384
    assert abs(float(yunet_ref.rect_overlap((-8, -8, 16, 16), (0, -8, 16, 16))) - 1 / 3) < 1e-6
    assert yunet_ref.nms(faces, 0.6, 0.3, 5000).shape[0] == 1
    assert yunet_ref.nms(faces, 0.6, 0.34, 5000).shape[0] == 2
    o["bbox_8"][0] = [-0.46, 0.0, 0.0, 0.0]                  # x = (0 - 0.46) * 8 - 4 = -7.68 -> int -7
    faces = yunet_ref.decode(o, 64, 64, 0.6)
    assert faces[0, :4].astype(np.int64)[0] == -7


def test_infer_refuses_a_wrong_size_before_any_device_work():
    from af_mi355x.detector import YuNet
    y = YuNet(MODEL, inputSize=[320, 240])
    with pytest.raises(ValueError, match="input size"):
        y.infer(np.zeros((320, 240, 3), np.uint8))
    with pytest.raises(ValueError):
        y.infer(np.zeros((240, 320, 4), np.uint8))
    assert y._dev_weights == {} and y._workspaces == {}     # nothing was uploaded or allocated
    y.setInputSize((240, 320))
    assert y._inputSize == (240, 320)


def test_drop_in_signature():
    import sys
    sys.path.insert(0, ROOT)
    from integration.yunet_mi355x import YuNet as Shim
    from af_mi355x.detector import YuNet
    assert Shim is YuNet
    # preprocessing/yunet/yunet.py
    assert str(inspect.signature(YuNet.__init__)) == \
        "(self, modelPath, inputSize=[320, 320], confThreshold=0.6, nmsThreshold=0.3, topK=5000, backendId=0, targetId=0)"
    assert str(inspect.signature(YuNet.setBackendAndTarget)) == "(self, backendId, targetId)"
    assert str(inspect.signature(YuNet.setInputSize)) == "(self, input_size)"
    assert str(inspect.signature(YuNet.infer)) == "(self, image)"
    y = YuNet(MODEL)
    assert y.name == "YuNet"
    y.setBackendAndTarget(3, 1)
    assert (y._backendId, y._targetId) == (3, 1)


def test_abi_rejects_bad_descriptors_without_a_gpu():
    from af_mi355x import _lib
    d = _lib.YunetDesc(1, 1080, 1920, 5000, 1080 * 1920 * 3, 1920 * 3, 0.6, 0.3)
    assert _lib.lib.af_yunet_workspace_bytes(C.byref(d)) > 0
    for field, bad in (("top_k", 0), ("top_k", 8193), ("width", 0), ("row_pitch", 100)):
        e = _lib.YunetDesc.from_buffer_copy(d)
        setattr(e, field, bad)
        assert _lib.lib.af_yunet_workspace_bytes(C.byref(e)) == 0
        assert _lib.lib.af_yunet_detect(C.byref(e), None, None, None, 0, None, None, None, None) == -1
    assert _lib.lib.af_yunet_detect(None, None, None, None, 0, None, None, None, None) == -1
