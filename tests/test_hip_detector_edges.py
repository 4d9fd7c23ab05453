"""GPU: the two face detectors (csrc/af_yunet.hip, csrc/af_retinaface.hip, csrc/af_detect.h) where their index arithmetic
is thinnest: frames smaller than a kernel tile or than YuNet's padding, levels one pixel wide or high, and the RetinaFace
post-process on the chunked sort, exact score ties, no candidate at all and a batch of frames with different candidate
counts.  The references are the ones of test_hip_yunet / test_hip_retinaface; test_detector_edges_host pins on the CPU what
makes the exact comparison of the post-process fair.

Measured on an MI355X, max |d| / max(1, |ref|) of the raw heads against fp64:
  YuNet      (w, h)  1x1 7.09e-07, 32x32 5.59e-07, 33x17 1.14e-06, 31x33 1.12e-06, 65x97 2.05e-06, 100x16 1.06e-06  (gate 3e-5)
  RetinaFace (h, w)  1x1 7.97e-08, 7x9 8.05e-08, 16x16 3.51e-07, 17x33 1.39e-06, 31x65 2.58e-06, 64x8 2.01e-07     (gate 5e-5)
Post-process: every case equal to the restatement row for row, scores bit for bit, coordinates within 2 ulp.
NMS margins of the inputs (min |ovr - 0.4|, required >= 1e-5): chunked 6.01e-05, chunked_ties 6.01e-05,
post_sparse 1.15e-05, all 4.05e-05, straddle 2.11e-04, none: no box."""
import numpy as np
import pytest
import torch

from af_mi355x import retinaface as rf, synth

import retinaface_edge_cases as E
import retinaface_ref as R
import yunet_ref
from test_hip_retinaface import detector
from test_hip_yunet import MODEL, RAW_TOL, frames as yunet_frames

pytestmark = pytest.mark.gpu

YUNET_SIZES = [(1, 1), (32, 32), (33, 17), (31, 33), (65, 97), (100, 16)]           # (w, h)
RETINAFACE_SIZES = [(1, 1), (7, 9), (16, 16), (17, 33), (31, 65), (64, 8)]          # (h, w)
RETINAFACE_RAW_TOL = 5e-5           # test_hip_retinaface's gate on |d| / max(1, |ref|)


@pytest.fixture(scope="module")
def yunet():
    from af_mi355x.detector import YuNet
    return YuNet(MODEL)


@pytest.fixture(scope="module")
def graph():
    from af_mi355x import onnx_min
    return onnx_min.load(MODEL)


def _dev():
    return torch.device("cuda", torch.cuda.current_device())


def yunet_anchors(w, h):
    pw, ph = ((w - 1) // 32 + 1) * 32, ((h - 1) // 32 + 1) * 32
    return sum((pw // s) * (ph // s) for s in (8, 16, 32))


# ---- a. YuNet on frames below its padding and its 16 x 16 tile
@pytest.mark.parametrize("w,h", YUNET_SIZES)
def test_yunet_raw_heads_on_small_frames(yunet, graph, w, h):
    from af_mi355x.detector import split_raw
    fr = yunet_frames(3, w, h, seed=11)
    assert fr.shape == (3, h, w, 3)
    x = torch.from_numpy(fr).to(_dev())
    _, _, raw3 = yunet.detect(x, raw=True)
    _, _, raw1 = yunet.detect(x[:1], raw=True)
    raw3, raw1 = raw3.cpu().numpy(), raw1.cpu().numpy()
    assert raw3.shape == (3, yunet_anchors(w, h), 16)
    assert np.array_equal(raw1[0], raw3[0])
    got = split_raw(raw3, w, h)
    worst = 0.0
    for b in range(3):
        want = yunet_ref.run_graph(graph, yunet_ref.preprocess(fr[b]))
        for k, v in want.items():
            g = got[k][b].astype(np.float64)
            assert g.shape == v[0].shape, (k, g.shape, v.shape)
            rel = np.abs(g - v[0]) / np.maximum(1.0, np.abs(v[0]))
            worst = max(worst, float(rel.max()))
    print("yunet raw %dx%d: max |d| / max(1, |ref|) = %.3g" % (w, h, worst))
    assert worst <= RAW_TOL, worst


@pytest.mark.parametrize("w,h", [(33, 17), (65, 97)])
def test_yunet_detections_on_small_frames(yunet, w, h):
    from af_mi355x.detector import split_raw
    conf, nms, top_k = 0.0, 0.3, 300
    fr = yunet_frames(3, w, h, seed=23)
    x = torch.from_numpy(fr).to(_dev())
    rows, counts, raw = yunet.detect(x, raw=True, conf=conf, nms=nms, top_k=top_k)
    rows, counts, raw = rows.cpu().numpy(), counts.cpu().numpy(), raw.cpu().numpy()
    outs = split_raw(raw, w, h)
    for b in range(3):
        cand = yunet_ref.decode({k: v[b] for k, v in outs.items()}, w, h, conf)
        want = yunet_ref.nms(cand, conf, nms, top_k)
        got = rows[b, :counts[b]]
        print("yunet %dx%d conf %g: %d candidates, %d kept" % (w, h, conf, len(cand), len(want)))
        assert len(cand) == yunet_anchors(w, h) == {(33, 17): 42, (65, 97): 252}[(w, h)]     # conf 0: every anchor
        assert len(want) >= 1
        assert got.shape == want.shape, (got.shape, want.shape)
        np.testing.assert_allclose(got, want, rtol=1e-4, atol=1e-4)


# ---- b. RetinaFace with levels down to 1 x 1
@pytest.mark.parametrize("h,w", RETINAFACE_SIZES)
def test_retinaface_raw_heads_on_small_frames(h, w):
    seed = 1
    sd = synth.retinaface_state_dict(seed, "sparse")
    det = detector(seed, "sparse")
    fr = synth.retinaface_frames(3, h, w, seed=17)
    x = torch.from_numpy(fr).cuda()
    _, _, raw3 = det.detect_device(x, raw=True)
    _, _, raw1 = det.detect_device(x[1:2], raw=True)
    torch.cuda.synchronize()
    assert raw3[0].shape[1] == rf.num_anchors(h, w)
    want = R.forward(sd, torch.from_numpy(fr), torch.float64)
    worst = 0.0
    for got3, got1, ref, k in zip(raw3, raw1, want, (4, 2, 10)):
        assert tuple(got3.shape) == (3, rf.num_anchors(h, w), k) == tuple(ref.shape)
        assert torch.equal(got1[0], got3[1])
        g, r = got3.cpu().numpy().astype(np.float64), ref.numpy()
        worst = max(worst, float((np.abs(g - r) / np.maximum(1.0, np.abs(r))).max()))
    print("retinaface raw %dx%d: max |d| / max(1, |ref|) = %.3g" % (h, w, worst))
    assert worst < RETINAFACE_RAW_TOL, worst


# ---- c. the RetinaFace post-process alone, exact
def assert_rows_exact(got, ref, h, w, name):
    """test_postprocess_matches_reference's rule: same rows in the same order, scores bit-equal, coordinates within 2 ulp
    (or, for a coordinate near 0, within 2 ulp of the frame size); returns the largest ulp distance of any element"""
    assert got.shape == ref.shape, (name, got.shape, ref.shape)
    if got.shape[0] == 0:
        return 0
    assert np.array_equal(got[:, 4], ref[:, 4]), name
    ulp = np.abs(got.view(np.int32).astype(np.int64) - ref.view(np.int32).astype(np.int64))
    near = np.abs(got - ref) <= 2 * np.spacing(np.float32(max(h, w)))
    assert ((ulp <= 2) | near).all(), (name, int(ulp.max()))
    return int(ulp.max())


def run_post(det, names, **kw):
    """one postprocess_device call on the cases `names` as one batch: [(count, rows[:count])] per frame, as numpy"""
    h, w = E.size(names[0])
    assert all(E.size(n) == (h, w) for n in names)
    dev = [torch.from_numpy(np.stack([E.inputs(n)[i] for n in names])).cuda() for i in range(3)]
    rows, counts = det.postprocess_device(*dev, h, w, **kw)
    rows, counts = rows.cpu().numpy(), counts.cpu().numpy()
    return [(int(counts[b]), np.ascontiguousarray(rows[b, :int(counts[b])])) for b in range(len(names))]


@pytest.mark.parametrize("name", ["chunked", "chunked_ties"])
def test_postprocess_through_the_chunked_sort(name):
    h, w = E.size(name)
    (n, got), = run_post(detector(1, "sparse"), [name])
    ref = E.expected(name)
    assert ref.shape[0] == rf.KEEP_TOP_K
    worst = assert_rows_exact(got, ref, h, w, name)
    print("%s: %d candidates, %d rows, max %d ulp" % (name, E.sorted_dets(name)[1], n, worst))


def test_postprocess_without_a_candidate_then_the_next_call():
    det = detector(1, "sparse")
    (n, got), = run_post(det, ["none"])
    assert n == 0 and got.shape == (0, 15)
    torch.cuda.synchronize()                     # no error is pending on the device
    (n, got), = run_post(det, ["post_sparse"])
    h, w = E.size("post_sparse")
    assert n == 494
    assert_rows_exact(got, E.expected("post_sparse"), h, w, "post_sparse after none")


@pytest.mark.parametrize("names", [E.MIXED_BATCH, E.MIXED_BATCH[::-1]], ids=["forward", "reversed"])
def test_postprocess_of_a_batch_with_different_candidate_counts(names):
    det = detector(1, "sparse")
    h, w = E.size(names[0])
    batch = run_post(det, list(names))
    alone = [run_post(det, [n])[0] for n in names]
    assert len({E.sorted_dets(n)[1] for n in names}) == len(names)
    for name, (n, got), (n1, got1) in zip(names, batch, alone):
        worst = assert_rows_exact(got, E.expected(name), h, w, name)
        assert n == n1 and np.array_equal(got.view(np.int32), got1.view(np.int32)), name
        print("%s in a batch of %d: %d candidates, %d rows, max %d ulp" % (name, len(names), E.sorted_dets(name)[1], n, worst))
    assert batch[names.index("none")][0] == 0


def test_postprocess_cut_after_the_chunked_sort():
    name, keep_top_k, max_count, min_score = "chunked", 5000, 40, 0.3
    h, w = E.size(name)
    (n, got), = run_post(detector(1, "sparse"), [name], keep_top_k=keep_top_k, max_count=max_count, min_score=min_score)
    rows = E.expected(name, keep_top_k)[:max_count]
    want = rows[[float(s) >= min_score for s in rows[:, 4]]]
    assert want.shape[0] >= 1
    worst = assert_rows_exact(got, want, h, w, name)
    print("%s cut to %d, score >= %g: %d rows, max %d ulp" % (name, max_count, min_score, n, worst))
