"""GPU: the HIP YuNet detector (csrc/af_yunet.hip) against the fp64 interpreter of the parsed ONNX graph (raw head outputs)
and the numpy restatement of OpenCV's decode + NMS (detections), plus batching / determinism / ABI checks."""
import ctypes as C
import os

import numpy as np
import pytest
import torch

from conftest import GOLDEN
import yunet_ref

MODEL = os.path.join(GOLDEN, "yunet_2023mar.onnx")
SIZES = [(320, 320), (641, 359), (1920, 1080)]          # (w, h)
AF_ERR_ARG = -1                                         # include/af_hip.h
RAW_TOL = 3e-5                                          # |d| <= RAW_TOL * max(1, |ref|); measured max 1.1e-5 (1920x1080)


def frames(n, w, h, seed):
    """seeded synthetic BGR frames: "smooth" and "uniform" kinds alternately (n, h, w, 3) uint8"""
    from af_mi355x import synth
    out = []
    for i in range(n):
        kind = "smooth" if i % 2 == 0 else "uniform"
        c = synth.synthetic_clips_u8(1, seed=seed + i, kind=kind, num_frames=1, size=max(w, h))
        out.append(c[0, 0, :h, :w].numpy())
    return np.stack(out)


@pytest.fixture(scope="module")
def det():
    from af_mi355x.detector import YuNet
    return YuNet(MODEL)


@pytest.fixture(scope="module")
def graph():
    from af_mi355x import onnx_min
    return onnx_min.load(MODEL)


def _dev():
    return torch.device("cuda", torch.cuda.current_device())


@pytest.mark.gpu
@pytest.mark.parametrize("w,h", SIZES)
def test_raw_outputs_match_the_fp64_graph(det, graph, w, h):
    from af_mi355x.detector import split_raw
    fr = frames(3, w, h, seed=11)
    x = torch.from_numpy(fr).to(_dev())
    _, _, raw3 = det.detect(x, raw=True)
    _, _, raw1 = det.detect(x[:1], raw=True)
    raw3, raw1 = raw3.cpu().numpy(), raw1.cpu().numpy()
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


@pytest.mark.gpu
@pytest.mark.parametrize("w,h", [(641, 359), (1920, 1080)])
@pytest.mark.parametrize("conf,nms,top_k", [(0.05, 0.3, 5000), (0.0, 0.3, 300)])
def test_detections_match_the_restatement(det, w, h, conf, nms, top_k):
    from af_mi355x.detector import split_raw
    fr = frames(2, w, h, seed=23)
    x = torch.from_numpy(fr).to(_dev())
    rows, counts, raw = det.detect(x, raw=True, conf=conf, nms=nms, top_k=top_k)
    rows, counts, raw = rows.cpu().numpy(), counts.cpu().numpy(), raw.cpu().numpy()
    outs = split_raw(raw, w, h)
    for b in range(2):
        cand = yunet_ref.decode({k: v[b] for k, v in outs.items()}, w, h, conf)
        want = yunet_ref.nms(cand, conf, nms, top_k)
        got = rows[b, :counts[b]]
        print("yunet %dx%d conf %g: %d candidates, %d kept" % (w, h, conf, len(cand), len(want)))
        assert len(cand) >= (1000 if conf == 0.0 else 1)
        assert got.shape == want.shape, (got.shape, want.shape)
        np.testing.assert_allclose(got, want, rtol=1e-4, atol=1e-4)


@pytest.mark.gpu
def test_batch_equals_single_frames_bitwise(det):
    fr = frames(4, 641, 359, seed=31)
    x = torch.from_numpy(fr).to(_dev())
    rows4, c4 = det.detect(x, conf=0.05)
    rows4, c4 = rows4.cpu(), c4.cpu()
    for b in range(4):
        r1, c1 = det.detect(x[b:b + 1].contiguous(), conf=0.05)
        n = int(c1[0])
        assert n == int(c4[b])
        assert torch.equal(r1[0, :n].cpu(), rows4[b, :n])


@pytest.mark.gpu
def test_two_runs_are_bitwise_identical(det):
    from af_mi355x import _lib
    x = torch.from_numpy(frames(3, 1920, 1080, seed=41)).to(_dev())
    a = [t.cpu() for t in det.detect(x, conf=0.0, top_k=2000)]
    ms = []
    b = [t.cpu() for t in det.detect(x, conf=0.0, top_k=2000, timings=ms)]       # the timed entry point
    assert len(ms) == _lib.YUNET_LAUNCHES and all(t > 0 for t in ms), ms
    assert torch.equal(a[1], b[1]) and int(a[1].min()) > 0
    for i in range(3):
        n = int(a[1][i])
        assert torch.equal(a[0][i, :n], b[0][i, :n])


@pytest.mark.gpu
def test_infer_contract(det):
    from af_mi355x.detector import YuNet
    fr = frames(1, 320, 320, seed=51)[0]
    y = YuNet(MODEL, confThreshold=0.05)
    out = y.infer(fr)
    assert out.dtype == np.float32 and out.ndim == 2 and out.shape[1] == 15 and out.shape[0] >= 1
    none = YuNet(MODEL, confThreshold=1.0).infer(fr)
    assert none.shape == (0, 5)


@pytest.mark.gpu
def test_c_abi_rejects_a_bad_argument_before_any_launch(det):
    from af_mi355x import _lib
    x = torch.from_numpy(frames(1, 320, 320, seed=61)).to(_dev())
    d = _lib.YunetDesc(1, 320, 320, 5000, 320 * 320 * 3, 320 * 3, 0.6, 0.3)
    need = _lib.lib.af_yunet_workspace_bytes(C.byref(d))
    ws = torch.empty(need, dtype=torch.uint8, device=x.device)
    wt = torch.from_numpy(det.weights_host).to(x.device)
    rows = torch.empty(1, 5000, 15, device=x.device)
    cnt = torch.empty(1, dtype=torch.int32, device=x.device)
    args = [C.c_void_p(wt.data_ptr()), C.c_void_p(x.data_ptr()), C.c_void_p(ws.data_ptr()), need, C.c_void_p(rows.data_ptr()),
            C.c_void_p(cnt.data_ptr()), None, None]
    assert _lib.lib.af_yunet_detect(C.byref(d), *args[:3], need - 16, *args[4:]) == AF_ERR_ARG    # workspace too small
    assert b"workspace" in _lib.lib.af_last_error()
    d.top_k = 0
    assert _lib.lib.af_yunet_detect(C.byref(d), *args) == AF_ERR_ARG
    d.top_k = 5000
    assert _lib.lib.af_yunet_detect(C.byref(d), *args) == 0
    torch.cuda.synchronize()


@pytest.mark.gpu
def test_one_instance_on_two_streams(det):
    """a multi-stream service shares one YuNet: calls on two streams, in flight together and with different frame sizes
    (stream A's workspace grows behind its own queued small-frame call), give the single-stream results bitwise"""
    from af_mi355x.detector import YuNet
    y = YuNet(MODEL, confThreshold=0.05)
    dev = _dev()
    xa = torch.from_numpy(frames(2, 641, 359, seed=71)).to(dev)
    xb = torch.from_numpy(frames(3, 1920, 1080, seed=73)).to(dev)
    want_a = [t.cpu() for t in det.detect(xa, conf=0.05)]
    want_b = [t.cpu() for t in det.detect(xb, conf=0.05)]
    torch.cuda.synchronize()
    sa, sb = torch.cuda.Stream(dev), torch.cuda.Stream(dev)
    got = []
    for _ in range(3):
        with torch.cuda.stream(sa):
            ra = y.detect(xa)
        with torch.cuda.stream(sb):
            rb = y.detect(xb)
        with torch.cuda.stream(sa):
            rab = y.detect(xb)
        got.append((ra, rb, rab))
    torch.cuda.synchronize()
    assert {k[1] for k in y._workspaces} == {sa.cuda_stream, sb.cuda_stream}
    for ra, rb, rab in got:
        for (rows, cnt), (wr, wc) in ((ra, want_a), (rb, want_b), (rab, want_b)):
            cnt = cnt.cpu()
            assert torch.equal(cnt, wc)
            for i in range(len(cnt)):
                assert torch.equal(rows[i, :int(cnt[i])].cpu(), wr[i, :int(wc[i])])
