"""RetinaFace host side without a GPU: the state-dict layout, synthetic weights, prior tables, checkpoint loading, argument
checks, the torch / numpy restatement against the reference's fp64 outputs (tests/golden/retinaface*) and the C ABI."""
import ctypes as C
import hashlib
import json
import os
import re

import numpy as np
import pytest
import torch

import af_mi355x  # noqa: F401
from af_mi355x import retinaface as rf, synth

import retinaface_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden")


@pytest.fixture(scope="module")
def golden():
    with open(os.path.join(GOLDEN, "retinaface.json")) as f:
        return json.load(f)


def test_layout_matches_reference(golden):
    mine = [(k, list(s)) for k, s in rf.state_dict_layout()]
    assert mine == [(k, list(s)) for k, s in golden["layout"]]
    assert len(mine) == 300
    assert sum(int(np.prod(s)) for k, s in mine if not k.endswith("num_batches_tracked")) == golden["num_floats"] == 433296


def _sd_hash(sd):
    h = hashlib.sha256()
    for k, v in sd.items():
        h.update(k.encode())
        h.update(v.numpy().tobytes())
    return h.hexdigest()


def test_synthetic_recipe_is_deterministic():
    a, b = synth.retinaface_state_dict(1, "sparse"), synth.retinaface_state_dict(1, "sparse")
    assert _sd_hash(a) == _sd_hash(b)
    assert _sd_hash(a) != _sd_hash(synth.retinaface_state_dict(1, "dense"))
    assert _sd_hash(a) != _sd_hash(synth.retinaface_state_dict(2, "sparse"))
    rf.check_state_dict(a)
    f1, f2 = synth.retinaface_frames(2, 37, 53, seed=4), synth.retinaface_frames(2, 37, 53, seed=4)
    assert f1.dtype == np.uint8 and f1.shape == (2, 37, 53, 3) and np.array_equal(f1, f2)
    with pytest.raises(ValueError):
        synth.retinaface_state_dict(1, "hot")


def test_priors_match_reference_bitwise(golden):
    for size, g in golden["priors"].items():
        h, w = (int(v) for v in size.split("x"))
        p = rf.priors(h, w)
        assert p.shape == (g["n"], 4) and p.shape[0] == rf.num_anchors(h, w)
        assert hashlib.sha256(p.tobytes()).hexdigest() == g["sha256"], size
        assert np.array_equal(p[g["idx"]], np.asarray(g["rows"], np.float32))


@pytest.fixture
def no_fetch(monkeypatch):
    def boom(*a, **k):
        raise AssertionError("a URL loader was called")
    monkeypatch.setattr(torch.hub, "load_state_dict_from_url", boom)
    monkeypatch.setattr(torch.hub, "download_url_to_file", boom)
    import torch.utils.model_zoo as mz
    monkeypatch.setattr(mz, "load_url", boom)


def test_load_semantics(tmp_path, no_fetch):
    sd = synth.retinaface_state_dict(3, "sparse")
    wrapped = {"state_dict": {"module." + k: v for k, v in sd.items()}}
    p = tmp_path / "wrapped.pth"
    torch.save(wrapped, p)
    got = rf.load(str(p))
    assert list(got) == list(sd) and all(torch.equal(got[k], sd[k]) for k in sd)
    plain = tmp_path / "plain.pth"
    torch.save(sd, plain)
    assert list(rf.load(str(plain))) == list(sd)
    missing = dict(sd)
    missing.pop("ssh2.conv7X7_2.1.running_var")
    torch.save(missing, tmp_path / "missing.pth")
    with pytest.raises(KeyError, match="ssh2.conv7X7_2.1.running_var"):
        rf.load(str(tmp_path / "missing.pth"))
    bad = dict(sd)
    bad["fpn.merge1.0.weight"] = torch.zeros(64, 64, 1, 1)
    torch.save(bad, tmp_path / "bad.pth")
    with pytest.raises(ValueError, match="fpn.merge1.0.weight"):
        rf.load(str(tmp_path / "bad.pth"))
    with pytest.raises(ValueError):
        rf.FaceDetector(0, str(p), network="resnet50")
    with pytest.raises(ValueError):
        rf.FaceDetector(-1, str(p))
    with pytest.raises(ValueError, match="never fetches"):
        rf.FaceDetector(0, None)


def test_pack_weights_size_matches_library():
    from af_mi355x import _lib
    w = rf.pack_weights(synth.retinaface_state_dict(1, "sparse"))
    assert w.dtype == np.float32 and w.size == _lib.lib.af_retinaface_weight_floats()


def test_argument_checks():
    t, single = rf.FaceDetector._as_batch(np.zeros((9, 11, 3), np.uint8))
    assert single and tuple(t.shape) == (1, 9, 11, 3)
    frame = np.arange(9 * 11 * 3, dtype=np.uint8).reshape(9, 11, 3)
    t, _ = rf.FaceDetector._as_batch(frame[..., ::-1])
    assert np.array_equal(t[0].numpy(), frame[..., ::-1])
    t, single = rf.FaceDetector._as_batch([frame, frame[..., ::-1]])
    assert not single and tuple(t.shape) == (2, 9, 11, 3)
    t, single = rf.FaceDetector._as_batch(torch.zeros(2, 9, 11, 3, dtype=torch.uint8))
    assert not single and tuple(t.shape) == (2, 9, 11, 3)
    with pytest.raises(TypeError):
        rf.FaceDetector._as_batch(np.zeros((9, 11, 3), np.float32))
    with pytest.raises(TypeError):
        rf.FaceDetector._as_batch(torch.zeros(9, 11, 3))
    with pytest.raises(TypeError):
        rf.FaceDetector._as_batch([np.zeros((9, 11, 3), np.int16)])
    with pytest.raises(ValueError, match="same size"):
        rf.FaceDetector._as_batch([np.zeros((9, 11, 3), np.uint8), np.zeros((9, 12, 3), np.uint8)])
    with pytest.raises(NotImplementedError):
        rf.FaceDetector._as_batch("frame.png")


def test_restatement_matches_reference_fp64(golden):
    """tests/retinaface_ref.py (functional torch, fp64) against the reference module's own fp64 heads, every anchor"""
    npz = np.load(os.path.join(GOLDEN, "retinaface_raw_240x320.npz"))
    for case in golden["cases"]:
        if (case["h"], case["w"]) != (240, 320):
            continue
        sd = synth.retinaface_state_dict(golden["weight_seed"], case["recipe"])
        frames = torch.from_numpy(synth.retinaface_frames(1, case["h"], case["w"], seed=case["frame_seed"]))
        loc, conf, landms = (t[0].numpy() for t in R.forward(sd, frames, torch.float64))
        n = case["name"]
        idx = npz[n + "/idx"]
        for got, key in ((loc, "loc"), (conf, "conf"), (landms, "landms")):
            ref = npz[n + "/" + key].astype(np.float64)
            err = np.abs(got[idx] - ref) / np.maximum(1.0, np.abs(ref))
            assert err.max() < 1e-6, (n, key, err.max())      # the golden is fp64 rounded to fp32


def test_numpy_post_process_matches_reference(golden):
    dets = np.load(os.path.join(GOLDEN, "retinaface_dets.npz"))
    for case in golden["post_cases"]:
        loc, conf, landms = R.post_inputs(case["h"], case["w"], case["seed"], case["bias"], case["spread"])
        rows = R.post_process_np(loc, conf, landms, case["h"], case["w"])
        ref = dets[case["name"]]
        assert rows.shape == ref.shape, case["name"]
        np.testing.assert_allclose(rows, ref, rtol=0, atol=1e-3)
        assert np.array_equal(rows[:, 4], ref[:, 4])


def test_abi_version_and_descriptor():
    from af_mi355x import _lib
    hdr = open(os.path.join(ROOT, "include", "af_hip.h")).read()
    assert _lib.lib.af_version() == _lib.AF_ABI_VERSION == int(re.search(r"#define AF_ABI_VERSION (\d+)", hdr).group(1)) == 6
    for name, val in (("LAUNCHES", _lib.RETINAFACE_LAUNCHES), ("POST_LAUNCHES", _lib.RETINAFACE_POST_LAUNCHES),
                      ("TOP_K", _lib.RETINAFACE_TOP_K), ("MAX_KEEP", _lib.RETINAFACE_MAX_KEEP), ("MAX_SIDE", _lib.RETINAFACE_MAX_SIDE)):
        assert int(re.search(r"#define AF_RETINAFACE_%s (\d+)" % name, hdr).group(1)) == val
    assert C.sizeof(_lib.RetinafaceDesc) == 48
    d = _lib.RetinafaceDesc(2, 1080, 1920, 750, 1080 * 1920 * 3, 1920 * 3, 10, 0, 0.5)
    assert _lib.lib.af_retinaface_anchors(C.byref(d)) == rf.num_anchors(1080, 1920) == 85200
    assert _lib.lib.af_retinaface_max_rows(C.byref(d)) == 10
    assert _lib.lib.af_retinaface_workspace_bytes(C.byref(d)) > 0
    d.keep_top_k = 0
    assert _lib.lib.af_retinaface_workspace_bytes(C.byref(d)) == 0
    assert b"keep_top_k" in _lib.lib.af_last_error()
    d.keep_top_k = 750
    assert _lib.lib.af_retinaface_detect(C.byref(d), None, None, None, 0, None, None, None, None) == -1
    assert b"null" in _lib.lib.af_last_error()
