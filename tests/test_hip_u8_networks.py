"""GPU: the uint8 clip surface (forward_clips_u8 / infer_scores / LiveScorer / TrackScorer / VideoScorer) on FTCN-TT and SlowFast,
and the one pack launch that feeds both SlowFast inputs (af_pack_input_u8_pathways).

  pack kernel       every byte of both outputs equals what af_pack_input_u8 / af_pack_input_u8_rgb3 write into the same pre-filled
                    buffers for the clip and for clip[:, ::alpha]
  uint8 vs fp32     torch.equal in every dtype: the pack kernels normalise with the callers' own two fp32 operations, and I3D is
                    bit-equal between its two input forms in f16 / bf16 as well (asserted here first)
  golden logits     the tolerances of tests/test_hip_ftcn.py and tests/test_hip_slowfast.py, read from their parametrize marks
Shrunken networks (8 frames, 64 x 64, alpha 4) except for the golden clips.
"""
import ctypes as C
import os
import sys

import numpy as np
import pytest
import torch

from conftest import ROOT, load_json

sys.path.insert(0, os.path.join(ROOT, "oracle"))
import i3d_oracle as oracle  # noqa: E402
import hip_helpers as hh  # noqa: E402
import test_hip_ftcn  # noqa: E402
import test_hip_slowfast  # noqa: E402
from af_mi355x import aligner, arch, evaluator, synth  # noqa: E402
from af_mi355x.classifier import FtcnTT8x8, FtcnTTClassifier, I3D8x8, LiveScorer, SlowFast8x8  # noqa: E402

pytestmark = pytest.mark.gpu
CLIP, SIZE, ALPHA = 8, 64, 4
FTCN_TOL = dict(test_hip_ftcn.test_ftcn_logits_match_reference.pytestmark[0].args[1])
SLOWFAST_TOL = dict(test_hip_slowfast.test_slowfast_logits_match_reference.pytestmark[0].args[1])
SMALL = {"i3d": lambda dt: I3D8x8(clip_size=CLIP, crop_size=SIZE, precision=dt),
         "ftcn": lambda dt: FtcnTT8x8(clip_size=CLIP, crop_size=SIZE, precision=dt),
         "slowfast": lambda dt: SlowFast8x8(clip_size=CLIP, crop_size=SIZE, alpha=ALPHA, precision=dt)}
POOLED_WIDTH = {"ftcn": 1024, "slowfast": 2304}
_nets = {}


def _small(kind, dtype, copy=0):
    """the shrunken network `kind` with W(5), one per (kind, dtype, copy)"""
    if (kind, dtype, copy) not in _nets:
        net = SMALL[kind](dtype)
        net.load_state_dict(synth.synthetic_state_dict(net.spec, seed=5))
        _nets[(kind, dtype, copy)] = net.cuda().eval()
    return _nets[(kind, dtype, copy)]


def _clips(batch, seed, kind="smooth"):
    return synth.synthetic_clips_u8(batch, seed=seed, kind=kind, num_frames=CLIP, size=SIZE)


# ---- 1. the pathways pack kernel, bit for bit ----------------------------------------------------------------------------------------

def _mean_std():
    m, s = synth.pixel_mean_std_f32()
    return (C.c_float * 3)(*m.tolist()), (C.c_float * 3)(*s.tolist())


def _input_bytes(n, t, h, w, dtype, layout):
    L = hh.lib()
    fn = L.lib.af_stem_input_bytes_rgb3 if layout == L.AF_PACK_RGB3 else L.lib.af_stem_input_bytes
    return int(fn(n, t, h, w, L.DTYPE_CODES[dtype]))


def _sentinel(nbytes, salt):
    """a byte pattern no pack kernel writes by accident; torch's allocations are 16-byte aligned"""
    return ((torch.arange(nbytes, dtype=torch.int64) * 37 + salt) % 251).to(torch.uint8).cuda()


def _pack_existing(clip, dtype, layout, buf):
    L = hh.lib()
    n, t, h, w, _ = clip.shape
    mean, std = _mean_std()
    fn = L.lib.af_pack_input_u8_rgb3 if layout == L.AF_PACK_RGB3 else L.lib.af_pack_input_u8
    L.check(fn(hh._p(clip), n, t, h, w, mean, std, L.DTYPE_CODES[dtype], hh._p(buf), hh._stream()), "pack_input_u8")


def _random_clip(n, t, h, w, seed):
    g = torch.Generator().manual_seed(seed)
    clip = torch.randint(0, 256, (n, t, h, w, 3), dtype=torch.uint8, generator=g)
    clip[0, 0, 0, 0, :] = 0
    clip[-1, -1, -1, -1, :] = 255
    clip[0, 0, -1, 0, 1], clip[0, -1, 0, -1, 2] = 255, 0
    return clip


def _check_pathways(clip, alpha, dtype, slow_layout, fast_layout):
    L = hh.lib()
    n, t, h, w, _ = clip.shape
    mean, std = _mean_std()
    slow0 = _sentinel(_input_bytes(n, t // alpha, h, w, dtype, slow_layout), 11)
    fast0 = _sentinel(_input_bytes(n, t, h, w, dtype, fast_layout), 97)
    slow, fast, slow_ref, fast_ref = slow0.clone(), fast0.clone(), slow0.clone(), fast0.clone()
    L.check(L.lib.af_pack_input_u8_pathways(hh._p(clip), n, t, h, w, mean, std, alpha, L.DTYPE_CODES[dtype], hh._p(slow), slow_layout,
                                            hh._p(fast), fast_layout, hh._stream()), "pack_input_u8_pathways")
    _pack_existing(clip, dtype, fast_layout, fast_ref)
    strided = clip[:, ::alpha].contiguous()
    _pack_existing(strided, dtype, slow_layout, slow_ref)
    torch.cuda.synchronize()
    assert not torch.equal(fast_ref, fast0) and not torch.equal(slow_ref, slow0)       # the reference side wrote something
    assert torch.equal(fast, fast_ref), "Fast output differs in %d bytes" % int((fast != fast_ref).sum())
    assert torch.equal(slow, slow_ref), "Slow output differs in %d bytes" % int((slow != slow_ref).sum())


# (n, t, h, w, alpha): the five shapes of the issue, then a row of exactly one 8-pixel run and rows of five (the vector path's edges)
PACK_SHAPES = [(1, 8, 6, 10, 4), (2, 16, 8, 32, 8), (1, 4, 5, 7, 2), (1, 8, 6, 10, 8), (3, 2, 4, 4, 1), (1, 4, 3, 8, 2), (2, 2, 2, 40, 2)]
PACK_FORMS = [("f32", "c4", "c4"), ("f16", "c4", "c4"), ("bf16", "c4", "c4"), ("f16", "rgb3", "c4"), ("bf16", "rgb3", "c4"),
              ("f16", "rgb3", "rgb3"), ("bf16", "c4", "rgb3")]


@pytest.mark.parametrize("dtype,slow_layout,fast_layout", PACK_FORMS)
@pytest.mark.parametrize("shape", PACK_SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_pathways_pack_writes_the_bytes_of_the_two_single_packs(shape, dtype, slow_layout, fast_layout):
    n, t, h, w, alpha = shape
    L = hh.lib()
    code = {"c4": L.AF_PACK_C4, "rgb3": L.AF_PACK_RGB3}
    clip = _random_clip(n, t, h, w, seed=1000 + w + t).cuda()
    assert int(clip.min()) == 0 and int(clip.max()) == 255
    _check_pathways(clip, alpha, dtype, code[slow_layout], code[fast_layout])


@pytest.mark.parametrize("dtype,slow_layout", [("f32", "c4"), ("bf16", "rgb3")])
def test_pathways_pack_of_a_clip_at_an_odd_address(dtype, slow_layout):
    """w % 8 == 0 but the clip starts one byte behind an aligned address: the 8-byte loads are not taken"""
    L = hh.lib()
    n, t, h, w, alpha = 2, 4, 3, 16, 2
    store = torch.zeros(n * t * h * w * 3 + 1, dtype=torch.uint8, device="cuda")
    clip = store[1:].view(n, t, h, w, 3)
    clip.copy_(_random_clip(n, t, h, w, seed=5))
    assert clip.data_ptr() % 8 == 1 and clip.is_contiguous()
    _check_pathways(clip, alpha, dtype, L.AF_PACK_RGB3 if slow_layout == "rgb3" else L.AF_PACK_C4, L.AF_PACK_C4)


def test_pathways_pack_refuses_bad_arguments():
    L = hh.lib()
    n, t, h, w = 1, 8, 6, 10
    mean, std = _mean_std()
    clip = _random_clip(n, t, h, w, seed=3).cuda()
    slow = _sentinel(_input_bytes(n, t, h, w, "bf16", L.AF_PACK_C4) + 16, 1)
    fast = _sentinel(_input_bytes(n, t, h, w, "f32", L.AF_PACK_C4) + 16, 2)
    keep = (slow.clone(), fast.clone())

    def call(clip_p=hh._p(clip), alpha=4, dtype="bf16", slow_p=hh._p(slow), slow_layout=L.AF_PACK_C4, fast_p=hh._p(fast),
             fast_layout=L.AF_PACK_C4, mean_p=mean):
        return L.lib.af_pack_input_u8_pathways(clip_p, n, t, h, w, mean_p, std, alpha, L.DTYPE_CODES[dtype], slow_p, slow_layout,
                                               fast_p, fast_layout, hh._stream())

    assert call(alpha=3) == -1 and b"multiple of alpha" in L.lib.af_last_error()
    assert call(dtype="f32", slow_layout=L.AF_PACK_RGB3) == -1 and b"16-bit" in L.lib.af_last_error()
    assert call(dtype="f32", fast_layout=L.AF_PACK_RGB3) == -1
    assert call(slow_p=C.c_void_p(slow.data_ptr() + 8)) == -1 and b"aligned" in L.lib.af_last_error()
    assert call(fast_p=C.c_void_p(fast.data_ptr() + 2)) == -1
    for null in ("clip_p", "slow_p", "fast_p", "mean_p"):
        assert call(**{null: None}) == -1 and b"null" in L.lib.af_last_error(), null
    assert call(alpha=0) == -1 and call(slow_layout=2) == -1
    torch.cuda.synchronize()
    assert torch.equal(slow, keep[0]) and torch.equal(fast, keep[1])                    # a refused call launches nothing
    assert call() == 0


# ---- 2. uint8 path against fp32 path ---------------------------------------------------------------------------------------------------

def _both_forms(net, u8):
    with torch.inference_mode():
        yu = net.forward_clips_u8(u8)["final_output"]
        yf = net(synth.normalize_like_callers(u8))["final_output"]
    return yu, yf


@pytest.mark.parametrize("batch", [1, 2])
@pytest.mark.parametrize("kind", ["ftcn", "slowfast"])
def test_u8_path_equals_fp32_path_f32(kind, batch):
    net = _small(kind, "f32")
    u8 = _clips(batch, seed=31).cuda()
    yu, yf = _both_forms(net, u8)
    print(kind, "f32 B=%d" % batch, yu.flatten().tolist())
    assert yu.shape == (batch, 1) and torch.isfinite(yu).all() and torch.equal(yu, yf)
    if kind == "slowfast":
        x = synth.normalize_like_callers(u8)
        with torch.inference_mode():
            y2 = net([x[:, :, ::ALPHA], x])["final_output"]
        assert torch.equal(yu, y2)


@pytest.mark.parametrize("dtype", ["f16", "bf16"])
def test_u8_path_equals_fp32_path_16bit(dtype):
    """I3D first: its two input forms are bit-equal in 16-bit too (the K-packed stem's input included), so the same is
    asked of the two other networks"""
    for kind in ("i3d", "ftcn", "slowfast"):
        net = _small(kind, dtype)
        for batch in (1, 2):
            yu, yf = _both_forms(net, _clips(batch, seed=33).cuda())
            print(kind, dtype, "B=%d" % batch, "u8", yu.flatten().tolist(), "f32-input", yf.flatten().tolist())
            assert torch.isfinite(yu).all() and torch.equal(yu, yf), (kind, dtype, batch)


# ---- 3. golden logits through the uint8 path -------------------------------------------------------------------------------------------

def _golden_u8(c):
    u8 = synth.synthetic_clips_u8(c["index"] + 1, seed=c["seed"], kind=c["kind"])[c["index"]:c["index"] + 1]
    assert synth.tensor_sha256(u8) == c["clip_sha256"]
    return u8.cuda()


@pytest.mark.parametrize("dtype", ["f32", "f16", "bf16"])
@pytest.mark.parametrize("kind", ["ftcn", "slowfast"])
def test_golden_logits_through_the_u8_path(kind, dtype):
    if kind == "ftcn":
        g, tol, net = load_json("f6_ftcn.json"), FTCN_TOL[dtype], FtcnTT8x8(precision=dtype)
        spec = arch.ftcn_tt_spec()
    else:
        g, tol, net = load_json("f5_slowfast.json"), SLOWFAST_TOL[dtype], SlowFast8x8(precision=dtype)
        spec = arch.slowfast_r50_spec()
        assert g["alpha"] == spec.alpha
    sd = synth.synthetic_state_dict(spec, seed=g["weights_seed"])
    assert synth.state_dict_sha256(sd) == g["weights_sha256"]
    net.load_state_dict(sd)
    net = net.cuda().eval()
    for c in g["clips"]:
        with torch.inference_mode():
            y = net.forward_clips_u8(_golden_u8(c))["final_output"]
        err = abs(float(y[0, 0]) - c["logit_f32"])
        print("%s %s %s: hip(u8) %.6f ref %.6f |d| %.2e (gate %.0e)" % (kind, dtype, c["kind"], float(y[0, 0]), c["logit_f32"], err, tol))
        assert y.shape == (1, 1) and err <= tol


# ---- 4. scores and pooled --------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("kind", ["ftcn", "slowfast"])
def test_infer_scores_and_pooled(kind):
    L = hh.lib()
    net = _small(kind, "f32")
    u8 = _clips(2, seed=41)
    eng = lambda: net._engines[("f32", 2, (CLIP, SIZE, SIZE))]
    s = net.infer_scores(u8.numpy())
    assert isinstance(s, np.ndarray) and s.shape == (2,) and s.dtype == np.float32
    assert eng().ops[0].kind == (L.AF_OP_PACK_U8 if kind == "ftcn" else L.AF_OP_PACK_PATHWAYS_U8)
    with torch.inference_mode():
        out = net.forward_clips_u8(u8.cuda(), return_scores=True, return_pooled=True)
    want = oracle.scores(out["final_output"].cpu())
    assert np.abs(s - want.numpy()).max() <= 1e-6 and np.array_equal(s, out["scores"].cpu().numpy())
    # non-integral pixels: the callers' normalisation in torch, then the fp32 input pack
    xf = u8.float() + 0.25
    s2 = net.infer_scores(xf, as_numpy=False)
    assert eng().ops[0].kind == L.AF_OP_PACK_F32
    with torch.inference_mode():
        want2 = net(synth.normalize_like_callers(xf.cuda()), return_scores=True)
    assert s2.is_cuda and s2.shape == (2,) and torch.equal(s2, want2["scores"])
    assert (s2.cpu() - oracle.scores(want2["final_output"].cpu())).abs().max().item() <= 1e-6
    assert not torch.equal(s2.cpu(), torch.from_numpy(s))
    # the pooled row is what the last nn.Linear is given
    assert out["pooled"].shape == (2, POOLED_WIDTH[kind]) and torch.isfinite(out["pooled"]).all()
    last = [m for m in net.modules() if isinstance(m, torch.nn.Linear)][-1]
    assert last.in_features == POOLED_WIDTH[kind]
    seen = {}
    hdl = last.register_forward_hook(lambda m, i, o: seen.update(i=i[0].detach().clone(), o=o.detach().clone()))
    with torch.inference_mode():
        hooked = net.forward_clips_u8(u8.cuda(), return_pooled=True)
    hdl.remove()
    assert torch.equal(seen["i"].reshape(2, -1), hooked["pooled"]) and torch.equal(hooked["pooled"], out["pooled"])
    assert torch.allclose(hooked["final_output"], out["final_output"], rtol=0, atol=1e-5)      # torch's Linear against the head kernel


# ---- 5. one engine, alternating input forms --------------------------------------------------------------------------------------------

@pytest.mark.parametrize("dtype", ["f32", "bf16"])
@pytest.mark.parametrize("kind", ["ftcn", "slowfast"])
def test_one_engine_alternates_between_u8_and_fp32_runs(kind, dtype):
    net, fresh = _small(kind, dtype), _small(kind, dtype, copy=1)
    u8 = _clips(2, seed=51).cuda()
    x = synth.normalize_like_callers(_clips(2, seed=52).cuda())
    m, s = synth.pixel_mean_std_f32()
    with torch.inference_mode():
        net.forward_clips_u8(u8)                                    # builds the engine
        eng = net._engines[(dtype, 2, (CLIP, SIZE, SIZE))]
        names, n_ops = list(eng.op_names), eng.n_ops
        first = eng.run_u8(u8, m.tolist(), s.tolist())[0].clone()
        second = eng.run_f32(x)[0].clone()
        third = eng.run_u8(u8, m.tolist(), s.tolist())[0].clone()
        want = fresh(x)["final_output"]
    assert torch.equal(first, third) and torch.equal(second.view(2, -1), want) and not torch.equal(first, second)
    assert eng.op_names == names and eng.n_ops == n_ops == len(names)
    assert names[:2] == (["input_pack_IN_S", "input_pack_IN_F"] if kind == "slowfast" else ["input_pack", "resnet.s1.pathway0_stem.conv"])


# ---- 6. LiveScorer ---------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("kind", ["ftcn", "slowfast"])
def test_live_scorer_graph_replay_equals_infer_scores(kind):
    net = _small(kind, "f16")
    scorer = LiveScorer(net, clip_size=CLIP, crop=SIZE)
    seen = set()
    with torch.inference_mode():
        for seed in (1, 2, 3):
            u8 = _clips(1, seed=seed).cuda()
            want = net.infer_scores(u8)
            got = scorer(u8[0])
            assert got.shape == want.shape and float(got[0]) == float(want[0]), (got, want)
            scorer.clip.zero_()
            scorer.clip.copy_(u8)
            assert float(scorer()[0]) == float(want[0])
            seen.add(float(want[0]))
    assert len(seen) == 3 and all(0.0 < v < 1.0 for v in seen)


# ---- 7. TrackScorer / VideoScorer ------------------------------------------------------------------------------------------------------

def _ftcn_classifier():
    if "ftcn_clf" not in _nets:
        clf = FtcnTTClassifier(clip_size=CLIP, crop_size=SIZE, precision="f16")
        clf.network.load_state_dict(synth.synthetic_state_dict(clf.network.spec, seed=5))
        _nets["ftcn_clf"] = clf.cuda().eval()
    return _nets["ftcn_clf"]


@pytest.mark.parametrize("kind", ["ftcn", "slowfast"])
def test_track_scorer_equals_forward_clips_u8_on_its_windows(kind):
    net = _ftcn_classifier() if kind == "ftcn" else _small("slowfast", "f16")
    infos, crops = aligner.synthetic_clip(frames=40, seed=22)
    scorer = evaluator.TrackScorer(net, clip_size=CLIP, size=SIZE, batch=16)
    windows = evaluator.clip_windows(40, CLIP)
    assert len(windows) == 33 and scorer.partition(33) == [(0, 16, 16), (16, 16, 16), (32, 1, 1)]
    got = scorer.score_track(infos, crops)
    clips = scorer.aligned_windows(infos, crops, windows)
    assert tuple(clips.shape) == (33, CLIP, SIZE, SIZE, 3) and bool(clips.any())
    want = []
    for lo, n, run in scorer.partition(len(windows)):
        batch = torch.cat([clips[lo:lo + n]] + [clips[lo + n - 1:lo + n]] * (run - n))
        with torch.inference_mode():
            want.append(scorer.network.forward_clips_u8(batch, return_scores=True)["scores"][:n])
    want = torch.cat(want).float().cpu()
    print(kind, "track scores", got[:4], "...")
    assert got.dtype == np.float32 and got.shape == (33,) and torch.equal(torch.from_numpy(got), want)
    assert ((got > 0) & (got < 1)).all() and len(set(got.tolist())) > 1


def test_video_scorer_with_an_ftcn_classifier_equals_score_video_on_host_cut_crops():
    rng = np.random.default_rng(71)
    shape, n_frames = (360, 640, 3), 40
    frames = [rng.integers(0, 256, shape, dtype=np.uint8) for _ in range(n_frames)]
    std = (aligner.STD_POINTS_317 - aligner.STD_POINTS_317.mean(0)) * (45.0 / 90.0) * (180.0 / 317.0)
    detections = []
    for i in range(n_frames):                                   # one face that walks to the right
        cx, cy = 150.0 + 8.5 * i + rng.normal(0, 1.0), 150.0 + rng.normal(0, 1.0)
        half = 45.0 + rng.normal(0, 0.5)
        box = np.array([cx - half, cy - half, cx + half, cy + half], dtype=np.float32)
        detections.append([(box, (std + [cx, cy] + rng.normal(0, 0.5, (5, 2))).astype(np.float32), np.float32(0.99))])
    detections = evaluator.get_valid_faces(detections)
    clf = _ftcn_classifier()
    tracks = evaluator.multiple_tracking(detections)
    assert len(tracks) == 1
    with_lm68 = [[(f[0], f[1], np.zeros((0, 2)), f[-1]) for f in t] for t in tracks]
    host = evaluator.TrackScorer(clf, clip_size=CLIP, size=SIZE)
    want = host.score_video(shape, frames, with_lm68, [(0, n_frames)], 0.04)
    got = evaluator.VideoScorer(None, clf, clip_size=CLIP, size=SIZE).score(frames, detections=detections)
    print("ftcn video_score", got["video_score"], "preds", got["preds"][:3])
    assert len(got["preds"]) == 33 and got["preds"] == want["preds"] and got["video_score"] == want["video_score"]
    assert got["frame_res"] == want["frame_res"] and got["pred_label"] == want["pred_label"] and 0.0 < got["video_score"] < 1.0
