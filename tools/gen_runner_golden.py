"""Writes tests/golden/runner_video.json: scripted videos driven through the REFERENCE's own ``VideoRunner.run``
(altfreezing/TEST2.py:303-797), with what its loop did on the way and what it returned.  tests/test_runner_host.py replays the file
through ``af_mi355x.runner.VideoRunner`` with a scripted detector, scripted quality figures and scripted scores.

    python tools/gen_runner_golden.py [--reference DIR]

TEST2.py is loaded by path.  What it imports and is not installed where this runs, or is of no use without a GPU, a checkpoint or
a video file, gets a stand-in of this script's own in ``sys.modules`` first:
  cv2          ``VideoCapture`` over a scripted list of small frames; ``cvtColor`` reverses the channels (BGR2RGB) or is
               tests/quality_ref.py's grey (RGB2GRAY); ``resize`` is its INTER_AREA half size; ``Laplacian`` its Laplacian, returned
               as an array whose ``var()`` is the exact-integer variance ``quality_ref.variance`` forms;
  mediapipe, tqdm, config, test_tools.faster_crop_align_xray, utils.plugin_loader, preprocessing.yunet.yunet: names only
               (test_tools/utils.py, for ``get_crop_box``, is the reference's own file, loaded by path);
  lap, cython_bbox   as tools/gen_bytetrack_golden.py has them: scipy's assignment, which ASSERTS that every optimum is unique.
The runner is made with ``VideoRunner.__new__`` and given the attributes ``__init__`` would set: no singleton service, no yaml and no
checkpoint is touched.  YuNet returns scripted rows, FaceMesh finds nothing, ``crop_align`` records what it is handed and returns
zeros, the classifier returns scripted scores.  A frame is an array that remembers its index, and so do the crops cut from it;
the tid of a clip is found by its last box among the tracks the tracker returned on that frame.

The scripted faces sit near the frame's origin on purpose: TEST2.py:535 hands ``STrack`` - which takes tlwh - a tlbr box, so a track's
box is ``(x, y, 2x + w, 2y + h)``, and YuNet's five points are used only when that box and the detection overlap with IoU >= 0.4.

Runs (each property is asserted before the file is written):
  a  plain: ``stride=0``, two tracks (a third, small one under ``min_track_side``), detections that each of the three filters drops,
     more than 50 gate calls (the ``_qstat`` cap), at least four clips, flush groups of ``batch_clips`` and a final one; run again
     with every pool method on the same scores;
  b  ``smart_start`` with a late first face and a ``linspace``-thinned window list.  The budget break cannot happen with a frame
     count: the budget is the sum of the ranges' lengths, at least the number of kept frames - it is in d;
  c  a blurry span the gate rejects, everything gone for longer than the track buffer (a new id at the old place: an id switch),
     ``low_quality`` true and the QA rule flipping the label;
  d  ``total_frames=0``: every frame kept, the budget break at ``max_frame``, no clip, score 0.0.
"""
import argparse
import contextlib
import hashlib
import importlib.util
import io
import json
import os
import sys
import types

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for _p in ("oracle", "tests", "tools", ""):
    sys.path.insert(0, os.path.join(ROOT, _p))
import gen_bytetrack_golden as G       # noqa: E402
import quality_ref as Q                # noqa: E402

H, W, CLIP, SIZE = 120, 160, 8, 64
STD5 = np.array([[0.3, 0.35], [0.7, 0.35], [0.5, 0.55], [0.35, 0.75], [0.65, 0.75]])
NOW = {"frame": -1, "vars": [], "half_cache": {}}
VIDEOS = {}                                # "path" -> scripted video, for the VideoCapture stand-in


# ---- the stand-ins ----------------------------------------------------------------------------------------------------------------

class Frame(np.ndarray):
    """an array that remembers which frame it is (cut from)"""
    frame_idx = -1

    def __array_finalize__(self, obj):
        self.frame_idx = getattr(obj, "frame_idx", -1)


class _Lap(np.ndarray):
    def var(self, *a, **k):
        v = np.asarray(self)
        out = Q.variance(int(v.size), int(v.sum()), int((v * v).sum()))
        NOW["vars"].append(out)
        return out


class _Capture:
    CAP_PROP_FPS, CAP_PROP_FRAME_COUNT, CAP_PROP_POS_FRAMES = 5, 7, 1

    def __init__(self, path):
        self.video, self.at = VIDEOS[path], 0

    def isOpened(self):
        return True

    def get(self, prop):
        return {self.CAP_PROP_FPS: self.video["fps"], self.CAP_PROP_FRAME_COUNT: self.video["total_frames"]}[prop]

    def set(self, prop, value):
        assert prop == self.CAP_PROP_POS_FRAMES
        self.at = int(value)

    def read(self):
        if self.at >= len(self.video["frames"]):
            return False, None
        f = self.video["frames"][self.at].view(Frame)
        f.frame_idx = NOW["frame"] = self.at
        self.at += 1
        return True, f

    def release(self):
        pass


def _cv2():
    cv2 = types.ModuleType("cv2")
    cv2.COLOR_BGR2RGB, cv2.COLOR_RGB2GRAY, cv2.CV_64F, cv2.INTER_AREA, cv2.INTER_LINEAR = "bgr2rgb", "rgb2gray", "f64", "area", "linear"
    cv2.CAP_PROP_FPS, cv2.CAP_PROP_FRAME_COUNT, cv2.CAP_PROP_POS_FRAMES = _Capture.CAP_PROP_FPS, _Capture.CAP_PROP_FRAME_COUNT, _Capture.CAP_PROP_POS_FRAMES
    cv2.setNumThreads = lambda n: None
    cv2.VideoCapture = lambda video: _Capture(video)

    def cvtColor(img, code):
        if code == cv2.COLOR_BGR2RGB:
            return img[..., ::-1]
        assert code == cv2.COLOR_RGB2GRAY
        return Q.grey(np.asarray(img), "rgb")

    def resize(img, dsize, interpolation=None):
        h, w = img.shape[:2]
        assert interpolation == cv2.INTER_AREA and tuple(dsize) == (max(1, w // 2), max(1, h // 2))
        key = hashlib.sha1(np.ascontiguousarray(img).tobytes() + bytes(str(img.shape), "ascii")).hexdigest()
        if key not in NOW["half_cache"]:
            NOW["half_cache"][key] = Q.half_size(np.asarray(img))
        return NOW["half_cache"][key]

    def Laplacian(grey, depth):
        assert depth == cv2.CV_64F
        return Q.laplacian(grey).view(_Lap)
    cv2.cvtColor, cv2.resize, cv2.Laplacian = cvtColor, resize, Laplacian
    return cv2


class _Tqdm:
    def __init__(self, *a, **k):
        pass

    def update(self, n):
        pass

    def close(self):
        pass


def load_reference_runner(reference):
    names = {"cv2": _cv2(), "lap": {"lapjv": G._lapjv}, "cython_bbox": {"bbox_overlaps": G._bbox_overlaps},
             "mediapipe": {}, "tqdm": {"tqdm": _Tqdm}, "config": {"config": types.SimpleNamespace()},
             "test_tools": {}, "test_tools.faster_crop_align_xray": {"FasterCropAlignXRay": object},
             "utils": {}, "utils.plugin_loader": {"PluginLoader": object},
             "preprocessing.yunet": {}, "preprocessing.yunet.yunet": {"YuNet": object}}
    for name, attrs in names.items():
        mod = attrs if isinstance(attrs, types.ModuleType) else types.ModuleType(name)
        if isinstance(attrs, dict):
            mod.__dict__.update(attrs)
        sys.modules[name] = mod
    for pkg in ("test_tools", "utils", "preprocessing.yunet"):
        sys.modules[pkg].__path__ = []
    # test_tools/utils.py needs numpy and the cv2 stand-in alone: get_crop_box is the reference's own
    spec = importlib.util.spec_from_file_location("test_tools.utils", os.path.join(reference, "altfreezing", "test_tools", "utils.py"))
    sys.modules["test_tools.utils"] = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(sys.modules["test_tools.utils"])
    spec = importlib.util.spec_from_file_location("ref_test2", os.path.join(reference, "altfreezing", "TEST2.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


# ---- the scripts ------------------------------------------------------------------------------------------------------------------

def _row(rng, x, y, w, h, score):
    j = rng.uniform(-0.3, 0.3, 4)
    x, y, w, h = x + j[0], y + j[1], w + j[2], h + j[3]
    lm = STD5 * [w, h] + [x, y] + rng.normal(0, 0.4, (5, 2))
    return np.concatenate([[x, y, w, h], [score + rng.uniform(-0.004, 0.004)], lm.ravel()]).astype(np.float32)


FACE_A = lambda f: (6 + 0.10 * f, 5 + 0.05 * f, 60, 66, 0.95)            # noqa: E731
FACE_B = lambda f: (30 - 0.05 * f, 20 + 0.04 * f, 60, 64, 0.93)           # noqa: E731
FACE_C = (2, 2, 38, 44, 0.91)                                            # its track stays under min_track_side


def video(seed, n, faces_of, total_frames=None, fps=30.0, flat=None):
    """frames of seeded noise; ``faces_of(f)`` -> the faces (x, y, w, h, score) YuNet is scripted to find on frame f;
    ``flat``: ``(first, last, (x0, y0, x1, y1))`` - frames whose rectangle is one grey level, so a crop inside it has no Laplacian"""
    rng = np.random.default_rng(seed)
    frames, rows = [], []
    for f in range(n):
        frame = rng.integers(0, 256, (H, W, 3), dtype=np.uint8)
        if flat is not None and flat[0] <= f <= flat[1]:
            x0, y0, x1, y1 = flat[2]
            frame[y0:y1, x0:x1] = 90
        frames.append(frame)
        found = [_row(rng, *face) for face in faces_of(f)]
        rows.append(np.asarray(found, dtype=np.float32).reshape(-1, 15))
    return {"seed": seed, "frames": frames, "rows": rows, "fps": fps, "total_frames": n if total_frames is None else total_frames,
            "flat": flat}


BASE = dict(optimal_threshold=0.4, max_frame=400, clip_size=CLIP, crop_scale=0.2, conf=0.7, track_thresh=0.6, track_buffer=2000,
            match_thresh=0.6, mot20=False, detect_every=3, stride=5, smart_start=False, start_after_n=5, start_conf=0.6, start_min_size=20, roi_scale=2.0,
            mesh_every=3, q_weighting=True, q_min_size_soft=72, q_min_size_hard=48, q_lap_soft=24, q_lap_hard=8, batch_clips=3,
            pool_method="median", percentile_p=70.0, trim_ratio=0.2, topk_ratio=0.3, min_clips=1, verbose_pool=False, disable_penalty=False,
            qa_min_side=240, qa_min_lap=16.0, qa_q75_thr=0.30, qa_q90_thr=0.90, min_det_side=30, min_det_area=1500,
            exclude_bottom_frac=0.10, min_track_side=50)


def faces_a(f):
    faces = [FACE_A(f), FACE_B(f)]
    if f >= 6:
        faces.append(FACE_C)
    if f % 7 == 3:
        faces.append((80, 6, 22, 26, 0.9))             # under min_det_side
    if f % 7 == 5:
        faces.append((90, 40, 35, 40, 0.9))            # side enough, area 1400 under min_det_area
    if f % 5 == 0:
        faces.append((100, 96, 40, 40, 0.9))           # its centre in the bottom tenth
    return faces


def scores_a(tid, k):
    """track 1 spreads wide under a low median (the stability penalty bites), track 2 sits high and tight"""
    wide, tight = [0.12, 0.81, 0.35, 0.66, 0.22, 0.93, 0.48, 0.57], [0.88, 0.91, 0.86, 0.9, 0.93, 0.87, 0.89, 0.92]
    return (wide if tid % 2 == 1 else tight)[k % 8] + 0.001 * (k // 8)


def scores_c(tid, k):
    return [0.22, 0.36, 0.38, 0.31, 0.27, 0.39, 0.33, 0.29][k % 8]       # never over the 0.4 threshold; q75 over 0.30


RUNS = {
    "a": dict(video=lambda: video(31, 64, faces_a), args=dict(stride=0, qa_min_side=40), scores=scores_a),
    "b": dict(video=lambda: video(32, 120, lambda f: [FACE_A(f)] if f >= 36 else []),
              args=dict(smart_start=True, start_after_n=3, stride=2, max_frame=32, detect_every=1, qa_min_side=40), scores=scores_a),
    "c": dict(video=lambda: video(33, 90, lambda f: [FACE_A(f % 45)] if not 30 <= f < 45 else [], flat=(12, 17, (0, 0, 110, 110))),
              args=dict(track_buffer=6, detect_every=1, stride=3, batch_clips=2), scores=scores_c),
    "d": dict(video=lambda: video(34, 40, lambda f: [FACE_A(f), FACE_B(f)], total_frames=0),
              args=dict(max_frame=25, detect_every=2, qa_min_side=40), scores=scores_a),
}


# ---- one run through the reference ------------------------------------------------------------------------------------------------

def run_reference(T2, vid, args, score_of):
    a = types.SimpleNamespace(**args)
    log = {"infer": [], "tracks": {}, "gate": [], "clips": [], "groups": [], "pending": [], "scores": [], "per_tid": {}}
    NOW["frame"], NOW["vars"] = -1, []

    class YuNetStub:
        def set_frame_size(self, w, h):
            assert (w, h) == (W, H)

        def infer(self, frame):
            assert frame.frame_idx == NOW["frame"]
            log["infer"].append(frame.frame_idx)
            return vid["rows"][frame.frame_idx].copy()

    class MeshStub:
        def process(self, roi):
            return None

    def crop_align(infos, imgs):
        ids = [int(im.frame_idx) for im in imgs]
        nb, _, _, big = infos[-1]
        last = nb + np.array([big[0], big[1], big[0], big[1]], dtype=np.float32)
        near = [tid for tid, box in log["tracks"][ids[-1]] if np.abs(box - last).max() < 1e-3]
        assert len(near) == 1, (ids[-1], near)
        assert all(lm68.shape == (68, 2) and not lm68.any() for _, _, lm68, _ in infos)       # FaceMesh found nothing (:368-369)
        clip = {"tid": int(near[0]), "frame_ids": ids, "boxes": [[float(v) for v in i[0]] for i in infos],
                "lm5": [[float(v) for v in i[1].ravel()] for i in infos], "big": [[int(v) for v in i[3]] for i in infos],
                "crop_shapes": [[int(im.shape[0]), int(im.shape[1])] for im in imgs]}
        for c, im in zip(clip["big"], imgs):
            assert (c[3] - c[1], c[2] - c[0]) == im.shape[:2]
        log["clips"].append(clip)
        log["pending"].append(clip["tid"])
        return None, np.zeros((len(imgs), SIZE, SIZE, 3), dtype=np.uint8)

    class ClassifierStub:
        def infer_scores(self, arr):
            assert arr.shape == (len(log["pending"]), CLIP, SIZE, SIZE, 3) and arr.dtype == np.uint8
            out = []
            for tid in log["pending"]:
                k = log["per_tid"].get(tid, 0)
                log["per_tid"][tid] = k + 1
                out.append(np.float32(score_of(tid, k)))
            log["groups"].append(list(log["pending"]))
            log["scores"].append([float(s) for s in out])
            log["pending"].clear()
            return np.asarray(out, dtype=np.float32)

    runner = T2.VideoRunner.__new__(T2.VideoRunner)
    runner.args, runner.device, runner.cfg, runner.clip_size = a, "cpu", types.SimpleNamespace(imsize=SIZE), CLIP
    runner.classifier, runner.crop_align, runner.yunet = ClassifierStub(), crop_align, YuNetStub()
    runner.facemesh = types.SimpleNamespace(pick=lambda tlbr: MeshStub())
    svc = T2.ByteTrackSvc.__new__(T2.ByteTrackSvc)                         # not ByteTrackSvc(...): that would make the singleton
    svc.args, svc.fps, svc.tracker = a, 30.0, T2.BYTETracker(a, frame_rate=30.0)
    inner_update = svc.update

    def update(tracks_in, wh, wh2):
        G._frame[0] = NOW["frame"]
        online = inner_update(tracks_in, wh, wh2)
        log["tracks"][NOW["frame"]] = [(int(t.track_id), t.tlbr.astype(np.float32)) for t in online]
        return online
    svc.update = update
    runner.bytetrack = svc
    inner_gate = runner._frame_quality_weight

    def gate(crop_rgb):
        n0 = len(NOW["vars"])
        wq = inner_gate(crop_rgb)
        seen = NOW["vars"][n0:]
        log["gate"].append({"frame": int(crop_rgb.frame_idx), "shape": [int(crop_rgb.shape[0]), int(crop_rgb.shape[1])], "lap": float(seen[0]),
                            "full": float(seen[1]) if len(seen) > 1 else None, "weight": float(wq)})
        return wq
    runner._frame_quality_weight = gate
    VIDEOS["scripted.mp4"] = vid
    with contextlib.redirect_stdout(io.StringIO()) as printed:
        ret = runner.run("scripted.mp4")
    # _qstat is cleared at the end of run (:694); its records are the gate's calls with a full-size figure, in order
    qstat = [[min(g["shape"]), g["full"]] for g in log["gate"] if g["full"] is not None]
    assert "[QA]" in printed.getvalue() or not qstat
    assert not log["pending"]
    return ret, log, qstat, printed.getvalue()


def returned(ret):
    drop = ("video_path", "elapsed_s", "fps", "latency_ms_clip_mean", "gpu_mem_alloc_peak_mb", "gpu_mem_reserved_peak_mb", "cpu_mem_peak_mb")
    out = {k: v for k, v in ret.items() if k not in drop}
    out["per_person_scores"] = {str(k): float(v) for k, v in ret["per_person_scores"].items()}
    out["per_person_labels"] = {str(k): int(v) for k, v in ret["per_person_labels"].items()}
    return out


def record(T2, name):
    spec = RUNS[name]
    vid, args = spec["video"](), dict(BASE, **spec["args"])
    ret, log, qstat, printed = run_reference(T2, vid, args, spec["scores"])
    tcs = {}
    for tids, scores in zip(log["groups"], log["scores"]):
        for tid, s in zip(tids, scores):
            tcs.setdefault(str(tid), []).append(s)
    doc = {"frame_shape": [H, W, 3], "n_frames": len(vid["frames"]), "seed": vid["seed"], "flat": vid["flat"], "fps": vid["fps"],
           "total_frames": vid["total_frames"], "args": args, "rows": [[[float(v) for v in r] for r in rows] for rows in vid["rows"]],
           "detected": log["infer"], "processed": sorted(log["tracks"]), "gate": log["gate"], "clips": log["clips"],
           "flush_groups": log["groups"], "scores": log["scores"], "qstat": qstat, "track_clip_scores": tcs, "returned": returned(ret),
           "low_quality": "low_quality=True" in printed}
    return doc, vid, args, log


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reference", default=None)
    ap.add_argument("--out", default=os.path.join(ROOT, "tests", "golden", "runner_video.json"))
    opt = ap.parse_args()
    if opt.reference is None:
        import ref_import
        opt.reference = ref_import.REFERENCE_ROOT
    T2 = load_reference_runner(opt.reference)
    runs = {}
    for name in RUNS:
        runs[name], vid, args, log = record(T2, name)
        if name == "a":                                                    # every pool method on the same clips and scores
            pools = {}
            for method in ("median", "mean", "topk", "topk_median", "percentile", "trimmed_mean", "logit_median", "adaptive"):
                ret, log_m, _, _ = run_reference(T2, vid, dict(args, pool_method=method), RUNS["a"]["scores"])
                assert log_m["groups"] == log["groups"] and log_m["scores"] == log["scores"]
                pools[method] = returned(ret)
            runs["a"]["pool_methods"] = pools

    a, b, c, d = (runs[k] for k in "abcd")
    # a
    assert a["args"]["stride"] == 0 and len(a["track_clip_scores"]) >= 2 and len(a["clips"]) >= 4, (len(a["clips"]), a["track_clip_scores"])
    assert len(a["gate"]) > 50 and len(a["qstat"]) == 50, (len(a["gate"]), len(a["qstat"]))
    assert len(a["flush_groups"]) >= 2 and len(a["flush_groups"][0]) == a["args"]["batch_clips"]
    assert len(a["detected"]) < len(a["processed"]), "detect_every never skipped a frame"
    assert not a["low_quality"]
    values = [tuple(sorted(p["per_person_scores"].items())) for p in a["pool_methods"].values()]
    assert len(set(values)) >= 6, "the pool methods barely differ on these scores"
    med = a["pool_methods"]["median"]
    assert any(abs(med["per_person_scores"][t] - float(np.median(s))) > 1e-3 for t, s in a["track_clip_scores"].items()), "no penalty"
    assert med == a["returned"]
    # b
    first_face = 36
    assert b["processed"] and min(b["processed"]) == first_face + b["args"]["start_after_n"], b["processed"][:4]
    kept = [f for f in b["detected"]]
    assert max(kept) >= 112 and not any(8 <= f < 36 for f in kept), "the window list was not thinned"
    assert len(b["clips"]) >= 1
    # c
    assert any(g["weight"] == 0.0 and g["lap"] < c["args"]["q_lap_hard"] for g in c["gate"]), "the gate rejected nothing"
    assert c["low_quality"] and c["returned"]["pred_label"] == 1 and c["returned"]["video_score"] <= c["args"]["optimal_threshold"]
    assert c["returned"]["id_switch_rate_per_1k_frames"] > 0 and len(c["track_clip_scores"]) >= 2
    # d
    assert d["total_frames"] == 0 and not d["clips"] and d["returned"]["video_score"] == 0.0 and d["returned"]["num_tracks"] == 0
    assert len(d["processed"]) == d["args"]["max_frame"] < d["n_frames"] and len(d["gate"]) > 0, "no budget break"
    assert G.EVENTS["solved"] > 100                                        # every one of them asserted unique

    doc = {"what": "what the reference's VideoRunner.run (altfreezing/TEST2.py) did on scripted videos (tools/gen_runner_golden.py)",
           "clip_size": CLIP, "imsize": SIZE, "runs": runs}
    with open(opt.out, "w") as fh:
        json.dump(doc, fh, separators=(",", ":"), sort_keys=True)
    print("wrote %s: %d bytes; clips %s, gate calls %s, matrices solved %d" % (
        opt.out, os.path.getsize(opt.out), {k: len(r["clips"]) for k, r in runs.items()}, {k: len(r["gate"]) for k, r in runs.items()},
        G.EVENTS["solved"]))


if __name__ == "__main__":
    main()
