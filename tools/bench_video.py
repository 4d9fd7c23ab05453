"""The offline evaluator from decoded frames to the video's score on one MI355X: VideoScorer.score against the composition of
the stages it joins, in one process.

    python tools/bench_video.py [--frames 400] [--reps 3] [--sizes 1080x1920,360x640] [--faces 1,2] [--dtype f16] [--json out.json]

Workload: a video of `--frames` frames (eight distinct seeded frames in turn, handed over as the channel-reversed views
grab_all_frames(cvt=True) returns), seeded detector and classifier weights.  A detector with seeded weights finds noise, so the
detector here does ALL of its device work on the frames it is given and then hands back scripted detections: one or two faces that
drift across the video (device-independent seeds).  Both paths get the same ones.
  new     VideoScorer.score(frames): every frame uploaded once, detector on views of the frame store, tracks on the host, window
          batches warped out of rectangles of the resident frames
  parent  detector.detect on partition(frames, 50) -> get_valid_faces -> multiple_tracking -> crops cut on the host ->
          TrackScorer.score_video: the frames uploaded for the detector, the crops staged and uploaded again
Host-inclusive: wall clock from the list of frames to video_score.  Both are warmed up; new / parent alternate `--reps` times;
median and spread (max - min), frames/s, and the bytes each path sends to the device.  `host_pass`: the time of the strided host
copy that makes one channel-reversed frame packed (the new path does it into the pinned slot, the parent in its np.stack).
`kernel`: device-event time of one window-batch launch of 16 windows out of the resident frames against the pool form on crops
cut from the same frames, alternated.  Prints one JSON line.  A run without a GPU fails."""
import argparse
import ctypes as C
import json
import os
import platform
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import numpy as np  # noqa: E402
import torch  # noqa: E402


def _stats(v):
    return {"median": statistics.median(v), "spread": max(v) - min(v), "all": [round(x, 4) for x in v]}


def scripted_rows(n_frames, h, w, faces, seed):
    """(n_frames, 10, 15) float32 rows x1 y1 x2 y2 score l0x .. l4y and (n_frames,) int32 counts: `faces` faces drifting sideways"""
    from af_mi355x import aligner
    rng = np.random.default_rng(seed)
    rows = np.zeros((n_frames, 10, 15), dtype=np.float32)
    half = h / 6.0
    std = (aligner.STD_POINTS_317 - aligner.STD_POINTS_317.mean(0)) * (half / 90.0) * (180.0 / 317.0)
    for k in range(faces):
        cx, cy = w * (0.3 + 0.4 * k), h * (0.45 + 0.1 * k)
        for i in range(n_frames):
            cx, cy = cx + (0.2 if k == 0 else -0.2) + rng.normal(0, 0.5), cy + rng.normal(0, 0.5)
            hh = half + rng.normal(0, 0.3)
            rows[i, k, :4] = [cx - hh, cy - hh, cx + hh, cy + hh]
            rows[i, k, 4] = 0.99 - 0.02 * k
            rows[i, k, 5:] = (std + [cx, cy] + rng.normal(0, 0.4, (5, 2))).reshape(-1)
    return rows, np.full(n_frames, faces, dtype=np.int32)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", type=int, default=400)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--sizes", default="1080x1920,360x640")
    ap.add_argument("--faces", default="1,2")
    ap.add_argument("--dtype", default="f16")
    ap.add_argument("--kernel-iters", type=int, default=20)
    ap.add_argument("--json", default=None)
    args = ap.parse_args()
    assert torch.cuda.is_available(), "bench_video needs a GPU"
    import af_mi355x  # noqa: F401
    from af_mi355x import _lib, evaluator, retinaface as rf, synth
    from af_mi355x.classifier import Classifier

    clf = Classifier(precision=args.dtype)
    clf.network.load_state_dict(synth.synthetic_state_dict(seed=0))
    net = clf.cuda().eval().network

    class ScriptedDetector(rf.FaceDetector):
        """the detector's whole device work, then the scripted rows of the frames it was given (in call order)"""
        script, cursor = None, 0

        def detect_device(self, frames_u8, keep_top_k=rf.KEEP_TOP_K, max_count=0, min_score=0.0, raw=False, timings=None):
            rows, counts = super().detect_device(frames_u8, keep_top_k, max_count, min_score)
            b, lo = frames_u8.shape[0], self.cursor
            self.cursor += b
            k = rows.shape[1]
            out_rows = torch.zeros_like(rows)
            out_rows[:, :min(k, 10)] = self.script[0][lo:lo + b, :min(k, 10)]
            return out_rows, self.script[1][lo:lo + b].clone()

    det = ScriptedDetector.from_state_dict(synth.retinaface_state_dict(1, "sparse"), gpu_id=0)
    props = torch.cuda.get_device_properties(0)
    out = {"tool": "bench_video", "device": props.name, "arch": props.gcnArchName, "compute_units": props.multi_processor_count,
           "hbm_gib": round(props.total_memory / 2 ** 30), "host": platform.node(), "frames": args.frames, "reps": args.reps,
           "dtype": args.dtype, "cases": {}}

    for size in args.sizes.split(","):
        h, w = (int(v) for v in size.split("x"))
        rng = np.random.default_rng(h)
        distinct = [np.ascontiguousarray(rng.integers(0, 256, (h, w, 3), dtype=np.uint8)) for _ in range(8)]
        frames = [distinct[i % 8][..., ::-1] for i in range(args.frames)]
        t0 = time.perf_counter()
        for _ in range(5):
            np.ascontiguousarray(frames[0])
        host_pass = (time.perf_counter() - t0) / 5
        for faces in (int(v) for v in args.faces.split(",")):
            rows, counts = scripted_rows(args.frames, h, w, faces, seed=1000 * faces + h)
            det.script = (torch.from_numpy(rows).cuda(), torch.from_numpy(counts).cuda())
            vs = evaluator.VideoScorer(det, net)
            ts = evaluator.TrackScorer(net)
            sent = {}

            def run_new():
                det.cursor = 0
                res = vs.score(frames)
                sent["new"] = vs.uploaded_bytes
                return res

            def run_parent():
                det.cursor = 0
                raw = []
                for lo in range(0, len(frames), 50):
                    raw += det.detect(frames[lo:lo + 50])
                detections = evaluator.get_valid_faces(raw, thres=0.5)
                tracks = evaluator.multiple_tracking(detections)
                spans = [(0, len(detections))] * len(tracks)
                if not tracks:
                    spans, tracks = evaluator.find_longest(detections)
                res = ts.score_video(frames[0].shape, frames, [[(f[0], f[1], np.zeros((0, 2)), f[-1]) for f in t] for t in tracks], spans)
                sent["parent"] = ts.uploaded_bytes + sum(f.nbytes for f in frames)
                return res

            a, b = run_new(), run_parent()                         # warm-up, and the two paths must agree
            assert a["preds"] == b["preds"] and len(a["preds"]) == faces * (args.frames - 31), (len(a["preds"]), len(b["preds"]))
            times = {"new": [], "parent": []}
            for _ in range(args.reps):
                for name, fn in (("new", run_new), ("parent", run_parent)):
                    torch.cuda.synchronize()
                    t0 = time.perf_counter()
                    fn()
                    torch.cuda.synchronize()
                    times[name].append(time.perf_counter() - t0)
            case = {"windows": len(a["preds"]), "video_score": a["video_score"], "host_pass_per_frame_s": host_pass}
            for name in ("new", "parent"):
                st = _stats(times[name])
                case[name] = {"seconds": st, "frames_per_s": args.frames / st["median"], "uploaded_bytes": int(sent[name])}
            out["cases"]["%s_faces%d" % (size, faces)] = case
            print(size, faces, json.dumps(case), file=sys.stderr, flush=True)

        # the kernel alone: 16 windows out of the resident frames against the pool form on host-cut crops of the same frames
        rows, _ = scripted_rows(48, h, w, 1, seed=h)
        recs = evaluator.crop_records((h, w), [(rows[i, 0, :4].astype(np.float64), rows[i, 0, 5:].reshape(5, 2).astype(np.float64),
                                                np.zeros((0, 2)), 0.99) for i in range(47)])
        infos = [info for _, info in recs]
        packed = [np.ascontiguousarray(f) for f in frames[:47]]
        crops = [packed[i][b[1]:b[3], b[0]:b[2]] for i, (b, _) in enumerate(recs)]
        windows = evaluator.clip_windows(47, 32)
        vs, ts = evaluator.VideoScorer(None, net), evaluator.TrackScorer(net)
        got, want = vs.aligned_windows(packed, range(47), infos, windows), ts.aligned_windows(infos, crops, windows)
        assert torch.equal(got, want)
        vtrack, ttrack = evaluator._FrameTrack(infos, range(47), (h, w)), evaluator._Track(infos, crops)
        voffs, toffs = np.arange(47), np.concatenate([[0], np.cumsum(ttrack.bytes)[:-1]])
        ms = {"rects": [], "pool": []}
        for _ in range(args.kernel_iters):
            for name, sc, tr, offs in (("rects", vs, vtrack, voffs), ("pool", ts, ttrack, toffs)):
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                table = sc.warp.tables.last.dev                     # the table the last warp left on the device: launch it again
                stream = C.c_void_p(torch.cuda.current_stream().cuda_stream)
                if _ == 0:
                    sc.warp(tr, windows, offs, 0, got, [evaluator._fit(tr, idx, sc.std_points) for idx in windows])
                    torch.cuda.synchronize()
                    continue
                e0.record()
                _lib.check(getattr(_lib.lib, sc.warp.form.launch)(C.c_void_p(sc.source.dev.data_ptr()), C.c_void_p(table.data_ptr()), 16, 32, 224,
                                                         C.c_void_p(got.data_ptr()), stream), "launch")
                e1.record()
                torch.cuda.synchronize()
                ms[name].append(e0.elapsed_time(e1))
        out.setdefault("kernel", {})[size] = {k: _stats(v) for k, v in ms.items()}
    line = json.dumps(out)
    print(line)
    if args.json:
        with open(args.json, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
