"""The dataset evaluator's per-video loop on one MI355X: runner.VideoRunner.run over a scripted video, at detect_batch 1 and 16,
against RealtimeCall.step over the frames the loop keeps - the closest thing the tree offered before the runner.

    python tools/bench_runner.py [--frames 600] [--sizes 720,1080] [--reps 3] [--dtype f16] [--json profiles/runner_bench.json]
    python tools/bench_runner.py --tracker host,device [--json profiles/runner_tracker_bench.json]

Workload: a `--frames`-frame video of 720p and of 1080p (32 distinct seeded BGR noise frames in turn), 30 fps, with its frame
count, and the evaluator's defaults (altfreezing/TEST2.py:963-1042: clip 32, stride 5, max_frame 400, detect_every 3, crop_scale 1,
batch_clips 8) - so 12 linspace-thinned windows of 32 frames are kept and processed, 384 of 600.  There are no face photographs
here, so the REAL YuNet runs on every detected frame for its cost and its rows are thrown away: two scripted faces drive the
tracks, the same rows for every leg.  The faces sit near the frame's origin because the loop hands STrack a tlbr box where it
takes tlwh (TEST2.py:535): a track's box is (x, y, 2x + w, 2y + h), and YuNet's five points - the only landmarks without FaceMesh -
are used only where that box and the detection overlap with IoU >= 0.4.
  runner1   VideoRunner(detect_batch=1): a chunk is one frame - per frame one detect and read-back, one quality launch and read-back
  runner16  VideoRunner(detect_batch=16): per 16 frames one detect, one read-back, one quality launch per 64 crops
  realtime  RealtimeCall.step over the kept frames, in order (its own defaults: stride 52, a ring of 128 frames, every frame
            detected; the self-view rectangle moved out of the faces' way)
Per size and leg: frames/s = frames processed / host-inclusive wall clock of the whole video (a leg ends in a score read-back, a
device synchronise), the runner's latency_ms_clip_mean and its launches and waits.  Every leg is warmed up by one whole run; the
legs then alternate `--reps` times; `spread` is (max - min) / min of a leg's frames/s over its repetitions, against which a
difference between legs is to be read.
`--tracker host,device`: the legs are runner1 and runner16 in each tracker mode (``VideoRunner(tracker=...)``: the host stage of a
chunk on the host, or as one launch - DESIGN 28), alternating in one session, without the realtime leg; per leg also the launches
and waits per chunk, and per size the device time of one ``af_runner_track_chunk`` launch over a 16-frame and a 1-frame chunk of
the scripted rows (events around 200 launches, after 20 to warm up).  Every phase runs under a time limit of its own.  Prints one JSON line and writes it to
`--json`.  A run without a GPU fails."""
import argparse
import json
import os
import platform
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import numpy as np  # noqa: E402
import torch  # noqa: E402

from bench_live import phase  # noqa: E402
from bench_realtime import MODEL  # noqa: E402

SIZES = {720: (720, 1280), 1080: (1080, 1920)}
STD5 = np.array([[0.3, 0.35], [0.7, 0.35], [0.5, 0.55], [0.35, 0.75], [0.65, 0.75]])


def scripted_rows(n_frames, h, seed):
    """per frame the (2, 15) float32 YuNet rows of two faces near the origin, sized by the frame height"""
    rng = np.random.default_rng(seed)
    out = []
    for _ in range(n_frames):
        rows = []
        for x, y, w, hh, score in ((0.04, 0.03, 0.40, 0.45, 0.95), (0.20, 0.12, 0.50, 0.55, 0.93)):
            x, y, w, hh = (np.array([x, y, w, hh]) * h + rng.uniform(-0.3, 0.3, 4)).tolist()
            rows.append(np.concatenate([[x, y, w, hh], [score + rng.uniform(-0.004, 0.004)], (STD5 * [w, hh] + [x, y]).ravel()]))
        out.append(np.asarray(rows, dtype=np.float32))
    return out


class ScriptedYuNet:
    """the real detector for its cost, scripted rows for its answer: the b-th frame it is shown gets ``rows[b]``"""

    def __init__(self, yunet, rows):
        self.yunet, self.rows, self.at, self.calls = yunet, rows, 0, 0

    def detect(self, frames_u8):
        self.yunet.detect(frames_u8)
        b, dev = frames_u8.shape[0], frames_u8.device
        mine = self.rows[self.at:self.at + b]
        self.at += b
        self.calls += 1
        rows = torch.zeros(b, 16, 15, dtype=torch.float32)
        for k, r in enumerate(mine):
            rows[k, :len(r)] = torch.from_numpy(r)
        counts = torch.tensor([len(r) for r in mine], dtype=torch.int32)
        return rows.to(dev, non_blocking=True), counts.to(dev, non_blocking=True)


def track_launch_ms(runner, shape, rows, n_frames, launches=200, warm=20):
    """the device time of one ``af_runner_track_chunk`` over `n_frames` frames of the scripted rows: events around `launches`
    launches that walk the video's frames in order (every frame processed, two tracked faces), after `warm` of them"""
    import ctypes as C
    from types import SimpleNamespace
    from af_mi355x import _lib, runner_device as RD
    plan = RD.ChunkPlan(SimpleNamespace(**runner.DEFAULTS), shape, runner.DEFAULTS["detect_every"], 1 << 30, 30.0)
    state = torch.from_numpy(plan.reset()).cuda()
    record = torch.zeros(RD.record_bytes(n_frames), dtype=torch.uint8, device="cuda")
    chunks = []
    for lo in range(0, (launches + warm) * n_frames, n_frames):
        part = [rows[(lo + j) % len(rows)] for j in range(n_frames)]
        laid = torch.zeros(n_frames, 16, 15, dtype=torch.float32)
        for j, r in enumerate(part):
            laid[j, :len(r)] = torch.from_numpy(r)
        chunks.append((laid.cuda(), torch.tensor([len(r) for r in part], dtype=torch.int32).cuda(), list(range(lo, lo + n_frames))))
    stream = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    begin, end = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    calls = [plan.chunk(state.data_ptr(), laid.data_ptr(), counts.data_ptr(), record.data_ptr(), laid.numel(), 16, 15, 0, ids)
             for laid, counts, ids in chunks]
    for i, c in enumerate(calls):
        if i == warm:
            begin.record()
        _lib.check(_lib.lib.af_runner_track_chunk(C.byref(c), stream), "af_runner_track_chunk")
    end.record()
    torch.cuda.synchronize()
    head = RD.parse_record(record.cpu().numpy(), n_frames)["head"]
    assert not int(head["overflow"]) and int(head["frames_seen"]) == (launches + warm) * n_frames
    return begin.elapsed_time(end) / launches


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", type=int, default=600)
    ap.add_argument("--sizes", default="720,1080")
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--dtype", default="f16")
    ap.add_argument("--phase-seconds", type=int, default=240)
    ap.add_argument("--tracker", default="host", help="host (the legs above), or host,device: runner1 / runner16 in both tracker modes")
    ap.add_argument("--json", default=None)
    args = ap.parse_args()
    trackers = args.tracker.split(",")
    assert trackers in (["host"], ["host", "device"]), "--tracker host | host,device"
    if args.json is None:
        args.json = os.path.join(ROOT, "profiles", "runner_bench.json" if trackers == ["host"] else "runner_tracker_bench.json")
    assert torch.cuda.is_available(), "bench_runner needs a GPU"
    from af_mi355x import live, runner, synth
    from af_mi355x.classifier import Classifier
    from af_mi355x.detector import YuNet

    with phase("network", args.phase_seconds):
        clf = Classifier(precision=args.dtype)
        clf.network.load_state_dict(synth.synthetic_state_dict(seed=0))
        net = clf.cuda().eval().network
    props = torch.cuda.get_device_properties(0)
    out = {"tool": "bench_runner", "device": props.name, "arch": props.gcnArchName, "host": platform.node(), "frames": args.frames, "fps": 30.0,
           "reps": args.reps, "dtype": args.dtype, "clip_size": 32, "size": 224,
           "detections": "scripted: the real YuNet runs on every detected frame for its cost, its rows are discarded (no face photographs)",
           "frames_per_s": "frames processed / host-inclusive wall clock of the whole video", "cases": {}}
    for size in (int(v) for v in args.sizes.split(",")):
        h, w = SIZES[size]
        rng = np.random.default_rng(size)
        distinct = [rng.integers(0, 256, (h, w, 3), dtype=np.uint8) for _ in range(32)]
        frames = [distinct[i % len(distinct)] for i in range(args.frames)]
        plan = runner.WindowPlan(args.frames, 32, runner.DEFAULTS["stride"], runner.DEFAULTS["max_frame"], 30.0)
        kept = [i for i in range(args.frames) if plan.keep(i)]
        rows = scripted_rows(len(kept), h, seed=size + 1)
        with phase("%dp: detector" % size, args.phase_seconds):
            yunet = YuNet(MODEL, inputSize=[w, h], confThreshold=0.7, nmsThreshold=0.3, topK=5000)
        runners = {}
        fps = {"runner1": [], "runner16": [], "realtime": []} if trackers == ["host"] else \
            {"runner%d_%s" % (b, t): [] for b in (1, 16) for t in trackers}
        last = {}
        for rep in range(args.reps + 1):                          # repetition 0 warms up: stores, graphs, workspaces
            for leg in fps:
                with phase("%dp: %s, repetition %d" % (size, leg, rep), args.phase_seconds):
                    det = ScriptedYuNet(yunet, rows)
                    torch.cuda.synchronize()
                    if leg == "realtime":
                        call = live.RealtimeCall(net, detector=det, exclude_rect=(0.95, 0.95, 1.0, 1.0), start_conf=0.6, track_thresh=0.6,
                                                 match_thresh=0.6)
                        t0 = time.perf_counter()
                        closes = sum(len(call.step(frames[i])) for i in kept)
                        torch.cuda.synchronize()
                        elapsed = time.perf_counter() - t0
                        assert closes, "no window closed"
                        rate, last[leg] = len(kept) / elapsed, {"windows_scored": closes, "detect_calls": det.calls}
                        del call
                    else:
                        if leg not in runners:                        # one runner per leg, as batch_eval.py keeps its own for every video
                            runners[leg] = runner.VideoRunner(net, detector=det, detect_batch=1 if leg.startswith("runner1_") or leg == "runner1" else 16,
                                                              tracker="device" if leg.endswith("_device") else "host")
                        r = runners[leg]
                        r.detector = det
                        t0 = time.perf_counter()
                        res = r.run(frames, fps=30.0)
                        torch.cuda.synchronize()
                        elapsed = time.perf_counter() - t0
                        clips = sum(len(v) for v in res["track_clip_scores"].values())
                        assert clips, "no clip was scored"
                        rate = res["frames_processed"] / elapsed
                        last[leg] = {"frames_processed": res["frames_processed"], "clips_scored": clips, "latency_ms_clip_mean": res["latency_ms_clip_mean"],
                                     "stats": res["stats"], "gpu_mem_alloc_peak_mb": res["gpu_mem_alloc_peak_mb"], "video_score": res["video_score"]}
                        with_frames = [c for c in r.chunks if c["frames"]]
                        last[leg]["per_chunk"] = {k: sum(c.get(k, 0) for c in with_frames) / len(with_frames)
                                                  for k in ("detect", "track", "quality", "wait", "warp", "replay")}
                    if rep:
                        fps[leg].append(rate)
                    torch.cuda.empty_cache()
        case = {}
        for leg, v in fps.items():
            case[leg] = dict(last[leg], frames_per_s=statistics.median(v), frames_per_s_runs=v, spread=(max(v) - min(v)) / min(v))
        if trackers == ["host"]:
            case["runner16_over_runner1"] = case["runner16"]["frames_per_s"] / case["runner1"]["frames_per_s"]
            case["runner16_over_realtime"] = case["runner16"]["frames_per_s"] / case["realtime"]["frames_per_s"]
        else:
            for b in (1, 16):
                case["runner%d_device_over_host" % b] = case["runner%d_device" % b]["frames_per_s"] / case["runner%d_host" % b]["frames_per_s"]
                assert case["runner%d_device" % b]["video_score"] == case["runner%d_host" % b]["video_score"], "the two modes disagree"
            with phase("%dp: the track launch alone" % size, args.phase_seconds):
                case["track_launch_device_ms"] = {str(n): track_launch_ms(runner, (h, w, 3), rows, n) for n in (16, 1)}
        case["frame_size"], case["frames_kept"] = [h, w], len(kept)
        out["cases"]["%dp" % size] = case
        print(size, json.dumps(case), file=sys.stderr, flush=True)
        runners.clear()
        del yunet
        torch.cuda.empty_cache()
    line = json.dumps(out)
    print(line)
    if args.json:
        os.makedirs(os.path.dirname(os.path.abspath(args.json)), exist_ok=True)
        with open(args.json, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
