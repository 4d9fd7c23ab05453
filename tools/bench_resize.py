"""Detection on downscaled frames on one MI355X: the resize launch alone, and the three pipelines with and without it.

    python tools/bench_resize.py [--launch-reps 100] [--reps 3] [--frames 200] [--calls 16] [--ticks 120] [--json profiles/resize_bench.json]

launch   af_resize_frames_u8 on 1 and 50 resident 1080p frames -> 960x540 (the 2 x 2 path) and -> 640x640 (bilinear), device events
         around `--launch-reps` back-to-back launches of one planned table after a warm-up: microseconds per launch, and the bytes
         of the whole source frames plus the destination per second.  `copy`: a device-to-device copy that reads and writes the same
         number of bytes, timed the same way in the same run - the ceiling such a launch can reach.
detect   RetinaFace detect_device at B = 50 on 1080p frames (seeded weights and frames: the work does not depend on what is found)
         against FrameResizer.resize to 960x540 + detect_device there; device events around `--detect-iters` calls, the two legs
         alternating `--reps` times.
video    VideoScorer.score on a synthetic 1080p video of `--frames` frames with one scripted face (tools/bench_video.py's workload:
         the detector does all its device work and hands back scripted rows), scale_detect False against True, host-inclusive wall
         clock, alternating `--reps` times after a warm-up.
server   CallServer ticks at N = `--calls` calls of 720p (tools/bench_server.py's workload), detect_size None against (640, 360),
         host-inclusive tick p50, alternating `--reps` times after a warm-up repetition.
Every comparison is against the full-size leg of the same run; `full_spread` is that leg's own run-to-run spread (max - min over
min of its repetitions), `scaled_spread` the scaled leg's, and `faster_than_spread` says whether the scaled leg's gain exceeds
both - a gain inside the spread is a tie.  Every phase runs under a time limit of its own.  Prints one JSON line and writes it to `--json`.  A run without a GPU fails."""
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
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import numpy as np  # noqa: E402
import torch  # noqa: E402

from bench_live import _pct, phase  # noqa: E402
from bench_realtime import EXCLUDE, H as CALL_H, MODEL, W as CALL_W  # noqa: E402
from bench_server import scripts_for  # noqa: E402
from bench_video import scripted_rows  # noqa: E402

H, W = 1080, 1920


def _timed(fn, reps):
    """microseconds per call of `fn`, device events around `reps` back-to-back calls after 5 warm-up calls"""
    for _ in range(5):
        fn()
    torch.cuda.synchronize()
    t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    t0.record()
    for _ in range(reps):
        fn()
    t1.record()
    torch.cuda.synchronize()
    return t0.elapsed_time(t1) * 1e3 / reps


def _compare(full, scaled):
    """two lists of repetitions (smaller is better) -> medians, the full leg's spread, the gain and whether it exceeds the spread"""
    mf, ms = statistics.median(full), statistics.median(scaled)
    spread = (max(full) - min(full)) / min(full) if len(full) > 1 else None
    scaled_spread = (max(scaled) - min(scaled)) / min(scaled) if len(scaled) > 1 else None
    gain = (mf - ms) / mf
    return {"full": {"median": mf, "all": full}, "scaled": {"median": ms, "all": scaled}, "full_spread": spread, "scaled_spread": scaled_spread,
            "gain": gain, "ratio": mf / ms, "faster_than_spread": None if spread is None else bool(gain > max(spread, scaled_spread))}


def bench_launch(reps):
    from af_mi355x import _lib, frames as F
    dev = torch.device("cuda", torch.cuda.current_device())
    stream = C.c_void_p(torch.cuda.current_stream(dev).cuda_stream)
    out = {}
    for n in (1, 50):
        src = torch.randint(0, 256, (n, H, W, 3), dtype=torch.uint8, device=dev)
        ref, _ = F._tensor_ref(src)
        for name, (dw, dh) in (("960x540_area2", (960, 540)), ("640x640_bilinear", (640, 640))):
            dst = torch.empty((n, dh, dw, 3), dtype=torch.uint8, device=dev)
            need = F.FrameResizer.table_bytes([(dw, dh)] * n)
            table = torch.zeros(need // 8 + 1, dtype=torch.int64)
            F.FrameResizer.plan([(0, k, dst.data_ptr() + k * dh * dw * 3, dw * 3, dw, dh) for k in range(n)], [ref], table.data_ptr(), need)
            table_dev = table.to(dev)
            us = _timed(lambda: _lib.check(_lib.lib.af_resize_frames_u8(C.c_void_p(table_dev.data_ptr()), n, stream), "resize_frames_u8"), reps)
            moved = src.numel() + dst.numel()
            a, b = (torch.empty(moved // 2, dtype=torch.uint8, device=dev) for _ in range(2))
            copy_us = _timed(lambda: b.copy_(a), reps)
            out["n%d_%s" % (n, name)] = {"us_per_launch": us, "bytes_moved": moved, "bytes_per_s": moved / (us * 1e-6), "copy_us": copy_us,
                                         "copy_bytes_per_s": moved / (copy_us * 1e-6), "launch_over_copy": us / copy_us, "launches_timed": reps}
            del dst, a, b
        del src
    return out


def bench_detect(reps, iters):
    from af_mi355x import frames as F, retinaface as rf, synth
    dev = torch.device("cuda", torch.cuda.current_device())
    det = rf.FaceDetector.from_state_dict(synth.retinaface_state_dict(1, "sparse"), gpu_id=dev.index)
    frames = torch.randint(0, 256, (50, H, W, 3), dtype=torch.uint8, device=dev)
    rs = F.FrameResizer(dev)
    dw, dh = rf.scale_detect_size(H, W)
    full = lambda: det.detect_device(frames, max_count=10, min_score=0.5)                                   # noqa: E731
    scaled = lambda: det.detect_device(rs.resize(frames, (dw, dh)), min_score=0.5)                          # noqa: E731
    resize = lambda: rs.resize(frames, (dw, dh))                                                            # noqa: E731
    runs = {"full": [], "scaled": [], "resize": []}
    for _ in range(reps):
        for name, fn in (("full", full), ("scaled", scaled), ("resize", resize)):
            runs[name].append(_timed(fn, iters) * 1e-3)
    out = _compare(runs["full"], runs["scaled"])
    out.update(unit="ms per call of 50 frames, device events", detect_size=[dw, dh], resize_alone={"median": statistics.median(runs["resize"]), "all": runs["resize"]},
               resize_alone_note="FrameResizer.resize: the plan on the host, the table's copy and the launch")
    return out


def bench_video(n_frames, reps, dtype):
    from af_mi355x import evaluator, retinaface as rf, synth
    from af_mi355x.classifier import Classifier
    clf = Classifier(precision=dtype)
    clf.network.load_state_dict(synth.synthetic_state_dict(seed=0))
    net = clf.cuda().eval().network
    scale = rf.scale_detect_scale(H, W)

    class ScriptedDetector(rf.FaceDetector):
        """the detector's whole device work, then the scripted rows of the frames it was given, in the coordinates of those frames"""
        script, cursor = None, 0

        def detect_device(self, frames_u8, keep_top_k=rf.KEEP_TOP_K, max_count=0, min_score=0.0, raw=False, timings=None):
            rows, counts = super().detect_device(frames_u8, keep_top_k, max_count, min_score)
            b, lo = frames_u8.shape[0], self.cursor
            self.cursor += b
            mine = self.script[0][lo:lo + b, :min(rows.shape[1], 10)]
            out_rows = torch.zeros_like(rows)
            out_rows[:, :mine.shape[1]] = mine if frames_u8.shape[1] == H else torch.cat([mine[..., :4] / scale, mine[..., 4:5], mine[..., 5:] / scale], -1)
            return out_rows, self.script[1][lo:lo + b].clone()

    det = ScriptedDetector.from_state_dict(synth.retinaface_state_dict(1, "sparse"), gpu_id=0)
    rng = np.random.default_rng(H)
    distinct = [np.ascontiguousarray(rng.integers(0, 256, (H, W, 3), dtype=np.uint8)) for _ in range(8)]
    frames = [distinct[i % 8][..., ::-1] for i in range(n_frames)]
    rows, counts = scripted_rows(n_frames, H, W, 1, seed=1000 + H)
    det.script = (torch.from_numpy(rows).cuda(), torch.from_numpy(counts).cuda())
    scorers = {"full": evaluator.VideoScorer(det, net), "scaled": evaluator.VideoScorer(det, net, scale_detect=True)}
    windows = {}
    runs = {"full": [], "scaled": []}
    for rep in range(reps + 1):                                    # repetition 0 warms up
        for name, vs in scorers.items():
            det.cursor = 0
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            res = vs.score(frames)
            torch.cuda.synchronize()
            if rep:
                runs[name].append(time.perf_counter() - t0)
            windows[name] = len(res["preds"])
    assert windows["full"] == windows["scaled"] == n_frames - 31, windows
    out = _compare(runs["full"], runs["scaled"])
    out.update(unit="seconds per video, host-inclusive", frames=n_frames, windows=windows["full"], dtype=dtype,
               frames_per_s={k: n_frames / out[k]["median"] for k in ("full", "scaled")})
    return out


class _ScriptedYuNet:
    """tools/bench_server.py's ScriptedYuNet for a server whose calls may detect on resized views: the real detector for its cost
    on whatever it is shown, and the scripted rows divided by `back` so that the server's scaling gives the script"""

    def __init__(self, yunet, scripts, back):
        self.yunet, self.scripts, self.turn, self.back = yunet, scripts, 0, back

    def detect_views(self, views):
        self.yunet.detect_views(views)
        dev = views[0].device
        rows = torch.zeros(len(views), 16, 15, dtype=torch.float32, device=dev)
        counts = []
        for b, script in enumerate(self.scripts[:len(views)]):
            mine = script[self.turn % len(script)]
            if len(mine):
                rows[b, :len(mine)] = torch.from_numpy((mine / self.back).astype(np.float32)).to(dev, non_blocking=True)
            counts.append(len(mine))
        self.turn += 1
        return rows, torch.tensor(counts, dtype=torch.int32).to(dev, non_blocking=True)


def bench_server(n, ticks, reps, stride, dtype, seconds):
    from af_mi355x import live, synth
    from af_mi355x.classifier import Classifier
    from af_mi355x.detector import YuNet
    clf = Classifier(precision=dtype)
    clf.network.load_state_dict(synth.synthetic_state_dict(seed=0))
    net = clf.cuda().eval().network
    yunet = YuNet(MODEL, inputSize=[CALL_W, CALL_H], confThreshold=0.8, nmsThreshold=0.3, topK=5000)
    rng = np.random.default_rng(720)
    frames = [rng.integers(0, 256, (CALL_H, CALL_W, 3), dtype=np.uint8) for _ in range(8)]
    scripts = scripts_for(n, ticks, stride)
    size = (640, 360)
    legs = {"full": (None, np.ones(15)), "scaled": (size, np.array([CALL_W / size[0], CALL_H / size[1]] * 7 + [1.0]))}
    runs, p50s, per_tick = {k: [] for k in legs}, {k: [] for k in legs}, {}
    for rep in range(reps + 1):
        for leg, (detect_size, back) in legs.items():
            with phase("server: %s, repetition %d" % (leg, rep), seconds):
                server = live.CallServer(net, detector=_ScriptedYuNet(yunet, scripts, back), stride=stride, exclude_rect=EXCLUDE, detect_size=detect_size)
                cids = [server.open() for _ in range(n)]
                times, counts = [], {}
                torch.cuda.synchronize()
                for s in range(ticks):
                    batch = {cid: frames[(s + i) % len(frames)] for i, cid in enumerate(cids)}
                    t0 = time.perf_counter()
                    server.step(batch)
                    times.append(time.perf_counter() - t0)
                    for k, v in server.stats.last.items():
                        counts[k] = counts.get(k, 0) + v
                torch.cuda.synchronize()
                assert server.stats.total["replay"] > 0, "no window closed"
                per_tick[leg] = {k: v / ticks for k, v in counts.items()}
                for cid in cids:
                    server.close(cid)
                del server
                torch.cuda.empty_cache()
                if rep:
                    runs[leg].extend(times)
                    p50s[leg].append(_pct(times, 0.5))
    out = _compare(p50s["full"], p50s["scaled"])
    out.update(unit="tick p50 in seconds per repetition, host-inclusive, all calls", calls=n, ticks=ticks, frame_size=[CALL_H, CALL_W],
               detect_size=list(size), per_tick=per_tick, p95={k: _pct(runs[k], 0.95) for k in runs})
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--launch-reps", type=int, default=100)
    ap.add_argument("--detect-iters", type=int, default=10)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--frames", type=int, default=200)
    ap.add_argument("--calls", type=int, default=16)
    ap.add_argument("--ticks", type=int, default=120)
    ap.add_argument("--stride", type=int, default=8)
    ap.add_argument("--dtype", default="f16")
    ap.add_argument("--phase-seconds", type=int, default=240)
    ap.add_argument("--json", default=os.path.join(ROOT, "profiles", "resize_bench.json"))
    args = ap.parse_args()
    assert torch.cuda.is_available(), "bench_resize needs a GPU"
    import af_mi355x  # noqa: F401
    props = torch.cuda.get_device_properties(0)
    out = {"tool": "bench_resize", "device": props.name, "arch": props.gcnArchName, "host": platform.node(), "frame_size": [H, W], "reps": args.reps}
    with phase("launch", args.phase_seconds):
        out["launch"] = bench_launch(args.launch_reps)
        out["launch_note"] = ("bytes_moved counts the whole source frames and the destination; the launches repeat on the same buffers, so one "
                              "frame (7.8 MB) may be served by the Infinity Cache, 50 frames (311 MB of source) not")
    print("launch", json.dumps(out["launch"]), file=sys.stderr, flush=True)
    with phase("detect", args.phase_seconds):
        out["detect"] = bench_detect(args.reps, args.detect_iters)
    print("detect", json.dumps(out["detect"]), file=sys.stderr, flush=True)
    with phase("video", args.phase_seconds):
        out["video"] = bench_video(args.frames, args.reps, args.dtype)
    print("video", json.dumps(out["video"]), file=sys.stderr, flush=True)
    out["server"] = bench_server(args.calls, args.ticks, args.reps, args.stride, args.dtype, args.phase_seconds)
    print("server", json.dumps(out["server"]), file=sys.stderr, flush=True)
    line = json.dumps(out)
    print(line)
    if args.json:
        os.makedirs(os.path.dirname(os.path.abspath(args.json)), exist_ok=True)
        with open(args.json, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
