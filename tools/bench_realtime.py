"""The whole live step on one MI355X: RealtimeCall.step(frame) against the composition the parent commit offers, in one process.

    python tools/bench_realtime.py [--frames 240] [--faces 1,2,4] [--stride 8] [--reps 2] [--dtype f16] [--json profiles/realtime_bench.json]

Workload: `--frames` captured 720p frames at 30 fps pace-free (eight distinct seeded BGR frames in turn), 1, 2 and 4 faces in a
gallery grid; clip 32, crop 224, `--stride` 8.  There are no face photographs here, so the REAL YuNet runs on every frame for its
cost and its rows are thrown away: the tracks are driven by scripted detections (the same rows for both paths).
  new     RealtimeCall.step(frame): one upload into the ring, YuNet on the resident frame, counts + rows in one pinned read-back,
          ByteTracker, one af_face_quality_u8 launch over the faces' rectangles and its read-back, LiveCall.advance
  parent  YuNet.infer(frame) (its own upload and read-back), the same ByteTracker and host loop, a host numpy quality gate on
          crops cut from the frame reversed on the host (2 x 2 box means where the reference calls cv2.resize INTER_AREA - a lower
          bound of that cost), then LiveCall.step(frame, faces), which uploads the frame a second time
Host-inclusive wall clock per step, p50 / p95, over the steps without a window close and over the closing steps; uploaded bytes
per step for both.  Both paths are warmed up by one whole script and alternate `--reps` times.  Every phase runs under a time limit
of its own.  Prints one JSON line and writes it to `--json`.  A run without a GPU fails."""
import argparse
import json
import os
import platform
import sys
import time
import types

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import numpy as np  # noqa: E402
import torch  # noqa: E402

from bench_live import _stats, phase  # noqa: E402

H, W, CLIP, SIZE = 720, 1280, 32, 224
EXCLUDE = (0.9, 0.9, 1.0, 1.0)          # the gallery's bottom-right face stays outside the self-view rectangle
MODEL = os.path.join(ROOT, "tests", "golden", "yunet_2023mar.onnx")


def scripted_rows(n_frames, faces, seed):
    """per frame the (faces, 15) float32 YuNet rows of `faces` faces in a gallery grid, each jittering in its tile"""
    rng = np.random.default_rng(seed)
    grid = int(np.ceil(np.sqrt(faces)))
    tile_w, tile_h = W / grid, H / grid
    std = np.array([[0.3, 0.35], [0.7, 0.35], [0.5, 0.55], [0.35, 0.75], [0.65, 0.75]])
    centres = [np.array([(k % grid + 0.5) * tile_w, (k // grid + 0.5) * tile_h]) for k in range(faces)]
    out = []
    for _ in range(n_frames):
        rows = []
        for k in range(faces):
            centres[k] = centres[k] + rng.normal(0, 0.4, 2)
            side = 0.4 * tile_h + rng.normal(0, 0.3)
            x, y = centres[k] - side / 2
            rows.append(np.concatenate([[x, y, side, side, 0.95 + rng.uniform(-0.004, 0.004)], (std * side + [x, y]).ravel()]))
        out.append(np.asarray(rows, dtype=np.float32))
    return out


class ScriptedYuNet:
    """the real detector for its cost, scripted rows for its answer"""

    def __init__(self, yunet, script):
        self.yunet, self.script, self.turn = yunet, script, 0

    def detect(self, frames_u8):
        self.yunet.detect(frames_u8)
        mine = self.script[self.turn % len(self.script)]
        self.turn += 1
        rows = torch.zeros(1, 16, 15, dtype=torch.float32, device=frames_u8.device)
        rows[0, :len(mine)] = torch.from_numpy(mine).to(frames_u8.device, non_blocking=True)
        return rows, torch.full((1,), len(mine), dtype=torch.int32, device=frames_u8.device)


def host_gate(crop_rgb):
    """(min_side, lap) of a host crop in numpy: 2 x 2 box means, the 15-bit grey, the reflected 4-neighbour Laplacian, its variance"""
    h, w = crop_rgb.shape[:2]
    dh, dw = max(1, h // 2), max(1, w // 2)
    c = crop_rgb[:2 * dh, :2 * dw].astype(np.int32)
    small = (c[0::2, 0::2] + c[0::2, 1::2] + c[1::2, 0::2] + c[1::2, 1::2] + 2) >> 2
    g = ((small[..., 0] * 9798 + small[..., 1] * 19235 + small[..., 2] * 3735 + 16384) >> 15).astype(np.float64)
    p = np.pad(g, 1, mode="reflect") if min(g.shape) > 1 else np.pad(g, 1, mode="edge")
    lap = p[:-2, 1:-1] + p[2:, 1:-1] + p[1:-1, :-2] + p[1:-1, 2:] - 4 * g
    return float(min(h, w)), float(lap.var())


class ParentCall:
    """what a caller of the parent commit composes: YuNet.infer, a tracker, a host gate, LiveCall.step"""

    def __init__(self, net, yunet, script, stride):
        from af_mi355x import live
        from af_mi355x.tracker import ByteTracker
        self.yunet, self.script, self.turn = yunet, script, 0
        self.call = live.LiveCall(net, clip_size=CLIP, size=SIZE, stride=stride)
        self.tracker = ByteTracker(types.SimpleNamespace(track_thresh=0.8, track_buffer=90, match_thresh=0.8, mot20=False), frame_rate=30.0)
        self.state, self.live, self.extra_bytes = live.CallState(), live, 0

    @property
    def uploaded_bytes(self):
        return self.call.uploaded_bytes + self.extra_bytes

    def step(self, frame):
        from af_mi355x.tracker import STrack
        self.yunet.infer(frame)
        self.extra_bytes += frame.nbytes
        dets = self.script[self.turn % len(self.script)]
        self.turn += 1
        online = self.tracker.update([STrack(d[:4], score=float(d[4])) for d in dets if d[4] >= 0.76 and max(d[2], d[3]) >= 80], (H, W), (H, W))
        frgb = frame[..., ::-1]
        quality = lambda rects: [host_gate(frgb[y0:y1, x0:x1]) for x0, y0, x1, y1 in rects]
        faces, alive, _, _ = self.live.track_faces(self.state, self.call.frame_idx + 1, (H, W), dets, online, quality, self.live.quality_weight,
                                                     exclude_rect=EXCLUDE)
        return self.call.step(frame, faces, alive=alive)


def play(call, frames, n):
    quiet, closing = [], []
    torch.cuda.synchronize()
    for s in range(n):
        t0 = time.perf_counter()
        res = call.step(frames[s % len(frames)])
        (closing if res else quiet).append(time.perf_counter() - t0)
    torch.cuda.synchronize()
    return quiet, closing


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", type=int, default=240)
    ap.add_argument("--faces", default="1,2,4")
    ap.add_argument("--stride", type=int, default=8)
    ap.add_argument("--reps", type=int, default=2)
    ap.add_argument("--dtype", default="f16")
    ap.add_argument("--phase-seconds", type=int, default=240)
    ap.add_argument("--json", default=os.path.join(ROOT, "profiles", "realtime_bench.json"))
    args = ap.parse_args()
    assert torch.cuda.is_available(), "bench_realtime needs a GPU"
    from af_mi355x import live, synth
    from af_mi355x.classifier import Classifier
    from af_mi355x.detector import YuNet

    with phase("network", args.phase_seconds):
        clf = Classifier(precision=args.dtype)
        clf.network.load_state_dict(synth.synthetic_state_dict(seed=0))
        net = clf.cuda().eval().network
        yunet = YuNet(MODEL, inputSize=[W, H], confThreshold=0.8, nmsThreshold=0.3, topK=5000)
    rng = np.random.default_rng(720)
    frames = [rng.integers(0, 256, (H, W, 3), dtype=np.uint8) for _ in range(8)]
    props = torch.cuda.get_device_properties(0)
    out = {"tool": "bench_realtime", "device": props.name, "arch": props.gcnArchName, "host": platform.node(), "frames": args.frames,
           "frame_size": [H, W], "clip_size": CLIP, "size": SIZE, "stride": args.stride, "reps": args.reps, "dtype": args.dtype,
           "detections": "scripted: the real YuNet runs on every frame for its cost, its rows are discarded (no face photographs)",
           "parent_gate": "numpy, 2 x 2 box means in place of cv2.resize INTER_AREA", "cases": {}}
    for faces in (int(v) for v in args.faces.split(",")):
        script = scripted_rows(args.frames, faces, seed=2000 + faces)
        runs = {"new": ([], []), "parent": ([], [])}
        sent = {}
        for rep in range(args.reps + 1):                          # repetition 0 warms up: rings, graphs, workspaces
            for name in ("new", "parent"):
                with phase("faces %d: %s, repetition %d" % (faces, name, rep), args.phase_seconds):
                    if name == "new":
                        call = live.RealtimeCall(net, detector=ScriptedYuNet(yunet, script), stride=args.stride, exclude_rect=EXCLUDE)
                    else:
                        call = ParentCall(net, yunet, script, args.stride)
                    quiet, closing = play(call, frames, args.frames)
                    assert closing, "no window closed"
                    sent[name] = call.uploaded_bytes / args.frames
                    if rep:
                        runs[name][0].extend(quiet)
                        runs[name][1].extend(closing)
                    del call
        case = {name: {"step_without_close_s": _stats(runs[name][0]), "step_with_close_s": _stats(runs[name][1]),
                       "uploaded_bytes_per_step": sent[name]} for name in runs}
        out["cases"]["faces%d" % faces] = case
        print(faces, json.dumps(case), file=sys.stderr, flush=True)
    line = json.dumps(out)
    print(line)
    if args.json:
        os.makedirs(os.path.dirname(os.path.abspath(args.json)), exist_ok=True)
        with open(args.json, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
