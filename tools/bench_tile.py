"""TilePicker on one MI355X: the device time of its two launch sequences and the host-inclusive cost of a pick.

    python tools/bench_tile.py [--reps 50] [--windows 5] [--picks 200] [--ticks 60] [--json profiles/tile_bench.json]

device   af_tile_candidates_u8 and af_tile_motion_u8 on a device-resident drawn call grid (four tiles, one of them flat, on a dark
         background) of 960 x 540 and 1280 x 720, timed with device events around `--reps` back-to-back sequences after a warm-up,
         `--windows` such windows, no read-back inside the window.  The motion pair differs by a block that moves.
pick     TilePicker.pick, host-inclusive (wall clock around the call, which ends in its own read-back), on device-resident frames:
         `tile` - the grid, one sequence and one read-back per pick; `motion` - a flat moving block, both sequences and two read-backs
realtime RealtimeCall.step on a 2560 x 1440 bgra capture with max_w = 960 (tools/bench_capture.py's max_w960 leg, same script),
         host-inclusive: the live step a pick would sit in front of
Nothing is gated on these figures, and there is no cv2 leg to compare against: OpenCV is not installed where this runs.
Every phase runs under a time limit of its own.  Prints one JSON line and writes it to `--json`.  A run without a GPU fails."""
import argparse
import ctypes as C
import json
import os
import platform
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import numpy as np  # noqa: E402
import torch  # noqa: E402

from bench_capture import _timed, _windows, play, scripts_for, CAP_H, CAP_W, STORED  # noqa: E402
from bench_live import _pct, _stats, phase  # noqa: E402
from bench_realtime import EXCLUDE, MODEL  # noqa: E402
from bench_server import ScriptedYuNet  # noqa: E402

SIZES = [(960, 540), (1280, 720)]


def grid(w, h):
    """a drawn call grid, BGR: two ramp-textured tiles, a flat one and a narrow one on a background of 30"""
    f = np.full((h, w, 3), 30, np.uint8)
    u = lambda v, n: int(round(v * n))                            # noqa: E731
    for x, y, tw, th, kind in ((0.03, 0.05, 0.47, 0.5, "ramp"), (0.56, 0.08, 0.38, 0.42, "ramp"), (0.03, 0.6, 0.4, 0.37, "flat"),
                               (0.62, 0.56, 0.15, 0.36, "flat")):
        x0, y0, x1, y1 = u(x, w), u(y, h), u(x + tw, w), u(y + th, h)
        if kind == "ramp":
            ramp = np.linspace(60, 220, x1 - x0)[None, :] + 12 * np.sin(np.arange(y1 - y0) / 9.0)[:, None]
            f[y0:y1, x0:x1] = np.clip(ramp, 0, 255).astype(np.uint8)[..., None]
        else:
            f[y0:y1, x0:x1] = 120
    return f


def block(w, h, x):
    f = np.full((h, w, 3), 30, np.uint8)
    f[h // 4:h // 4 + h // 3, x:x + w // 3] = 90
    return f


def bench_size(w, h, reps, windows, picks):
    from af_mi355x import _lib, TilePicker
    dev = torch.device("cuda", torch.cuda.current_device())
    stream = C.c_void_p(torch.cuda.current_stream(dev).cuda_stream)
    picker = TilePicker(dev)
    tile_frame = torch.from_numpy(grid(w, h)).to(dev)
    moving = [torch.from_numpy(block(w, h, x)).to(dev) for x in (w // 8, w // 4)]
    found = picker.tiles(tile_frame)
    assert found is not None, "the drawn grid has a tile"
    ws = picker._ws
    params = _lib.TileParams(200, 120, 1.2, 2.2, 0.10 * w * h)
    greys = torch.empty((2, h * w), dtype=torch.uint8, device=dev)

    def desc(t):
        return _lib.TileSource(t.data_ptr(), 3 * w, h, w, 1, 0)

    d0, d1, d2 = desc(tile_frame), desc(moving[0]), desc(moving[1])

    def candidates():
        _lib.check(_lib.lib.af_tile_candidates_u8(C.byref(d0), C.byref(params), C.c_void_p(ws.data_ptr()), ws.numel(), None, stream), "candidates")

    turn = [0]

    def motion():
        k = turn[0] = 1 - turn[0]
        _lib.check(_lib.lib.af_tile_motion_u8(C.byref(d2 if k else d1), C.c_void_p(greys[1 - k].data_ptr()), C.c_void_p(greys[k].data_ptr()),
                                              0.01 * w * h, C.c_void_p(ws.data_ptr()), ws.numel(), None, stream), "motion")

    _lib.check(_lib.lib.af_tile_motion_u8(C.byref(d1), None, C.c_void_p(greys[0].data_ptr()), 0.01 * w * h, C.c_void_p(ws.data_ptr()), ws.numel(),
                                          None, stream), "motion")
    out = {"tile_found": list(found), "workspace_bytes": ws.numel(), "sequences_per_window": reps,
           "candidates_device": _windows(_timed(candidates, reps, windows)), "motion_device": _windows(_timed(motion, reps, windows))}

    def timed_picks(frames):
        picker.reset()
        for k in range(10):
            picker.pick(frames[k % len(frames)])
        torch.cuda.synchronize()
        times, boxes = [], set()
        for k in range(picks):
            t0 = time.perf_counter()
            boxes.add(picker.pick(frames[k % len(frames)]))
            times.append(time.perf_counter() - t0)
        return _stats(times), len(boxes)

    out["pick_tile_s"], _ = timed_picks([tile_frame])
    out["pick_motion_s"], n_boxes = timed_picks(moving)
    assert n_boxes >= 1 and picker.prev_tile is not None, "the moving block is found"
    out["readbacks_per_pick"] = {"tile": 1, "motion": 2}
    return out


def bench_realtime(ticks, phase_seconds, dtype="f16", stride=8, ring_frames=64):
    from af_mi355x import live, synth
    from af_mi355x.classifier import Classifier
    from af_mi355x.detector import YuNet
    with phase("network", phase_seconds):
        clf = Classifier(precision=dtype)
        clf.network.load_state_dict(synth.synthetic_state_dict(seed=0))
        net = clf.cuda().eval().network
        yunet = YuNet(MODEL, inputSize=[CAP_W, CAP_H], confThreshold=0.8, nmsThreshold=0.3, topK=5000)
    rng = np.random.default_rng(2560)
    bitmaps = [rng.integers(0, 256, (CAP_H, CAP_W, 4), dtype=np.uint8) for _ in range(4)]
    p50s, all_times = [], []
    for rep in range(3):                                          # repetition 0 warms up
        with phase("realtime, repetition %d" % rep, phase_seconds):
            script = scripts_for(1, ticks, stride, STORED["max_w960"])
            call = live.RealtimeCall(net, detector=ScriptedYuNet(yunet, script), stride=stride, exclude_rect=EXCLUDE, ring_frames=ring_frames,
                                     drop_after=ring_frames - 32)
            times = play(call.step, None, "max_w960", bitmaps, ticks)
            del call
            torch.cuda.synchronize()
            if rep:
                p50s.append(_pct(times, 0.5))
                all_times.extend(times)
    return {"leg": "bench_capture max_w960: 2560 x 1440 bgra, stored 960 x 540", "step_s": _stats(all_times), "p50_per_repetition": p50s,
            "spread": (max(p50s) - min(p50s)) / min(p50s)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=50)
    ap.add_argument("--windows", type=int, default=5)
    ap.add_argument("--picks", type=int, default=200)
    ap.add_argument("--ticks", type=int, default=60)
    ap.add_argument("--phase-seconds", type=int, default=120)
    ap.add_argument("--json", default=os.path.join(ROOT, "profiles", "tile_bench.json"))
    args = ap.parse_args()
    assert torch.cuda.is_available(), "bench_tile needs a GPU"
    props = torch.cuda.get_device_properties(0)
    out = {"tool": "bench_tile", "device": props.name, "arch": props.gcnArchName, "host": platform.node(),
           "cv2_leg": "none: OpenCV is not installed where this runs", "gated": False}
    for w, h in SIZES:
        with phase("%dx%d" % (w, h), args.phase_seconds):
            out["%dx%d" % (w, h)] = bench_size(w, h, args.reps, args.windows, args.picks)
        print(w, h, json.dumps(out["%dx%d" % (w, h)]), file=sys.stderr, flush=True)
    out["realtime_step"] = bench_realtime(args.ticks, args.phase_seconds)
    line = json.dumps(out)
    print(line)
    if args.json:
        os.makedirs(os.path.dirname(os.path.abspath(args.json)), exist_ok=True)
        with open(args.json, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
