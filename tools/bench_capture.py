"""Captured BGRA bitmaps into the frame stores on one MI355X: the capture launch alone, RealtimeCall steps and CallServer ticks on a
2560 x 1440 capture handed over three ways.

    python tools/bench_capture.py [--calls 4,16] [--ticks 60] [--reps 2] [--stride 8] [--dtype f16] [--json profiles/capture_bench.json]

launch   af_capture_to_stores_u8 on 1 and 16 device-resident 2560 x 1440 BGRA frames into a B, G, R store of 960 x 540 (TABLE mode,
         capture_tile.py's max_w = 960) and of 1280 x 720 (AREA2), timed with device events around `--launch-reps` back-to-back
         launches after a warm-up, `--windows` such windows; next to it a device copy that reads and writes the same number of bytes
         as the launch must (source rectangle read + destination written), timed the same way.  The launches repeat on the same
         buffers: a working set under 256 MB may be served by the Infinity Cache and not by HBM.
realtime RealtimeCall.step, host-inclusive (wall clock around the step and a device synchronise), the real YuNet run for its cost with
         scripted rows for its answer, two faces, three legs on the same pictures, alternating in one process, `--reps` measured
         repetitions after a warm-up one:
           bgra_full  a bgra CapturedFrame at full size: 4 bytes per pixel staged and uploaded, alpha dropped on the device
           strip      np.ascontiguousarray(frame[..., :3]) inside the timed step, then the numpy path: the only route before
                      CapturedFrame, 3 bytes per pixel uploaded after a full-frame host pass
           max_w960   a bgra CapturedFrame with max_w = 960: the same upload as bgra_full, a 960 x 540 frame stored and detected on
server   CallServer ticks at N calls for the same three legs.
Every leg is reported with the run-to-run spread of its p50 over the repetitions; `against_strip` compares a leg's p50 with the
strip leg's and says "tie" when the difference lies inside the larger of the two spreads.  Nothing is gated on these figures.
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

from bench_live import _pct, _stats, phase  # noqa: E402
from bench_realtime import EXCLUDE, MODEL, scripted_rows  # noqa: E402
from bench_realtime import H as SCRIPT_H, W as SCRIPT_W  # noqa: E402
from bench_server import FACES, ScriptedYuNet  # noqa: E402

CAP_H, CAP_W = 1440, 2560
LEGS = ("bgra_full", "strip", "max_w960")
STORED = {"bgra_full": (CAP_H, CAP_W), "strip": (CAP_H, CAP_W), "max_w960": (540, 960)}


def _timed(fn, reps, windows):
    """microseconds per call of `fn` in each of `windows` windows of `reps` back-to-back calls, by device events"""
    for _ in range(5):
        fn()
    torch.cuda.synchronize()
    out = []
    for _ in range(windows):
        t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        t0.record()
        for _ in range(reps):
            fn()
        t1.record()
        torch.cuda.synchronize()
        out.append(t0.elapsed_time(t1) * 1e3 / reps)
    return out


def _windows(us):
    return {"us_p50": _pct(us, 0.5), "us_min": min(us), "us_max": max(us), "spread": (max(us) - min(us)) / min(us), "windows": len(us)}


def bench_launch(counts, targets, reps, windows):
    from af_mi355x import _lib, evaluator, frames as F
    dev = torch.device("cuda", torch.cuda.current_device())
    stream = C.c_void_p(torch.cuda.current_stream(dev).cuda_stream)
    out = {}
    for n in counts:
        bitmaps = torch.randint(0, 256, (n, CAP_H, CAP_W, 4), dtype=torch.uint8, device=dev)
        for dw, dh in targets:
            store = evaluator.FrameStore(dev, "bgr")
            store.open((dh, dw, 3), n)
            frames = [F.CapturedFrame(bitmaps[k], "bgra", size=(dw, dh)) for k in range(n)]
            ref = F.store_ref(store, "bgr")
            room = F.CaptureConverter.table_bytes(frames)
            host = torch.empty(room, dtype=torch.uint8, pin_memory=True)
            used = F.CaptureConverter.table(frames, [None] * n, [ref] * n, list(range(n)), host.data_ptr(), room)
            table = host[:used].to(dev)
            mode = _lib.CaptureItem.from_buffer_copy(bytes(host[C.sizeof(_lib.CaptureHeader):C.sizeof(_lib.CaptureHeader) + 72].numpy())).mode
            launch = lambda: _lib.check(_lib.lib.af_capture_to_stores_u8(C.c_void_p(table.data_ptr()), n, stream), "capture_to_stores_u8")  # noqa: E731
            moved = n * (CAP_H * CAP_W * 4 + dh * dw * 3)
            a = torch.empty(moved // 2, dtype=torch.uint8, device=dev)
            b = torch.empty_like(a)
            row = {"mode": ["copy", "area2", "box", "table"][mode], "bytes_read": n * CAP_H * CAP_W * 4, "bytes_written": n * dh * dw * 3,
                   "launch": _windows(_timed(launch, reps, windows)), "device_copy_of_the_same_bytes": _windows(_timed(lambda: b.copy_(a), reps, windows)),
                   "calls_per_window": reps}
            row["bytes_per_s"] = moved / (row["launch"]["us_p50"] * 1e-6)
            row["launch_over_copy"] = row["launch"]["us_p50"] / row["device_copy_of_the_same_bytes"]["us_p50"]
            out["n%d_to_%dx%d" % (n, dw, dh)] = row
            del store, frames, table, a, b
        del bitmaps
    return out


def scripts_for(n_calls, ticks, stride, stored):
    """bench_server's scripts - two faces in a gallery grid, a call's first faces `i % stride` ticks late - scaled to the stored frame"""
    sy, sx = stored[0] / SCRIPT_H, stored[1] / SCRIPT_W
    scale = np.array([sx, sy, sx, sy, 1.0] + [sx, sy] * 5, dtype=np.float32)
    out = []
    for i in range(n_calls):
        rows = [r * scale for r in scripted_rows(ticks, FACES, seed=3000 + i)]
        late = i % stride
        out.append([np.zeros((0, 15), np.float32)] * late + rows[:ticks - late])
    return out


def hand_over(leg, bitmap):
    from af_mi355x import frames as F
    if leg == "bgra_full":
        return F.CapturedFrame(bitmap, "bgra")
    if leg == "max_w960":
        return F.CapturedFrame(bitmap, "bgra", max_w=960)
    return np.ascontiguousarray(bitmap[..., :3])


def play(step, n_calls, leg, bitmaps, ticks):
    """`ticks` steps of `step({i: frame})` (or `step(frame)` for one RealtimeCall: n_calls None); the hand-over is inside the clock"""
    times = []
    torch.cuda.synchronize()
    for s in range(ticks):
        t0 = time.perf_counter()
        if n_calls is None:
            step(hand_over(leg, bitmaps[s % len(bitmaps)]))
        else:
            step({i: hand_over(leg, bitmaps[(s + i) % len(bitmaps)]) for i in range(n_calls)})
        torch.cuda.synchronize()
        times.append(time.perf_counter() - t0)
    return times


def summarise(runs, p50s, extra):
    case = {}
    for leg in LEGS:
        spread = (max(p50s[leg]) - min(p50s[leg])) / min(p50s[leg]) if len(p50s[leg]) > 1 else None
        case[leg] = dict(extra[leg], step_s=_stats(runs[leg]), p50_per_repetition=p50s[leg], spread=spread)
    base = case["strip"]
    for leg in LEGS:
        if leg == "strip":
            continue
        gain = (base["step_s"]["p50"] - case[leg]["step_s"]["p50"]) / base["step_s"]["p50"]
        spreads = [s for s in (base["spread"], case[leg]["spread"]) if s is not None]
        verdict = "unknown spread" if not spreads else "tie" if abs(gain) <= max(spreads) else "faster" if gain > 0 else "slower"
        case[leg]["against_strip"] = {"gain": gain, "verdict": verdict}
    return case


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--calls", default="4,16")
    ap.add_argument("--ticks", type=int, default=60)
    ap.add_argument("--stride", type=int, default=8)
    ap.add_argument("--reps", type=int, default=2)
    ap.add_argument("--dtype", default="f16")
    ap.add_argument("--ring-frames", type=int, default=64)
    ap.add_argument("--launch-reps", type=int, default=100)
    ap.add_argument("--windows", type=int, default=5)
    ap.add_argument("--phase-seconds", type=int, default=180)
    ap.add_argument("--json", default=os.path.join(ROOT, "profiles", "capture_bench.json"))
    args = ap.parse_args()
    assert torch.cuda.is_available(), "bench_capture needs a GPU"
    from af_mi355x import live, synth
    from af_mi355x.classifier import Classifier
    from af_mi355x.detector import YuNet

    props = torch.cuda.get_device_properties(0)
    out = {"tool": "bench_capture", "device": props.name, "arch": props.gcnArchName, "host": platform.node(), "capture": [CAP_H, CAP_W, 4],
           "bytes_per_frame": {"bgra_2560x1440": CAP_H * CAP_W * 4, "bgr_2560x1440": CAP_H * CAP_W * 3, "bgr_960x540": 540 * 960 * 3}}
    with phase("launch", args.phase_seconds):
        out["launch"] = bench_launch([1, 16], [(960, 540), (1280, 720)], args.launch_reps, args.windows)
    print("launch", json.dumps(out["launch"]), file=sys.stderr, flush=True)

    with phase("network", args.phase_seconds):
        clf = Classifier(precision=args.dtype)
        clf.network.load_state_dict(synth.synthetic_state_dict(seed=0))
        net = clf.cuda().eval().network
        yunet = YuNet(MODEL, inputSize=[CAP_W, CAP_H], confThreshold=0.8, nmsThreshold=0.3, topK=5000)
    rng = np.random.default_rng(2560)
    bitmaps = [rng.integers(0, 256, (CAP_H, CAP_W, 4), dtype=np.uint8) for _ in range(4)]
    keywords = dict(stride=args.stride, exclude_rect=EXCLUDE, ring_frames=args.ring_frames, drop_after=args.ring_frames - 32)
    out.update({"ticks": args.ticks, "faces_per_call": FACES, "clip_size": 32, "size": 224, "stride": args.stride, "reps": args.reps,
                "dtype": args.dtype, "ring_frames": args.ring_frames, "stored": {leg: list(STORED[leg]) for leg in LEGS},
                "detections": "scripted: the real YuNet runs on every stored frame for its cost, its rows are discarded",
                "step": "host-inclusive wall clock around the hand-over, the step and a device synchronise"})

    runs, p50s, extra = {leg: [] for leg in LEGS}, {leg: [] for leg in LEGS}, {}
    for rep in range(args.reps + 1):                              # repetition 0 warms up: rings, graphs, workspaces
        for leg in LEGS:
            with phase("realtime: %s, repetition %d" % (leg, rep), args.phase_seconds):
                script = scripts_for(1, args.ticks, args.stride, STORED[leg])
                call = live.RealtimeCall(net, detector=ScriptedYuNet(yunet, script), **keywords)
                times = play(call.step, None, leg, bitmaps, args.ticks)
                assert call.running_scores, "no window closed"
                extra[leg] = {"uploaded_bytes_per_step": call.uploaded_bytes / args.ticks}
                del call
                torch.cuda.synchronize()
                torch.cuda.empty_cache()
                if rep:
                    runs[leg].extend(times)
                    p50s[leg].append(_pct(times, 0.5))
    out["realtime"] = summarise(runs, p50s, extra)
    print("realtime", json.dumps(out["realtime"]), file=sys.stderr, flush=True)

    out["server"] = {}
    for n in (int(v) for v in args.calls.split(",")):
        runs, p50s, extra = {leg: [] for leg in LEGS}, {leg: [] for leg in LEGS}, {}
        for rep in range(args.reps + 1):
            for leg in LEGS:
                with phase("calls %d: %s, repetition %d" % (n, leg, rep), args.phase_seconds):
                    server = live.CallServer(net, detector=ScriptedYuNet(yunet, scripts_for(n, args.ticks, args.stride, STORED[leg])), **keywords)
                    cids = [server.open() for _ in range(n)]
                    assert cids == list(range(n))
                    times = play(server.step, n, leg, bitmaps, args.ticks)
                    assert server.stats.total["replay"] > 0, "no window closed"
                    extra[leg] = {"uploaded_bytes_per_tick": server.uploaded_bytes / args.ticks,
                                  "capture_launches_per_tick": server.stats.total["capture"] / args.ticks}
                    for cid in cids:
                        server.close(cid)
                    del server
                    torch.cuda.synchronize()
                    torch.cuda.empty_cache()
                    if rep:
                        runs[leg].extend(times)
                        p50s[leg].append(_pct(times, 0.5))
        out["server"]["calls%d" % n] = summarise(runs, p50s, extra)
        print(n, json.dumps(out["server"]["calls%d" % n]), file=sys.stderr, flush=True)
    line = json.dumps(out)
    print(line)
    if args.json:
        os.makedirs(os.path.dirname(os.path.abspath(args.json)), exist_ok=True)
        with open(args.json, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
