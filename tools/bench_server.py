"""Many live calls on one MI355X: CallServer.step({call: frame}) against the same calls as RealtimeCall objects stepped in turn.

    python tools/bench_server.py [--calls 1,4,16,32] [--ticks 200] [--stride 8] [--reps 2] [--dtype f16] [--json profiles/server_bench.json]

Workload: N calls, each sending captured 720p frames (eight distinct seeded BGR frames in turn) with two faces in a gallery grid;
clip 32, crop 224, `--stride` 8; call i sees its faces i % stride ticks late, so the calls' windows do not all close on one tick.
There are no face photographs here, so the REAL YuNet runs on every frame for its cost and its rows are thrown away: the tracks
are driven by scripted detections, the same rows for both legs (tools/bench_realtime.py's way).
  server   one CallServer, one step per tick for all N calls: N uploads, one af_yunet_detect_frames per 64 frames, one quality
           launch per 64 crops, one plan + warp + replay per 16 closed windows, at most three host waits
  in_turn  N RealtimeCall objects stepped one after another in the same process - the code as it was before CallServer: per call
           one upload, one YuNet launch at B = 1, one quality launch, and on a close one warp and one replay; two to three host
           waits per call
A tick is host-inclusive wall clock from the first call's frame handed in to the last call's results returned (every leg ends in
its score / quality read-back, a device synchronise).  Reported per N and leg: ticks/s, p50 / p95 tick time, and for the server
the launches and waits per tick from server.stats (the in-turn leg's detector calls are counted, its waits follow from the code:
2 per call, 3 on a close).  Both legs are warmed up by one whole run and alternate `--reps` times; `in_turn_spread` is the
run-to-run spread of the in-turn leg's p50, against which a difference at N = 1 is to be read.  `ratio` = in_turn p50 / server
p50.  Every phase runs under a time limit of its own.  Prints one JSON line and writes it to `--json`.  A run without a GPU fails.

`--tracker host,device` measures something else with the same workload, ticks and repetitions: one CallServer per leg, the legs
differing only in `tracker=`, alternating within the session after one warm-up run each; per N the tick times of both
legs, `host_spread` (the run-to-run spread of the host leg's p50, the yardstick for a difference), `ratio` = host p50 / device p50
and the launches and waits per tick; and `kernel`: the device time of one af_bytetrack_update_calls launch for 1, 4, 16, 32 and 64
trackers that each follow two faces.  The default `--json` is then profiles/server_tracker_bench.json.

`--candidates host,device` does the same for `candidates=` with `tracker="device"` in both legs - the host leg is the
device-tracker leg of `--tracker` - and `kernel` is the device time of one af_live_update_calls call (tracker and candidate stage;
its launches follow from the argument space) and of one af_face_quality_records_u8 launch on the records it left, for 1, 4, 16,
32 and 64 calls.  The default `--json` is then profiles/server_candidates_bench.json."""
import argparse
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
from bench_realtime import EXCLUDE, H, MODEL, W, scripted_rows  # noqa: E402

FACES = 2


class ScriptedYuNet:
    """the real detector for its cost, scripted rows for its answer: ``detect`` for one RealtimeCall (its own script),
    ``detect_views`` for the server (view i of a tick belongs to call i of the mapping)"""

    def __init__(self, yunet, scripts):
        self.yunet, self.scripts, self.turn, self.calls = yunet, scripts, 0, 0

    def _rows(self, dev, which):
        rows = torch.zeros(len(which), 16, 15, dtype=torch.float32, device=dev)
        counts = []
        for b, script in enumerate(which):
            mine = script[self.turn % len(script)]
            if len(mine):
                rows[b, :len(mine)] = torch.from_numpy(mine).to(dev, non_blocking=True)
            counts.append(len(mine))
        self.turn += 1
        self.calls += 1
        return rows, torch.tensor(counts, dtype=torch.int32).to(dev, non_blocking=True)

    def detect(self, frames_u8):
        self.yunet.detect(frames_u8)
        return self._rows(frames_u8.device, self.scripts[:1])

    def detect_views(self, views):
        self.yunet.detect_views(views)
        return self._rows(views[0].device, self.scripts[:len(views)])


def scripts_for(n_calls, ticks, stride):
    out = []
    for i in range(n_calls):
        rows = scripted_rows(ticks, FACES, seed=3000 + i)
        late = i % stride
        out.append([np.zeros((0, 15), np.float32)] * late + rows[:ticks - late])
    return out


def play_server(server, cids, frames, ticks):
    times, counts = [], dict.fromkeys(server.stats.KEYS, 0)
    torch.cuda.synchronize()
    for s in range(ticks):
        batch = {cid: frames[(s + i) % len(frames)] for i, cid in enumerate(cids)}
        t0 = time.perf_counter()
        server.step(batch)
        times.append(time.perf_counter() - t0)
        for k, v in server.stats.last.items():
            counts[k] = counts.get(k, 0) + v
    torch.cuda.synchronize()
    return times, {k: v / ticks for k, v in counts.items()}


def play_in_turn(calls, frames, ticks):
    times, closes = [], 0
    torch.cuda.synchronize()
    for s in range(ticks):
        t0 = time.perf_counter()
        for i, call in enumerate(calls):
            closes += bool(call.step(frames[(s + i) % len(frames)]))
        times.append(time.perf_counter() - t0)
    torch.cuda.synchronize()
    return times, closes


def tracker_kernel_times(n_list, launches=200):
    """device time of one tracker launch: n trackers that each follow two faces, in steady state"""
    from types import SimpleNamespace
    from af_mi355x import device_tracker as dt
    args = SimpleNamespace(track_thresh=0.8, track_buffer=90, match_thresh=0.8, mot20=False)
    dev, out = torch.device("cuda:0"), {}
    script = scripted_rows(launches + 20, FACES, seed=3000)
    for n in n_list:
        trackers = [dt.DeviceByteTracker(args, 30.0, device=dev) for _ in range(n)]
        ticks = []
        for rows in script:
            batch = torch.from_numpy(np.stack([np.pad(rows, ((0, 16 - len(rows)), (0, 0)))] * n)).to(dev)
            ticks.append((batch, torch.full((n,), len(rows), dtype=torch.int32, device=dev)))
        records = torch.empty(n, dt.RECORD_BYTES, dtype=torch.uint8, device=dev)
        start, stop = [torch.cuda.Event(enable_timing=True) for _ in script], [torch.cuda.Event(enable_timing=True) for _ in script]
        for i, (batch, counts) in enumerate(ticks):
            jobs = [tr.rows_job(batch[b], counts[b:b + 1], 0.76, 80) for b, tr in enumerate(trackers)]
            start[i].record()
            dt.update_calls(jobs, dev, records)
            stop[i].record()
        torch.cuda.synchronize()
        online = [len(tr.absorb(rec)) for tr, rec in zip(trackers, dt.parse_records(records.cpu().numpy()))]
        assert min(online) == FACES, online
        ms = sorted(a.elapsed_time(b) for a, b in zip(start[20:], stop[20:]))
        out["trackers%d" % n] = {"device_ms_p50": ms[len(ms) // 2], "device_ms_p95": ms[int(len(ms) * 0.95)], "launches": len(ms)}
    return out


def live_kernel_times(n_list, launches=200):
    """device time of one af_live_update_calls call and of the af_face_quality_records_u8 launch behind it: n calls that each
    follow two faces on a resident 720p frame, in steady state"""
    from types import SimpleNamespace
    from af_mi355x import device_tracker as dt
    from af_mi355x import evaluator, live
    args = SimpleNamespace(track_thresh=0.8, track_buffer=90, match_thresh=0.8, mot20=False)
    dev, out = torch.device("cuda:0"), {}
    script = scripted_rows(launches + 20, FACES, seed=3000)
    store = evaluator.FrameStore(dev, "bgr")
    store.open((H, W, 3), 1)
    store.put([np.random.default_rng(7).integers(0, 256, (H, W, 3), dtype=np.uint8)], 0)
    quality = live.RecordsQuality(dev)
    for n in n_list:
        trackers = [dt.DeviceByteTracker(args, 30.0, device=dev, candidates=True) for _ in range(n)]
        ticks = []
        for rows in script:
            batch = torch.from_numpy(np.stack([np.pad(rows, ((0, 16 - len(rows)), (0, 0)))] * n)).to(dev)
            ticks.append((batch, torch.full((n,), len(rows), dtype=torch.int32, device=dev)))
        trecs = torch.empty(n, dt.RECORD_BYTES, dtype=torch.uint8, device=dev)
        recs = torch.empty(n, dt.LIVE_RECORD_BYTES, dtype=torch.uint8, device=dev)
        ev = [[torch.cuda.Event(enable_timing=True) for _ in script] for _ in range(3)]
        for i, (batch, counts) in enumerate(ticks):
            jobs = [tr.live_rows_job(batch[b], counts[b:b + 1], 0.76, 80, (1.0, 1.0), frame_idx=i, slot=0, shape=(H, W), mesh_every=1, crop_scale=0.6,
                                     exclude_rect=EXCLUDE) for b, tr in enumerate(trackers)]
            ev[0][i].record()
            dt.update_live_calls(jobs, dev, trecs, recs)
            ev[1][i].record()
            quality.enqueue([(recs[b], store, "bgr", 0) for b in range(n)])
            ev[2][i].record()
        torch.cuda.synchronize()
        cands = [int(r["n_cands"]) for r in dt.parse_live_records(recs.cpu().numpy())]
        assert min(cands) >= 1, cands
        case = {"launches": launches, "kernels_per_call": dt.live_launches(n)}
        for name, a, b in (("live_update", 0, 1), ("quality_records", 1, 2)):
            ms = sorted(x.elapsed_time(y) for x, y in zip(ev[a][20:], ev[b][20:]))
            case[name] = {"device_ms_p50": ms[len(ms) // 2], "device_ms_p95": ms[int(len(ms) * 0.95)]}
        out["calls%d" % n] = case
    return out


def tracker_legs(args, net, yunet, frames, keywords, out):
    from af_mi355x import live
    what = "candidates" if args.candidates else "tracker"
    legs = (args.candidates or args.tracker).split(",")
    assert legs[0] == "host" and set(legs) <= {"host", "device"} and len(legs) == 2, "--%s host,device" % what
    out.update(tool="bench_server --%s" % what, legs=legs)
    if args.candidates:
        keywords = dict(keywords, tracker="device")
    for n in (int(v) for v in args.calls.split(",")):
        scripts = scripts_for(n, args.ticks, args.stride)
        runs, per_tick, p50s = {leg: [] for leg in legs}, {}, {leg: [] for leg in legs}
        for rep in range(args.reps + 1):                          # repetition 0 warms up: rings, graphs, workspaces
            for leg in legs:
                with phase("calls %d: %s=%s, repetition %d" % (n, what, leg, rep), args.phase_seconds):
                    server = live.CallServer(net, detector=ScriptedYuNet(yunet, scripts), **dict(keywords, **{what: leg}))
                    cids = [server.open() for _ in range(n)]
                    times, per_tick[leg] = play_server(server, cids, frames, args.ticks)
                    assert server.stats.total["replay"] > 0, "no window closed"
                    for cid in cids:
                        server.close(cid)
                    del server
                    torch.cuda.synchronize()
                    torch.cuda.empty_cache()
                    if rep:
                        runs[leg].extend(times)
                        p50s[leg].append(_pct(times, 0.5))
        case = {leg: {"tick_s": _stats(runs[leg]), "ticks_per_s": len(runs[leg]) / sum(runs[leg]), "per_tick": per_tick[leg],
                      "p50_per_repetition": p50s[leg]} for leg in legs}
        for leg in legs:
            case["%s_spread" % leg] = (max(p50s[leg]) - min(p50s[leg])) / min(p50s[leg]) if len(p50s[leg]) > 1 else None
        case["ratio"] = case["host"]["tick_s"]["p50"] / case["device"]["tick_s"]["p50"]
        out["cases"]["calls%d" % n] = case
        print(n, json.dumps(case), file=sys.stderr, flush=True)
    with phase("%s kernel" % what, args.phase_seconds):
        out["kernel"] = (live_kernel_times if args.candidates else tracker_kernel_times)([1, 4, 16, 32, 64])
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--calls", default="1,4,16,32")
    ap.add_argument("--ticks", type=int, default=200)
    ap.add_argument("--stride", type=int, default=8)
    ap.add_argument("--reps", type=int, default=2)
    ap.add_argument("--dtype", default="f16")
    ap.add_argument("--ring-frames", type=int, default=128)
    ap.add_argument("--phase-seconds", type=int, default=240)
    ap.add_argument("--tracker", default=None, help="host,device: the two tracker modes of one CallServer instead of server / in_turn")
    ap.add_argument("--candidates", default=None, help="host,device: the two candidate modes of one CallServer with device trackers")
    ap.add_argument("--json", default=None)
    args = ap.parse_args()
    assert not (args.tracker and args.candidates), "--tracker or --candidates, not both"
    if args.json is None:
        args.json = os.path.join(ROOT, "profiles", "server_candidates_bench.json" if args.candidates else
                                 "server_tracker_bench.json" if args.tracker else "server_bench.json")
    assert torch.cuda.is_available(), "bench_server needs a GPU"
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
    keywords = dict(stride=args.stride, exclude_rect=EXCLUDE, ring_frames=args.ring_frames)
    out = {"tool": "bench_server", "device": props.name, "arch": props.gcnArchName, "host": platform.node(), "ticks": args.ticks,
           "frame_size": [H, W], "faces_per_call": FACES, "clip_size": 32, "size": 224, "stride": args.stride, "reps": args.reps,
           "dtype": args.dtype, "ring_frames": args.ring_frames,
           "detections": "scripted: the real YuNet runs on every frame for its cost, its rows are discarded (no face photographs)",
           "tick": "host-inclusive wall clock, all N calls, ends in a device synchronise", "cases": {}}
    if args.tracker or args.candidates:
        tracker_legs(args, net, yunet, frames, keywords, out)
    for n in (int(v) for v in args.calls.split(",") if not (args.tracker or args.candidates)):
        scripts = scripts_for(n, args.ticks, args.stride)
        runs = {"server": [], "in_turn": []}
        per_tick, p50s, in_turn_detects, closes = {}, [], 0, 0
        for rep in range(args.reps + 1):                          # repetition 0 warms up: rings, graphs, workspaces
            for leg in ("server", "in_turn"):
                with phase("calls %d: %s, repetition %d" % (n, leg, rep), args.phase_seconds):
                    if leg == "server":
                        server = live.CallServer(net, detector=ScriptedYuNet(yunet, scripts), **keywords)
                        cids = [server.open() for _ in range(n)]
                        times, per_tick = play_server(server, cids, frames, args.ticks)
                        assert server.stats.total["replay"] > 0, "no window closed"
                        for cid in cids:
                            server.close(cid)
                        del server
                    else:
                        dets = [ScriptedYuNet(yunet, scripts[i:i + 1]) for i in range(n)]
                        calls = [live.RealtimeCall(net, detector=dets[i], **keywords) for i in range(n)]
                        times, closes = play_in_turn(calls, frames, args.ticks)
                        assert closes, "no window closed"
                        in_turn_detects = sum(d.calls for d in dets) / args.ticks
                        if rep:
                            p50s.append(_pct(times, 0.5))
                        del calls, dets
                    torch.cuda.synchronize()
                    torch.cuda.empty_cache()
                    if rep:
                        runs[leg].extend(times)
        case = {leg: {"tick_s": _stats(runs[leg]), "ticks_per_s": len(runs[leg]) / sum(runs[leg])} for leg in runs}
        case["server"]["per_tick"] = per_tick
        case["in_turn"]["per_tick"] = {"detect": in_turn_detects, "closing_steps": closes / args.ticks,
                                       "wait": "2 per call, 3 on a closing step (live.RealtimeCall; not counted)"}
        case["in_turn_spread"] = (max(p50s) - min(p50s)) / min(p50s) if len(p50s) > 1 else None
        case["ratio"] = case["in_turn"]["tick_s"]["p50"] / case["server"]["tick_s"]["p50"]
        out["cases"]["calls%d" % n] = case
        print(n, json.dumps(case), file=sys.stderr, flush=True)
    line = json.dumps(out)
    print(line)
    if args.json:
        os.makedirs(os.path.dirname(os.path.abspath(args.json)), exist_ok=True)
        with open(args.json, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
