"""YUV 4:2:0 frames into the frame stores on one MI355X: the conversion launch alone, and CallServer ticks on BGR, I420 and NV12 frames.

    python tools/bench_yuv.py [--calls 1,4,16,32] [--ticks 160] [--reps 2] [--stride 8] [--dtype f16] [--json profiles/yuv_bench.json]

launch   af_yuv420_to_rgb_u8 on 1, 16 and 64 device-resident NV12 frames of 720p and 1080p into one B, G, R store each, timed with
         device events around `--launch-reps` back-to-back launches after a warm-up: microseconds per launch and the bytes the
         conversion must move (1.5 read + 3 written per pixel) per second.  `copy_roof` is the 6.29 TB/s copy ceiling of DESIGN 4,
         quoted as context; a single 720p frame is 4.1 MB of traffic and launch-bound, so no share of the roof is stated for it.
server   tools/bench_server.py's method (720p, two scripted faces per call, the real YuNet run for its cost, `--ticks` x `--reps`
         after a warm-up repetition, the legs alternating in one process), three legs on the same pictures:
           bgr    numpy B, G, R frames: the path as it was before YuvFrame, the yardstick
           i420   host I420 planes: one pinned fill of 1.5 bytes per pixel and one copy for all calls, one conversion launch
           nv12   device-resident NV12 planes (a hardware decoder's output): no copy, one conversion launch
         Per N and leg: host-inclusive tick p50 / p95, uploaded bytes per tick, launches and copies per tick from server.stats;
         `bgr_spread` is the run-to-run spread of the bgr leg's p50, against which the other legs' gain is to be read
         (`faster_than_spread`).
Converting I420 to BGR on a host core with numpy is no fair stand-in for cv2 and is not timed: `staged_bytes_per_frame` states what
an integrator stages per frame before (3 bytes per pixel, after a host conversion) and after (1.5, or none).
Every phase runs under a time limit of its own.  Prints one JSON line and writes it to `--json`.  A run without a GPU fails.

    python tools/bench_yuv.py --formats [--calls 4,16,32] [--ticks 160] [--host-ticks 12] [--reps 2] [--rounds 5] [--no-server]
                              [--json profiles/yuv_formats_bench.json]

The formats beyond 8-bit 4:2:0 at OpenCV's colour (af_yuv_to_rgb_ex_u8, csrc/af_yuv_formats.hip), all legs in one session:
launch   per format, 1 and 64 device-resident frames of 720p and 1080p: microseconds per launch of the new kernel, beside a device copy
         that moves the same bytes (read + written) and beside af_yuv420_to_rgb_u8 on NV12 frames of that size.  The legs alternate
         over `--rounds` rounds of `--launch-reps` launches; each leg reports its median round and its spread (max - min) / min.  The
         `nv12` row is the new kernel on the old kernel's frames: `new_over_old` and whether it exceeds both spreads.
server   CallServer tick p50 at 720p: host yuy2 frames and device p010 frames through the new launch, host I420 through the old one
         (the path as it was), and `host_numpy`: the same yuy2 frames converted on a host core by the numpy statement
         (tests/yuv_formats_ref.py) inside the tick and handed in as B, G, R - no cv2 here, so that leg is a ratio to numpy, over
         `--host-ticks` ticks only.
staged   bytes staged per 720p host frame, per format."""
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
sys.path.insert(0, os.path.join(ROOT, "tests"))

import numpy as np  # noqa: E402
import torch  # noqa: E402

from bench_live import _pct, _stats, phase  # noqa: E402
from bench_realtime import EXCLUDE, H, MODEL, W  # noqa: E402
from bench_server import ScriptedYuNet, scripts_for  # noqa: E402

COPY_ROOF = 6.29e12        # bytes/s, DESIGN 4: the measured device-to-device copy ceiling
LEGS = ("bgr", "i420", "nv12")


def bench_launch(sizes, counts, reps):
    from af_mi355x import _lib, evaluator, frames as F
    dev = torch.device("cuda", torch.cuda.current_device())
    stream = C.c_void_p(torch.cuda.current_stream(dev).cuda_stream)
    out = {}
    for h, w in sizes:
        for n in counts:
            store = evaluator.FrameStore(dev, "bgr")
            store.open((h, w, 3), n)
            planes = torch.randint(0, 256, (n, h * 3 // 2, w), dtype=torch.uint8, device=dev)
            frames = [F.YuvFrame.from_packed(planes[k], h, w, "nv12") for k in range(n)]
            ref = F.store_ref(store, "bgr")
            items = F.YuvConverter.table(frames, [None] * n, [ref] * n, list(range(n)))
            launch = lambda: _lib.check(_lib.lib.af_yuv420_to_rgb_u8(C.byref(items), n, stream), "yuv420_to_rgb_u8")  # noqa: E731
            for _ in range(5):
                launch()
            torch.cuda.synchronize()
            t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            t0.record()
            for _ in range(reps):
                launch()
            t1.record()
            torch.cuda.synchronize()
            us = t0.elapsed_time(t1) * 1e3 / reps
            moved = n * h * w * 4.5
            out["%dx%d_n%d" % (w, h, n)] = {"us_per_launch": us, "bytes_moved": moved, "bytes_per_s": moved / (us * 1e-6),
                                            "launches_timed": reps}
            del store, planes, frames
    return out


LAYOUT_FORMATS = ("nv12", "i420", "yuy2", "uyvy", "i422", "nv16", "i444", "p010", "i010")      # one of each layout and order that differs in loads


def _device_frames(fmt, n, h, w, dev, **colour):
    import yuv_formats_ref as X
    from af_mi355x import frames as F
    out = []
    for k in range(n):
        planes = X.random_planes(fmt, h, w, seed=k % 4)
        out.append(F.YuvFrame(fmt, **X.kwargs([torch.from_numpy(p).to(dev) for p in planes], fmt), **colour))
    return out


def _timed(fn, reps):
    t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    t0.record()
    for _ in range(reps):
        fn()
    t1.record()
    torch.cuda.synchronize()
    return t0.elapsed_time(t1) * 1e3 / reps


def _leg(us):
    us = sorted(us)
    return {"us_per_launch": us[len(us) // 2], "spread": (us[-1] - us[0]) / us[0], "rounds": us}


def bench_format_launches(sizes, counts, reps, rounds):
    from af_mi355x import _lib, evaluator, frames as F
    dev = torch.device("cuda", torch.cuda.current_device())
    stream = C.c_void_p(torch.cuda.current_stream(dev).cuda_stream)
    out = {}
    for h, w in sizes:
        for n in counts:
            store = evaluator.FrameStore(dev, "bgr")
            store.open((h, w, 3), n)
            ref = F.store_ref(store, "bgr")
            old_frames = _device_frames("nv12", n, h, w, dev)
            old_items = F.YuvConverter.table(old_frames, [None] * n, [ref] * n, list(range(n)))
            old = lambda: _lib.check(_lib.lib.af_yuv420_to_rgb_u8(C.byref(old_items), n, stream), "yuv420_to_rgb_u8")  # noqa: E731
            for fmt in LAYOUT_FORMATS:
                colour = {} if fmt in F.FORMATS else dict(matrix="bt709")
                frames = old_frames if fmt == "nv12" else _device_frames(fmt, n, h, w, dev, **colour)
                items = F.YuvConverter.table_ex(frames, [None] * n, [ref] * n, list(range(n)))
                new = lambda: _lib.check(_lib.lib.af_yuv_to_rgb_ex_u8(C.byref(items), n, stream), "yuv_to_rgb_ex_u8")  # noqa: E731
                moved = n * (frames[0].nbytes + h * w * 3)
                src = torch.empty(moved // 2, dtype=torch.uint8, device=dev)
                dst = torch.empty_like(src)
                copy = lambda: dst.copy_(src)  # noqa: E731
                legs = {"new": (new, []), "copy": (copy, []), "old_nv12": (old, [])}
                for fn, _ in legs.values():
                    _timed(fn, 5)
                for _ in range(rounds):                           # the legs alternate
                    for fn, us in legs.values():
                        us.append(_timed(fn, reps))
                row = {k: _leg(us) for k, (_, us) in legs.items()}
                row.update(bytes_moved=moved, bytes_per_s=moved / (row["new"]["us_per_launch"] * 1e-6), launches_timed=reps,
                           new_over_copy=row["new"]["us_per_launch"] / row["copy"]["us_per_launch"],
                           new_over_old=row["new"]["us_per_launch"] / row["old_nv12"]["us_per_launch"])
                if fmt == "nv12":
                    gap = abs(row["new_over_old"] - 1.0)
                    row["differs_beyond_spread"] = bool(gap > max(row["new"]["spread"], row["old_nv12"]["spread"]))
                out["%s_%dx%d_n%d" % (fmt, w, h, n)] = row
                del src, dst, frames
            del store, old_frames
            torch.cuda.empty_cache()
    return out


def formats_main(args):
    import yuv_formats_ref as X
    from af_mi355x import frames as F, live, synth
    from af_mi355x.classifier import Classifier
    from af_mi355x.detector import YuNet
    props = torch.cuda.get_device_properties(0)
    staged = {fmt: F.YuvFrame(fmt, **X.kwargs(X.random_planes(fmt, 2, 2, 0), fmt)).nbytes * H * W // 4 for fmt in X.FORMATS}
    out = {"tool": "bench_yuv --formats", "device": props.name, "arch": props.gcnArchName, "host": platform.node(),
           "staged_bytes_per_frame": dict(staged, frame_size=[H, W], bgr_after_a_host_conversion=H * W * 3, device_resident=0)}
    with phase("launch", args.phase_seconds):
        out["launch"] = bench_format_launches([(720, 1280), (1080, 1920)], [1, 64], args.launch_reps, args.rounds)
        out["launch_note"] = ("device events around back-to-back launches on the same buffers: working sets under 256 MB may be served by the "
                              "Infinity Cache; one frame is launch-bound; `copy` moves as many bytes as the conversion reads and writes")
    print("launch", json.dumps(out["launch"]), file=sys.stderr, flush=True)
    if not args.no_server:
        with phase("network", args.phase_seconds):
            clf = Classifier(precision=args.dtype)
            clf.network.load_state_dict(synth.synthetic_state_dict(seed=0))
            net = clf.cuda().eval().network
            yunet = YuNet(MODEL, inputSize=[W, H], confThreshold=0.8, nmsThreshold=0.3, topK=5000)
        dev = torch.device("cuda", torch.cuda.current_device())
        yuy2 = [X.random_planes("yuy2", H, W, seed=720 + k) for k in range(8)]
        p010 = [X.random_planes("p010", H, W, seed=720 + k) for k in range(8)]
        i420 = [X.random_planes("i420", H, W, seed=720 + k) for k in range(8)]
        frames = {"yuy2_host": [F.YuvFrame("yuy2", p[0]) for p in yuy2],
                  "p010_device": [F.YuvFrame("p010", torch.from_numpy(p[0]).to(dev), uv=torch.from_numpy(p[1]).to(dev)) for p in p010],
                  "i420_host_old_launch": [F.YuvFrame("i420", *p) for p in i420],
                  "host_numpy": [(lambda p=p: X.convert(p, "yuy2")) for p in yuy2]}
        legs = tuple(frames)
        keywords = dict(stride=args.stride, exclude_rect=EXCLUDE, ring_frames=args.ring_frames)
        out.update({"ticks": args.ticks, "host_ticks": args.host_ticks, "frame_size": [H, W], "faces_per_call": 2, "stride": args.stride,
                    "reps": args.reps, "dtype": args.dtype, "tick": "host-inclusive wall clock, all N calls, ends in a device synchronise",
                    "host_numpy": "the yuy2 frames converted inside the tick by tests/yuv_formats_ref.py on one host core: a ratio to numpy, not to cv2",
                    "cases": {}})
        for n in (int(v) for v in args.calls.split(",")):
            scripts = scripts_for(n, args.ticks, args.stride)
            runs, per_tick, p50s = {leg: [] for leg in legs}, {}, {leg: [] for leg in legs}
            for rep in range(args.reps + 1):                      # repetition 0 warms up
                for leg in legs:
                    ticks = args.host_ticks if leg == "host_numpy" else args.ticks
                    with phase("calls %d: %s, repetition %d" % (n, leg, rep), args.phase_seconds):
                        server = live.CallServer(net, detector=ScriptedYuNet(yunet, scripts), **keywords)
                        cids = [server.open() for _ in range(n)]
                        times, per_tick[leg] = play(server, cids, frames[leg], ticks)
                        for cid in cids:
                            server.close(cid)
                        del server
                        torch.cuda.synchronize()
                        torch.cuda.empty_cache()
                        if rep:
                            runs[leg].extend(times)
                            p50s[leg].append(_pct(times, 0.5))
            case = {leg: {"tick_s": _stats(runs[leg]), "per_tick": per_tick[leg], "p50_per_repetition": p50s[leg],
                          "spread": (max(p50s[leg]) - min(p50s[leg])) / min(p50s[leg]) if len(p50s[leg]) > 1 else None} for leg in legs}
            for leg in ("yuy2_host", "p010_device"):
                case[leg]["p50_over_host_numpy"] = case[leg]["tick_s"]["p50"] / case["host_numpy"]["tick_s"]["p50"]
                case[leg]["p50_over_i420_old_launch"] = case[leg]["tick_s"]["p50"] / case["i420_host_old_launch"]["tick_s"]["p50"]
            out["cases"]["calls%d" % n] = case
            print(n, json.dumps(case), file=sys.stderr, flush=True)
    line = json.dumps(out)
    print(line)
    if args.json:
        os.makedirs(os.path.dirname(os.path.abspath(args.json)), exist_ok=True)
        with open(args.json, "w") as f:
            f.write(line + "\n")


def make_frames(n_pictures, seed=720):
    """the same pictures three ways: host I420 planes, yuv_ref's B, G, R arrays of them, packed NV12 buffers"""
    import yuv_ref as R
    rng = np.random.default_rng(seed)
    out = []
    for _ in range(n_pictures):
        y, u, v = (rng.integers(0, 256, s, dtype=np.uint8) for s in ((H, W), (H // 2, W // 2), (H // 2, W // 2)))
        out.append((R.pack(y, u, v, "i420"), np.ascontiguousarray(R.planes_to_bgr(y, u, v)), R.pack(y, u, v, "nv12")))
    return out


def play(server, cids, frames, ticks):
    times, counts = [], {}
    torch.cuda.synchronize()
    start = server.uploaded_bytes
    for s in range(ticks):
        batch = {cid: frames[(s + i) % len(frames)] for i, cid in enumerate(cids)}
        t0 = time.perf_counter()
        batch = {cid: f() if callable(f) else f for cid, f in batch.items()}       # a host conversion is part of the tick
        server.step(batch)
        times.append(time.perf_counter() - t0)
        for k, v in server.stats.last.items():
            counts[k] = counts.get(k, 0) + v
    torch.cuda.synchronize()
    per_tick = {k: v / ticks for k, v in counts.items()}
    per_tick["uploaded_bytes"] = (server.uploaded_bytes - start) / ticks
    return times, per_tick


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--calls", default="1,4,16,32")
    ap.add_argument("--ticks", type=int, default=160)
    ap.add_argument("--stride", type=int, default=8)
    ap.add_argument("--reps", type=int, default=2)
    ap.add_argument("--dtype", default="f16")
    ap.add_argument("--ring-frames", type=int, default=128)
    ap.add_argument("--launch-reps", type=int, default=200)
    ap.add_argument("--phase-seconds", type=int, default=240)
    ap.add_argument("--json", default=None)
    ap.add_argument("--formats", action="store_true", help="the formats of af_yuv_to_rgb_ex_u8 -> profiles/yuv_formats_bench.json")
    ap.add_argument("--no-server", action="store_true", help="with --formats: the launches and the staged bytes only")
    ap.add_argument("--host-ticks", type=int, default=12)
    ap.add_argument("--rounds", type=int, default=5)
    args = ap.parse_args()
    assert torch.cuda.is_available(), "bench_yuv needs a GPU"
    if args.json is None:
        args.json = os.path.join(ROOT, "profiles", "yuv_formats_bench.json" if args.formats else "yuv_bench.json")
    if args.formats:
        return formats_main(args)
    from af_mi355x import frames as F, live, synth
    from af_mi355x.classifier import Classifier
    from af_mi355x.detector import YuNet

    props = torch.cuda.get_device_properties(0)
    out = {"tool": "bench_yuv", "device": props.name, "arch": props.gcnArchName, "host": platform.node(),
           "copy_roof_bytes_per_s": COPY_ROOF, "copy_roof": "DESIGN 4's device copy ceiling, context only",
           "staged_bytes_per_frame": {"frame_size": [H, W], "bgr_after_a_host_conversion": H * W * 3, "i420_host": H * W * 3 // 2,
                                      "nv12_device_resident": 0}}
    with phase("launch", args.phase_seconds):
        out["launch"] = bench_launch([(720, 1280), (1080, 1920)], [1, 16, 64], args.launch_reps)
        out["launch_note"] = ("one 720p frame is 4.1 MB of traffic: launch-bound, no share of the roof is claimed for it; the launches "
                              "repeat on the same buffers, so a working set under 256 MB (all but 64 frames of 720p and 16 or 64 of "
                              "1080p) may be served by the Infinity Cache and not by HBM")
    print("launch", json.dumps(out["launch"]), file=sys.stderr, flush=True)

    with phase("network", args.phase_seconds):
        clf = Classifier(precision=args.dtype)
        clf.network.load_state_dict(synth.synthetic_state_dict(seed=0))
        net = clf.cuda().eval().network
        yunet = YuNet(MODEL, inputSize=[W, H], confThreshold=0.8, nmsThreshold=0.3, topK=5000)
    dev = torch.device("cuda", torch.cuda.current_device())
    pictures = make_frames(8)
    frames = {"bgr": [bgr for _, bgr, _ in pictures],
              "i420": [F.YuvFrame.from_packed(buf, H, W, "i420") for buf, _, _ in pictures],
              "nv12": [F.YuvFrame.from_packed(torch.from_numpy(nv).to(dev), H, W, "nv12") for _, _, nv in pictures]}
    keywords = dict(stride=args.stride, exclude_rect=EXCLUDE, ring_frames=args.ring_frames)
    out.update({"ticks": args.ticks, "frame_size": [H, W], "faces_per_call": 2, "clip_size": 32, "size": 224, "stride": args.stride,
                "reps": args.reps, "dtype": args.dtype, "ring_frames": args.ring_frames,
                "detections": "scripted: the real YuNet runs on every frame for its cost, its rows are discarded (no face photographs)",
                "tick": "host-inclusive wall clock, all N calls, ends in a device synchronise", "cases": {}})
    for n in (int(v) for v in args.calls.split(",")):
        scripts = scripts_for(n, args.ticks, args.stride)
        runs, per_tick, p50s = {leg: [] for leg in LEGS}, {}, {leg: [] for leg in LEGS}
        for rep in range(args.reps + 1):                          # repetition 0 warms up: rings, graphs, workspaces
            for leg in LEGS:
                with phase("calls %d: %s, repetition %d" % (n, leg, rep), args.phase_seconds):
                    server = live.CallServer(net, detector=ScriptedYuNet(yunet, scripts), **keywords)
                    cids = [server.open() for _ in range(n)]
                    times, per_tick[leg] = play(server, cids, frames[leg], args.ticks)
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
                      "p50_per_repetition": p50s[leg]} for leg in LEGS}
        base = case["bgr"]["tick_s"]["p50"]
        spread = (max(p50s["bgr"]) - min(p50s["bgr"])) / min(p50s["bgr"]) if len(p50s["bgr"]) > 1 else None
        case["bgr_spread"] = spread
        for leg in LEGS[1:]:
            gain = (base - case[leg]["tick_s"]["p50"]) / base
            case[leg]["gain_over_bgr"] = gain
            case[leg]["faster_than_spread"] = None if spread is None else bool(gain > spread)
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
