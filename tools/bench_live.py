"""The live call on one MI355X: LiveCall.step against the composition of the parts it joins, in one process.

    python tools/bench_live.py [--frames 300] [--faces 1,4,16] [--stride 8] [--reps 3] [--dtype f16] [--json profiles/live_bench.json]

Workload: `--frames` captured 720p frames (eight distinct seeded BGR frames in turn) and 1, 4 and 16 scripted faces in a gallery
grid that all appear on the first frame, so their windows close on the same captured frames (device-independent seeds); clip 32,
crop 224, `--stride` 8.  Both paths get the same frames and faces.
  new     LiveCall.step(frame_bgr, faces): the frame uploaded once into the ring, the windows that close together warped by one
          BGR launch and scored by one graph replay at the padded batch size, one read-back
  parent  per step the frame reversed on the host (what cv2.cvtColor costs the reference, af_realtime.py:434), per face a host-cut
          crop pushed into its own StreamingCropAligner; on a close per face align_last into its own LiveScorer's clip and a B = 1
          replay with its own read-back
Host-inclusive wall clock per step: p50 / p95 over all steps, and over the closing steps alone (frame in -> scores out: the
enqueue-to-score latency); sustained faces x frames per second over the whole script (device drained at the end); bytes sent to the
device (pixels; the window tables of the new path are counted too).  Both paths are warmed up by one whole script; new / parent
alternate `--reps` times.  With one face both paths run the same kernels at B = 1 and their scores must be equal; with more the
batch size differs and the largest difference is reported.
`kernel`: device-event time of one BGR launch (16 windows x 32 frames out of the ring) against the RGB launch of the same table on
a ring whose pixels were reversed beforehand, alternated.
Every phase runs under a time limit of its own (a watchdog ends the process with status 124 and says which phase).  Prints one JSON
line and writes it to `--json`.  A run without a GPU fails."""
import argparse
import ctypes as C
import json
import os
import platform
import statistics
import sys
import threading
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import numpy as np  # noqa: E402
import torch  # noqa: E402

H, W, CLIP, SIZE = 720, 1280, 32, 224


class phase:
    """a step of the benchmark under its own time limit: past it the process ends, whatever the main thread is waiting in"""

    def __init__(self, name, seconds):
        self.name, self.seconds = name, seconds

    def _expire(self):
        print("bench_live: phase %r exceeded its %d s" % (self.name, self.seconds), file=sys.stderr, flush=True)
        os._exit(124)

    def __enter__(self):
        self.timer = threading.Timer(self.seconds, self._expire)
        self.timer.daemon = True
        self.timer.start()

    def __exit__(self, *exc):
        self.timer.cancel()


def _pct(v, q):
    v = sorted(v)
    return v[min(len(v) - 1, int(round(q * (len(v) - 1))))]


def _stats(v):
    return {"p50": _pct(v, 0.5), "p95": _pct(v, 0.95), "mean": statistics.fmean(v), "n": len(v)}


def scripted_faces(n_frames, faces, seed):
    """per frame [(tid, tlbr float32[4], lm5 float32[5,2])]: `faces` faces in a gallery grid, each jittering in its tile"""
    from af_mi355x import aligner
    rng = np.random.default_rng(seed)
    grid = int(np.ceil(np.sqrt(faces)))
    tile_w, tile_h = W / grid, H / grid
    std = (aligner.STD_POINTS_317 - aligner.STD_POINTS_317.mean(0)) / 317.0
    centres = [np.array([(k % grid + 0.5) * tile_w, (k // grid + 0.5) * tile_h]) for k in range(faces)]
    out = []
    for _ in range(n_frames):
        row = []
        for k in range(faces):
            centres[k] = centres[k] + rng.normal(0, 0.4, 2)
            half = 0.2 * tile_h + rng.normal(0, 0.3)
            cx, cy = centres[k]
            tlbr = np.array([cx - half, cy - half, cx + half, cy + half], dtype=np.float32)
            row.append((k, tlbr, (std * 2.2 * half + centres[k] + rng.normal(0, 0.4, (5, 2))).astype(np.float32)))
        out.append(row)
    return out


class ParentCall:
    """the parent's composition behind the same interface: one StreamingCropAligner + one LiveScorer per face, the reference's
    window bookkeeping for tracks that are seen on every step"""

    def __init__(self, net, faces, stride, max_crop_pixels, crop_scale=0.6):
        from af_mi355x import aligner
        from af_mi355x.classifier import LiveScorer
        self.stride, self.crop_scale = stride, crop_scale
        self.aligners = [aligner.StreamingCropAligner(size=SIZE, capacity=CLIP + 8, max_crop_pixels=max_crop_pixels) for _ in range(faces)]
        self.scorers = [LiveScorer(net, clip_size=CLIP, crop=SIZE) for _ in range(faces)]
        self.uploaded_bytes = 0
        self.reset()

    def reset(self):
        self.held, self.since = [0] * len(self.aligners), [0] * len(self.aligners)
        for al in self.aligners:
            al.frames.clear()

    def step(self, frame_bgr, faces):
        from af_mi355x.evaluator import get_crop_box
        frgb = np.ascontiguousarray(frame_bgr[..., ::-1])                       # cv2.cvtColor(frame_bgr, cv2.COLOR_BGR2RGB)
        ready = []
        for k, tlbr, lm5 in faces:
            x1, y1, x2, y2 = map(int, get_crop_box((H, W), tlbr, scale=self.crop_scale))
            top_left = np.array([[x1, y1]], dtype=np.float32)
            record = ((tlbr.reshape(2, 2) - top_left).reshape(-1), lm5 - top_left, np.zeros((68, 2), np.float32),
                      np.array([x1, y1, x2, y2], dtype=np.int32))
            crop = frgb[y1:y2, x1:x2]
            self.aligners[k].push(record, crop)
            self.uploaded_bytes += crop.size
            self.held[k] = min(CLIP, self.held[k] + 1)
            self.since[k] += 1
            if self.held[k] == CLIP and self.since[k] >= self.stride:
                self.since[k] = 0
                ready.append(k)
        results = []
        for k in ready:
            self.aligners[k].align_last(CLIP, out=self.scorers[k].clip[0])
            results.append((k, float(self.scorers[k]()[0])))
        for k in ready:
            self.held[k] = min(self.held[k], max(0, CLIP - self.stride)) if self.stride < CLIP else self.held[k]
        return results


def play(call, frames, script, tid_offset=0):
    """-> (per-step seconds, indices of the closing steps, total seconds with the device drained, results per closing step)"""
    per_step, closing, results = [], [], []
    torch.cuda.synchronize()
    t_all = time.perf_counter()
    for s, faces in enumerate(script):
        if tid_offset:
            faces = [(tid + tid_offset, tlbr, lm5) for tid, tlbr, lm5 in faces]
        t0 = time.perf_counter()
        res = call.step(frames[s % len(frames)], faces)
        per_step.append(time.perf_counter() - t0)
        if res:
            closing.append(s)
            results.append([sc for _, sc in res])
    torch.cuda.synchronize()
    return per_step, closing, time.perf_counter() - t_all, results


def kernel_times(call, iters):
    """device-event ms of the BGR launch on the call's ring against the RGB launch of the same table on a reversed copy of it"""
    from af_mi355x import _lib
    ring = call._ring.store
    table = call._ring.warp.tables.last.dev                                      # the table the last full batch left on the device
    n = int(np.frombuffer(table[:4].cpu().numpy().tobytes(), dtype=np.int32)[0])
    pix = call.ring_frames * ring.frame_nbytes
    swapped = torch.cat([ring.dev[:pix].view(-1, 3).flip(1).contiguous().view(-1), ring.dev[pix:]])
    out = [torch.empty((n, CLIP, SIZE, SIZE, 3), dtype=torch.uint8, device=ring.device) for _ in range(2)]
    stream = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    ms = {"bgr": [], "rgb": []}
    for it in range(iters + 2):
        for name, fn, src, dst in (("bgr", "af_warp_affine_window_rects_bgr_u8", ring.dev, out[0]),
                                   ("rgb", "af_warp_affine_window_rects_u8", swapped, out[1])):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            _lib.check(getattr(_lib.lib, fn)(C.c_void_p(src.data_ptr()), C.c_void_p(table.data_ptr()), n, CLIP, SIZE,
                                             C.c_void_p(dst.data_ptr()), stream), fn)
            e1.record()
            torch.cuda.synchronize()
            if it >= 2:
                ms[name].append(e0.elapsed_time(e1))
    assert torch.equal(out[0], out[1]) and bool(out[0].any())
    return {"windows": n, "bgr_ms": _stats(ms["bgr"]), "rgb_ms": _stats(ms["rgb"])}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", type=int, default=300)
    ap.add_argument("--faces", default="1,4,16")
    ap.add_argument("--stride", type=int, default=8)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--dtype", default="f16")
    ap.add_argument("--kernel-iters", type=int, default=30)
    ap.add_argument("--phase-seconds", type=int, default=240)
    ap.add_argument("--json", default=os.path.join(ROOT, "profiles", "live_bench.json"))
    args = ap.parse_args()
    assert torch.cuda.is_available(), "bench_live needs a GPU"
    import af_mi355x  # noqa: F401
    from af_mi355x import live, synth
    from af_mi355x.classifier import Classifier

    with phase("network", args.phase_seconds):
        clf = Classifier(precision=args.dtype)
        clf.network.load_state_dict(synth.synthetic_state_dict(seed=0))
        net = clf.cuda().eval().network
    rng = np.random.default_rng(720)
    frames = [rng.integers(0, 256, (H, W, 3), dtype=np.uint8) for _ in range(8)]
    props = torch.cuda.get_device_properties(0)
    out = {"tool": "bench_live", "device": props.name, "arch": props.gcnArchName, "compute_units": props.multi_processor_count,
           "host": platform.node(), "frames": args.frames, "frame_size": [H, W], "clip_size": CLIP, "size": SIZE, "stride": args.stride,
           "reps": args.reps, "dtype": args.dtype, "cases": {}}

    call = None
    for faces in (int(v) for v in args.faces.split(",")):
        script = scripted_faces(args.frames, faces, seed=1000 + faces)
        with phase("faces %d: set-up and warm-up" % faces, args.phase_seconds):
            call = live.LiveCall(net, clip_size=CLIP, size=SIZE, stride=args.stride)
            side = max(float(max(t[2] - t[0], t[3] - t[1])) for row in script for _, t, _ in row) * (1.0 + 2 * 0.6) + 4.0
            parent = ParentCall(net, faces, args.stride, max_crop_pixels=int(side * side))       # slots as small as the script's crops allow
            _, closing_new, _, res_new = play(call, frames, script)
            _, closing_parent, _, res_parent = play(parent, frames, script)
            assert closing_new == closing_parent and len(closing_new) > 0, (closing_new[:4], closing_parent[:4])
            diff = max(abs(a - b) for ra, rb in zip(res_new, res_parent) for a, b in zip(ra, rb))
            if faces == 1:
                assert diff == 0.0, diff                      # the same kernels at B = 1 on the same bytes
        runs = {"new": [], "parent": []}
        for rep in range(args.reps):
            for name in ("new", "parent"):
                with phase("faces %d: %s, repetition %d" % (faces, name, rep), args.phase_seconds):
                    if name == "new":
                        before = call.uploaded_bytes
                        turns = call._ring.warp.tables.turn
                        r = play(call, frames, script, tid_offset=1000 * (rep + 1))      # new tids: the tracks start empty
                        sent = call.uploaded_bytes - before + (call._ring.warp.tables.turn - turns) * call._ring.warp.table_bytes
                    else:
                        parent.reset()
                        before = parent.uploaded_bytes
                        r = play(parent, frames, script)
                        sent = parent.uploaded_bytes - before
                    runs[name].append((r, sent))
        case = {"closing_steps": len(closing_new), "windows": faces * len(closing_new), "max_score_difference_new_vs_parent": diff}
        for name in ("new", "parent"):
            steps = [t for (per, _, _, _), _ in runs[name] for t in per]
            closes = [per[s] for (per, closing, _, _), _ in runs[name] for s in closing]
            totals = [total for (_, _, total, _), _ in runs[name]]
            case[name] = {"step_s": _stats(steps), "closing_step_s": _stats(closes), "script_s": sorted(totals),
                          "faces_x_frames_per_s": faces * args.frames / statistics.median(totals), "uploaded_bytes": int(runs[name][0][1])}
        out["cases"]["faces%d" % faces] = case
        print(faces, json.dumps(case), file=sys.stderr, flush=True)
        del parent
    with phase("kernel", args.phase_seconds):
        out["kernel"] = kernel_times(call, args.kernel_iters)
    line = json.dumps(out)
    print(line)
    if args.json:
        os.makedirs(os.path.dirname(os.path.abspath(args.json)), exist_ok=True)
        with open(args.json, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
