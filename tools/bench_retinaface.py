"""Throughput of the HIP RetinaFace detector (csrc/af_retinaface.hip) on the current device, and of the same network
through PyTorch-ROCm fp32 (MIOpen; the functional restatement in tests/retinaface_ref.py) on the same device.

    python tools/bench_retinaface.py [--iters 20] [--warmup 3] [--batches 1,16,50] [--json out.json]

Per frame size (640x360, 1280x720, 1920x1080) and batch: frames/s from device events over `iters` back-to-back
detect_device calls after `warmup` calls; per-launch device times (af_retinaface_detect_timed: events between launches,
launch gaps included) with FLOP / byte counts from shapes and each launch's fraction of its lower bound
max(FLOP / 157.3 TFLOP/s fp32, bytes / 8 TB/s); the post-process alone (af_retinaface_postprocess_timed) on the sparse and
dense recipes' heads; and the MIOpen forward (network only, no post-process) for comparison.  Synthetic weights and frames
(synth.retinaface_state_dict / retinaface_frames)."""
import argparse
import json
import math
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

PEAK_FLOPS, PEAK_BYTES = 157.3e12, 8.0e12
SIZES = [(640, 360), (1280, 720), (1920, 1080)]


def launch_costs(w, h, b):
    """[(name, flop, bytes)] per launch in launch order for a batch of b frames (fp32 activations, 4 B)"""
    from af_mi355x import retinaface as rf
    c2 = lambda v: (v + 1) // 2
    h1, w1 = c2(h), c2(w)
    out = [("stem 3->8 s2", b * h1 * w1 * 8 * 27 * 2, b * (h * w * 3 + h1 * w1 * 8 * 4))]
    hh, ww = h1, w1
    for i, (cin, cout, st) in enumerate(rf.DW_BLOCKS, 1):
        hi, wi = hh, ww
        if st == 2:
            hh, ww = c2(hh), c2(ww)
        n = hh * ww
        out.append(("dw%d %d s%d" % (i, cin, st), b * n * cin * 9 * 2, b * (hi * wi + n) * cin * 4))
        out.append(("pw%d %d->%d" % (i, cin, cout), b * n * cin * cout * 2, b * n * (cin + cout) * 4))
    lv = [(math.ceil(h / s), math.ceil(w / s)) for s in rf.STEPS]
    px = [a * c for a, c in lv]
    out.append(("fpn out3 256->64", b * px[2] * 256 * 64 * 2, b * px[2] * (256 + 64) * 4))
    out.append(("fpn out2 128->64 +up", b * px[1] * 128 * 64 * 2, b * (px[1] * (128 + 64) + px[2] * 64) * 4))
    out.append(("fpn merge2 3x3", b * px[1] * 64 * 64 * 18, b * px[1] * 128 * 4))
    out.append(("fpn out1 64->64 +up", b * px[0] * 64 * 64 * 2, b * (px[0] * 128 + px[1] * 64) * 4))
    out.append(("fpn merge1 3x3", b * px[0] * 64 * 64 * 18, b * px[0] * 128 * 4))
    for l in range(3):
        n = px[l]
        for name, cin, cout in rf.SSH_CONVS:
            out.append(("ssh%d %s" % (l + 1, name), b * n * cin * cout * 18, b * n * (cin + cout) * 4))
        out.append(("head%d 64->32" % (l + 1), b * n * 64 * 32 * 2, b * n * (64 + 32) * 4))
    a = rf.num_anchors(h, w)
    out += [("decode", b * a * 40, b * a * (64 + 64)), ("sort", 0, b * a * 8), ("nms mask", 0, b * 5000 * 79 * 8),
            ("nms scan", 0, b * 750 * 79 * 8)]
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--batches", default="1,16,50")
    ap.add_argument("--json")
    ap.add_argument("--no-miopen", action="store_true")
    args = ap.parse_args()
    import torch
    import af_mi355x  # noqa: F401
    from af_mi355x import retinaface as rf, synth
    dev = torch.device("cuda", 0)
    res = {"device": torch.cuda.get_device_name(0), "runs": [], "post": [], "miopen": []}
    sd = synth.retinaface_state_dict(1, "sparse")
    det = rf.FaceDetector.from_state_dict(sd, gpu_id=0)
    batches = [int(v) for v in args.batches.split(",")]
    for w, h in SIZES:
        for b in batches:
            frames = torch.from_numpy(synth.retinaface_frames(min(b, 4), h, w, seed=5)).to(dev)
            frames = frames.repeat((b + frames.shape[0] - 1) // frames.shape[0], 1, 1, 1)[:b].contiguous()
            for _ in range(args.warmup):
                det.detect_device(frames)
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for _ in range(args.iters):
                det.detect_device(frames)
            e1.record()
            torch.cuda.synchronize()
            ms = e0.elapsed_time(e1) / args.iters
            t = []
            det.detect_device(frames, timings=t)
            costs = launch_costs(w, h, b)
            per = []
            for (name, fl, by), tm in zip(costs, t):
                bound = max(fl / PEAK_FLOPS, by / PEAK_BYTES) * 1e3
                per.append({"launch": name, "ms": round(tm, 4), "bound_ms": round(bound, 4),
                            "fraction": round(bound / tm, 3) if tm > 0 else None,
                            "bound": "flop" if fl / PEAK_FLOPS >= by / PEAK_BYTES else "bytes"})
            r = {"w": w, "h": h, "batch": b, "ms_per_call": round(ms, 4), "frames_per_s": round(b / ms * 1e3, 1),
                 "launches_ms_sum": round(sum(t), 4), "per_launch": per}
            res["runs"].append(r)
            print("hip %4dx%-4d B=%2d  %.3f ms/call  %.1f frames/s" % (w, h, b, ms, r["frames_per_s"]), flush=True)
    import retinaface_ref as R
    for recipe in ("sparse", "dense"):
        d2 = rf.FaceDetector.from_state_dict(synth.retinaface_state_dict(1, recipe), gpu_id=0)
        frames = torch.from_numpy(synth.retinaface_frames(16, 1080, 1920, seed=5)).to(dev)
        _, _, (loc, conf, landms) = d2.detect_device(frames, raw=True)
        loc, conf, landms = loc.contiguous(), conf.contiguous(), landms.contiguous()
        for _ in range(args.warmup):
            d2.postprocess_device(loc, conf, landms, 1080, 1920)
        t = []
        d2.postprocess_device(loc, conf, landms, 1080, 1920, timings=t)
        res["post"].append({"recipe": recipe, "w": 1920, "h": 1080, "batch": 16, "ms": [round(v, 4) for v in t],
                            "total_ms": round(sum(t), 4)})
        print("post-process %s 1080p B=16: %s ms" % (recipe, [round(v, 3) for v in t]), flush=True)
    if not args.no_miopen:
        sdd = {k: v.to(dev) for k, v in sd.items()}
        for w, h in SIZES:
            for b in batches:
                frames = torch.from_numpy(synth.retinaface_frames(1, h, w, seed=5)).to(dev).repeat(b, 1, 1, 1)
                with torch.no_grad():
                    for _ in range(args.warmup):
                        R.forward(sdd, frames, torch.float32)
                    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                    e0.record()
                    for _ in range(args.iters):
                        R.forward(sdd, frames, torch.float32)
                    e1.record()
                torch.cuda.synchronize()
                ms = e0.elapsed_time(e1) / args.iters
                res["miopen"].append({"w": w, "h": h, "batch": b, "ms_per_call": round(ms, 4), "frames_per_s": round(b / ms * 1e3, 1)})
                print("miopen %4dx%-4d B=%2d  %.3f ms/call  %.1f frames/s (network only)" % (w, h, b, ms, b / ms * 1e3), flush=True)
    if args.json:
        with open(args.json, "w") as f:
            json.dump(res, f, indent=1)


if __name__ == "__main__":
    main()
