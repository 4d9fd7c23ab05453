"""Throughput of the HIP YuNet detector (csrc/af_yunet.hip) on the current device.

    python tools/bench_yunet.py [--iters 50] [--warmup 5] [--json out.json]

Per frame size (640x360, 1280x720, 1920x1080) and batch (1, 16): frames/s from device events over `iters` back-to-back
af_yunet_detect calls after `warmup` calls; per-kernel device times (af_yunet_detect_timed: events between launches, so
launch gaps are included); FLOP and byte counts from shapes; and each launch's fraction of its lower bound
max(FLOP / 157.3 TFLOP/s fp32, bytes / 8 TB/s), naming the bound.  Kernel times from a profiler: run
`rocprofv3 --kernel-trace --stats -- python tools/bench_yunet.py` separately."""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

PEAK_FLOPS, PEAK_BYTES = 157.3e12, 8.0e12
SIZES = [(640, 360), (1280, 720), (1920, 1080)]
UNITS = [(1, 16, 16, 4, "full"), (2, 16, 32, 4, "full"), (3, 32, 32, 4, "full"), (4, 32, 64, 4, "pool"),
         (5, 64, 64, 8, "full"), (6, 64, 64, 8, "both"), (7, 64, 64, 16, "full"), (8, 64, 64, 16, "both"),
         (9, 64, 64, 32, "full"), (10, 64, 64, 32, "full"), (11, 64, 64, 32, "full"), (12, 64, 64, 16, "neck"),
         (13, 64, 64, 8, "neck")]


def launch_costs(w, h, b):
    """[(name, flop, bytes)] per launch, in launch order, for a batch of b frames (fp32 activations, 4 B)"""
    pw, ph = ((w - 1) // 32 + 1) * 32, ((h - 1) // 32 + 1) * 32
    px = lambda s: (ph // s) * (pw // s)
    out = [("stem+unit0+pool", b * (px(2) * 16 * (27 + 16 + 9) * 2), b * (h * w * 3 + px(4) * 16 * 4))]
    for u, cin, cout, s, kind in UNITS:
        n = px(s)
        fl = n * (cin * cout + 9 * cout) * 2
        by = n * cin * 4 + (n // 4 * cin * 4 if kind == "neck" else 0)
        by += {"full": n * cout * 4, "pool": n // 4 * cout * 4, "both": n * cout * 4 * 5 // 4, "neck": n * cout * 4}[kind]
        out.append(("unit%d %d->%d s%d" % (u, cin, cout, s), b * fl, b * by))
    for s in (8, 16, 32):
        n = px(s)
        out.append(("head+decode s%d" % s, b * n * (64 * 16 + 9 * 16) * 2, b * n * 64 * 4))
    anchors = px(8) + px(16) + px(32)
    out.append(("sort+nms", 0, b * 8))                 # reads the candidate count; the rest depends on the frame
    assert anchors > 0
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=50)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--json", default=None)
    args = ap.parse_args()
    import torch
    import af_mi355x  # noqa: F401
    from af_mi355x import synth
    from af_mi355x.detector import YuNet
    if not torch.cuda.is_available():
        raise SystemExit("bench_yunet needs a HIP device")
    dev = torch.device("cuda", torch.cuda.current_device())
    det = YuNet(os.path.join(ROOT, "tests", "golden", "yunet_2023mar.onnx"))
    results = []
    for w, h in SIZES:
        one = synth.synthetic_clips_u8(1, seed=7, kind="smooth", num_frames=1, size=max(w, h))[0, 0, :h, :w]
        for b in (1, 16):
            x = one.unsqueeze(0).repeat(b, 1, 1, 1).contiguous().to(dev)
            for _ in range(args.warmup):
                det.detect(x)
            torch.cuda.synchronize()
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for _ in range(args.iters):
                rows, counts = det.detect(x)
            e1.record()
            torch.cuda.synchronize()
            ms = e0.elapsed_time(e1) / args.iters
            per = []
            det.detect(x, timings=per)
            costs = launch_costs(w, h, b)
            kernels = []
            for (name, fl, by), t in zip(costs, per):
                lb_f, lb_b = fl / PEAK_FLOPS, by / PEAK_BYTES
                bound = "flop" if lb_f >= lb_b else "bytes"
                kernels.append({"kernel": name, "ms": round(t, 4), "gflop": round(fl / 1e9, 3), "mb": round(by / 1e6, 2),
                                "bound": bound, "frac_of_bound": round(max(lb_f, lb_b) * 1e3 / t, 3) if t > 0 else None})
            r = {"w": w, "h": h, "batch": b, "ms_per_call": round(ms, 4), "frames_per_s": round(b * 1e3 / ms, 1),
                 "faces_frame0": int(counts[0]), "sum_kernel_ms": round(sum(per), 4),
                 "gflop_per_frame": round(sum(c[1] for c in costs) / b / 1e9, 3), "kernels": kernels}
            results.append(r)
            print("%4dx%-4d B=%-2d %8.3f ms/call %9.1f frames/s  (%d faces in frame 0)" % (w, h, b, ms, r["frames_per_s"],
                                                                                           r["faces_frame0"]))
            for k in kernels:
                print("    %-22s %8.4f ms  %8.3f GFLOP %9.2f MB  %-5s bound, %.3f of it" % (
                    k["kernel"], k["ms"], k["gflop"], k["mb"], k["bound"], k["frac_of_bound"] or 0.0))
    print(json.dumps({"device": torch.cuda.get_device_name(dev),
                      "results": [{k: v for k, v in r.items() if k != "kernels"} for r in results]}))
    if args.json:
        with open(args.json, "w") as f:
            json.dump(results, f, indent=1)


if __name__ == "__main__":
    main()
