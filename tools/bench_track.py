"""The offline evaluator's clip loop (reference altfreezing/demo.py:304-339) on one MI355X: windows/s of TrackScorer.score_track
on a synthetic face track against what the per-clip API gives for the same windows, in one process.

    python tools/bench_track.py [--frames 400] [--reps 3] [--dtypes f16,bf16] [--json out.json]

Workload: a track of `--frames` frames (default 400, the evaluator's --max_frame: 369 windows of 32), crops of 380-460 px
(aligner.synthetic_clip), seeded weights.  Host-inclusive: wall clock around the call, ending in a device synchronise, staging
and upload included.
  new  TrackScorer.score_track: each crop uploaded once, one window-batch warp per 16 windows, forward at B = 16
  a    per window FasterCropAlignXRay(224)(..., device_output=True), sixteen stacked, forward_clips_u8 at B = 16
  b    the same at B = 1 (the reference loop's shape)
Every shape is warmed up; new / a / b alternate `--reps` times; median and spread (max - min) of each, and the crop bytes
each uploads.  `stages`: one instrumented pass of the new path (host clock for staging + upload calls and the fits, device
events for the warps and the forwards; it synchronises per batch, so its sum is not the pipelined time).
Kernel alone (`kernel`): device-event time of ONE window-batch launch of 16 windows against the sixteen
af_warp_affine_clip_u8 launches that write the same bytes from the same resident crops (their launch gaps included: that path
is bound by the host's launch rate), alternated; bytes/s over the algorithmic bytes (output + each distinct crop once).
Prints one JSON line.  A run without a GPU fails."""
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

import numpy as np  # noqa: E402
import torch  # noqa: E402


def _stats(v):
    return {"median": statistics.median(v), "spread": max(v) - min(v), "all": [round(x, 4) for x in v]}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", type=int, default=400)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--dtypes", default="f16,bf16")
    ap.add_argument("--kernel-iters", type=int, default=20)
    ap.add_argument("--json", default=None)
    args = ap.parse_args()
    assert torch.cuda.is_available(), "bench_track needs a GPU"
    import af_mi355x  # noqa: F401
    from af_mi355x import _lib, aligner, evaluator, synth
    from af_mi355x.classifier import Classifier

    infos, crops = aligner.synthetic_clip(frames=args.frames, seed=7)
    windows = evaluator.clip_windows(args.frames, 32)
    crop_bytes = [c.shape[0] * c.shape[1] * 3 for c in crops]
    sd = synth.synthetic_state_dict(seed=0)
    props = torch.cuda.get_device_properties(0)
    out = {"tool": "bench_track", "device": props.name, "arch": props.gcnArchName, "compute_units": props.multi_processor_count,
           "hbm_gib": round(props.total_memory / 2 ** 30), "host": platform.node(), "frames": args.frames, "windows": len(windows), "reps": args.reps,
           "crop_bytes_total": int(sum(crop_bytes)), "dtypes": {}}

    def sync():
        torch.cuda.synchronize()

    for dtype in args.dtypes.split(","):
        clf = Classifier(precision=dtype)
        clf.network.load_state_dict(sd)
        clf = clf.cuda().eval()
        net = clf.network
        scorer = evaluator.TrackScorer(net)
        al = aligner.FasterCropAlignXRay(224)

        def run_new():
            return scorer.score_track(infos, crops)

        def run_per_clip(B):
            res, up = [], 0
            with torch.inference_mode():
                for lo in range(0, len(windows), B):
                    clips = []
                    for w in windows[lo:lo + B]:
                        _, clip = al([infos[j] for j in w], [crops[j] for j in w], device_output=True)
                        clips.append(clip)
                        up += sum(crop_bytes[j] for j in w)           # an upper bound: the aligner cuts rows the warp cannot reach
                    res.append(net.forward_clips_u8(torch.stack(clips), return_scores=True)["scores"])
            return torch.cat(res).float().cpu().numpy(), up

        # warm up every shape (engines at 16, 1 and the short last batches), and check the three paths agree
        s_new = run_new(); sync()
        s_a, up_a = run_per_clip(16); sync()
        s_b, up_b = run_per_clip(1); sync()
        agree = {"new_vs_a": float(np.abs(s_new - s_a).max()), "new_vs_b": float(np.abs(s_new - s_b).max())}
        t = {"new": [], "a": [], "b": []}
        for _ in range(args.reps):
            for name, fn in (("new", run_new), ("a", lambda: run_per_clip(16)), ("b", lambda: run_per_clip(1))):
                sync()
                t0 = time.perf_counter()
                fn()
                sync()
                t[name].append(len(windows) / (time.perf_counter() - t0))
        res = {k: _stats(v) for k, v in t.items()}
        res["uploaded_bytes"] = {"new": int(scorer.uploaded_bytes), "a": int(up_a), "b": int(up_b)}
        res["max_abs_score_difference"] = agree
        res["new_above_a_by_more_than_spread"] = bool(res["new"]["median"] - res["a"]["median"] > max(res["new"]["spread"], res["a"]["spread"]))

        # one instrumented pass of the new path
        track = evaluator._Track(infos, crops)
        st = {"stage_and_upload_host_ms": 0.0, "fits_host_ms": 0.0, "table_and_launch_host_ms": 0.0, "warp_device_ms": 0.0, "forward_device_ms": 0.0}
        with torch.inference_mode():
            sync(); t0 = time.perf_counter()
            offs = scorer._upload(track, 0, track.n)
            sync(); st["stage_and_upload_host_ms"] = (time.perf_counter() - t0) * 1e3
            for first, n, run in scorer.partition(len(windows)):
                batch = windows[first:first + n]
                t0 = time.perf_counter()
                fits = [evaluator._fit(track, idx, scorer.std_points) for idx in batch]
                st["fits_host_ms"] += (time.perf_counter() - t0) * 1e3
                batch, fits = batch + [batch[-1]] * (run - n), fits + [fits[-1]] * (run - n)
                e = [torch.cuda.Event(enable_timing=True) for _ in range(3)]
                t0 = time.perf_counter()
                e[0].record()
                scorer.warp(track, batch, offs, 0, scorer._clips[0][:run], fits)
                e[1].record()
                st["table_and_launch_host_ms"] += (time.perf_counter() - t0) * 1e3
                net.forward_clips_u8(scorer._clips[0][:run], return_scores=True)
                e[2].record()
                sync()
                st["warp_device_ms"] += e[0].elapsed_time(e[1])
                st["forward_device_ms"] += e[1].elapsed_time(e[2])
        res["stages"] = {k: round(v, 3) for k, v in st.items()}
        out["dtypes"][dtype] = res

        if "kernel" not in out:                                   # the warp does not depend on the classifier's dtype
            n16 = windows[:16]
            last = max(max(w) for w in n16) + 1
            fits = [evaluator._fit(track, idx, scorer.std_points) for idx in n16]
            buf_new, buf_old = scorer._clips[0], scorer._clips[1]
            stream = C.c_void_p(torch.cuda.current_stream().cuda_stream)
            scorer.warp(track, n16, offs, 0, buf_new, fits)          # leaves the batch's table in the slot it used
            table = scorer.warp.tables.last.dev.clone()
            sync()

            def launch_new():
                _lib.check(_lib.lib.af_warp_affine_windows_u8(C.c_void_p(scorer.source.dev.data_ptr()), C.c_void_p(table.data_ptr()), 16, 32, 224,
                                                              C.c_void_p(buf_new.data_ptr()), stream), "warp_affine_windows_u8")

            def launch_old():
                for w, (idx, (tfm, h, wd, diff)) in enumerate(zip(n16, fits)):
                    al.launch_warps(scorer.source.dev, [int(offs[j]) for j in idx], [crops[j].shape for j in idx], diff, h, wd, tfm, buf_old[w])

            def timed(fn):
                a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                a.record(); fn(); b.record(); sync()
                return a.elapsed_time(b)

            for fn in (launch_new, launch_old):
                fn(); sync()
            same = bool(torch.equal(buf_new, buf_old))
            k = {"window_batch_launch": [], "sixteen_single_clip_launches": []}
            for _ in range(args.kernel_iters):
                k["window_batch_launch"].append(timed(launch_new))
                k["sixteen_single_clip_launches"].append(timed(launch_old))
            alg = 16 * 32 * 224 * 224 * 3 + int(sum(crop_bytes[:last]))
            out["kernel"] = {"ms": {n: _stats(v) for n, v in k.items()}, "same_bytes_as_single_clip_launches": same, "algorithmic_bytes": alg,
                             "bytes_per_s": {n: alg / (statistics.median(v) * 1e-3) for n, v in k.items()}}
        del scorer, clf, net
        torch.cuda.empty_cache()

    line = json.dumps(out)
    print(line)
    if args.json:
        with open(args.json, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
