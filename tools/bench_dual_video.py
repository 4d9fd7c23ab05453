"""dualrun at video level on one MI355X: ``DualVideoScorer.score`` on raw landmark / AU tracks against the same work done the way
the reference does it, in one process.

    python tools/bench_dual_video.py [--tracks 4] [--frames 1800] [--reps 7] [--kernel-iters 50] [--json profiles/dual_video_bench.json]

Workload: one video of `--tracks` face tracks of `--frames` frames (defaults: 4 x 1800, 449 clips of 8 frames a track, 1796 clips),
478-point landmarks and 12 AUs per frame, seeded weights, clip-mode z-score, median per track, max per video.
  kernels   device-event time of ONE af_dual_clip_features launch over all clips and ONE af_dual_video_reduce launch (fusion family,
            median / max; best family, track_median), `--kernel-iters` launches each after a warm-up; p50, min, max.
  new       host-inclusive ``score``: wall clock around the call, which ends in its read-back; staging and upload included.
  host      the reference's shape of the same work: per clip on the CPU the landmark features (numpy, ``np.linalg.norm``), the AU
            differences (``np.diff``), fixT and the clip z-score (torch), stacked, ONE upload, the same DualEncoderAU_LMK forward on
            the GPU, ``torch.median`` per track and the max on the host after one read-back.
new and host alternate `--reps` times after a warm-up of each; p50 and spread (max - min) of each leg.  No ratio is formed here.
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
sys.path.insert(0, os.path.join(ROOT, "tests"))

import numpy as np  # noqa: E402
import torch  # noqa: E402

from dualvideo_ref import KEY_IDX  # noqa: E402  (the statement's key-point table)


def _stats(v):
    return {"p50": statistics.median(v), "min": min(v), "max": max(v), "spread": max(v) - min(v), "n": len(v)}


def host_clip(lmk, aus, T=8):
    """one clip the way the reference's host code makes it: per frame features, differences, fixT, clip z-score"""
    rows = []
    for xy in lmk:
        scale = np.linalg.norm(xy[78] - xy[308])
        if not np.isfinite(scale) or scale < 1e-8:
            continue
        rows.append(((xy[list(KEY_IDX)] - xy[1]) / (scale + 1e-6)).reshape(-1).astype(np.float32))
    L = torch.from_numpy(np.stack(rows))
    d1 = np.diff(aus, axis=0, prepend=aus[:1])
    A = torch.from_numpy(np.concatenate([aus, d1, np.diff(d1, axis=0, prepend=d1[:1])], axis=-1).astype(np.float32))
    out = []
    for x in (A, L):
        if x.shape[0] > T:
            s = (x.shape[0] - T) // 2
            x = x[s:s + T]
        elif x.shape[0] < T:
            x = torch.cat([x, x[-1:].repeat(T - x.shape[0], 1)], 0)
        out.append(torch.nan_to_num((x - x.mean(0, keepdim=True)) / x.std(0, keepdim=True).clamp_min(1e-6)))
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--tracks", type=int, default=4)
    ap.add_argument("--frames", type=int, default=1800)
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--kernel-iters", type=int, default=50)
    ap.add_argument("--json", default=None)
    args = ap.parse_args()
    assert torch.cuda.is_available(), "bench_dual_video needs a GPU"
    import af_mi355x  # noqa: F401
    from af_mi355x import _lib, dual_video as DV, dualrun

    sp = dualrun.DualSpec()
    net = dualrun.DualEncoderAU_LMK(au_dim=sp.au_dim, lmk_dim=sp.lmk_dim, d_model=sp.d_model, depth=sp.depth, heads=sp.heads,
                                    mlp_ratio=float(sp.ff) / sp.d_model, pool_tau=sp.pool_tau)
    net.load_state_dict(dualrun.dual_synthetic_state_dict(sp, seed=0))
    net = net.cuda().eval()
    rng = np.random.default_rng(1)
    raw = []
    for t in range(args.tracks):
        base = rng.uniform(0.2, 0.8, (478, 2))
        base[78], base[308] = (0.4, 0.7), (0.6, 0.7)
        raw.append(((base[None] + rng.normal(0, 0.01, (args.frames, 478, 2))).astype(np.float32),
                    rng.uniform(0, 1, (args.frames, 12)).astype(np.float32), str(t)))
    videos = [[DV.DualTrack(lmk, au, key) for lmk, au, key in raw]]
    scorer = DV.DualVideoScorer(net)
    n_clips = sum(len(t.clips) for t in videos[0])
    props = torch.cuda.get_device_properties(0)
    out = {"tool": "bench_dual_video", "device": props.name, "arch": props.gcnArchName, "compute_units": props.multi_processor_count,
           "host": platform.node(), "tracks": args.tracks, "frames": args.frames, "clips": n_clips, "reps": args.reps,
           "raw_bytes": int(sum(l.nbytes + a.nbytes for l, a, _ in raw)), "chunk_clips": DV.CHUNK_CLIPS}

    # ---- the two launches alone, by device events ----
    def timed(fn, iters):
        for _ in range(5):
            fn()
        torch.cuda.synchronize()
        ms = []
        for _ in range(iters):
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            fn()
            b.record()
            b.synchronize()
            ms.append(a.elapsed_time(b))
        return _stats(ms)

    p = scorer._plan(videos)
    slot = scorer._upload(p)
    out["kernel_ms"] = {"af_dual_clip_features": timed(lambda: scorer._features(p, slot), args.kernel_iters)}
    A, L, nvalid = scorer._features(p, slot)
    with torch.inference_mode():
        logits = net(A, L)["bin_logits"].contiguous()
    nt, nv, base = p.n_reduced, p.n_videos, slot.dev.data_ptr()
    f32 = lambda n: torch.empty(n, dtype=torch.float32, device="cuda")          # noqa: E731
    i32 = lambda n: torch.empty(n, dtype=torch.int32, device="cuda")            # noqa: E731
    f64 = lambda n: torch.empty(n, dtype=torch.float64, device="cuda")          # noqa: E731
    outs = [f32(nt), f32(nt), f32(nv), f32(nv), f32(n_clips), f64(nt), i32(nt), f64(nv), i32(nv), i32(nt)]
    st = C.c_void_p(torch.cuda.current_stream().cuda_stream)

    def reduce(family, tmode):
        _lib.check(_lib.lib.af_dual_video_reduce(C.c_void_p(logits.data_ptr()), C.c_void_p(nvalid.data_ptr()), n_clips, C.c_void_p(base + p.off_vt),
                                                 nv, C.c_void_p(base + p.off_tc), nt, C.c_void_p(base + p.off_ci), family, tmode, 0, C.c_double(0.5),
                                                 *[C.c_void_p(t.data_ptr()) for t in outs], st), "af_dual_video_reduce")
    out["kernel_ms"]["af_dual_video_reduce fusion median/max"] = timed(lambda: reduce(_lib.DUALV_FAMILY_FUSION, 0), args.kernel_iters)
    out["kernel_ms"]["af_dual_video_reduce best track_median"] = timed(lambda: reduce(_lib.DUALV_FAMILY_BEST, 1), args.kernel_iters)
    slot.record()

    # ---- host-inclusive: score against the reference's shape of the same work ----
    def leg_new():
        return scorer.score(videos)[0]["logit_video"]

    def leg_host():
        As, Ls, keys = [], [], []
        for lmk, au, key in raw:
            for s in DV.clip_windows(len(lmk)):
                a, l = host_clip(lmk[s:s + 8], au[s:s + 8])
                As.append(a), Ls.append(l), keys.append(key)
        with torch.inference_mode():
            ld = net(torch.stack(As).cuda(), torch.stack(Ls).cuda())["bin_logits"].cpu()
        per_track = [ld[[i for i, k in enumerate(keys) if k == key]].median() for key in DV.person_key_order(keys)]
        return float(torch.stack(per_track).max())

    got_new, got_host = leg_new(), leg_host()                                   # warm-up of both, and the check that they agree
    out["logit_video"] = {"new": got_new, "host": got_host}
    assert abs(got_new - got_host) <= 1e-3, (got_new, got_host)
    t_new, t_host = [], []
    for _ in range(args.reps):
        for leg, acc in ((leg_new, t_new), (leg_host, t_host)):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            leg()
            acc.append((time.perf_counter() - t0) * 1e3)
    out["score_ms"] = {"new": _stats(t_new), "host": _stats(t_host)}
    line = json.dumps(out, sort_keys=True)
    print(line)
    if args.json:
        with open(args.json, "w") as fh:
            fh.write(line + "\n")


if __name__ == "__main__":
    main()
