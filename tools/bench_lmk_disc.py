"""cli/test.py's LMKDisc path on one MI355X: ``LmkVideoScorer.score`` on raw landmark tracks against the same work done the way
the reference does it, in one process.

    python tools/bench_lmk_disc.py [--tracks 4] [--frames 1800] [--reps 7] [--kernel-iters 50] [--json profiles/lmk_disc_bench.json]

Workload (tools/bench_dual_video.py's shape): one video of `--tracks` face tracks of `--frames` frames (defaults: 4 x 1800, 449 clips
of 8 frames a track, 1796 clips), 478-point landmarks, seeded ``LMKDisc`` weights (four layers, dim_ff 512), no rotation.
  kernels   device-event time of ONE launch each over all clips: af_dual_clip_features_ex (landmarks alone, zero padding),
            af_dual_branch_encoders (one branch), af_dual_head (n = 256), af_lmk_video_reduce; `--kernel-iters` launches each after a
            warm-up; p50, min, max.
  new       host-inclusive ``score``: wall clock around the call, which ends in its read-back; staging and upload included.
  host      the reference's shape of the same work: per clip on the CPU the landmark features (numpy, ``np.linalg.norm``), zero
            padding and the mask (``collate_pad``), ONE upload, the same LMKDisc forward on the GPU, sigmoid, ``np.median`` per track
            and noisy-OR on the host after one read-back.
new and host alternate `--reps` times after a warm-up of each; p50 and spread (max - min) of each leg.  ``encoder_share_of_score`` is
the encoder launch's device p50 over ``score``'s host-inclusive p50: the number that decides whether batching clips into one M = 128
problem is worth building.  Nothing is gated on these figures.  Prints one JSON line.  A run without a GPU fails."""
import argparse
import ctypes as C
import json
import os
import platform
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, os.path.join(ROOT, "tools"))

import numpy as np  # noqa: E402
import torch  # noqa: E402

from bench_dual_video import _stats  # noqa: E402
from dualvideo_ref import KEY_IDX  # noqa: E402  (the statement's key-point table)


def host_clip(lmk):
    """one clip's surviving rows the way make_lmk_features.py makes them"""
    rows = []
    for xy in lmk:
        scale = np.linalg.norm(xy[78] - xy[308])
        if not np.isfinite(scale) or scale < 1e-8:
            continue
        rows.append(((xy[list(KEY_IDX)] - xy[1]) / (scale + 1e-6)).reshape(-1).astype(np.float32))
    return np.stack(rows)


def collate_pad(batch, T):
    out = torch.zeros(len(batch), T, batch[0].shape[1])
    pad = torch.ones(len(batch), T, dtype=torch.bool)
    for i, x in enumerate(batch):
        out[i, :x.shape[0]] = torch.from_numpy(x)
        pad[i, :x.shape[0]] = False
    return out, pad


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--tracks", type=int, default=4)
    ap.add_argument("--frames", type=int, default=1800)
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--kernel-iters", type=int, default=50)
    ap.add_argument("--json", default=None)
    args = ap.parse_args()
    assert torch.cuda.is_available(), "bench_lmk_disc needs a GPU"
    import af_mi355x  # noqa: F401
    from af_mi355x import _lib, dual_video as DV, dualrun

    net = dualrun.LMKDisc(132)
    net.load(dualrun.lmk_disc_synthetic_state_dict(132, seed=0))
    net = net.cuda().eval()
    rng = np.random.default_rng(1)
    raw = []
    for t in range(args.tracks):
        base = rng.uniform(0.2, 0.8, (478, 2))
        base[78], base[308] = (0.4, 0.7), (0.6, 0.7)
        raw.append(((base[None] + rng.normal(0, 0.01, (args.frames, 478, 2))).astype(np.float32), "track_%d" % t))
    videos = [[DV.DualTrack(lmk, None, key) for lmk, key in raw]]
    scorer = DV.LmkVideoScorer(net)
    n_clips = sum(len(t.clips) for t in videos[0])
    props = torch.cuda.get_device_properties(0)
    out = {"tool": "bench_lmk_disc", "device": props.name, "arch": props.gcnArchName, "compute_units": props.multi_processor_count,
           "host": platform.node(), "tracks": args.tracks, "frames": args.frames, "clips": n_clips, "reps": args.reps,
           "raw_bytes": int(sum(l.nbytes for l, _ in raw)), "chunk_clips": DV.CHUNK_CLIPS}
    assert n_clips <= DV.CHUNK_CLIPS, "the kernel timings below are of one forward over all clips"

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

    # ---- the four launches alone, by device events ----
    p = scorer._plan(videos)
    slot = scorer._upload(p)
    out["kernel_ms"] = {"af_dual_clip_features_ex": timed(lambda: scorer._features(p, slot), args.kernel_iters)}
    L, nvalid = scorer._features(p, slot)
    sp, T, D = net.spec, scorer.T, net.spec.d_model
    branch, head = net._pack(L.device)
    pe = dualrun.sinusoid_table(T, D).cuda()
    lengths = nvalid.clamp(min=1).contiguous()
    z = torch.empty((n_clips, D), dtype=torch.float32, device="cuda")
    logits = torch.empty((n_clips,), dtype=torch.float32, device="cuda")
    st = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    xp, wp, dins = (C.c_void_p * 1)(L.data_ptr()), (C.c_void_p * 1)(branch.data_ptr()), (C.c_int * 1)(sp.lmk_dim)

    def encoder():
        _lib.check(_lib.lib.af_dual_branch_encoders(1, xp, wp, dins, C.c_void_p(lengths.data_ptr()), C.c_void_p(pe.data_ptr()), n_clips, T, D,
                                                    sp.depth, sp.heads, sp.ff, C.c_float(sp.pool_tau), C.c_void_p(z.data_ptr()), D, st),
                   "af_dual_branch_encoders")

    def head_launch():
        _lib.check(_lib.lib.af_dual_head(C.c_void_p(z.data_ptr()), C.c_void_p(head.data_ptr()), n_clips, D, C.c_void_p(logits.data_ptr()), st),
                   "af_dual_head")
    out["kernel_ms"]["af_dual_branch_encoders"] = timed(encoder, args.kernel_iters)
    out["kernel_ms"]["af_dual_head"] = timed(head_launch, args.kernel_iters)
    with torch.inference_mode():
        assert torch.equal(logits, net.forward_lengths(L, lengths))
    nt, nv, base = p.n_reduced, p.n_videos, slot.dev.data_ptr()
    i32 = lambda n: torch.empty(n, dtype=torch.int32, device="cuda")            # noqa: E731
    f64 = lambda n: torch.empty(n, dtype=torch.float64, device="cuda")          # noqa: E731
    outs = [f64(n_clips), f64(nt), i32(nt), i32(nt), f64(nv), i32(nv), i32(nv)]

    def reduce():
        _lib.check(_lib.lib.af_lmk_video_reduce(C.c_void_p(logits.data_ptr()), C.c_void_p(nvalid.data_ptr()), n_clips, C.c_void_p(base + p.off_vt),
                                                nv, C.c_void_p(base + p.off_tc), nt, C.c_void_p(base + p.off_ci), 0, C.c_double(0.5),
                                                *[C.c_void_p(t.data_ptr()) for t in outs], st), "af_lmk_video_reduce")
    out["kernel_ms"]["af_lmk_video_reduce"] = timed(reduce, args.kernel_iters)
    slot.record()

    # ---- host-inclusive: score against the reference's shape of the same work ----
    def leg_new():
        return scorer.score(videos)[0]["score_video_or"]

    def leg_host():
        rows, keys = [], []
        for lmk, key in raw:
            for s in DV.clip_windows(len(lmk)):
                rows.append(host_clip(lmk[s:s + 8]))
                keys.append(key)
        X, pad = collate_pad(rows, T)
        with torch.inference_mode():
            s = torch.sigmoid(net(X.cuda(), key_padding_mask=pad.cuda())).clamp(0, 1).cpu().tolist()
        bins = {}
        for k, v in zip(keys, s):
            bins.setdefault(k, []).append(float(v))
        pt = np.clip(np.asarray([float(np.median(v)) for v in bins.values()], np.float64), 1e-6, 1 - 1e-6)
        return float(1.0 - np.exp(np.log1p(-pt).sum()))

    got_new, got_host = leg_new(), leg_host()                                   # warm-up of both, and the check that they agree
    out["score_video_or"] = {"new": got_new, "host": got_host}
    assert abs(got_new - got_host) <= 1e-5, (got_new, got_host)
    t_new, t_host = [], []
    for _ in range(args.reps):
        for leg, acc in ((leg_new, t_new), (leg_host, t_host)):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            leg()
            acc.append((time.perf_counter() - t0) * 1e3)
    out["score_ms"] = {"new": _stats(t_new), "host": _stats(t_host)}
    out["encoder_share_of_score"] = out["kernel_ms"]["af_dual_branch_encoders"]["p50"] / out["score_ms"]["new"]["p50"]
    line = json.dumps(out, sort_keys=True)
    print(line)
    if args.json:
        with open(args.json, "w") as fh:
            fh.write(line + "\n")


if __name__ == "__main__":
    main()
