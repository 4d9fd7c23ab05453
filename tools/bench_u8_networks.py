"""The uint8 input path of SlowFast and FTCN-TT on one MI355X, in one process.

    python tools/bench_u8_networks.py [--batch 16] [--dtype bf16] [--reps 30] [--steps 10] [--networks slowfast,ftcn] [--json out.json]

pack     device time (hipEvents around each op, af_run_ops_timed) of the ONE af_pack_input_u8_pathways launch that writes both
         SlowFast inputs of `--batch` clips of 32 x 224 x 224, alpha 8, against the two existing launches that write the same bytes:
         af_pack_input_u8_rgb3 on a pre-strided copy of every 8th frame (16-bit; f32: af_pack_input_u8) + af_pack_input_u8 on the
         clip.  The strided copy itself is NOT timed.  The two forms alternate `--reps` times after a warm-up; median and spread
         (max - min); bytes/s over the algorithmic bytes (the clip read once + the interior cells of both outputs written once).
networks clips/s of forward_clips_u8 on resident uint8 clips against forward() on the resident normalised fp32 tensor (the figure
         the fp32-input benchmarks report) and against normalize_like_callers on the device + forward() (what a caller without the
         uint8 path runs), host clock around `--steps` forwards ending in a synchronise, alternated `--reps` // 5 times.
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

import torch  # noqa: E402


def _stats(v):
    return {"median": statistics.median(v), "spread": max(v) - min(v), "min": min(v), "max": max(v), "n": len(v)}


def bench_pack(batch, dtype, reps):
    from af_mi355x import _lib, synth
    lib, code = _lib.lib, _lib.DTYPE_CODES[dtype]
    n, t, h, w, alpha = batch, 32, 224, 224, 8
    slow3 = dtype != "f32"
    clip = torch.randint(0, 256, (n, t, h, w, 3), dtype=torch.uint8, device="cuda")
    strided = clip[:, ::alpha].contiguous()
    slow_bytes = int((lib.af_stem_input_bytes_rgb3 if slow3 else lib.af_stem_input_bytes)(n, t // alpha, h, w, code))
    fast_bytes = int(lib.af_stem_input_bytes(n, t, h, w, code))
    bufs = {k: (torch.zeros(slow_bytes, dtype=torch.uint8, device="cuda"), torch.zeros(fast_bytes, dtype=torch.uint8, device="cuda"))
            for k in ("one", "two")}
    mean, std = (v.tolist() for v in synth.pixel_mean_std_f32())

    def pack_op(op, kind, src, frames, out):
        op.kind, op.in_, op.out = kind, src.data_ptr(), out.data_ptr()
        op.conv.n, op.conv.t, op.conv.h, op.conv.w, op.conv.dtype = n, frames, h, w, code
        for i in range(3):
            op.mean[i], op.std_[i] = mean[i], std[i]

    one = (_lib.Op * 1)()
    pack_op(one[0], _lib.AF_OP_PACK_PATHWAYS_U8, clip, t, bufs["one"][0])
    one[0].aux, one[0].x_sub, one[0].pack_rgb3 = bufs["one"][1].data_ptr(), alpha, int(slow3)
    two = (_lib.Op * 2)()
    pack_op(two[0], _lib.AF_OP_PACK3_U8 if slow3 else _lib.AF_OP_PACK_U8, strided, t // alpha, bufs["two"][0])
    pack_op(two[1], _lib.AF_OP_PACK_U8, clip, t, bufs["two"][1])
    stream = C.c_void_p(torch.cuda.current_stream().cuda_stream)

    def timed(ops, k):
        ms = (C.c_float * k)()
        _lib.check(lib.af_run_ops_timed(ops, k, stream, ms), "af_run_ops_timed")
        return float(sum(ms))

    for _ in range(3):
        timed(one, 1), timed(two, 2)
    same = bool(torch.equal(bufs["one"][0], bufs["two"][0]) and torch.equal(bufs["one"][1], bufs["two"][1]))
    ms = {"pathways_one_launch": [], "two_existing_launches": []}
    for _ in range(reps):
        ms["pathways_one_launch"].append(timed(one, 1))
        ms["two_existing_launches"].append(timed(two, 2))
    es = 4 if dtype == "f32" else 2
    px = n * t * h * w
    written = px * 4 * es + (px // alpha) * (3 * es if slow3 else 4 * es)
    alg = {"pathways_one_launch": px * 3 + written, "two_existing_launches": px * 3 + (px // alpha) * 3 + written}
    return {"shape": [n, t, h, w], "alpha": alpha, "dtype": dtype, "slow_layout": "rgb3" if slow3 else "c4", "fast_layout": "c4",
            "same_bytes": same, "ms": {k: _stats(v) for k, v in ms.items()}, "algorithmic_bytes": alg,
            "bytes_per_s": {k: alg[k] / (statistics.median(v) * 1e-3) for k, v in ms.items()}}


def bench_network(kind, batch, dtype, steps, rounds):
    from af_mi355x import arch, synth
    from af_mi355x.classifier import FtcnTT8x8, SlowFast8x8
    net = (SlowFast8x8 if kind == "slowfast" else FtcnTT8x8)(precision=dtype)
    net.load_state_dict(synth.synthetic_state_dict(arch.slowfast_r50_spec() if kind == "slowfast" else arch.ftcn_tt_spec(), seed=0))
    net = net.cuda().eval()
    u8 = synth.synthetic_clips_u8(batch, seed=2026, kind="uniform").cuda()
    x = synth.normalize_like_callers(u8)
    forms = {"u8": lambda: net.forward_clips_u8(u8), "f32_resident": lambda: net(x),
             "f32_with_normalisation": lambda: net(synth.normalize_like_callers(u8))}
    rates = {k: [] for k in forms}
    with torch.inference_mode():
        for fn in forms.values():
            for _ in range(3):
                fn()
        torch.cuda.synchronize()
        same = bool(torch.equal(forms["u8"]()["final_output"], forms["f32_resident"]()["final_output"]))
        for _ in range(rounds):
            for k, fn in forms.items():
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                for _ in range(steps):
                    fn()
                torch.cuda.synchronize()
                rates[k].append(batch * steps / (time.perf_counter() - t0))
    return {"batch": batch, "dtype": dtype, "steps": steps, "u8_logits_equal_f32_input_logits": same,
            "clips_per_s": {k: _stats(v) for k, v in rates.items()}}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=16)
    ap.add_argument("--dtype", default="bf16")
    ap.add_argument("--reps", type=int, default=30)
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--networks", default="slowfast,ftcn")
    ap.add_argument("--json", default=None)
    args = ap.parse_args()
    assert torch.cuda.is_available(), "bench_u8_networks needs a GPU"
    assert args.reps >= 20, "at least 20 repetitions"
    import af_mi355x  # noqa: F401
    props = torch.cuda.get_device_properties(0)
    out = {"tool": "bench_u8_networks", "device": props.name, "arch": props.gcnArchName, "compute_units": props.multi_processor_count,
           "host": platform.node(), "reps": args.reps, "pack": bench_pack(args.batch, args.dtype, args.reps), "networks": {}}
    for kind in [k for k in args.networks.split(",") if k]:
        out["networks"][kind] = bench_network(kind, args.batch, args.dtype, args.steps, max(args.reps // 5, 3))
        torch.cuda.empty_cache()
    line = json.dumps(out)
    print(line)
    if args.json:
        with open(args.json, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
