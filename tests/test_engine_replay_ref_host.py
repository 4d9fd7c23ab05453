"""No GPU: the replay's windowed fp64 reference (engine_replay_ref.Reference over engine_graph) reproduces the CPU oracle.

Shrunken networks (8 or 16 frames, 64 x 64) with synthetic weights, two clips.  The oracle (oracle/i3d_oracle.py, F.conv3d in fp64)
runs stem by stem and block by block; each of its outputs is handed to the Reference as the snapshot of that graph tensor, and the
Reference's value of the next graph tensor on the replay's own windows must equal the oracle's to fp64 rounding: tap order, stride,
padding, BN, pool_after_bn, the pools, the block's add, the lateral's concatenation and the even-(h, w) restriction are all the
graph's.  In fp32 "storage" the weights are not rounded, so nothing but fp64 summation order differs (asserted at 1e-10).  The folded
form (scale into the weights in fp32) is the same function up to fp32 rounding of the weights (asserted at 1e-5)."""
import os
import sys

import torch

from conftest import ROOT

sys.path.insert(0, os.path.join(ROOT, "oracle"))
import i3d_oracle as oracle  # noqa: E402
import engine_graph  # noqa: E402
import engine_replay_ref as ref  # noqa: E402
from af_mi355x import arch, synth  # noqa: E402

N = 2


def _nd(x):
    return x.permute(0, 2, 3, 4, 1).contiguous()


def _input(shape, seed):
    return torch.randn(shape, generator=torch.Generator().manual_seed(seed), dtype=torch.float64)


def _check(R, name, made, want_ncdhw, folded=(), tol=1e-10, sub=1):
    want_all = _nd(want_ncdhw)
    dims = tuple(want_all.shape[1:4])
    assert dims == R.g[name].dims and want_all.shape[4] == R.g[name].ch, (name, want_all.shape, R.g[name])
    pos = ref.rows_to_pos(ref.window_rows(N, *dims, seed=7), dims, "cpu")
    if sub == 2:
        pos = pos[(pos[:, 2] % 2 == 0) & (pos[:, 3] % 2 == 0)]
    got = R.value(name, pos, (set(made), set(), set(folded)))
    want = want_all[pos[:, 0], pos[:, 1], pos[:, 2], pos[:, 3]]
    ratio, top, share = ref.compare(got, want, name)
    assert ratio <= tol and top > 0, (name, ratio)
    R.put(name, want_all)


def _blocks(R, stage, x, sd, block_fn, fold_tol=None):
    for blk in stage.blocks:
        made = [cv.conv for cv in (blk.branch1, blk.a, blk.b, blk.c) if cv is not None] + [blk.name]
        y = block_fn(x, blk)
        _check(R, blk.name, made, y)
        if blk.branch1 is not None and blk.branch1.pool_after_bn is None:
            _check(R, blk.name, made, y, folded=(blk.c.conv, blk.branch1.conv), tol=1e-5)
        x = y
    return x


def test_i3d_graph_and_reference_reproduce_the_oracle():
    spec = arch.i3d_r50_spec(8, 64)
    sd = {k: v.double() for k, v in synth.synthetic_state_dict(spec, seed=3).items()}
    g = engine_graph.build(spec)
    R = ref.Reference(g, sd, "f32", "cpu")
    x = _input((N, 3, 8, 64, 64), 1)
    R.put("input", _nd(x))
    _check(R, spec.stem.conv, [spec.stem.conv], oracle.conv_bn_act(x, sd[spec.stem.conv + ".weight"], sd, spec.stem.bn, (1, 2, 2), (2, 3, 3), True))
    x = oracle.stem(x, sd)
    _check(R, "stem_pool", ["stem_pool"], x)
    _check(R, "stem_pool", [spec.stem.conv, "stem_pool"], x)           # the fused stem launches: conv and pool in one
    for si, stage in enumerate(spec.stages):
        stride = 1 if si == 0 else 2
        x = _blocks(R, stage, x, sd, lambda x, blk: oracle.res_block(x, sd, blk.name, stride if blk is stage.blocks[0] else 1))
        if si == 0:
            last = stage.blocks[-1]
            p = torch.nn.functional.max_pool3d(x, (2, 1, 1), (2, 1, 1))
            # the pool rides behind the last block (tpool = 1) or is a launch of its own
            _check(R, "pool_after_s2", [last.a.conv, last.b.conv, last.c.conv, last.name, "pool_after_s2"], p)
            _check(R, "pool_after_s2", ["pool_after_s2"], p)
            x = p
            # s3's stride-(1,2,2) shortcut over the even-(h, w) restriction (x_sub = 2) is the same function
            b0 = spec.stages[1].blocks[0]
            R.put("pool_after_s2", _nd(p)[:, :, ::2, ::2].contiguous(), sub=2)
            want = oracle.conv_bn_act(p, sd[b0.branch1.conv + ".weight"], sd, b0.branch1.bn, (1, 2, 2), (0, 0, 0), False)
            _check(R, b0.branch1.conv, [b0.branch1.conv], want)
            R.put("pool_after_s2", _nd(p))
    assert tuple(x.shape) == (N, 2048, 4, 2, 2)
    R.put(spec.stages[-1].blocks[-1].name, _nd(x))
    pooled = R.avgpool("pooled")
    want = torch.nn.functional.avg_pool3d(x, spec.head_pool, stride=1)
    assert torch.allclose(pooled.view(N, -1), want.view(N, -1), rtol=0, atol=1e-12)
    logits = R.linear(pooled, spec.head).reshape(N, -1)
    assert torch.allclose(logits, oracle.head(x, sd, spec.head_pool), rtol=0, atol=1e-12)


def test_ftcn_graph_and_reference_reproduce_the_oracle():
    spec = arch.ftcn_tt_spec(8, 64)
    sd = {k: (v.double() if v.is_floating_point() else v) for k, v in synth.synthetic_state_dict(spec, seed=4).items()}
    g = engine_graph.build(spec)
    R = ref.Reference(g, sd, "f32", "cpu")
    x = _input((N, 3, 8, 64, 64), 2)
    R.put("input", _nd(x))
    x = oracle.ftcn_stem(x, sd)
    _check(R, "stem_pool", [spec.stem.conv, "stem_pool"], x)             # tstem_pool3: conv, BN, 1x2x2 pool, ReLU, 1x3x3 pool
    for si, stage in enumerate(spec.stages):
        x = _blocks(R, stage, x, sd, lambda x, blk: oracle.ftcn_block(x, sd, blk.name))
        if si == 0:
            x = torch.nn.functional.max_pool3d(x, (2, 1, 1), (2, 1, 1))
            _check(R, "pool_after_s2", ["pool_after_s2"], x)
    R.put(spec.stages[-1].blocks[-1].name, _nd(x))
    tok = R.avgpool("tokens")
    want = torch.nn.functional.avg_pool3d(x, (1, x.shape[3], x.shape[4])).reshape(N, x.shape[1], x.shape[2]).permute(0, 2, 1)
    assert torch.allclose(tok, want, rtol=0, atol=1e-12)


def test_slowfast_graph_and_reference_reproduce_the_oracle():
    spec = arch.slowfast_r50_spec(16, 64)
    sd = {k: v.double() for k, v in synth.synthetic_state_dict(spec, seed=5).items()}
    g = engine_graph.build(spec)
    R = ref.Reference(g, sd, "f32", "cpu")
    xf = _input((N, 3, 16, 64, 64), 3)
    xs = xf[:, :, ::spec.alpha].contiguous()
    R.put("input_slow", _nd(xs)); R.put("input_fast", _nd(xf))
    xs, xf = oracle.stem(xs, sd, "resnet.s1.pathway0_stem"), oracle.stem(xf, sd, "resnet.s1.pathway1_stem")
    _check(R, "stem_pool0", [spec.stems[0].conv, "stem_pool0"], xs)
    _check(R, "stem_pool1", [spec.stems[1].conv, "stem_pool1"], xf)

    def fuse(fz, xs, xf):
        cat = oracle.fuse_fast_to_slow(xs, xf, sd, engine_graph.fuse_name(fz), spec.alpha)
        _check(R, fz.conv, [fz.conv], cat[:, xs.shape[1]:])
        pos = ref.rows_to_pos(ref.window_rows(N, *g[fz.conv].dims, seed=1), g[fz.conv].dims, "cpu")
        assert torch.equal(R.gather(engine_graph.fuse_name(fz), pos), _nd(cat)[pos[:, 0], pos[:, 1], pos[:, 2], pos[:, 3]])
        return cat

    xs = fuse(spec.fuses[0], xs, xf)
    for si, (slow, fast) in enumerate(spec.stages):
        stride = 1 if si == 0 else 2
        xs = _blocks(R, slow, xs, sd, lambda x, blk: oracle.res_block(x, sd, blk.name, stride if blk is slow.blocks[0] else 1))
        xf = _blocks(R, fast, xf, sd, lambda x, blk: oracle.res_block(x, sd, blk.name, stride if blk is fast.blocks[0] else 1))
        if si + 1 < len(spec.fuses):
            xs = fuse(spec.fuses[si + 1], xs, xf)
    assert (xs.shape[1], xf.shape[1]) == (2048, 256)


def test_windows_are_what_the_replay_states():
    rows = ref.window_rows(16, 16, 28, 28, seed=5)
    R = 16 * 16 * 28 * 28
    assert rows == sorted(set(rows)) and 150 <= len(rows) <= 400 and rows[:4] == [0, 1, 2, 3] and rows[-4:] == list(range(R - 4, R))
    for m in (128, 224, 256, 512):
        last = (R - 1) // m
        for k in (1, last // 2, last):
            assert {k * m - 2, k * m - 1, k * m, k * m + 1} <= set(rows), (m, k)
    frame = 28 * 28
    for n in (0, 14):          # the last frame of clip n and the first frame of clip n + 1, one interior pixel
        assert ((n + 1) * 16 - 1) * frame + 14 * 28 + 14 in rows and (n + 1) * 16 * frame + 14 * 28 + 14 in rows
    for r in (0, 27, 27 * 28, frame - 1, 15 * frame, 15 * 16 * frame, R - 1):       # corners of the first and the last clip
        assert r in rows, r
    assert ref.window_rows(1, 1, 1, 1, seed=0) == [0]
