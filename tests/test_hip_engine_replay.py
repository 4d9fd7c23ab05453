"""GPU: every launch of the engine against fp64, teacher-forced by graph name.

The kernels have their own fp64 tests and the plans their digests; here the two meet.  Per case one forward is run normally, then
the same bound forward is stepped launch by launch (Engine.run_ops).  Around every launch:
  * an integer checksum of every activation buffer, of `pooled`, `logits` and `tokens_pooled` is taken: only the buffers the launch
    names as dst / dst_a (and the head's own outputs) may change; in rows wider than the launch's channels (SlowFast's concatenated
    rows) the other channels of the sampled rows are bit-equal to what their producer stored;
  * each stored graph tensor (engine_graph.py) is snapshotted under its graph name and dropped behind its last graph reader;
  * for every tensor the launch stores, engine_replay_ref.Reference computes in fp64 the value the GRAPH says it is, on the windows
    of engine_replay_ref.window_rows, from the snapshots looked up by graph name - never from the buffers the launch was bound to -
    with weights and BN from the state dict by the conv's own name.  Wrong wiring, a clobbered buffer and a mis-bound weight all show
    up as a mismatch at the launch that suffers from them.  Tolerances are the kernel tests' own (engine_replay_ref.TOL);
  * not vacuous: at least 10 % of the reference values on the windows are non-zero and max|want| >= 0.25.
The heads are compared dense.  After the last step the logits equal those of the normal run bit for bit.
test_replay_reports_a_misbound_bn_at_its_launch binds one s3 `a` conv's BN vectors to its neighbour's: the replay reports exactly
that launch.

Measured on one MI355X (gfx950, 256 CUs), all 17 tests in 12 s.  Seconds per case (engine, clips, both forwards, references):
    i3d_r50   bf16 b1 1.6 (the first: weights and clips)  b4 0.4  b16 1.2   f16 b16 1.2   f32 b1 0.2   CPA b16 1.2   BC b16 1.0
    ftcn_tt   bf16 b1 0.2  b4 0.4  b16 1.2   f16 b4 0.4   f32 b1 0.2
    slowfast  bf16 b1 0.5  b16 1.1   f16 b1 0.3   f32 b1 0.3
so nothing was cut from the windows (69 - 184 distinct positions per tensor, all channels each).  Over all compared tensors the
smallest max|want| was 1.14 and the smallest non-zero share 0.33.  Worst max|d| / max|want| per (kind, variant) over the cases,
f32 / f16 / bf16 (tolerance):
    conv  conv_igemm, 7 tiles    1.4e-6 / 4.5e-4 / 3.7e-3  (2e-6 / 1.5e-3 / 1.2e-2; the f32 worst is the 64x128 tile)
    conv  conv111                   -   / 4.0e-4 / 3.6e-3      conv  conv311_c64   9.5e-7 / 3.3e-4 / 3.4e-3
    conv  conv133_c64               -   / 4.1e-4 / 3.7e-3      conv  conv311g         -   / 4.1e-4 / 3.7e-3
    conv  conv133g                  -   / 4.0e-4 / 3.6e-3      conv  conv_small       -   / 3.9e-4 / 3.1e-3
    stem                         1.1e-6 / 3.3e-4 / 3.5e-3      stem3_pool             -   / 4.3e-4 / 3.1e-3
    tstem                        1.5e-7 /    -   /    -        tstem_pool3            -   / 2.5e-4 / 2.7e-3
    pool                         0 / 0 / 0
    dual  conv_igemm, 4 tiles    1.2e-6 / 4.7e-4 / 3.4e-3  (5e-6 / 3e-3 / 2.4e-2)
    ca    trunk                     -   / 3.8e-4 / 3.0e-3  (1.5e-3 / 1.2e-2)     a   3.9e-4 / 3.3e-3  (2.25e-3 / 1.8e-2)
    cpa   trunk                     -   /    -   / 2.7e-3  (1.2e-2)              a      -   / 2.8e-3  (1.8e-2)
    bc                              -   /    -   / 2.9e-3  (1.6e-2)
    abc   (both forms)              -   / 4.0e-4 / 3.2e-3  (3e-3 / 2.4e-2)
    heads, as a share of their fp32 bound: pooled <= 5.3e-3, tokens <= 9.3e-3, logits <= 7.9e-4; FTCN-TT logits <= 7.9e-7 of 5e-5
No launch needs more than its kernel test's tolerance on real activations; every 16-bit figure is the storage rounding of the
output itself (2^-9 for bf16, 2^-12 for f16, of a value near max|want|).
"""
import collections
import os
import sys
import time

import pytest
import torch

from conftest import ROOT, load_json

sys.path.insert(0, os.path.join(ROOT, "oracle"))
sys.path.insert(0, os.path.join(ROOT, "tests"))
import i3d_oracle as oracle  # noqa: E402
import engine_graph  # noqa: E402
import engine_replay_ref as ref  # noqa: E402
import plan_cases  # noqa: E402
import plan_dataflow  # noqa: E402
from af_mi355x import _lib, engine, synth  # noqa: E402

pytestmark = pytest.mark.gpu
NONZERO_SHARE, MIN_MAX = 0.10, 0.25
LOGIT_TOL = {"f32": 2e-4, "f16": 1e-3, "bf16": 3e-3}           # test_hip_forward.LOGIT_TOL

# (network, dtype, batch, switches) - the smallest batches at which the plan still holds the launches in question
CASES = [("i3d_r50", "bf16", 1, {}), ("i3d_r50", "bf16", 4, {}), ("i3d_r50", "bf16", 16, {}), ("i3d_r50", "f16", 16, {}),
         ("i3d_r50", "f32", 1, {}), ("i3d_r50", "bf16", 16, {"AF_FUSE_CPA": "1"}), ("i3d_r50", "bf16", 16, {"AF_FUSE_BC": "1"}),
         ("ftcn_tt", "bf16", 1, {}), ("ftcn_tt", "bf16", 4, {}), ("ftcn_tt", "bf16", 16, {}), ("ftcn_tt", "f16", 4, {}),
         ("ftcn_tt", "f32", 1, {}),
         ("slowfast_r50", "bf16", 1, {}), ("slowfast_r50", "bf16", 16, {}), ("slowfast_r50", "f16", 1, {}), ("slowfast_r50", "f32", 1, {})]


def case_id(case):
    net, dtype, batch, env = case
    return "%s-%s-b%d%s" % (net, dtype, batch, "".join("-%s=%s" % kv for kv in env.items()))


def variant_of(launch):
    """the library's name of the kernel a conv / dual launch goes to ("" for the other kinds)"""
    if launch.kind not in ("conv", "dual"):
        return ""
    refs = (launch.refs() + [None])[:2]
    return _lib.lib.af_conv_variant_name(_lib.lib.af_conv_variant(*refs)).decode()


def expected_kinds(case, plan):
    """what each case is there for, from its plan"""
    net, dtype, batch, env = case
    kinds = collections.Counter(l.kind for l in plan.launches)
    variants = {variant_of(l) for l in plan.launches}
    if net != "slowfast_r50" and dtype != "f32":
        assert (kinds["ca"] > 0) == (batch >= 4), kinds
    if net == "i3d_r50" and batch == 16 and dtype != "f32":
        assert any("111" in v for v in variants) and any("311g" in v for v in variants), variants
        assert any("133g" in v for v in variants) == (env.get("AF_FUSE_BC") != "1"), variants         # (bc takes the b convs)
        assert kinds["dual"] == 3 and (kinds["stem3_pool"] == 1)
    if net == "i3d_r50" and dtype == "f32":
        assert kinds["stem"] == 1 and kinds["pool"] >= 1 and kinds["dual"] == 4
    if env.get("AF_FUSE_CPA") == "1":
        assert [l.x_sub for l in plan.launches if l.kind == "cpa"] == [2]
    if env.get("AF_FUSE_BC") == "1":
        assert kinds["bc"] >= 1
    if net == "ftcn_tt":
        assert sorted(l.tpool for l in plan.launches if l.kind == "conv" and l.tpool) == [1, 2, 2, 2, 2]
        assert kinds["tstem" if dtype == "f32" else "tstem_pool3"] == 1 and kinds["tt_head"] == 1
    if net == "slowfast_r50":
        assert len([l for l in plan.launches if l.kind == "conv" and l.ch_off > 0]) == 4 and kinds["avgpool"] == 2 and kinds["linear"] == 1
        if dtype != "f32":
            assert kinds["abc"] == 6 and kinds["dual"] == 7 and kinds["stem3_pool"] == 1
            assert sum("small" in variant_of(l) for l in plan.launches) == 3


_STATE = {}


def network(net):
    """(spec, graph, state dict) with the synthetic weights the golden tests use"""
    if net not in _STATE:
        spec = plan_cases.SPECS[net]
        if net == "i3d_r50":
            sd, want = synth.synthetic_state_dict(seed=0), load_json("f1_logits.json")["weights_sha256"]
        else:
            g = load_json({"slowfast_r50": "f5_slowfast.json", "ftcn_tt": "f6_ftcn.json"}[net])
            sd, want = synth.synthetic_state_dict(spec, seed=g["weights_seed"]), g["weights_sha256"]
        assert synth.state_dict_sha256(sd) == want
        _STATE[net] = (spec, engine_graph.build(spec), sd)
    return _STATE[net]


def clips(batch):
    """normalised synthetic clips, kinds alternating"""
    u8 = synth.synthetic_clips_u8(batch, seed=2026, kind="smooth")
    u8[1::2] = synth.synthetic_clips_u8(batch, seed=2027, kind="uniform")[1::2]
    return synth.normalize_like_callers(u8.cuda())


def checksums(eng):
    """name -> integer checksum of every activation buffer and head output of the engine"""
    named = dict(eng.buf)
    named.update({"pooled": eng.pooled, "logits": eng.logits})
    if hasattr(eng, "tokens_pooled"):
        named["tokens"] = eng.tokens_pooled
    sums = []
    for t in named.values():
        raw = t.view(torch.int16) if t.element_size() == 2 else t.view(torch.int32)
        sums.append(raw.sum(dtype=torch.int64) + 3 * raw[1::2].sum(dtype=torch.int64))
    return dict(zip(named, torch.stack(sums).tolist()))


def stored_view(eng, buf, s, batch):
    """the rows a Store names, (N, T, H, W, ld), of engine buffer ``buf``"""
    rows = batch * s.dims[0] * s.dims[1] * s.dims[2]
    n = (rows - 1) * s.ld + s.ch_off + s.ch
    assert n <= eng.buf[buf].numel(), (buf, n, eng.buf[buf].numel())
    assert rows * s.ld <= eng.buf[buf].numel(), (buf, rows, s.ld)
    return eng.buf[buf][:rows * s.ld].view(batch, *s.dims, s.ld)


def replay(case, corrupt=None, stats=None):
    """Steps the forward of ``case``; returns (failures [(launch, message)], logits of the normal run, logits of the stepped run).
    ``corrupt(eng, plan)``: rebinds something on the op array before the runs and returns a function that restores it."""
    net, dtype, batch, env = case
    spec, g, sd = network(net)
    dev = torch.device("cuda")
    tdt = ref.TORCH_DT[dtype]
    dims = (spec.num_frames, spec.crop, spec.crop)
    weights = engine.PackedWeights(spec, sd, dtype, dev)
    eng = engine.Engine(spec, weights, batch, dev)
    plan = engine.plan_network(spec, dtype, batch, dims, weights.w3)
    assert [(l.kind, l.src, l.dst, l.dst_a) for l in plan.launches] == [(l.kind, l.src, l.dst, l.dst_a) for l in eng.launches]
    expected_kinds(case, plan)
    ios, tables = {}, {}

    def see(i, launch, io, table):
        ios[i] = io
        tables[i] = {b: list(h.segs) for b, h in table.items()}
    errors = plan_dataflow.walk(plan, g, see)
    assert not errors, errors[:3]
    cons = g.consumers()
    x = clips(batch)
    restore = corrupt(eng, plan) if corrupt else None
    failures = []
    try:
        with torch.inference_mode():
            logits0 = eng.run_f32(x)[0].clone()
            torch.cuda.synchronize()
            R = ref.Reference(g, sd, dtype, dev)
            xr = x.to(tdt).permute(0, 2, 3, 4, 1)
            if len(plan.inputs) == 1:
                R.put("input", xr)
            else:
                R.put("input_slow", xr[:, ::spec.alpha]); R.put("input_fast", xr)
            n_pack = len(plan.inputs)
            before = checksums(eng)
            eng.run_ops(0, n_pack)
            after = checksums(eng)
            changed = {k for k in before if before[k] != after[k]}
            assert changed <= {b for b, _, _ in plan.inputs}, changed
            done = set(plan_dataflow.input_names(plan))
            for k, launch in enumerate(eng.launches):
                io, before = ios[k], after
                count = eng.TT_HEAD_OPS if launch.kind == "tt_head" else 1
                eng.run_ops(n_pack + k, count)
                after = checksums(eng)
                what = "%s launch %d (%s)" % (launch.kind, k, eng.op_names[n_pack + k])
                try:
                    _check_launch(eng, plan, g, R, launch, io, tables[k], before, after, k, what, stats, dtype)
                except AssertionError as e:
                    failures.append((k, "%s: %s" % (what, e)))
                done.update(io.made)
                if launch.kind not in ref.HEAD_KINDS:
                    for s in io.stores:
                        if s.ch_off:
                            cc = [c for c in cons[s.name] if g[c].op == "concat"]
                            done.update(cc)
                for name in list(R.snap):                       # drop a snapshot behind its last graph reader
                    if not _alive(g, cons, name, done):
                        del R.snap[name]
            torch.cuda.synchronize()
            logits1 = eng.logits.clone()
    finally:
        if restore:
            restore()
    return failures, logits0, logits1


def _alive(g, cons, name, done):
    return any(c not in done or (g[c].op == "concat" and _alive(g, cons, c, done)) for c in cons[name])


def _note(stats, key, ratio, tol):
    if stats is not None:
        stats[key] = max(stats.get(key, (0.0, tol)), (ratio, tol))


def _check_launch(eng, plan, g, R, launch, io, table, before, after, k, what, stats, dtype):
    batch = plan.batch
    # only its own outputs change
    own = {getattr(launch, s.operand) if s.operand in ("dst", "dst_a") else s.operand for s in io.stores}
    changed = {name for name in before if before[name] != after[name]}
    assert changed <= own, "changed %s, its outputs are %s" % (sorted(changed - own), sorted(own))
    if launch.kind in ref.HEAD_KINDS:
        return _check_head(eng, g, R, launch, io, what, stats, dtype)
    roles, fold = ref.rounding(launch)
    # "block": the trunk the launch stores (cpa: pooled - the max over frame pairs and the rounding commute)
    rounded = {io.stores[0].name if r == "block" else launch.convs[r].conv for r in roles}
    folded = {launch.convs[r].conv for r in ("c", "branch1")} if fold else set()
    for s in io.stores:                          # snapshot first: a launch that fails its comparison still teacher-forces the next
        view = stored_view(eng, getattr(launch, s.operand), s, batch)
        if s.operand == "dst":                   # Engine.activation names the same rows
            act = eng.activation(len(plan.inputs) + k)
            assert (act.shape, act.data_ptr()) == (view.shape, view.data_ptr()), (tuple(act.shape), tuple(view.shape))
        R.put(s.name, view[..., s.ch_off:s.ch_off + s.ch].clone(), s.sub)
    for s in io.stores:
        buf = getattr(launch, s.operand)
        view = stored_view(eng, buf, s, batch)
        got_all = view[..., s.ch_off:s.ch_off + s.ch]
        ctx = (set(io.made), rounded - {s.name}, folded)          # an output is compared before its own rounding
        rows = ref.window_rows(batch, *s.dims, seed=1000 + k)
        pos = ref.rows_to_pos(rows, s.dims, got_all.device)
        got = got_all[pos[:, 0], pos[:, 1], pos[:, 2], pos[:, 3]]
        gpos = pos if s.sub == 1 else pos * torch.tensor([1, 1, 2, 2], device=pos.device)
        want = R.value(s.name, gpos, ctx)
        ratio, top, share = ref.compare(got, want, s.name)
        tol = ref.tolerance(launch, s.operand, dtype)
        print("%s %s %s: max|d| / max|want| = %.3e (tolerance %.1e), max|want| %.3g, non-zero %.2f, %d positions"
              % (what, variant_of(launch), s.name, ratio, tol, top, share, len(rows)))
        _note(stats, (launch.kind, variant_of(launch), s.operand, dtype), ratio, tol)
        assert ratio <= tol, "%s: max|d| / max|want| = %.3e over %.1e" % (s.name, ratio, tol)
        assert share >= NONZERO_SHARE and top >= MIN_MAX, "%s: vacuous windows (non-zero %.2f, max|want| %.3g)" % (s.name, share, top)
        # the other channels of the sampled rows: bit-equal to what their producer stored
        for off, ch, other in table[buf]:
            if other != s.name:
                snap, _ = R.snap[other]
                there = view[..., off:off + ch][pos[:, 0], pos[:, 1], pos[:, 2], pos[:, 3]]
                assert torch.equal(there, snap[pos[:, 0], pos[:, 1], pos[:, 2], pos[:, 3]]), "channels of %s in the same rows changed" % other


def _check_head(eng, g, R, launch, io, what, stats, dtype):
    import math
    spec = eng.spec
    for s in io.stores:
        if s.operand in ("pooled", "tokens"):
            node = g[s.name]
            want = R.avgpool(s.name)
            got = (eng.tokens_pooled if s.operand == "tokens" else eng.pooled[..., s.ch_off:s.ch_off + s.ch]).double()
            win = node.pool.kernel[0] * node.pool.kernel[1] * node.pool.kernel[2]
            top = float(R.snap[node.reads[0]][0].abs().max())
            # test_avgpool_vs_fp64's fp32 bound for O(1) operands, scaled by the operands' size where they are larger
            bound = (2e-7 * math.sqrt(win) * 4 + 1e-7) * max(1.0, top)
            err = float((got - want.view(got.shape)).abs().max())
            print("%s %s: max|d| %.3e (bound %.3e), max|x| %.3g" % (what, s.name, err, bound, top))
            _note(stats, (launch.kind, "", s.operand, dtype), err / bound, 1.0)
            assert err <= bound, "%s: %.3e over %.3e" % (s.name, err, bound)
            assert float(want.abs().max()) >= MIN_MAX / 10 and float((want != 0).double().mean()) >= NONZERO_SHARE
        elif launch.kind == "tt_head":
            # the transformer in fp64 on the engine's own tokens (test_ftcn_head_known_answer's 5e-5)
            sd64 = {k: v.double() for k, v in R.sd.items() if k.startswith(spec.head)}
            want = oracle.time_transformer(eng.tokens_pooled.double().cpu(), sd64, p=spec.head, heads=spec.heads)
            err = float((eng.logits.double().cpu() - want.view(eng.logits.shape)).abs().max())
            print("%s logits: max|d| %.3e (5e-5)" % (what, err))
            _note(stats, (launch.kind, "", "logits", dtype), err, 5e-5)
            assert err <= 5e-5, "logits: %.3e over 5e-5" % err
        else:
            pooled = eng.pooled.double()
            want = R.linear(pooled, spec.head)
            w = R._p(spec.head + ".weight").double()
            # test_linear_scores_vs_fp64's bound
            bound = 2e-6 + 2e-7 * math.sqrt(pooled.shape[-1]) * float((pooled.abs() @ w.abs().t()).max())
            err = float((eng.logits.double() - want.reshape(eng.logits.shape)).abs().max())
            print("%s logits: max|d| %.3e (bound %.3e)" % (what, err, bound))
            _note(stats, (launch.kind, "", "logits", dtype), err / bound, 1.0)
            assert err <= bound, "logits: %.3e over %.3e" % (err, bound)


@pytest.mark.parametrize("case", CASES, ids=case_id)
def test_every_launch_matches_fp64(case, monkeypatch):
    plan_cases.set_switches(monkeypatch, case[3])
    stats = {}
    t0 = time.time()
    failures, logits0, logits1 = replay(case, stats=stats)
    for key, (ratio, tol) in sorted(stats.items()):
        print("WORST %s %s: %.3e of %.1e" % (case_id(case), " ".join(str(k) for k in key), ratio, tol))
    print("TIME %s: %.1f s" % (case_id(case), time.time() - t0))
    assert not failures, "\n".join(m for _, m in failures)
    assert torch.equal(logits0, logits1), "the stepped forward is not the normal one: %s vs %s" % (logits0.flatten()[:4], logits1.flatten()[:4])


def test_replay_reports_a_misbound_bn_at_its_launch(monkeypatch):
    """The replay can fail.  On the engine's own op array the scale / shift pointers of one s3 `a` conv (I3D, bf16, batch 1) are
    bound to those of the next block's `a` conv: same cout, so the same padded length, and every access stays inside an allocation
    (asserted on the host before anything runs).  The replay must report exactly that launch - none before it, and none behind it
    either, since every later launch is referred to the snapshot of what the engine stored.  Measured on an MI355X: the replay reports
    launch 13 alone; the logit of the corrupted forward moves by 6.8e-3, against LOGIT_TOL["bf16"] = 3e-3 - on this clip the pooled
    logit notices this corruption by a factor of 2.3 and says nothing about where; the replay measures max|d| / max|want| = 0.54 at that
    launch, 45 times its tolerance of 1.2e-2."""
    plan_cases.set_switches(monkeypatch, {})
    case = ("i3d_r50", "bf16", 1, {})
    mine, other = "resnet.s3.pathway0_res1.branch2.a", "resnet.s3.pathway0_res2.branch2.a"
    where = {}

    def corrupt(eng, plan):
        k, = [i for i, l in enumerate(plan.launches) if l.kind == "conv" and l.convs["conv"].conv == mine]
        op = eng.ops[len(plan.inputs) + k]
        w = eng.weights
        cv = plan.launches[k].convs["conv"]
        # every access stays inside an allocation: the neighbour's vectors have this conv's padded length
        need = _lib.lib.af_padded_channels(cv.cout)
        assert op.conv.cout == cv.cout and op.scale == w.scale[mine].data_ptr() and op.shift == w.shift[mine].data_ptr()
        for t in (w.scale[other], w.shift[other]):
            assert t.numel() == need == w.scale[mine].numel() and t.dtype == torch.float32 and t.is_cuda
        saved = (op.scale, op.shift)
        op.scale, op.shift = w.scale[other].data_ptr(), w.shift[other].data_ptr()
        where["k"] = k

        def restore():
            op.scale, op.shift = saved
        return restore

    _, clean, _ = replay(case)
    failures, logits, _ = replay(case, corrupt)
    delta = float((logits - clean).abs().max())
    print("mis-bound BN of %s: replay reports launches %s; |delta logit| = %.3e, LOGIT_TOL[bf16] = %.1e"
          % (mine, [k for k, _ in failures], delta, LOGIT_TOL["bf16"]))
    assert [k for k, _ in failures] == [where["k"]], failures
