"""GPU: every conv_igemm tile x epilogue form of af_conv3d_bn_act / af_conv3d_dual_bn_act against the oracle in fp64, at sizes
of a few hundred positions.  pick_variant chooses the tile from (cout, K-steps, M), the caller chooses the epilogue form, so any
reachable pair runs in production; the layer tests reach few of them.  Here AF_FORCE_VAR pins the tile (pick_variant reads it on
every call) and every case asserts the tile it ran on.

Tile ids (af_conv.hip): 0 = 128x256, 1 = 64x256, 2 = 128x128, 3 = 64x128, 5 = 128x128 with a 2-slot ring, 6 = 256x256,
7 = 128x512, 12 = 256x224 (channels x positions).

Operands are rounded to the storage type on both sides, the reference is oracle.conv_bn_act in fp64 (+ residual, ReLU,
F.max_pool3d, or a second conv_bn_act for the two-input form).  Tolerances, relative to max|want|, are the project's own:
single input f32 2e-6 * max(1, K / 1024), f16 1.5e-3, bf16 1.2e-2 (split-K as well); two inputs (BN scales folded into the packed
weights: one more rounding) f32 5e-6, f16 3e-3, bf16 2.4e-2.

Every launch writes into a view of a larger buffer prefilled with 7.0: GUARD rows before and after the M output rows and, with
out_ld > cout, 8 guard channels left and right.  All of them must still be 7.0 afterwards (tail-tile rows past M, channel-pad
columns past cout).

CASES is plain data (no device needed): tests/test_host_cpu.py::test_conv_matrix_covers_what_ships compares case_key() of every
case with what the three networks ship."""
import collections
import os
import sys
import zlib

import pytest
import torch
import torch.nn.functional as F

from conftest import ROOT

sys.path.insert(0, os.path.join(ROOT, "oracle"))
sys.path.insert(0, os.path.join(ROOT, "tests"))
import i3d_oracle as oracle  # noqa: E402
import hip_helpers as hh  # noqa: E402
from af_mi355x import synth  # noqa: E402

pytestmark = pytest.mark.gpu
DTYPES = ["f32", "f16", "bf16"]
TILES = (0, 1, 2, 3, 5, 6, 7, 12)
TILE_BN = {0: 128, 1: 64, 2: 128, 3: 64, 5: 128, 6: 256, 7: 128, 12: 256}      # channels per tile
TILE_ROWS = {0: 256, 1: 256, 2: 128, 3: 128, 5: 128, 6: 256, 7: 512, 12: 224}  # positions per tile
GUARD = 64
TOL = {"f32": 2e-6, "f16": 1.5e-3, "bf16": 1.2e-2}
TOL_DUAL = {"f32": 5e-6, "f16": 3e-3, "bf16": 2.4e-2}

# K-steps S = taps * ceil(cin / BK) (+ ceil(cin2 / BK)), BK = 64 elements (f32: 32), that pick_variant can give each tile, swept
# up to 12 (7..12 holds every residue mod 6, which is how the closure test classes the long loops), and 18 / 27 for the 1x3x3 /
# 3x3x3 kernels with a channel tail.  Derivation, from the conditions in pick_variant:
S_RANGE = {
    0: (4, 12),    # cout % 128 == 0 and S > 3 (short_k is S <= 3); 4..8 as a two-input layer or at cout = 256
    1: (4, 12),    # cout % 128 != 0 and S > 3
    2: (1, 12),    # cout % 128 == 0 and S <= 3 without the force; the sweep goes on to 12 (same loop as tile 3, 6 workgroups per CU)
    3: (1, 12),    # fewer than 64 workgroups of the widest tile: any S
    5: (4, 8),     # cout % 128 == 0, 4 <= S <= 8, cout >= 512 or == 128
    6: (4, 12),    # cout % 256 == 0 and S >= 4 with the 2x2 pool, >= 6 with a second input, >= 9 plain
    12: (6, 12),   # as tile 6 without a pool: S >= 6 with a second input, >= 9 plain
    7: (9, 12),    # cout == 128 and taps >= 9: S is a multiple of 9
}
# S -> (kernel, K-steps per tap, channel tail): the 1x1x1, 3x1x1, 5x1x1, 1x3x3 and 3x3x3 kernels with their usual padding; a tail is
# cin = 80 (f32: 40) at two K-steps per tap, i.e. the last K-step of every tap holds a quarter of its channels
S_FACTORS = {1: ((1, 1, 1), 1, False), 2: ((1, 1, 1), 2, True), 3: ((3, 1, 1), 1, False), 4: ((1, 1, 1), 4, False),
             5: ((5, 1, 1), 1, False), 6: ((3, 1, 1), 2, True), 7: ((1, 1, 1), 7, False), 8: ((1, 1, 1), 8, True),
             9: ((1, 3, 3), 1, False), 10: ((5, 1, 1), 2, True), 11: ((1, 1, 1), 11, False), 12: ((3, 1, 1), 4, False),
             16: ((1, 1, 1), 16, False), 18: ((1, 3, 3), 2, True), 20: ((5, 1, 1), 4, False), 27: ((3, 3, 3), 1, True)}
# split-K needs S >= 16 and fewer than 128 workgroups (plan_ksplit): tiles 6, 7 and 12 are only chosen at >= 128 workgroups, tiles 2
# and 5 only at S <= 8, so a split can meet tiles 0, 1 and 3.  S >= 16 is K >= 1024 at 16 bits: the one place K goes beyond 768.
SPLIT_TILES = (0, 1, 3)
# the form sweep's K loop per tile: (kernel, K-steps per tap, channel tail), an S inside S_RANGE with temporal or spatial taps
PRIMARY = {0: ((3, 1, 1), 2, True), 1: ((3, 1, 1), 2, True), 2: ((1, 1, 1), 2, True), 3: ((3, 1, 1), 1, False),
           5: ((3, 1, 1), 2, True), 6: ((1, 3, 3), 1, False), 12: ((1, 3, 3), 1, False), 7: ((1, 3, 3), 1, False)}
# two-input form: (K-steps of the first input, of the second), S = their sum inside S_RANGE
PRIMARY_DUAL = {0: (3, 3), 1: (2, 2), 2: (1, 1), 3: (1, 2), 5: (3, 3), 6: (3, 3), 12: (3, 3)}
# forms: name -> (relu, residual, out_ld > cout, tpool)
FORMS = collections.OrderedDict([
    ("relu", (True, False, False, 0)), ("linear", (False, False, False, 0)), ("res", (True, True, False, 0)),
    ("ld", (True, False, True, 0)), ("res_ld", (True, True, True, 0)), ("tp1", (True, False, False, 1)),
    ("tp1_res", (True, True, False, 1)), ("tp2", (True, False, False, 2))])
# further (form, S) pairs per tile: the K-step counts at which the three networks ship that form on that tile (batch 1..32), beyond
# the form sweep's one S per tile.  Non-dual entries name S (S_FACTORS), dual ones (K-steps, K-steps of the second input).
MORE = {
    0: [("ld", 8), ("ld", 10), ("tp2", 4), ("tp2", 8), ("res", 10), ("dual", (2, 2)), ("dual", (2, 3)), ("dual", (4, 4)),
        ("dual", (5, 5)), ("dual", (4, 8))],
    1: [("ld", 5)],
    2: [("res", 1), ("res_ld", 1), ("tp1_res", 1), ("dual", (1, 2))],
    3: [("ld", 5), ("ld", 8), ("ld", 10), ("res", 1), ("res", 2), ("res", 4), ("res", 8), ("res", 10), ("res_ld", 2), ("res_ld", 4),
        ("res_ld", 8), ("dual", (1, 1)), ("dual", (3, 3)), ("dual", (2, 5)), ("dual", (4, 4)), ("dual", (5, 5))],
    5: [("ld", 5), ("res", 4), ("res", 8), ("res_ld", 4), ("res_ld", 8), ("tp2", 4), ("dual", (2, 5))],
    6: [("tp2", 4), ("tp2", 8), ("tp2", 10), ("dual", (4, 8))],
    12: [("res", 10), ("dual", (2, 5)), ("dual", (4, 4)), ("dual", (5, 5)), ("dual", (4, 8))],
    7: [],
}

# name: unique id; kernel / kpt / tail: the first input's K loop; dims: input (n, t, h, w) (the kernels keep the size: padding k // 2);
# dual: None or (K-steps of the second input, its channel tail, its stride); nonfinite: one NaN and one +inf in the input
Case = collections.namedtuple("Case", "name tile kernel kpt tail cout dims relu res ld tpool split dual nonfinite")


def _shapes(tile, tpool):
    """(less than one tile of rows, whole tiles + a ragged tail, two clips) for this tile; the pooled forms keep the pooled
    dimensions even (the tail is then ragged, not odd)"""
    small = TILE_ROWS[tile] < 256
    if tpool == 1:
        return ((1, 2, 7, 9) if small else (1, 2, 9, 13)), (1, 4, 11, 13), (2, 2, 11, 13)
    if tpool == 2:
        return ((1, 2, 6, 10) if small else (1, 2, 8, 14)), (1, 3, 14, 14), (2, 3, 10, 10)
    return ((1, 2, 7, 9) if small else (1, 2, 9, 13)), (1, 3, 13, 15), (2, 3, 9, 11)


def _couts(tile):
    return TILE_BN[tile], 3 * TILE_BN[tile]          # 1 and 3 channel tiles: with 1..5 row tiles never a multiple of 8 workgroups


def _build_cases():
    cases = []

    def add(tile, label, kernel, kpt, tail, cout, dims, form="relu", split=False, dual=None, nonfinite=False):
        relu, res, ld, tpool = FORMS[form]
        s = kernel[0] * kernel[1] * kernel[2] * kpt + (dual[0] if dual else 0)
        name = "t%d-%s-S%d-%dx%dx%d-%s-c%d-%s" % (tile, label, s, kernel[0], kernel[1], kernel[2], "x".join(map(str, dims)), cout,
                                                   "tail" if tail else "full")
        cases.append(Case(name, tile, kernel, kpt, tail, cout, dims, relu, res, ld, tpool, split, dual, nonfinite))

    for tile in TILES:
        c1, c3 = _couts(tile)
        lo, hi = S_RANGE[tile]
        # (a) K-step sweep, ReLU, no residual
        sweep = [s for s in range(lo, hi + 1)] + ([18, 27] if hi == 12 else [])
        for s in sweep:
            kernel, kpt, tail = S_FACTORS[s]
            if tile == 7 and kernel[1] * kernel[2] < 9:
                continue
            small, large, clips = _shapes(tile, 0)
            dims = clips if kernel[0] == 3 else (small if s % 2 else large)       # two clips under temporal taps: a tile spans the clip boundary
            add(tile, "sweep", kernel, kpt, tail, c3 if s % 2 else c1, dims)
        # (b) forms at one S (both shapes, 1 and 3 channel tiles) and at the further S of MORE
        kernel, kpt, tail = PRIMARY[tile]
        for i, form in enumerate(FORMS):
            tpool = FORMS[form][3]
            if tpool and tile == 12:          # pick_variant gives 256x224 to unpooled layers only and refuses to force it on a pooled one
                continue
            small, large, clips = _shapes(tile, tpool)
            add(tile, form, kernel, kpt, tail, c1 if i % 2 else c3, small, form)
            add(tile, form, kernel, kpt, tail, c3 if i % 2 else c1, clips if (kernel[0] > 1 and i % 2) else large, form)
        if tile != 7:                          # no two-input kernel for 128x512 (the launcher would run 64x128 instead)
            k1, k2 = PRIMARY_DUAL[tile]
            small, large, _ = _shapes(tile, 0)
            add(tile, "dual_s1", (1, 1, 1), k1, False, c3, small, dual=(k2, True, (1, 1, 1)))
            add(tile, "dual_s1", (1, 1, 1), k1, False, c1, large, dual=(k2, False, (1, 1, 1)))
            add(tile, "dual_s2", (1, 1, 1), k1, True, c1, small, dual=(k2, False, (1, 2, 2)))
            add(tile, "dual_s2", (1, 1, 1), k1, False, c3, large, dual=(k2, True, (1, 2, 2)))
        for j, (form, s) in enumerate(MORE[tile]):
            if form == "dual":
                small, large, _ = _shapes(tile, 0)
                add(tile, "dual_s%d" % (1 + j % 2), (1, 1, 1), s[0], False, c1 if j % 2 else c3, small if j % 2 else large,
                    dual=(s[1], j % 3 == 0, (1, 2, 2) if j % 2 else (1, 1, 1)))
            else:
                kernel_s, kpt_s, tail_s = S_FACTORS[s]
                small, large, clips = _shapes(tile, FORMS[form][3])
                add(tile, form, kernel_s, kpt_s, tail_s, c1 if j % 2 else c3, small if j % 2 else (clips if kernel_s[0] > 1 else large), form)
        # cout padded up to the tile width (pick_variant sees the padded count): plain and into a wider row
        small, large, _ = _shapes(tile, 0)
        for cout in {64: (40,), 128: (72, 200), 256: (200,)}[TILE_BN[tile]]:
            add(tile, "coutpad", kernel, kpt, tail, cout, large, "relu")
            add(tile, "coutpad_ld", kernel, kpt, tail, cout, small, "ld")
        # split-K + finish kernel: plain, with a residual, into a wider row
        if tile in SPLIT_TILES:
            for j, s in enumerate((16, 18, 20)):
                kernel_s, kpt_s, tail_s = S_FACTORS[s]
                for i, form in enumerate(("relu", "res", "ld")):
                    add(tile, "split_" + form, kernel_s, kpt_s, tail_s, c3 if (i + j) % 2 else c1, small if (i + j) % 2 else large,
                        form, split=True)
        # one NaN and one +inf in the input (run in bf16 and f32)
        for form in ("relu", "res", "tp1", "tp2"):
            tpool = FORMS[form][3]
            if tpool and tile == 12:
                continue
            add(tile, "nonfinite_" + form, kernel, kpt, tail, c1, _shapes(tile, tpool)[1], form, nonfinite=True)
        if tile in SPLIT_TILES:
            add(tile, "nonfinite_split", (1, 1, 1), 16, False, c1, large, "relu", split=True, nonfinite=True)
    assert len({c.name for c in cases}) == len(cases)
    return cases


CASES = _build_cases()


def case_steps(case):
    return case.kernel[0] * case.kernel[1] * case.kernel[2] * case.kpt + (case.dual[0] if case.dual else 0)


def case_key(case, dtype):
    """what the closure test compares: the tile, the dtype, the form (two inputs, residual, tpool, out_ld != cout, split-K) and the
    class of the K-step count (the K loops special-case short loops and rotate a 2- or 3-slot ring: S itself up to 6, S mod 6 beyond)"""
    s = case_steps(case)
    return (case.tile, dtype, (case.dual is not None, case.res, case.tpool, case.ld, case.split), s if s <= 6 else ("big", s % 6))


def _cin(kpt, tail, dtype):
    bk = 32 if dtype == "f32" else 64
    return (kpt - 1) * bk + bk // 4 if tail else kpt * bk


def _bn_layout(prefix, ch):
    return [(prefix + s, (ch,), "float32") for s in (".weight", ".bias", ".running_mean", ".running_var")]


_compare = hh.compare          # NaN masks equal, infinities equal, the finite rest within tol * max|finite want|


def _cases_for(dtype):
    return [c for c in CASES if not (c.nonfinite and dtype == "f16")]


@pytest.mark.parametrize("dtype,case", [(dt, c) for dt in DTYPES for c in _cases_for(dt)],
                         ids=["%s-%s" % (dt, c.name) for dt in DTYPES for c in _cases_for(dt)])
def test_conv_tile_form(dtype, case, monkeypatch):
    tdt = hh.TORCH_DT[dtype]
    seed = 7000 + zlib.crc32(case.name.encode()) % 90000
    kt, kh, kw = case.kernel
    pad = (kt // 2, kh // 2, kw // 2)
    n, t, h, w = case.dims
    cin, cout = _cin(case.kpt, case.tail, dtype), case.cout
    lay = [("w.weight", (cout, cin, kt, kh, kw), "float32")] + _bn_layout("bn", cout)
    if case.dual:
        kpt2, tail2, stride2 = case.dual
        cin2 = _cin(kpt2, tail2, dtype)
        lay += [("w2.weight", (cout, cin2, 1, 1, 1), "float32")] + _bn_layout("bn2", cout)
    sd = synth.fill_layout(lay, seed)
    x = synth.synthetic_tensor((n, cin, t, h, w), seed).to(tdt).float()
    sd["w.weight"] = sd["w.weight"].to(tdt).float()
    if case.nonfinite:                           # rows of frames 0 and 1: clear of the ragged last tile and of each other's window
        x[0, 1, 0, 2, 2] = float("nan")
        x[0, 2, 1, 8, 9] = float("inf")
    sd64 = {k: v.double() for k, v in sd.items()}
    want = oracle.conv_bn_act(x.double(), sd64["w.weight"], sd64, "bn", (1, 1, 1), pad, False)
    res = x2 = None
    if case.dual:
        sd["w2.weight"] = sd["w2.weight"].to(tdt).float()
        x2 = synth.synthetic_tensor((n, cin2, (t - 1) * stride2[0] + 1, h * stride2[1], w * stride2[2]), seed + 2).to(tdt).float()
        want = want + oracle.conv_bn_act(x2.double(), sd["w2.weight"].double(), sd64, "bn2", stride2, (0, 0, 0), False)
    if case.res:
        res = synth.synthetic_tensor(tuple(want.shape), seed + 1).to(tdt).float()
        want = want + res.double()
    if case.relu:
        want = F.relu(want)
    if case.tpool == 1:
        want = F.max_pool3d(want, (2, 1, 1), (2, 1, 1))
    elif case.tpool == 2:
        want = F.max_pool3d(want, (1, 2, 2), (1, 2, 2))
    assert not case.nonfinite or (torch.isnan(want).any() and torch.isinf(want).any())
    rows = want.shape[0] * want.shape[2] * want.shape[3] * want.shape[4]
    assert rows < 2500 and cout <= 768 and (case.split or cin * kt * kh * kw <= 768)

    ldw, off = (cout + 16, 8) if case.ld else (cout, 0)
    monkeypatch.setenv("AF_FORCE_VAR", str(case.tile))

    def launch(workspace):
        buf = torch.full((GUARD + rows + GUARD, ldw), 7.0, dtype=tdt, device="cuda")
        view = buf[GUARD:GUARD + rows, off:off + cout]
        assert view.data_ptr() % 16 == 0
        if case.dual:
            hh.conv_dual(hh.to_ndhwc(x, dtype), sd["w.weight"], hh.fold_bn(sd, "bn"), hh.to_ndhwc(x2, dtype), sd["w2.weight"],
                         hh.fold_bn(sd, "bn2"), stride2, dtype, out=view, out_ld=ldw if case.ld else 0, tpool=case.tpool)
            variant = hh.conv_dual.last_variant
        else:
            hh.conv_bn_act(hh.to_ndhwc(x, dtype), sd["w.weight"], *hh.fold_bn(sd, "bn"), (1, 1, 1), pad, case.relu, dtype,
                           residual=None if res is None else hh.to_ndhwc(res, dtype), out=view, out_ld=ldw if case.ld else 0,
                           tpool=case.tpool, workspace=workspace)
            variant = hh.conv_bn_act.last_variant
        # a specialised kernel took the shape or the force was refused: the case tested nothing (change the shape, not this)
        assert variant == case.tile, "ran on variant %d, not on tile %d" % (variant, case.tile)
        host = buf.float().cpu()
        got = host[GUARD:GUARD + rows, off:off + cout].clone()
        host[GUARD:GUARD + rows, off:off + cout] = 7.0
        assert torch.all(host == 7.0), "%d guard elements around the output were written" % int((host != 7.0).sum())
        return got.reshape(want.shape[0], want.shape[2], want.shape[3], want.shape[4], cout).permute(0, 4, 1, 2, 3).double()

    if case.dual:
        tol = TOL_DUAL[dtype]
    else:
        tol = TOL[dtype] * (max(1.0, cin * kt * kh * kw / 1024.0) if dtype == "f32" else 1.0)
    got = launch("auto" if case.split else None)     # (the long unsplit loops of the sweep would otherwise split at these sizes)
    if case.split:
        assert hh.conv_bn_act.last_workspace_bytes > 0, "the layer was not split"
    _compare(got, want, tol, case.name + "[" + dtype + "]")
    if case.split:                               # the same layer without a workspace runs unsplit
        _compare(launch(None), want, tol, case.name + "[" + dtype + "] unsplit")
