"""GPU: conv111 (variant 10, csrc/af_conv111.hip), the persistent 1x1x1 stream, against fp64 at the tiles per workgroup it ships.
A workgroup of this kernel keeps its weights in registers and walks tiles first, first + streams, ...; the tile loop is unrolled
NSLOT times over static ring slots and residual register sets (NSLOT = 2 for K = 64 and K = 256, 4 for K = 128), its waits are
counted vmcnt immediates chosen from (my_tiles - 1 - q, q), and the rows of a ragged tile are masked store by store.  What a
workgroup does at the end of its stream depends on my_tiles % NSLOT; the networks ship every residue (K = 128 at batch 6 and 12
runs 2 and 3).

Sizing at run time.  af_conv_work_units (the launcher's own geometry and grid) answers (tiles, workgroups) for a layer; streams =
workgroups / (cout / 256).  A case names k and the position count is chosen so that tiles = k * streams + r with r = streams / 2
- 1 (0 < r < streams): r workgroups per column run k + 1 tiles, the others k.  "exact" cases have r = 0.  The last tile has
`last` live rows (plain form; the pooled form takes its raggedness from the frame size: tile = (clip, frame pair, 64 pixels)).
Every case asserts the variant, (tiles, workgroups) and the set of my_tiles % NSLOT among its workgroups, all from the library's
answer: a case that meant residues 2 and 3 and ran 0 and 1 would test nothing.

Operands are rounded to the storage type on both sides; the reference is oracle.conv_bn_act in fp64, residual added, ReLU and the
frame-pair max (F.max_pool3d, which propagates NaN) applied in fp64.  Tolerances, relative to max|want|, are the project's own:
f16 1.5e-3, bf16 1.2e-2; the two-input form (hh.conv_dual folds the BN scales into the packed weights: one more rounding of
every weight) f16 3e-3, bf16 2.4e-2.  The output is a view into a buffer prefilled with 7.0: 128 guard rows - a whole dead tile -
before and after and, in the "ld" form (out_ld = cout + 16), 8 guard channels left and right; all of them must still be 7.0.
The non-finite cases (bf16) put one NaN and one +inf into tiles that are NOT the first of their workgroup.

CASES is plain data (no device needed): tests/test_host_cpu.py::test_conv111_and_small_matrices_cover_what_ships compares
case_keys() of every case with what the three networks ship on this kernel."""
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
GUARD = 128
TOL = {"f16": 1.5e-3, "bf16": 1.2e-2}
TOL_DUAL = {"f16": 3e-3, "bf16": 2.4e-2}
DT16 = ("f16", "bf16")
FORMS = ("relu", "linear", "ld", "nonfinite")        # linear: no ReLU; ld: out_ld = cout + 16; nonfinite: ReLU, one NaN and one +inf

# cin2: channels of the second input (hh.conv_dual), 0: one input; hw: the frame of the pooled form (tpool = 1), None: plain; k: the
# tiles per workgroup are k and k + 1, "exact": k everywhere; last: live rows of the last tile (plain form); residues: my_tiles %
# NSLOT that must occur
Case = collections.namedtuple("Case", "name cin cin2 cout hw k exact last res form residues")


def nslot(cin):
    return 4 if cin == 128 else 2


def tile_rows(cin):
    return 64 if cin >= 128 else 128


def _build_cases():
    cases = []

    def add(cin, cout, k, last=None, res=True, form="relu", exact=False, cin2=0, hw=None):
        n = nslot(cin)
        residues = (k % n,) if exact else tuple(sorted({k % n, (k + 1) % n}))
        name = "%d%sto%d-%sk%d%s%s-%s-%s" % (cin, "+%d" % cin2 if cin2 else "", cout, "" if hw is None else "tpool%dx%d-" % hw, k,
                                              "exact" if exact else "", "" if last is None else "-last%d" % last, "res" if res else "nores", form)
        cases.append(Case(name, cin, cin2, cout, hw, k, exact, last, res, form, residues))

    # ---- 64 -> 256: 128-position tiles, 2-slot ring
    add(64, 256, 4, last=1)
    add(64, 256, 4, last=127, res=False)
    add(64, 256, 4, last=128, form="linear")
    add(64, 256, 5, exact=True)                                   # every workgroup 5 tiles
    add(64, 256, 4, last=77, form="ld")                           # ships in SlowFast
    add(64, 256, 4, last=77, form="nonfinite")
    # ... with the frame-pair max: 49 whole chunks of 64 pixels (the shipped frame); 65 pixels (the second chunk of every frame pair
    # has one live pixel: whole waves of the tile have no live row); 49 (every tile ragged, chunks == 1)
    for hw in ((56, 56), (5, 13), (7, 7)):
        add(64, 256, 4, hw=hw)
        add(64, 256, 4, hw=hw, res=False)
    add(64, 256, 4, hw=(5, 13), form="ld")
    add(64, 256, 4, hw=(5, 13), form="nonfinite")
    add(64, 512, 4, last=50)                                      # two columns: the XCD-remapped grid
    add(64, 768, 4, last=50)                                      # three columns: grid 255 of 256, not remapped
    # ... two inputs (c + projection shortcut)
    add(64, 256, 4, last=26, res=False, cin2=64)
    add(64, 256, 4, last=26, res=False, cin2=64, form="ld")
    # ---- 128 -> 512: 64-position tiles, 4-slot ring, three tiles ahead
    add(128, 512, 8, last=1)                                      # residues 0, 1
    add(128, 512, 9, exact=True)                                  # residue 1
    add(128, 512, 10, last=63)                                    # residues 2, 3
    add(128, 512, 10, last=37, res=False)
    add(128, 512, 18, last=20)                                    # residues 2, 3 behind four full turns of the unrolled loop
    add(128, 512, 8, last=33, form="ld")                          # ships in SlowFast at residues 0, 1, 2
    add(128, 512, 10, last=33, form="ld")
    add(128, 512, 10, last=63, form="nonfinite")
    add(128, 256, 10, last=9, res=False)                          # one column, 256 streams
    # ---- 256 -> 1024: 64-position tiles, 2-slot ring, four columns
    add(256, 1024, 8, last=17)
    add(256, 1024, 8, last=63, res=False)
    add(256, 1024, 9, exact=True)
    add(256, 1024, 8, last=40, form="ld")
    assert len({c.name for c in cases}) == len(cases)
    return cases


CASES = _build_cases()


def shipped_key(dtype, cin, cin2, cout, tpool, res, ld, residue):
    """what the closure test compares: one key per value of my_tiles % NSLOT among the workgroups of a launch"""
    return (dtype, cin, cin2, cout, int(tpool), bool(res), bool(ld), residue)


def case_keys(case, dtype):
    return {shipped_key(dtype, case.cin, case.cin2, case.cout, case.hw is not None, case.res, case.form == "ld", r) for r in case.residues}


def residues_of(tiles, workgroups, cin, cout):
    """my_tiles % NSLOT over the workgroups of a launch of `tiles` tiles: stream s of workgroups / (cout / 256) runs tiles s, s + streams, ..."""
    streams = workgroups // (cout // 256)
    k, r = divmod(tiles, streams)
    return tuple(sorted({(k + 1) % nslot(cin), k % nslot(cin)} if r else {k % nslot(cin)}))


def _shape(case, count):
    """input (n, t, h, w, cin): `count` positions in one row of pixels, or `count` frame pairs of the pooled form's frame"""
    return (1, 1, 1, count, case.cin) if case.hw is None else (count, 2) + tuple(case.hw) + (case.cin,)


def plan(case, dtype):
    """(input shape, tiles, workgroups, streams) of the case on this device"""
    def ask(count):
        shape = _shape(case, count)
        return hh.conv_work_units(shape, case.cout, (1, 1, 1), dtype, tpool=int(case.hw is not None),
                                  shape2_ndhwc=shape[:4] + (case.cin2,) if case.cin2 else None)
    bm, ncol = tile_rows(case.cin), case.cout // 256
    per = 1 if case.hw is None else -(-case.hw[0] * case.hw[1] // 64)          # tiles per frame pair
    v, tiles, W = ask(1 << 18)                             # more tiles than 4 per CU of any device: the full grid
    assert v == 10, "variant %d, not 10 (change the shape, not this)" % v
    assert W % ncol == 0 and tiles > W
    streams = W // ncol
    want = case.k * streams + (0 if case.exact else streams // 2 - 1)
    if case.hw is None:
        last = bm if case.last is None else case.last
        assert 0 < last <= bm
        count = (want - 1) * bm + last
    else:
        count = -(-want // per)
    v, tiles, groups = ask(count)
    what = "%s: %d tiles on %d workgroups in %d columns (change the shape, not this)" % (case.name, tiles, groups, ncol)
    assert v == 10, "variant %d, not 10; " % v + what
    assert groups == W and tiles == (want if case.hw is None else count * per), what
    k, r = divmod(tiles, streams)
    assert k == case.k and (r == 0 if case.exact else 0 < r < streams), what
    assert residues_of(tiles, groups, case.cin, case.cout) == case.residues, what
    return _shape(case, count), tiles, groups, streams


def _bn_layout(prefix, ch):
    return [(prefix + s, (ch,), "float32") for s in (".weight", ".bias", ".running_mean", ".running_var")]


def _ncdhw64(x_ndhwc):
    return x_ndhwc.permute(0, 4, 1, 2, 3).contiguous().double()       # (transposed in the storage type: the smaller copy)


def _reference(case, x, x2, sd):
    """fp64, before the residual: bn(conv(x)) [+ bn2(conv2(x2))] as (n, cout, t, h, w)"""
    sd64 = {k: v.double() for k, v in sd.items()}
    want = oracle.conv_bn_act(_ncdhw64(x), sd64["w.weight"], sd64, "bn", (1, 1, 1), (0, 0, 0), False)
    if x2 is not None:
        want = want + oracle.conv_bn_act(_ncdhw64(x2), sd64["w2.weight"], sd64, "bn2", (1, 1, 1), (0, 0, 0), False)
    return want


# the operands and the fp64 reference (before residual, ReLU and pool) of the last geometry: the forms of one geometry share them
_last = {}


def _operands(case, dtype, shape):
    key = (case.cin, case.cin2, case.cout, shape, dtype)
    if _last.get("key") == key:
        return _last["val"]
    _last.clear()
    tdt = hh.TORCH_DT[dtype]
    seed = 11000 + zlib.crc32(repr(key[:4]).encode()) % 90000
    lay = [("w.weight", (case.cout, case.cin, 1, 1, 1), "float32")] + _bn_layout("bn", case.cout)
    if case.cin2:
        lay += [("w2.weight", (case.cout, case.cin2, 1, 1, 1), "float32")] + _bn_layout("bn2", case.cout)
    sd = synth.fill_layout(lay, seed)
    for name in ("w.weight", "w2.weight"):
        if name in sd:
            sd[name] = sd[name].to(tdt).float()
    x = synth.synthetic_tensor(shape, seed).to(tdt)            # NDHWC, in the storage type
    x2 = synth.synthetic_tensor(shape[:4] + (case.cin2,), seed + 1).to(tdt) if case.cin2 else None
    res = synth.synthetic_tensor(shape[:4] + (case.cout,), seed + 2).to(tdt)
    _last["key"], _last["val"] = key, (x, x2, res, sd, _reference(case, x, x2, sd))
    return _last["val"]


def _poison(case, x, streams):
    """one NaN and one +inf in two tiles whose indices are not below `streams`: neither is the first tile of its workgroup.  The
    pooled form gets the NaN in the first frame of a pair, the +inf and a second NaN in the second frames of two others (the max
    must propagate a NaN from either side)"""
    bm = tile_rows(case.cin)
    q1, q2, q3 = streams + 3, 2 * streams + 7, 3 * streams + 2
    if case.hw is None:
        rows = x.reshape(-1, case.cin)
        assert rows.data_ptr() == x.data_ptr() and (q2 + 1) * bm <= rows.shape[0]
        rows[q1 * bm + 5, 3] = float("nan")
        rows[q2 * bm + bm - 2, case.cin - 1] = float("inf")
    else:
        h, w = case.hw
        chunks = -(-h * w // 64)
        frames = x.reshape(x.shape[0], 2, h * w, case.cin)
        assert frames.data_ptr() == x.data_ptr() and q3 // chunks < x.shape[0]
        frames[q1 // chunks, 0, (q1 % chunks) * 64, 3] = float("nan")
        frames[q2 // chunks, 1, min((q2 % chunks) * 64 + 37, h * w - 1), case.cin - 1] = float("inf")
        frames[q3 // chunks, 1, min((q3 % chunks) * 64 + 18, h * w - 1), 0] = float("nan")


def _params():
    out = [(dt, c) for c in CASES for dt in DT16 if c.form != "nonfinite" or dt == "bf16"]
    # the cases of one geometry and dtype next to each other (they share the reference)
    geo = lambda c: (c.cin, c.cin2, c.cout, c.hw is None, c.hw, c.k, c.exact, c.last)
    first = {}
    for i, c in enumerate(CASES):
        first.setdefault(geo(c), i)
    out.sort(key=lambda p: (first[geo(p[1])], p[0], FORMS.index(p[1].form), p[1].res))
    return out


PARAMS = _params()


@pytest.mark.parametrize("dtype,case", PARAMS, ids=["%s-%s" % (dt, c.name) for dt, c in PARAMS])
def test_conv111_tiles_per_workgroup(dtype, case):
    tdt = hh.TORCH_DT[dtype]
    shape, tiles, groups, streams = plan(case, dtype)
    n, t, h, w, cin = shape
    cout, tpool, dual = case.cout, case.hw is not None, bool(case.cin2)
    relu = case.form != "linear"
    assert not (dual and (case.res or not relu))             # af_conv3d_dual_bn_act: no residual, always the ReLU
    x, x2, res, sd, want = _operands(case, dtype, shape)
    if case.form == "nonfinite":
        x = x.clone()
        _poison(case, x, streams)
        want = _reference(case, x, x2, sd)
    if case.res:
        want = want + _ncdhw64(res)
    if relu:
        want = F.relu(want)
    if tpool:
        want = F.max_pool3d(want, (2, 1, 1), (2, 1, 1))
    if case.form == "nonfinite":
        assert torch.isnan(want).any() and torch.isinf(want).any()
        assert int(torch.isnan(want).any(dim=1).sum()) == (2 if tpool else 1)       # the NaN of both sides of the pair max came through
    to = t // 2 if tpool else t
    rows = n * to * h * w
    ld = case.form == "ld"
    ldw, off = (cout + 16, 8) if ld else (cout, 0)
    buf = torch.full((GUARD + rows + GUARD, ldw), 7.0, dtype=tdt, device="cuda")
    view = buf[GUARD:GUARD + rows, off:off + cout]
    assert view.data_ptr() % 16 == 0
    if dual:
        hh.conv_dual(x.cuda(), sd["w.weight"], hh.fold_bn(sd, "bn"), x2.cuda(), sd["w2.weight"], hh.fold_bn(sd, "bn2"), (1, 1, 1), dtype,
                     out=view, out_ld=ldw if ld else 0)
        ran = hh.conv_dual.last_variant
    else:
        hh.conv_bn_act(x.cuda(), sd["w.weight"], *hh.fold_bn(sd, "bn"), (1, 1, 1), (0, 0, 0), relu, dtype,
                       residual=res.cuda() if case.res else None, out=view, out_ld=ldw if ld else 0, tpool=int(tpool), workspace=None)
        ran = hh.conv_bn_act.last_variant
    # another kernel took the shape: the case tested nothing (change the shape, not this)
    assert ran == 10, "ran on variant %d, not on 10 (change the shape, not this)" % ran
    host = buf.cpu()
    got = host[GUARD:GUARD + rows, off:off + cout].double()
    host[GUARD:GUARD + rows, off:off + cout] = 7.0
    assert torch.all(host == 7.0), "%d guard elements around the output were written" % int((host != 7.0).sum())
    got = got.reshape(n, to, h, w, cout).permute(0, 4, 1, 2, 3)
    hh.compare(got, want, (TOL_DUAL if dual else TOL)[dtype], "%s[%s] %d tiles / %d workgroups in %d streams, my_tiles %% %d in %s" % (
        case.name, dtype, tiles, groups, streams, nslot(cin), list(case.residues)))


@pytest.mark.parametrize("cin,cout", [(64, 256), (128, 512), (256, 1024)])
def test_conv111_refuses_fp32(cin, cout):
    """the stream is a 16-bit kernel: the shapes it takes in f16 and bf16 get a generic tile in fp32"""
    shape = (1, 1, 1, 1 << 18, cin)
    for dtype in DT16:
        assert hh.conv_work_units(shape, cout, (1, 1, 1), dtype)[0] == 10, "change the shape, not this"
    v = hh.conv_work_units(shape, cout, (1, 1, 1), "f32")[0]
    assert v != 10 and v in (0, 1, 2, 3, 5, 6, 7, 12), v
