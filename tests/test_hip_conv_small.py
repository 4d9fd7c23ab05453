"""GPU: conv_small (variant 9, csrc/af_conv_small.hip), the direct-gather path of SlowFast's Fast pathway, against fp64.  A wave
of this kernel owns 64 output positions per step, gathers its K chunks (tap, 8 channels; nch = taps * cin / 8 [+ cin2 / 8] of
them, four per MFMA step, at most 32) straight from the NDHWC tensor with out-of-range offsets for padding taps, and walks its
groups of 64 positions grid-stride: the launch is capped at 8192 workgroups of 256 positions, so from M > 2 097 152 output
positions on some waves run a second group (the networks ship that at batch 24 and 32).

The cases:
  * the eight shapes the network ships, at small frames - two clips wherever kT > 1, so that the temporal padding must read zeros
    and not the neighbouring clip -, with M % 64 in {0, 1, 17, 63} among them, the stride-(1,2,2) shape on odd h and w, and the
    lateral (5x1x1, stride (8,1,1), 8 -> 16) also as it ships: out_ld = 80 at channel offset 64 of a wider buffer;
  * K-chunk edges: nch = 1, 5, 27, 32, and a refused neighbour (32 -> 8 1x3x3: nch = 36) that must report another variant and
    still match;
  * a second segment (hh.conv_dual: main 1x1x1 + strided 1x1x1) of 1 + 1, 2 + 3 (a partial MFMA step that mixes both segments)
    and 8 + 24 chunks, the second input at stride (1,2,2) for two of them;
  * residual with and without ReLU, and in the "ld" form;
  * grid-stride: every shape that ships beyond 2 097 152 positions, on one clip of 11 frames of 437 x 437 (2 100 659 positions =
    32 822 groups + 51 positions: 55 waves run two groups, the last group is ragged);
  * non-finite (bf16): one NaN and one +inf in the input, ReLU on.

Operands are rounded to the storage type on both sides, the reference is oracle.conv_bn_act in fp64, residual added and ReLU
applied in fp64.  Tolerances, relative to max|want|: f16 1.5e-3, bf16 1.2e-2; with a second segment (hh.conv_dual folds the BN
scales into the packed weights: one more rounding of every weight) f16 3e-3, bf16 2.4e-2.  The output is a view into a buffer
prefilled with 7.0: 128 guard rows before and after and, in the "ld" form (out_ld = cout + 16), 8 guard channels left and right
(the lateral's shipped form: 64 before, none behind); all of them must still be 7.0.  Every case asserts the variant the library
reports.

CASES is plain data (no device needed): tests/test_host_cpu.py::test_conv111_and_small_matrices_cover_what_ships compares
case_key() of every case with what SlowFast ships on this kernel."""
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
GRID_POSITIONS = 8192 * 256                    # the launch cap: beyond it the grid-stride loop runs a second time
TOL = {"f16": 1.5e-3, "bf16": 1.2e-2}
TOL_DUAL = {"f16": 3e-3, "bf16": 2.4e-2}
DT16 = ("f16", "bf16")

# dims: the input (n, t, h, w); cin2 / stride2: the second segment (hh.conv_dual), whose input is the output grid times stride2;
# form: relu, linear (no ReLU), ld (out_ld = cout + 16), lateral (out_ld = 80, channel offset 64), nonfinite; variant: 9, or None =
# refused (any other); mod64: what M % 64 must be (None: not pinned)
Case = collections.namedtuple("Case", "name cin cout kernel stride pad dims cin2 stride2 res form variant mod64")


def _build_cases():
    cases = []

    def add(name, cin, cout, kernel, stride, pad, dims, cin2=0, stride2=(1, 1, 1), res=False, form="relu", variant=9, mod64=None):
        cases.append(Case(name, cin, cout, kernel, stride, pad, dims, cin2, stride2, res, form, variant, mod64))

    one, t3, s3, t5 = (1, 1, 1), (3, 1, 1), (1, 3, 3), (5, 1, 1)
    # ---- the shipped shapes
    add("8to8-3x1x1", 8, 8, t3, one, (1, 0, 0), (2, 4, 8, 8), mod64=0)
    add("8to8-1x3x3", 8, 8, s3, one, (0, 1, 1), (1, 5, 7, 11), mod64=1)
    add("32to8-3x1x1", 32, 8, t3, one, (1, 0, 0), (2, 5, 6, 7))
    add("32to16-3x1x1", 32, 16, t3, one, (1, 0, 0), (2, 3, 7, 9))
    add("16to16-1x3x3-s2", 16, 16, s3, (1, 2, 2), (0, 1, 1), (1, 3, 9, 33), mod64=63)           # odd h, w: 5 x 17 outputs per frame
    add("16to16-1x3x3", 16, 16, s3, one, (0, 1, 1), (1, 3, 7, 13), mod64=17)
    add("64to16-3x1x1", 64, 16, t3, one, (1, 0, 0), (2, 4, 5, 9))
    add("lateral-8to16-5x1x1-s8", 8, 16, t5, (8, 1, 1), (2, 0, 0), (2, 32, 5, 7))               # nch = 5
    add("lateral-8to16-5x1x1-s8-at64of80", 8, 16, t5, (8, 1, 1), (2, 0, 0), (2, 32, 5, 7), form="lateral")
    # ---- K-chunk edges
    add("nch1-8to8-1x1x1", 8, 8, one, one, (0, 0, 0), (1, 3, 5, 9))
    add("nch27-8to16-3x3x3", 8, 16, (3, 3, 3), one, (1, 1, 1), (2, 3, 6, 7))
    add("nch32-64to8-1x2x2", 64, 8, (1, 2, 2), one, (0, 0, 0), (1, 3, 8, 10))
    add("nch36-32to8-1x3x3-refused", 32, 8, s3, one, (0, 1, 1), (1, 3, 7, 9), variant=None)
    # ---- second segment: 1 + 1, 2 + 3 and 8 + 24 chunks
    add("dual-8+8to8", 8, 8, one, one, (0, 0, 0), (2, 3, 5, 7), cin2=8)
    add("dual-16+24to16-s2", 16, 16, one, one, (0, 0, 0), (2, 3, 5, 7), cin2=24, stride2=(1, 2, 2))
    add("dual-64+192to8-s2", 64, 8, one, one, (0, 0, 0), (1, 3, 6, 7), cin2=192, stride2=(1, 2, 2))
    add("dual-8+8to8-ld", 8, 8, one, one, (0, 0, 0), (2, 3, 5, 7), cin2=8, form="ld")
    # ---- residual
    add("16to16-1x3x3-res", 16, 16, s3, one, (0, 1, 1), (1, 3, 7, 13), res=True)
    add("8to8-3x1x1-res-linear", 8, 8, t3, one, (1, 0, 0), (2, 4, 8, 8), res=True, form="linear")
    add("32to16-3x1x1-res-ld", 32, 16, t3, one, (1, 0, 0), (2, 3, 7, 9), res=True, form="ld")
    # ---- grid-stride: the shapes that ship beyond GRID_POSITIONS outputs (8 -> 8 and 32 -> 8 / 16 of s2 at batch 24 and 32)
    big = (1, 11, 437, 437)
    add("big-8to8-3x1x1", 8, 8, t3, one, (1, 0, 0), big, mod64=51)
    add("big-8to8-1x3x3", 8, 8, s3, one, (0, 1, 1), big, mod64=51)
    add("big-32to8-3x1x1", 32, 8, t3, one, (1, 0, 0), big, mod64=51)
    add("big-32to16-3x1x1", 32, 16, t3, one, (1, 0, 0), big, mod64=51)
    # ---- non-finite
    add("8to8-1x3x3-nonfinite", 8, 8, s3, one, (0, 1, 1), (1, 5, 7, 11), form="nonfinite")
    add("32to16-3x1x1-nonfinite", 32, 16, t3, one, (1, 0, 0), (2, 3, 7, 9), form="nonfinite")
    assert len({c.name for c in cases}) == len(cases)
    return cases


CASES = _build_cases()


def out_dims(case):
    return tuple((d + 2 * p - k) // s + 1 for d, p, k, s in zip(case.dims[1:], case.pad, case.kernel, case.stride))


def positions(case):
    to, ho, wo = out_dims(case)
    return case.dims[0] * to * ho * wo


def shipped_key(dtype, cin, cout, kernel, stride, second, res, ld, m):
    """what the closure test compares; m: the output positions of the launch"""
    return (dtype, cin, cout, tuple(kernel), tuple(stride), bool(second), bool(res), bool(ld), m > GRID_POSITIONS)


def case_key(case, dtype):
    return shipped_key(dtype, case.cin, case.cout, case.kernel, case.stride, case.cin2, case.res, case.form in ("ld", "lateral"), positions(case))


def _bn_layout(prefix, ch):
    return [(prefix + s, (ch,), "float32") for s in (".weight", ".bias", ".running_mean", ".running_var")]


def _ncdhw64(x_ndhwc):
    return x_ndhwc.permute(0, 4, 1, 2, 3).contiguous().double()


def _shape2(case):
    """the second input: the output grid times stride2"""
    return (case.dims[0],) + tuple(d * s for d, s in zip(out_dims(case), case.stride2)) + (case.cin2,)


def _reference(case, x, x2, sd):
    sd64 = {k: v.double() for k, v in sd.items()}
    want = oracle.conv_bn_act(_ncdhw64(x), sd64["w.weight"], sd64, "bn", case.stride, case.pad, False)
    if x2 is not None:
        want = want + oracle.conv_bn_act(_ncdhw64(x2), sd64["w2.weight"], sd64, "bn2", case.stride2, (0, 0, 0), False)
    return want


# the operands and the fp64 reference (before residual and ReLU) of the last geometry: computed once per geometry and dtype
_last = {}


def _operands(case, dtype):
    key = (case.cin, case.cout, case.kernel, case.stride, case.pad, case.dims, case.cin2, case.stride2, dtype)
    if _last.get("key") == key:
        return _last["val"]
    _last.clear()
    tdt = hh.TORCH_DT[dtype]
    seed = 12000 + zlib.crc32(repr(key[:8]).encode()) % 90000
    lay = [("w.weight", (case.cout, case.cin) + tuple(case.kernel), "float32")] + _bn_layout("bn", case.cout)
    if case.cin2:
        lay += [("w2.weight", (case.cout, case.cin2, 1, 1, 1), "float32")] + _bn_layout("bn2", case.cout)
    sd = synth.fill_layout(lay, seed)
    for name in ("w.weight", "w2.weight"):
        if name in sd:
            sd[name] = sd[name].to(tdt).float()
    x = synth.synthetic_tensor(tuple(case.dims) + (case.cin,), seed).to(tdt)            # NDHWC, in the storage type
    x2 = synth.synthetic_tensor(_shape2(case), seed + 1).to(tdt) if case.cin2 else None
    res = synth.synthetic_tensor((case.dims[0],) + out_dims(case) + (case.cout,), seed + 2).to(tdt)
    _last["key"], _last["val"] = key, (x, x2, res, sd, _reference(case, x, x2, sd))
    return _last["val"]


def _params():
    out = [(dt, c) for c in CASES for dt in DT16 if c.form != "nonfinite" or dt == "bf16"]
    first = {}
    for i, c in enumerate(CASES):
        first.setdefault(c[1:9], i)
    out.sort(key=lambda p: (first[p[1][1:9]], p[0], CASES.index(p[1])))          # one geometry and dtype next to each other
    return out


PARAMS = _params()


@pytest.mark.parametrize("dtype,case", PARAMS, ids=["%s-%s" % (dt, c.name) for dt, c in PARAMS])
def test_conv_small_vs_fp64(dtype, case):
    tdt = hh.TORCH_DT[dtype]
    n = case.dims[0]
    to, ho, wo = out_dims(case)
    rows, cout, dual = positions(case), case.cout, bool(case.cin2)
    assert case.mod64 is None or rows % 64 == case.mod64, "M = %d (change the shape, not this)" % rows
    relu = case.form != "linear"
    assert not (dual and (case.res or not relu))             # af_conv3d_dual_bn_act: no residual, always the ReLU
    x, x2, res, sd, want = _operands(case, dtype)
    if case.form == "nonfinite":                             # (kT = 3: the two frames are three apart or in two clips - no output sees both)
        x = x.clone()
        x[0, 1, 2, 3, 1] = float("nan")
        x[n - 1, case.dims[1] - 1, case.dims[2] - 1, case.dims[3] - 2, case.cin - 1] = float("inf")
        want = _reference(case, x, x2, sd)
        assert torch.isnan(want).any() and torch.isinf(want).any()
    if case.res:
        want = want + _ncdhw64(res)
    if relu:
        want = F.relu(want)
    ldw, off = {"ld": (cout + 16, 8), "lateral": (80, 64)}.get(case.form, (cout, 0))
    ld = ldw != cout
    buf = torch.full((GUARD + rows + GUARD, ldw), 7.0, dtype=tdt, device="cuda")
    view = buf[GUARD:GUARD + rows, off:off + cout]
    assert view.data_ptr() % 16 == 0
    if dual:
        hh.conv_dual(x.cuda(), sd["w.weight"], hh.fold_bn(sd, "bn"), x2.cuda(), sd["w2.weight"], hh.fold_bn(sd, "bn2"), case.stride2, dtype,
                     out=view, out_ld=ldw if ld else 0)
        ran = hh.conv_dual.last_variant
    else:
        hh.conv_bn_act(x.cuda(), sd["w.weight"], *hh.fold_bn(sd, "bn"), case.stride, case.pad, relu, dtype,
                       residual=res.cuda() if case.res else None, out=view, out_ld=ldw if ld else 0)
        ran = hh.conv_bn_act.last_variant
    # another kernel took the shape: the case tested nothing (change the shape, not this)
    assert (ran == 9) if case.variant == 9 else (ran != 9), "ran on variant %d (change the shape, not this)" % ran
    host = buf.cpu()
    got = host[GUARD:GUARD + rows, off:off + cout].double()
    host[GUARD:GUARD + rows, off:off + cout] = 7.0
    assert torch.all(host == 7.0), "%d guard elements around the output were written" % int((host != 7.0).sum())
    got = got.reshape(n, to, ho, wo, cout).permute(0, 4, 1, 2, 3)
    groups = -(-rows // 64)
    hh.compare(got, want, (TOL_DUAL if dual else TOL)[dtype], "%s[%s] M = %d: %d groups of 64 on %d waves, %d live in the last" % (
        case.name, dtype, rows, groups, min(-(-rows // 256), 8192) * 4, rows - (groups - 1) * 64))


def test_conv_small_refuses_fp32():
    """the narrow-layer path is a 16-bit kernel: every case's shape gets a generic tile in fp32 (and variant 9, where meant, at 16 bits)"""
    for case in CASES:
        ask = lambda dt: hh.conv_variant(tuple(case.dims) + (case.cin,), case.cout, case.kernel, dt, case.stride, case.pad,
                                         _shape2(case) if case.cin2 else None, case.stride2)
        assert ask("f32") != 9, case.name
        for dt in DT16:
            assert (ask(dt) == 9) == (case.variant == 9), "%s[%s]: change the shape, not this" % (case.name, dt)
