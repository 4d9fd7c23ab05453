"""GPU: the persistent conv kernels - conv133g / conv311g (variants 11 / 13), conv311 (8), conv133 (4) - with SEVERAL work units per
workgroup, against the oracle in fp64.  A workgroup of these kernels walks units b, b + grid, ... and issues the first operands of
its next unit under the epilogue of the current one (conv133g: `has_next` - the second patch buffer, a counted wait over the DMA
that is in flight; conv311: the stage stream runs on across the tile boundary, into the other ring slot).  The layer tests
(tests/test_hip_layers.py) run these kernels at no more units than a 256-CU device has workgroups, i.e. one unit each; the networks
ship them at up to 49 rounds.  The fifth persistent kernel, the 1x1x1 stream conv111 (variant 10), has its own file:
tests/test_hip_conv111.py, over the tiles per workgroup and the residues of its unrolled tile loop that ship.

Sizing at run time.  af_conv_work_units (the launchers' own geometry and grid expression) answers (units, workgroups) for a layer;
a case names a ROUNDS CLASS and the frame / clip count is computed from W = workgroups on this device (and the units per frame or
clip, also asked) so that the unit count U is
    "1"    U = W                 every workgroup one unit: the prefetch branch is skipped everywhere (conv311: the whole clips next below W)
    "1-2"  U = W + 44            44 workgroups run a second unit, the others end behind their first
    "2"    U = 2 W               every workgroup two (conv311: 11 tiles per clip, the whole clips next below 2 W)
    ">2"   U = 3 W + 37 (+ 38 where units come in pairs)
    "3W"   U = 3 W exactly       (key class ">2")
    "8"    U = 8 W + 37          (conv311 64 -> 64 only; key class ">2")
rounded up to whole frames (kT = 3: to two clips of equal length, so that a clip boundary falls into a later unit of a workgroup;
the temporal kernels always run several clips).  Every case asserts its variant and its class from the library's answer: a case
that meant three units per workgroup and ran one would test nothing.

Operands are rounded to the storage type on both sides, the reference is oracle.conv_bn_act in fp64.  Tolerances, relative to
max|want|, are the project's own: f32 2e-6 * max(1, K / 1024), f16 1.5e-3, bf16 1.2e-2.  The output is a view into a buffer
prefilled with 7.0: 64 guard rows before and after and, in the "ld" form (out_ld = cout + 16), 8 guard channels left and right;
all of them must still be 7.0.  The non-finite cases (bf16) put one NaN and one +inf into units that are NOT the first of their
workgroup.

CASES is plain data (no device needed): tests/test_host_cpu.py::test_persist_matrix_covers_what_ships compares case_key() of
every case with what the three networks ship on these kernels."""
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
GUARD = 64
TOL = {"f32": 2e-6, "f16": 1.5e-3, "bf16": 1.2e-2}
DT16 = ("f16", "bf16")
DT_ALL = ("f32", "f16", "bf16")
KEY_CLASS = {"1": "1", "1-2": "1-2", "2": "2", ">2": ">2", "3W": ">2", "8": ">2"}
FORMS = ("relu", "linear", "ld", "nonfinite")        # linear: no ReLU; ld: out_ld = cout + 16; nonfinite: ReLU, one NaN and one +inf

# variant: 4 conv133, 8 conv311, 11 conv133g, 13 conv311g; kernel (kt, kh, kw) with padding k // 2; t: frames per clip of the temporal
# kernels (None: spatial - the frame count is what the rounds class asks for); hw: the frame; rounds: the class (module docstring)
Case = collections.namedtuple("Case", "name variant kernel cin cout t hw rounds form dtypes")


def _build_cases():
    cases = []

    def add(variant, kernel, cin, cout, t, hw, rounds, more=False, forms=(), dtypes=DT16):
        """a ReLU case per rounds class; more: also linear, ld and nonfinite at "1-2"; forms: further forms at "1-2" """
        for r in rounds:
            for form in ("relu",) + ((("linear", "ld", "nonfinite") if more else tuple(forms)) if r == "1-2" else ()):
                name = "v%d-%dx%dx%d-%dto%d-%s%dx%d-r%s-%s" % (variant, kernel[0], kernel[1], kernel[2], cin, cout,
                                                                "" if t is None else "T%d-" % t, hw[0], hw[1], r, form)
                cases.append(Case(name, variant, kernel, cin, cout, t, hw, r, form, dtypes))

    s133, s333, t311 = (1, 3, 3), (3, 3, 3), (3, 1, 1)
    # ---- conv133g, 1x3x3.  256 channels: whole 14-row frames on the 3-slot ring, 5-piece instantiation
    add(11, s133, 64, 256, None, (14, 14), ("1-2", "2", ">2", "3W"))      # 1 slab: 9 steps per unit; 31 patch pieces, waves differ in piece count
    add(11, s133, 128, 256, None, (14, 14), ("1-2", ">2"))                # 2 slabs
    add(11, s133, 192, 256, None, (13, 14), ("1-2", ">2"))                # 3 slabs, ragged band
    add(11, s133, 256, 256, None, (14, 14), ("1", "1-2", "2", ">2"), more=True)      # ships (I3D s4 `b`): 4 slabs
    add(11, s133, 256, 256, None, (7, 20), ("1-2",))                      # 24 pieces: every wave the same count
    # 128 channels
    add(11, s133, 128, 128, None, (28, 28), ("1", "1-2", "2", ">2"), more=True)      # ships (s3 `b`): two bands, 2-slot ring, 8-piece instantiation
    add(11, s133, 64, 128, None, (28, 28), ("1-2", ">2"))                 # 1 slab on the 2-slot ring
    add(11, s133, 256, 128, None, (27, 26), ("1-2", ">2"))                # bands of 14 + 13 rows, 3-slot ring
    add(11, s133, 128, 128, None, (14, 28), ("1-2",))                     # one band per frame
    # ---- conv133g, 3x3x3 (two clips)
    add(11, s333, 64, 64, None, (56, 56), ("1-2", ">2"))                  # 7 bands per frame, 9-piece instantiation
    add(11, s333, 64, 64, None, (50, 53), ("1-2",))                       # 3-slot ring
    add(11, s333, 64, 128, None, (28, 28), ("1-2",))
    add(11, s333, 128, 256, None, (14, 14), ("1-2",))
    # ---- conv311g: the frame holds the stated number of chunks of P pixels (P = 448 / T into 128 channels, 224 / T into 256)
    add(13, t311, 256, 128, 16, (4, 7), ("1", "1-2", "2", ">2", "3W"), more=True)         # ships: P = 28, 1 chunk per clip
    add(13, t311, 256, 128, 16, (7, 7), (">2",))                          # 2 chunks, the last ragged
    add(13, t311, 512, 128, 16, (4, 7), ("1", "1-2", ">2"))                    # ships: 8 slabs
    add(13, t311, 512, 256, 16, (2, 7), ("1", "1-2", "2", ">2"), more=True)    # ships: P = 14, 1 chunk
    add(13, t311, 512, 256, 16, (3, 7), ("1-2",))                         # 2 chunks, the last ragged
    add(13, t311, 512, 256, 16, (7, 10), ("1-2",))                        # 5 chunks
    add(13, t311, 1024, 256, 16, (2, 7), ("1", "1-2", "2"))                    # ships: 16 slabs
    add(13, t311, 64, 256, 16, (2, 7), ("1-2", ">2"))                     # 1 slab: 3 steps per unit = the ring depth
    add(13, t311, 64, 128, 16, (4, 7), ("1-2", ">2"))
    add(13, t311, 128, 128, 32, (2, 7), ("1-2",))                         # P = 14
    add(13, t311, 64, 256, 8, (4, 7), ("1-2",))                           # P = 28 into 256 channels: 2 slots (reached through the C ABI only)
    add(13, t311, 64, 256, 32, (1, 7), ("1-2",))                          # P = 7 (C ABI only)
    # ---- conv311: 9 x 9 frames = 11 chunks at P = 8 (T = 32 into 64 channels, T = 16 into 128), 6 at P = 16 (T = 16 into 64), the last
    # one ragged and landing in later tiles of a workgroup.  64 channels also in f32 (K slabs of 32 channels)
    add(8, t311, 64, 64, 32, (9, 9), ("1-2", "2", ">2", "8"), more=True, dtypes=DT_ALL)   # ships at up to 49 rounds; 1 slab: the first slab alternates ring slots
    add(8, t311, 128, 64, 32, (9, 9), ("1", "1-2", ">2"), dtypes=DT_ALL)            # 2 slabs
    add(8, t311, 192, 64, 16, (9, 9), (">2",), dtypes=DT_ALL)            # 3 slabs
    add(8, t311, 256, 64, 32, (9, 9), ("1", "1-2", ">2"), dtypes=DT_ALL)            # 4 slabs
    add(8, t311, 32, 64, 32, (9, 9), (">2",), dtypes=("f32",))           # f32: 1 slab
    # the 128-channel form: 1, 4, 8 slabs.  conv311g comes first for these layers wherever it finds 192 units of 28 pixels with 60 % of
    # them real, which 74 clips of 9 x 9 are: the ">2" cases run 5 x 6 frames (30 of 56 pixels: refused there; here 4 chunks, the
    # last ragged)
    for cin_, more_ in ((64, ()), (256, ("ld",)), (512, ())):
        add(8, t311, cin_, 128, 16, (9, 9), (("1",) if cin_ == 512 else ()) + ("1-2",), forms=more_)
        add(8, t311, cin_, 128, 16, (5, 6), (">2",))
    # ---- conv133: several strips per workgroup into the guarded buffer (out_ld stays 0)
    add(4, s133, 64, 64, None, (30, 27), ("1-2",))
    add(4, s133, 64, 64, None, (56, 56), ("1-2",))
    assert len({c.name for c in cases}) == len(cases)
    return cases


CASES = _build_cases()


def kslabs(cin, dtype):
    return cin // (32 if dtype == "f32" else 64)


def case_key(case, dtype):
    """what the closure test compares: (variant, dtype, cout, kernel, K slabs, T of the temporal kernels or (h, w) of the spatial
    ones, rounds class)"""
    return (case.variant, dtype, case.cout, tuple(case.kernel), kslabs(case.cin, dtype), case.t if case.kernel[1] == 1 else tuple(case.hw),
            KEY_CLASS[case.rounds])


def rounds_class(units, workgroups):
    """the class of a launch of `units` work units on `workgroups` persistent workgroups, as the closure test keys shipped layers"""
    return "1" if units <= workgroups else "1-2" if units < 2 * workgroups else "2" if units == 2 * workgroups else ">2"


def _pad(kernel):
    return tuple(k // 2 for k in kernel)


def _shape(case, count):
    """input (n, t, h, w, cin) of `count` frames (spatial: one clip; kT = 3: two clips) or clips (temporal)"""
    if case.t is not None:
        return (count, case.t) + tuple(case.hw) + (case.cin,)
    if case.kernel[0] == 3:
        return (2, count // 2) + tuple(case.hw) + (case.cin,)
    return (1, count) + tuple(case.hw) + (case.cin,)


def plan(case, dtype):
    """(input shape, units, workgroups, units per frame / clip) for the case's rounds class on this device"""
    ask = lambda count: hh.conv_work_units(_shape(case, count), case.cout, case.kernel, dtype, _pad(case.kernel))
    # W and the units per frame from a launch of more units than a device has CUs: 2048 frames pass every gate of conv133g / conv311g;
    # conv311 into 128 channels has none and loses 9 x 9 frames to conv311g from 64 clips on (3 chunks of 28 pixels: 192 units)
    for probe in (2048, 32):
        v, units, W = ask(probe)
        if v == case.variant:
            break
    assert v == case.variant, "variant %d, not %d (change the shape, not this)" % (v, case.variant)
    assert units % probe == 0 and W < units
    per = units // probe
    target = {"1": W, "1-2": W + 44, "2": 2 * W, ">2": 3 * W + 37, "3W": 3 * W, "8": 8 * W + 37}[case.rounds]
    count = target // per if case.rounds in ("1", "2", "3W") else -(-target // per)
    if case.t is None and case.kernel[0] == 3:
        count += count % 2
    v, units, groups = ask(count)
    assert v == case.variant, "variant %d, not %d at %d frames (change the shape, not this)" % (v, case.variant, count)
    check_class(case, units, groups, per, W)
    return _shape(case, count), units, groups, per


def check_class(case, units, groups, per, W):
    """the launch is in the case's rounds class, W = the workgroups a launch of many units has (change the shape, not this)"""
    what = "%s: %d units on %d workgroups of %d (change the shape, not this)" % (case.name, units, groups, W)
    assert groups == min(units, W), what
    if case.rounds == "1":
        assert W - per < units <= W, what
    elif case.rounds == "1-2":
        assert W < units < 2 * W and units - W < W // 2, what
    elif case.rounds == "2":
        assert 2 * W - per < units <= 2 * W and (per > 1 or units == 2 * W), what
    elif case.rounds == "3W":
        assert units == 3 * W, what
    elif case.rounds == ">2":
        assert 3 * W < units < 4 * W and units % W != 0, what
    else:
        assert 8 * W < units < 9 * W, what
    assert rounds_class(units, W) == KEY_CLASS[case.rounds] or (case.rounds == "2" and per > 1), what


def _bn_layout(prefix, ch):
    return [(prefix + s, (ch,), "float32") for s in (".weight", ".bias", ".running_mean", ".running_var")]


def _ncdhw64(x_ndhwc):
    return x_ndhwc.permute(0, 4, 1, 2, 3).contiguous().double()       # (transposed in the storage type: the smaller copy)


# the operands and the fp64 reference (before the ReLU) of the last geometry: the forms of one geometry share them
_last = {}


def _operands(case, dtype, shape):
    key = (case.variant, case.kernel, case.cin, case.cout, shape, dtype, case.form == "nonfinite")
    if _last.get("key") == key:
        return _last["val"]
    _last.clear()
    tdt = hh.TORCH_DT[dtype]
    seed = 9000 + zlib.crc32(repr(key[:5]).encode()) % 90000
    kt, kh, kw = case.kernel
    sd = synth.fill_layout([("w.weight", (case.cout, case.cin, kt, kh, kw), "float32")] + _bn_layout("bn", case.cout), seed)
    sd["w.weight"] = sd["w.weight"].to(tdt).float()
    x = synth.synthetic_tensor(shape, seed).to(tdt)            # NDHWC, in the storage type
    val = (x, sd)
    if case.form != "nonfinite":
        sd64 = {k: v.double() for k, v in sd.items()}
        val += (oracle.conv_bn_act(_ncdhw64(x), sd64["w.weight"], sd64, "bn", (1, 1, 1), _pad(case.kernel), False),)
    _last["key"], _last["val"] = key, val
    return val


def _poison(case, x, W, per):
    """one NaN and one +inf, in two frames (kT = 1: no output sees both) / clips whose units all come behind the first W: neither
    is in the first unit of a workgroup"""
    first = -(-W // per) + 1
    assert case.kernel[0] == 1 or case.t is not None
    if case.t is not None:
        assert first + 1 < x.shape[0]
        x[first, 5, 1, 3, 1] = float("nan")
        x[first + 1, x.shape[1] - 1, x.shape[2] - 1, 2, 2] = float("inf")
    else:
        frames = x.reshape((-1,) + tuple(x.shape[2:]))
        assert first + 1 < frames.shape[0] and frames.data_ptr() == x.data_ptr()
        frames[first, 2, 3, 1] = float("nan")
        frames[first + 1, x.shape[2] - 3, x.shape[3] - 2, 2] = float("inf")


def _params():
    out = []
    for c in CASES:
        for dt in c.dtypes:
            if c.form == "nonfinite" and dt != "bf16":
                continue
            out.append((dt, c))
    # the forms of one geometry and dtype next to each other (they share the reference)
    order = {c.name: i for i, c in enumerate(CASES)}
    geo = lambda c: min(order[o.name] for o in CASES if o[1:8] == c[1:8])
    out.sort(key=lambda p: (geo(p[1]), p[0], FORMS.index(p[1].form)))
    return out


PARAMS = _params()


@pytest.mark.parametrize("dtype,case", PARAMS, ids=["%s-%s" % (dt, c.name) for dt, c in PARAMS])
def test_conv_persistent_rounds(dtype, case):
    tdt = hh.TORCH_DT[dtype]
    shape, units, groups, per = plan(case, dtype)
    n, t, h, w, cin = shape
    cout, pad = case.cout, _pad(case.kernel)
    relu = case.form != "linear"
    if case.form == "nonfinite":
        x, sd = _operands(case, dtype, shape)
        x = x.clone()
        _poison(case, x, groups, per)
        sd64 = {k: v.double() for k, v in sd.items()}
        want = oracle.conv_bn_act(_ncdhw64(x), sd64["w.weight"], sd64, "bn", (1, 1, 1), pad, False)
        assert torch.isnan(want).any() and torch.isinf(want).any()
    else:
        x, sd, want = _operands(case, dtype, shape)
    if relu:
        want = F.relu(want)
    rows = n * t * h * w
    ld = case.form == "ld"
    assert not (ld and case.variant == 4)                    # conv133 writes whole 64-channel rows only
    ldw, off = (cout + 16, 8) if ld else (cout, 0)
    buf = torch.full((GUARD + rows + GUARD, ldw), 7.0, dtype=tdt, device="cuda")
    view = buf[GUARD:GUARD + rows, off:off + cout]
    assert view.data_ptr() % 16 == 0
    hh.conv_bn_act(x.cuda(), sd["w.weight"], *hh.fold_bn(sd, "bn"), (1, 1, 1), pad, relu, dtype, out=view, out_ld=ldw if ld else 0,
                   workspace=None)
    # another kernel took the shape: the case tested nothing (change the shape, not this)
    assert hh.conv_bn_act.last_variant == case.variant, "ran on variant %d, not on %d" % (hh.conv_bn_act.last_variant, case.variant)
    host = buf.cpu()
    got = host[GUARD:GUARD + rows, off:off + cout].double()
    host[GUARD:GUARD + rows, off:off + cout] = 7.0
    assert torch.all(host == 7.0), "%d guard elements around the output were written" % int((host != 7.0).sum())
    got = got.reshape(n, t, h, w, cout).permute(0, 4, 1, 2, 3)
    kk = cin * case.kernel[0] * case.kernel[1] * case.kernel[2]
    tol = TOL[dtype] * (max(1.0, kk / 1024.0) if dtype == "f32" else 1.0)
    hh.compare(got, want, tol, "%s[%s] %d units / %d workgroups" % (case.name, dtype, units, groups))
