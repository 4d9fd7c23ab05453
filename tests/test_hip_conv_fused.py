"""GPU: the fused conv launches - conv_ca (af_conv3d_ca_bn_act), conv_cpa (af_conv3d_cpa_bn_act), block_abc (af_block_abc_bn_act)
and conv_bc (af_conv3d_bc_bn_act) - over K slabs, rounds of tiles per workgroup, kernel forms and time segments, against the oracle
in fp64.  conv_ca and conv_cpa are persistent: workgroup b walks tiles b, b + grid, ... as ONE stage stream (a stage = one
64-channel slab of one tile) through a 3-slot image ring and a 2-slot `a`-weight ring, with counted vmcnt waits and the residual
fetched two stages ahead.  Which ring slot a tile starts on depends on the slab count (1: both rings rotate every tile, 2 / 4: a
tile always starts on weight slot 0, 3: the image ring never rotates between tiles), how a workgroup ends on the tiles it has.  The
layer tests (tests/test_hip_layers.py) run 2 and 4 slabs at 4 to 5 tiles per workgroup; the networks ship 4.6 to 49.

Sizing at run time.  af_conv_ca_work_units / af_conv_cpa_work_units / af_block_abc_work_units (the launchers' own geometry) answer
how a launch is cut; a conv_ca / conv_cpa case names a ROUNDS CLASS and its clip count is computed from W = workgroups on this
device and the tiles per clip (also asked), so that the tile count U is
    "4"    U = 4 W exactly       every workgroup ends on the same stage (below 4 W the library does not fuse: asserted once per kernel)
    "4-5"  U = 4 W + 44          44 workgroups run a fifth tile
    ">5"   U = 6 W + 37          six to seven tiles per workgroup: a whole period of both rings for any slab count
rounded up to whole clips.  Every case asserts its form (plain / plain-CWL / projection) and its class from the library's answer: a
case that meant one form and ran another would test nothing.  block_abc launches one workgroup per unit, its variable is the
number of TIME SEGMENTS a clip is cut into (the `a` taps read across the segment boundaries): the shapes that ship (inner 8 at
56 x 56, inner 16 at 28 x 28, kT = 3, T = 32) at the clip counts that give 8, 4, 2 and 1 segments, asserted from the answer.

Reference: oracle.conv_bn_act in fp64 on operands rounded to the storage type on both sides, intermediates rounded where the kernel
rounds them (the trunk before the temporal conv; the a and b tensors of block_abc and the b tensor of conv_bc, which cross LDS in
the storage type), clip group by clip group.  The projection forms fold the BN scales into the weights in fp32 before the one
rounding, as the kernels' callers do.  Tolerances, relative to max|want|, are the layer tests' own: conv_ca / conv_cpa trunk f16
1.5e-3, bf16 1.2e-2, their `a` output 1.5 times that; conv_bc 2e-3 / 1.6e-2; block_abc 3e-3 / 2.4e-2, its projection form
4e-3 / 3e-2.  Every output - both outputs of conv_ca and conv_cpa - is a view into a buffer prefilled with 7.0 with 64 guard rows
before and after and, where the entry point takes out_ld (conv_bc, block_abc), out_ld = cout + 16 with 8 guard channels left and
right; all of them must still be 7.0.  The non-finite cases put one NaN and one +inf into `b` and one NaN into the residual, in
tiles that are NOT the first of their workgroup, and require the NaN on frames t - 1, t, t + 1 of its pixel in the `a` output and
nowhere else; the two-clip case puts them on both sides of a clip boundary that falls inside every workgroup's tile sequence
(the temporal padding is zero, the neighbouring clip is not read).

CASES is plain data (no device needed): tests/test_host_cpu.py::test_fused_matrix_covers_what_ships compares case_key() of every
case with what the three networks ship on these kernels.

Measured on an MI355X (W = 256): 63 cases, 122 tests, all pass in 261 - 283 s by machine - operands and the fp64 reference on
the CPU are most of it; the four 8-slab conv_ca tests (512 channels x 1068 tiles, the smallest their class allows) take 6 - 8 s,
every other test at most 6.5 s, the median 2 s.  The library's answers agree with the forms derived by hand from
conv_ca_lds_bytes at 160 KB (T = 16 with 512 channels fits LDS and is fused).
Worst max|d| / max|want| per kernel, f16 / bf16:
    conv_ca plain       trunk 4.4e-4 / 3.6e-3    a 4.3e-4 / 3.7e-3
    conv_ca projection  trunk 4.3e-4 / 3.7e-3    a 4.4e-4 / 3.3e-3
    conv_cpa            trunk 4.7e-4 / 3.7e-3    a 3.9e-4 / 3.2e-3
    block_abc           5.2e-4 / 3.4e-3          projection form 5.2e-4 / 4.3e-3
    conv_bc             4.1e-4 / 3.1e-3
"""
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
DT16 = ("f16", "bf16")
TOL = {"f16": 1.5e-3, "bf16": 1.2e-2}              # conv_ca / conv_cpa: the trunk; the `a` output 1.5 times that (a trunk value on a rounding boundary may round the other way)
TOL_BC = {"f16": 2e-3, "bf16": 1.6e-2}
TOL_ABC = {"f16": 3e-3, "bf16": 2.4e-2}
TOL_ABC_PROJ = {"f16": 4e-3, "bf16": 3e-2}
ROUNDS = ("4", "4-5", ">5")

# conv_ca: c trunk channels, t frames per clip, hw the frame, rounds the class, form what the library must answer, what: "" |
#   "nonfinite" | "clips2" (two clips, hw computed at run time)
CaCase = collections.namedtuple("CaCase", "name c t hw rounds form what dtypes")
# conv_cpa: T = 32 always
CpaCase = collections.namedtuple("CpaCase", "name c x_sub hw rounds what dtypes")
# block_abc: dims = (clips, t, h, w); rows / segments what the library must answer; what: "" | "nan"
AbcCase = collections.namedtuple("AbcCase", "name inner kta proj dims rows segments what dtypes")
# conv_bc: dims = (clips, t, h, w)
BcCase = collections.namedtuple("BcCase", "name cin cmid cout dims use_res dtypes")


def _build_cases():
    cases = []

    def ca(c, t, form, rounds, whats=("",), dtypes=DT16):
        # frames of 4 / 6 / 5 tiles per clip (4 divides 4 W; 5 and 6 leave the last clip's tiles spread over the workgroups)
        p = 256 // t
        for r in rounds:
            for what in whats:
                hw = {"4": (4, p), "4-5": (3, 2 * p), ">5": (5, p)}[r]
                cases.append(CaCase("ca-%s-T%d-C%d-r%s%s" % (form, t, c, r, "-" + what if what else ""), c, t, hw, r, form, what,
                                    ("bf16",) if what == "nonfinite" else dtypes))

    # ---- conv_ca, T = 32, plain: the c weights as an LDS image up to 320 channels (256 ships), plain loads from 512 on
    for c in (64, 128, 192, 256):
        ca(c, 32, "plain-CWL", ROUNDS)
    ca(512, 32, "plain", ("4-5",))                    # 8 slabs
    # T = 32, projection (256 ships)
    for c in (64, 192, 256):
        ca(c, 32, "projection", ("4-5", ">5"))
    # T = 16, plain: never the LDS image
    for c in (64, 128, 192, 512):
        ca(c, 16, "plain", ("4-5",))
    ca(256, 16, "plain", ROUNDS)
    for c in (128, 256):
        ca(c, 16, "projection", ("4-5",))
    # non-finite operands on the shipped form and on 3 slabs; the clip boundary inside every workgroup's tile sequence
    ca(256, 32, "plain-CWL", ("4-5",), ("nonfinite",))
    ca(192, 32, "plain-CWL", ("4-5",), ("nonfinite",))
    cases.append(CaCase("ca-plain-CWL-T32-C256-clips2", 256, 32, None, "4-5", "plain-CWL", "clips2", DT16))
    cases.append(CaCase("ca-plain-T16-C128-clips2", 128, 16, None, "4-5", "plain", "clips2", DT16))

    # ---- conv_cpa (off by default: AF_FUSE_CPA): tiles of 2 rows x 4 columns
    def cpa(c, rounds, what=""):
        for r in rounds:
            for sub in ((2,) if what else (1, 2)):
                hw = {"4": (4, 8), "4-5": (6, 8), ">5": (2, 20)}[r]
                cases.append(CpaCase("cpa-C%d-sub%d-r%s%s" % (c, sub, r, "-" + what if what else ""), c, sub, hw, r, what,
                                     ("bf16",) if what else DT16))

    for c in (64, 192, 512):
        cpa(c, ("4-5",))
    cpa(256, ROUNDS)                                  # ships when switched on
    cpa(256, ("4-5",), "nonfinite")

    # ---- block_abc: the Fast pathway's shapes, at the clip counts that give every time-segment count of batch 1 .. 32
    def abc(inner, hw, clips, segments, kta=3, proj=False, what="", rows=7, dtypes=DT16):
        cases.append(AbcCase("abc-i%d%s-%dx%d-n%d-s%d%s" % (inner, "-proj" if proj else "", hw[0], hw[1], clips, segments,
                                                            "-" + what if what else ""),
                             inner, kta, proj, (clips, 32) + hw, rows, segments, what, ("bf16",) if what else dtypes))

    for clips, seg in ((1, 8), (2, 4), (4, 2), (8, 1)):
        abc(8, (56, 56), clips, seg)                  # s2: 8 bands of 7 rows x 4 columns of 14 = 32 patches per frame
    for clips, seg in ((1, 8), (8, 4), (16, 2), (32, 1)):
        abc(16, (28, 28), clips, seg)                 # s3: 4 bands x 2 columns
    for clips, seg in ((1, 8), (2, 4), (4, 2), (8, 1)):
        abc(8, (56, 56), clips, seg, proj=True)       # 8 -> 8 -> 8 -> 32, block 0 of s2
    abc(32, (14, 14), 2, 8, rows=3)                   # s4 under AF_ABC_INNER32=1: 3-row patches
    abc(8, (56, 56), 1, 8, what="nan")
    abc(16, (28, 28), 8, 4, what="nan")

    # ---- conv_bc (off by default: AF_FUSE_BC): the layer file's shapes into out_ld = cout + 16
    cases.append(BcCase("bc-s4_like", 256, 256, 1024, (1, 192, 14, 14), True, DT16))
    cases.append(BcCase("bc-s3_like", 128, 128, 512, (2, 48, 28, 28), True, DT16))
    cases.append(BcCase("bc-ragged_no_res", 64, 128, 256, (1, 100, 27, 26), False, DT16))
    assert len({c.name for c in cases}) == len(cases)
    return cases


CASES = _build_cases()


def rounds_class(tiles, workgroups):
    """the class of a launch of `tiles` tiles on `workgroups` persistent workgroups, as the closure test keys shipped launches
    (larger counts add bytes, not states: everything above 5 W is one class)"""
    return "<4" if tiles < 4 * workgroups else "4" if tiles == 4 * workgroups else "4-5" if tiles <= 5 * workgroups else ">5"


def case_key(case, dtype):
    """what the closure test compares.  ca: (form, dtype, T, K slabs, rounds class); cpa: (dtype, K slabs, x_sub, rounds class); abc:
    (inner, kta, projection, dtype, patch rows, time segments); bc: (dtype, channels into b, out of b, out of c, (h, w))"""
    if isinstance(case, CaCase):
        return ("ca", case.form, dtype, case.t, case.c // 64, case.rounds)
    if isinstance(case, CpaCase):
        return ("cpa", dtype, case.c // 64, case.x_sub, case.rounds)
    if isinstance(case, AbcCase):
        return ("abc", case.inner, case.kta, case.proj, dtype, case.rows, case.segments)
    return ("bc", dtype, case.cin, case.cmid, case.cout, tuple(case.dims[2:]))


TARGET = {"4": lambda W: 4 * W, "4-5": lambda W: 4 * W + 44, ">5": lambda W: 6 * W + 37}


def check_class(name, rounds, tiles, groups, W):
    """the launch is in the case's rounds class, W = the workgroups a launch of many tiles has (change the shape, not this)"""
    what = "%s: %d tiles on %d workgroups of %d (change the shape, not this)" % (name, tiles, groups, W)
    assert groups == W, what
    if rounds == "4":
        assert tiles == 4 * W, what
    elif rounds == "4-5":
        assert 4 * W < tiles < 5 * W and tiles % W != 0, what
    else:
        assert 6 * W < tiles < 7 * W, what
    assert rounds_class(tiles, W) == rounds, what


def plan_ca(case, dtype):
    """(dims = (n, t, h, w), tiles, workgroups, tiles per clip) for the case's rounds class on this device; asserts form and class"""
    proj = case.form == "projection"
    probe = 4096                                               # clips: far more tiles than a device has CUs
    if case.what == "clips2":
        tiles, W, form, pix = hh.ca_work_units((probe, case.t, 16, 16), case.c, dtype, proj)
        hw, n = (-(-TARGET["4-5"](W) // 2), pix), 2            # two clips of 2 W + 22 tiles each
    else:
        hw = case.hw
        tiles, W, form, pix = hh.ca_work_units((probe, case.t) + hw, case.c, dtype, proj)
    assert pix * case.t == 256
    if case.what != "clips2":
        assert tiles % probe == 0
        n = -(-TARGET[case.rounds](W) // (tiles // probe))
    dims = (n, case.t) + tuple(hw)
    ans = hh.ca_work_units(dims, case.c, dtype, proj)
    assert ans is not None, "%s: not fused at %s" % (case.name, dims)
    tiles, groups, form, pix = ans
    assert form == case.form, "%s: the library runs the %s form, not %s" % (case.name, form, case.form)
    assert tiles % n == 0
    check_class(case.name, case.rounds, tiles, groups, W)
    return dims, tiles, groups, tiles // n


def plan_cpa(case, dtype):
    probe = 4096
    tiles, W = hh.cpa_work_units((probe, 32) + case.hw, case.c, dtype, case.x_sub)
    assert tiles % probe == 0
    per = tiles // probe
    n = -(-TARGET[case.rounds](W) // per)
    dims = (n, 32) + tuple(case.hw)
    ans = hh.cpa_work_units(dims, case.c, dtype, case.x_sub)
    assert ans is not None, "%s: not fused at %s" % (case.name, dims)
    check_class(case.name, case.rounds, ans[0], ans[1], W)
    return dims, ans[0], ans[1], per


def _bn_layout(prefix, ch):
    return [(prefix + s, (ch,), "float32") for s in (".weight", ".bias", ".running_mean", ".running_var")]


def _ncdhw64(x_ndhwc):
    return x_ndhwc.permute(0, 4, 1, 2, 3).contiguous().double()       # (transposed in the storage type: the smaller copy)


def _rows(y_ncdhw):
    return y_ncdhw.permute(0, 2, 3, 4, 1).reshape(-1, y_ncdhw.shape[1])


def _clip_groups(n, rows_per_clip, limit=1 << 16):
    """clip ranges of about `limit` positions: the fp64 reference runs group by group (clips are independent)"""
    step = max(1, limit // rows_per_clip)
    return [(i, min(n, i + step)) for i in range(0, n, step)]


def _guarded(rows, width, tdt, ld=False):
    """(buffer prefilled with 7.0, the view of `rows` x `width` the launch writes, out_ld or 0): 64 guard rows before and after and,
    with ld, rows of width + 16 with 8 guard channels on each side"""
    ldw, off = (width + 16, 8) if ld else (width, 0)
    buf = torch.full((GUARD + rows + GUARD, ldw), 7.0, dtype=tdt, device="cuda")
    view = buf[GUARD:GUARD + rows, off:off + width]
    assert view.data_ptr() % 16 == 0
    return buf, view, (ldw if ld else 0)


def _take(buf, rows, width, what):
    """the output rows as fp64 on the host; every guard element must still be 7.0"""
    host = buf.cpu()
    off = (host.shape[1] - width) // 2
    got = host[GUARD:GUARD + rows, off:off + width].double()
    host[GUARD:GUARD + rows, off:off + width] = 7.0
    assert torch.all(host == 7.0), "%s: %d guard elements around the output were written" % (what, int((host != 7.0).sum()))
    return got


def _seed(*key):
    return 9000 + zlib.crc32(repr(key).encode()) % 90000


# the operands and the fp64 reference of the last geometry: a case and its neighbour in PARAMS may share them
_last = {}


def _cached(key, make):
    if _last.get("key") != key:
        _last.clear()
        _last["key"], _last["val"] = key, make()
    return _last["val"]


# ---------------------------------------------------------------------------------------------------------------- conv_ca / conv_cpa
def _pair_operands(c, cout_a, dims, dtype, proj):
    """b, the residual (or the projection's input x0), the weights rounded to the storage type (those of the projection form
    are folded and rounded later)"""
    tdt = hh.TORCH_DT[dtype]
    n, t, h, w = dims
    seed = _seed(c, cout_a, dims, proj)
    lay = [("c.weight", (c, 64, 1, 1, 1), "float32"), ("a.weight", (cout_a, c, 3, 1, 1), "float32"), ("b1.weight", (c, 64, 1, 1, 1), "float32")]
    lay += _bn_layout("c_bn", c) + _bn_layout("a_bn", cout_a) + _bn_layout("b1_bn", c)
    sd = synth.fill_layout(lay, seed)
    sd["a.weight"] = sd["a.weight"].to(tdt).float()
    if not proj:
        sd["c.weight"] = sd["c.weight"].to(tdt).float()
    b = synth.synthetic_tensor((n, t, h, w, 64), seed).to(tdt)
    other = synth.synthetic_tensor((n, t, h, w, 64 if proj else c), seed + 1).to(tdt)
    return b, other, sd


def _pair_reference(b, other, sd, dtype, bn_c=None, bn_1=None, pool=False):
    """(trunk, a output) as fp64 rows.  plain: trunk = relu(bn_c(c(b)) + other); projection (bn_c / bn_1 = the folded BN of the c and
    shortcut convs): both scales folded into the weights in fp32 and rounded once, trunk = relu(c'(b) + s'(other) + shifts); pool:
    the frame-pair max behind the ReLU (conv_cpa; rounding is monotonic: pooling before or after it is the same).  The trunk is
    rounded to the storage type before the temporal conv."""
    tdt = hh.TORCH_DT[dtype]
    n, t, h, w, _ = b.shape
    c, cout_a = sd["c.weight"].shape[0], sd["a.weight"].shape[0]
    sd64 = {k: v.double() for k, v in sd.items()}
    if bn_c is not None:
        fold = lambda wk, bn: (sd[wk] * bn[0].cpu()[:c].view(-1, 1, 1, 1, 1)).to(tdt).double()      # scale folded in fp32, rounded once
        wc, w1 = fold("c.weight", bn_c), fold("b1.weight", bn_1)
        shift = (bn_c[1] + bn_1[1]).cpu()[:c].double().view(1, -1, 1, 1, 1)
    to = t // 2 if pool else t
    want_x = torch.empty((n * to * h * w, c), dtype=torch.float64)
    want_a = torch.empty((n * to * h * w, cout_a), dtype=torch.float64)
    per = to * h * w
    for n0, n1 in _clip_groups(n, t * h * w):
        b64, o64 = _ncdhw64(b[n0:n1]), _ncdhw64(other[n0:n1])
        if bn_c is not None:
            x = F.relu(F.conv3d(b64, wc) + F.conv3d(o64, w1) + shift)
        else:
            x = F.relu(oracle.conv_bn_act(b64, sd64["c.weight"], sd64, "c_bn", (1, 1, 1), (0, 0, 0), False) + o64)
        if pool:
            x = F.max_pool3d(x, (2, 1, 1), (2, 1, 1))
        a = oracle.conv_bn_act(x.to(tdt).double(), sd64["a.weight"], sd64, "a_bn", (1, 1, 1), (1, 0, 0), True)
        want_x[n0 * per:n1 * per] = _rows(x)
        want_a[n0 * per:n1 * per] = _rows(a)
    return want_x, want_a


def _later_clip(W, per):
    """the first clip whose tiles all come behind the first W: none of them is the first tile of its workgroup"""
    return -(-W // per) + 1


def _nan_frames(mask_rows, dims):
    """{(clip, frame, pixel)} of the rows of a per-row mask over (n, t, h, w)"""
    n, t, h, w = dims
    idx = mask_rows.reshape(n, t, h * w).nonzero().tolist()
    return {tuple(i) for i in idx}


CA_PARAMS = [(dt, c) for c in CASES if isinstance(c, CaCase) for dt in c.dtypes]


@pytest.mark.parametrize("dtype,case", CA_PARAMS, ids=["%s-%s" % (dt, c.name) for dt, c in CA_PARAMS])
def test_conv_ca(dtype, case):
    tdt = hh.TORCH_DT[dtype]
    dims, tiles, groups, per = plan_ca(case, dtype)
    n, t, h, w = dims
    proj = case.form == "projection"
    b, other, sd = _pair_operands(case.c, 64, dims, dtype, proj)
    expect_nan = None
    if case.what == "nonfinite":
        # one NaN and one +inf in b, one NaN in the residual: three clips whose tiles are all later tiles of their workgroups
        n1 = _later_clip(groups, per)
        assert n1 + 2 < n and t > 8
        b[n1, 5, 1, 3, 1] = float("nan")
        b[n1 + 1, t - 1, h - 1, 2, 2] = float("inf")
        other[n1 + 2, 0, 2, 1, 7] = float("nan")
        source = {(n1, 5, 1 * w + 3), (n1 + 1, t - 1, (h - 1) * w + 2), (n1 + 2, 0, 2 * w + 1)}
        expect_nan = {(n1, f, 1 * w + 3) for f in (4, 5, 6)} | {(n1 + 2, f, 2 * w + 1) for f in (0, 1)}
        maybe = {(n1 + 1, f, (h - 1) * w + 2) for f in (t - 2, t - 1)}          # inf - inf over the trunk channels, or inf through the ReLU
    elif case.what == "clips2":
        # tiles per clip: more than W and no multiple of it - every workgroup has tiles in both clips and the boundary falls at
        # another place of each one's sequence.  A NaN in the last frame of clip 0 and one in the first frame of clip 1, in tiles
        # that are not the first of their workgroup: each must stay in its clip (the padding frames are zero)
        assert n == 2 and per > groups and per % groups != 0 and h == per and h > groups + 9
        b[0, t - 1, groups + 3, 1, 5] = float("nan")
        other[1, 0, groups + 8, 2, 9] = float("nan")
        source = {(0, t - 1, (groups + 3) * w + 1), (1, 0, (groups + 8) * w + 2)}
        expect_nan = {(0, f, (groups + 3) * w + 1) for f in (t - 2, t - 1)} | {(1, f, (groups + 8) * w + 2) for f in (0, 1)}
        maybe = set()
    bn_c, bn_a = hh.fold_bn(sd, "c_bn"), hh.fold_bn(sd, "a_bn")
    bn_1 = hh.fold_bn(sd, "b1_bn") if proj else None
    want_x, want_a = _pair_reference(b, other, sd, dtype, bn_c if proj else None, bn_1)
    rows = n * t * h * w
    buf_x, view_x, _ = _guarded(rows, case.c, tdt)
    buf_a, view_a, _ = _guarded(rows, 64, tdt)
    bd, od = b.cuda(), other.cuda()
    out = hh.conv_ca(bd, sd["c.weight"], bn_c, None if proj else od, sd["a.weight"], bn_a, dtype, x0_ndhwc=od if proj else None,
                     w1_oidhw=sd["b1.weight"] if proj else None, bn_1=bn_1, out_x=view_x, out_a=view_a)
    assert out is not None, "the library should fuse this pair"
    what = "%s[%s] %s, class %s: %d tiles / %d workgroups" % (case.name, dtype, case.form, case.rounds, tiles, groups)
    got_x, got_a = _take(buf_x, rows, case.c, what + " trunk"), _take(buf_a, rows, 64, what + " a")
    if expect_nan is not None:
        nan_a = torch.isnan(got_a)
        assert _nan_frames(nan_a.all(1), dims) >= expect_nan, "%s: a NaN did not reach frames t - 1, t, t + 1 of its pixel" % what
        assert _nan_frames(nan_a.any(1), dims) <= expect_nan | maybe, "%s: NaN in rows no tap leads to" % what
        assert _nan_frames(~torch.isfinite(got_x).all(1), dims) == source, "%s: non-finite trunk rows" % what
    hh.compare(got_x, want_x, TOL[dtype], what + " trunk")
    hh.compare(got_a, want_a, 1.5 * TOL[dtype], what + " a")


# x_sub 1 and 2 of one geometry and dtype next to each other (they share operands and reference)
CPA_PARAMS = sorted([(dt, c) for c in CASES if isinstance(c, CpaCase) for dt in c.dtypes],
                    key=lambda p: (p[1].c, ROUNDS.index(p[1].rounds), p[1].what, p[0], p[1].x_sub))


@pytest.mark.parametrize("dtype,case", CPA_PARAMS, ids=["%s-%s" % (dt, c.name) for dt, c in CPA_PARAMS])
def test_conv_cpa(dtype, case):
    tdt = hh.TORCH_DT[dtype]
    dims, tiles, groups, per = plan_cpa(case, dtype)
    n, t, h, w = dims
    # x_sub 1 and 2 of one geometry share operands and reference
    key = ("cpa", case.c, dims, dtype, case.what)

    def make():
        b, res, sd = _pair_operands(case.c, 128, dims, dtype, False)
        if case.what == "nonfinite":
            n1 = _later_clip(groups, per)
            assert n1 + 2 < n
            b[n1, 5, 1, 3, 1] = float("nan")                       # frame pair 2: pooled frames 1, 2, 3 of the a output
            b[n1 + 1, t - 1, h - 1, 2, 2] = float("inf")
            res[n1 + 2, 0, 0, 5, 7] = float("nan")                 # pooled frame 0: frames 0, 1
        return (b, res, sd) + _pair_reference(b, res, sd, dtype, pool=True)

    b, res, sd, want_x, want_a = _cached(key, make)
    if case.what == "nonfinite":
        n1 = _later_clip(groups, per)
        nan_a, pooled = torch.isnan(want_a), (n, t // 2, h, w)
        expect_nan = {(n1, f, 1 * w + 3) for f in (1, 2, 3)} | {(n1 + 2, f, 5) for f in (0, 1)}
        maybe = {(n1 + 1, f, (h - 1) * w + 2) for f in (t // 2 - 2, t // 2 - 1)}      # inf - inf over the trunk channels, or inf through the ReLU
        assert _nan_frames(nan_a.all(1), pooled) >= expect_nan and _nan_frames(nan_a.any(1), pooled) <= expect_nan | maybe
    rows = n * (t // 2) * h * w
    rows_x = rows // 4 if case.x_sub == 2 else rows
    buf_x, view_x, _ = _guarded(rows_x, case.c, tdt)
    buf_a, view_a, _ = _guarded(rows, 128, tdt)
    out = hh.conv_cpa(b.cuda(), sd["c.weight"], hh.fold_bn(sd, "c_bn"), res.cuda(), sd["a.weight"], hh.fold_bn(sd, "a_bn"), dtype,
                      case.x_sub, out_x=view_x, out_a=view_a)
    assert out is not None, "the library should fuse this pair"
    what = "%s[%s] class %s: %d tiles / %d workgroups" % (case.name, dtype, case.rounds, tiles, groups)
    got_x, got_a = _take(buf_x, rows_x, case.c, what + " trunk"), _take(buf_a, rows, 128, what + " a")
    if case.x_sub == 2:          # the even (h, w) positions of the pooled trunk, packed (the tolerance relative to THEIR maximum: no wider)
        want_x = want_x.reshape(n, t // 2, h, w, case.c)[:, :, ::2, ::2].reshape(-1, case.c)
    hh.compare(got_x, want_x, TOL[dtype], what + " trunk")
    hh.compare(got_a, want_a, 1.5 * TOL[dtype], what + " a")


def test_below_four_rounds_the_pairs_keep_their_two_launches():
    """one clip less than 4 W tiles: af_conv_ca_fusable / af_conv_cpa_fusable refuse (the helpers assert that the query and the
    predicate agree); wide projection trunks do not fit LDS and are refused at any size"""
    for t, proj in ((32, False), (32, True), (16, False)):
        tiles, W, form, pix = hh.ca_work_units((4096, t, 4, 256 // t), 256, "bf16", proj)
        assert tiles == 4096 * 4 and pix == 256 // t
        assert hh.ca_work_units((W, t, 4, pix), 256, "bf16", proj)[0] == 4 * W
        assert hh.ca_work_units((W - 1, t, 4, pix), 256, "bf16", proj) is None
    for c in (320, 512, 1024):
        for t in (16, 32):
            assert hh.ca_work_units((4096, t, 16, 16), c, "f16", True) is None
    for sub in (1, 2):
        tiles, W = hh.cpa_work_units((4096, 32, 4, 8), 256, "bf16", sub)
        assert tiles == 4096 * 4
        assert hh.cpa_work_units((W, 32, 4, 8), 256, "bf16", sub) == (4 * W, W)
        assert hh.cpa_work_units((W - 1, 32, 4, 8), 256, "bf16", sub) is None


# ---------------------------------------------------------------------------------------------------------------------- block_abc
def _abc_operands(case, dtype):
    tdt = hh.TORCH_DT[dtype]
    n, t, h, w = case.dims
    inner, kta = case.inner, case.kta
    cin, cout = (8, 32) if case.proj else (4 * inner, 4 * inner)
    seed = _seed("abc", inner, kta, case.proj, case.dims)
    lay = [("a.weight", (inner, cin, kta, 1, 1), "float32"), ("b.weight", (inner, inner, 1, 3, 3), "float32"),
           ("c.weight", (cout, inner, 1, 1, 1), "float32"), ("s.weight", (cout, cin, 1, 1, 1), "float32")]
    lay += _bn_layout("a_bn", inner) + _bn_layout("b_bn", inner) + _bn_layout("c_bn", cout) + _bn_layout("s_bn", cout)
    sd = synth.fill_layout(lay, seed)
    for k in ("a.weight", "b.weight") + (() if case.proj else ("c.weight",)):
        sd[k] = sd[k].to(tdt).float()
    x = synth.synthetic_tensor((n, t, h, w, cin), seed).to(tdt)
    return x, sd


def _abc_reference(case, x, sd, dtype):
    """relu(shortcut(x) + bn_c(c(relu(bn_b(b(relu(bn_a(a(x)))))))))  as fp64 rows; a and b rounded to the storage type (they cross
    LDS in it).  The projection form's c and shortcut weights stay unrounded, as in the layer file: its tolerance covers the
    kernel's one more rounding of each"""
    tdt = hh.TORCH_DT[dtype]
    n, t, h, w, _ = x.shape
    sd64 = {k: v.double() for k, v in sd.items()}
    want = torch.empty((n * t * h * w, sd["c.weight"].shape[0]), dtype=torch.float64)
    per = t * h * w
    for n0, n1 in _clip_groups(n, per, 1 << 18):
        x64 = _ncdhw64(x[n0:n1])
        ya = oracle.conv_bn_act(x64, sd64["a.weight"], sd64, "a_bn", (1, 1, 1), (case.kta // 2, 0, 0), True).to(tdt).double()
        yb = oracle.conv_bn_act(ya, sd64["b.weight"], sd64, "b_bn", (1, 1, 1), (0, 1, 1), True).to(tdt).double()
        yc = oracle.conv_bn_act(yb, sd64["c.weight"], sd64, "c_bn", (1, 1, 1), (0, 0, 0), False)
        short = oracle.conv_bn_act(x64, sd64["s.weight"], sd64, "s_bn", (1, 1, 1), (0, 0, 0), False) if case.proj else x64
        want[n0 * per:n1 * per] = _rows(F.relu(yc + short))
    return want


ABC_PARAMS = [(dt, c) for c in CASES if isinstance(c, AbcCase) for dt in c.dtypes]


@pytest.mark.parametrize("dtype,case", ABC_PARAMS, ids=["%s-%s" % (dt, c.name) for dt, c in ABC_PARAMS])
def test_block_abc(dtype, case, monkeypatch):
    if case.inner == 32:
        monkeypatch.setenv("AF_ABC_INNER32", "1")                # correct but not faster than three launches: off by default
    tdt = hh.TORCH_DT[dtype]
    n, t, h, w = case.dims
    cin, cout = (8, 32) if case.proj else (4 * case.inner, 4 * case.inner)
    ans = hh.abc_work_units(case.dims + (cin,), case.inner, case.kta, cout, dtype, case.proj)
    assert ans is not None, "the library should fuse this block"
    rows_p, segments, units = ans
    assert (rows_p, segments) == (case.rows, case.segments), "%s: %d-row patches, %d time segments (change the shape, not this)" % (
        case.name, rows_p, segments)
    assert units == n * -(-h // rows_p) * -(-w // 14) * segments
    x, sd = _abc_operands(case, dtype)
    if case.what == "nan":
        # the last frame of time segment 0: the first frame of segment 1 - another workgroup - sees it through its t - 1 tap
        ts = t // segments
        assert segments > 1 and ts * segments == t
        x[0, ts - 1, 7, 14, 3] = float("nan")                    # ... and its 3 x 3 neighbourhood lies in four patches
    want = _abc_reference(case, x, sd, dtype)
    rows = n * t * h * w
    buf, view, ld = _guarded(rows, cout, tdt, ld=True)
    bn = {p: hh.fold_bn(sd, p + "_bn") for p in ("a", "b", "c", "s")}
    out = hh.block_abc(x.cuda(), sd["a.weight"], bn["a"], sd["b.weight"], bn["b"], sd["c.weight"], bn["c"], dtype, out_ld=ld,
                       w1_oidhw=sd["s.weight"] if case.proj else None, bn_1=bn["s"] if case.proj else None, out=view)
    assert out is not None, "the library should fuse this block"
    what = "%s[%s] %d-row patches, %d time segments, %d units" % (case.name, dtype, rows_p, segments, units)
    got = _take(buf, rows, cout, what)
    if case.what == "nan":
        nan = torch.isnan(got).all(1).reshape(n, t, h, w)
        ts = t // segments
        assert nan[0, ts - 2:ts + 1, 6:9, 13:16].all() and int(nan.sum()) == 27, "%s: the NaN must cross the segment boundary" % what
    hh.compare(got, want, (TOL_ABC_PROJ if case.proj else TOL_ABC)[dtype], what)


# ------------------------------------------------------------------------------------------------------------------------ conv_bc
BC_PARAMS = [(dt, c) for c in CASES if isinstance(c, BcCase) for dt in c.dtypes]


@pytest.mark.parametrize("dtype,case", BC_PARAMS, ids=["%s-%s" % (dt, c.name) for dt, c in BC_PARAMS])
def test_conv_bc(dtype, case):
    tdt = hh.TORCH_DT[dtype]
    n, t, h, w = case.dims
    seed = _seed("bc", case.cin, case.cmid, case.cout, case.dims)
    lay = [("b.weight", (case.cmid, case.cin, 1, 3, 3), "float32"), ("c.weight", (case.cout, case.cmid, 1, 1, 1), "float32")]
    sd = synth.fill_layout(lay + _bn_layout("b_bn", case.cmid) + _bn_layout("c_bn", case.cout), seed)
    for k in ("b.weight", "c.weight"):
        sd[k] = sd[k].to(tdt).float()
    sd64 = {k: v.double() for k, v in sd.items()}
    x = synth.synthetic_tensor((n, t, h, w, case.cin), seed).to(tdt)
    res = synth.synthetic_tensor((n, t, h, w, case.cout), seed + 1).to(tdt) if case.use_res else None
    mid = oracle.conv_bn_act(_ncdhw64(x), sd64["b.weight"], sd64, "b_bn", (1, 1, 1), (0, 1, 1), True)
    mid = mid.to(tdt).double()                                  # the one rounding of the b output (LDS tile in the storage type)
    want = oracle.conv_bn_act(mid, sd64["c.weight"], sd64, "c_bn", (1, 1, 1), (0, 0, 0), False)
    if res is not None:
        want = want + _ncdhw64(res)
    want = _rows(F.relu(want))
    rows = n * t * h * w
    buf, view, ld = _guarded(rows, case.cout, tdt, ld=True)
    out = hh.conv_bc(x.cuda(), sd["b.weight"], hh.fold_bn(sd, "b_bn"), sd["c.weight"], hh.fold_bn(sd, "c_bn"),
                     None if res is None else res.cuda(), dtype, out=view, out_ld=ld)
    assert out is not None, "the library should fuse this pair"
    what = "%s[%s] out_ld %d" % (case.name, dtype, ld)
    hh.compare(_take(buf, rows, case.cout, what), want, TOL_BC[dtype], what)
