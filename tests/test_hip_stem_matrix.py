"""GPU: the stem launches - the first launch of every network - against fp64, with a DERIVED per-element bound, over the classes of
launch the fused stems have: kT, kernel form, bands of pooled rows, rounds of units per workgroup, unit map, output stride.

Kernels.  `stem3_pool` (af_stem_conv_bn_relu_maxpool_rgb3[_ld], af_stem3.hip: the K-packed fused stem on the 3-channel input) and
`stem_pool` (af_stem_conv_bn_relu_maxpool, af_stem_pool.hip: the 4-channel layout) are persistent: min(units, CUs) workgroups walk
the (frame, band of pooled rows) units; a workgroup that starts its next unit resets the odd conv row it keeps for the vertical
max, issues the load prologue again and (pooling-wave form) restarts its three-line rotation.  `stem` (af_stem_conv_bn_relu: the
generic stem kernel, and the 16-bit row-sharing kernel for <= 16 output channels) with af_maxpool3d behind it is the unfused
pair; `tstem` / `tstem_pool3` (af_ftcn.hip) are FTCN-TT's temporal stems.  The input packs in front of them are compared byte for
byte with a host-built image of the documented layout.

Sizing at run time.  af_stem_work_units - the function both fused launchers take their bands and their grid from - answers (units,
bands, workgroups) for a descriptor.  A case names its class, the clip and frame count of the rounds classes is computed from W =
the workgroups of a launch that fills the device, and every case asserts its class from the library's answer:
    rounds "1"    U <= W   (the rounds cases: U = W)      "1-2"  U = W + 5: units % 8 != 0 on a full grid - the last XCD of the
    XCD-contiguous map gets fewer units and the `u_end` clamp cuts its workgroups' walk      "2"  U = 2 W      ">2"  U = 3 W + 37
    map    "xcd" (stem3_pool on a grid that is a multiple of 8) or "plain" (unit b, b + grid, ...)
    bands, a one-row last band, and the form: the pooling wave (at most 7 column tiles) or the plain form (8 tiles).
The cases are written for 256 CUs and assert that.  In the rounds classes beyond "1" the frames come as several clips (9 x 29,
16 x 32, 23 x 35 frames), so that clip boundaries - their temporal zero halos - fall into later units of a workgroup; in "2" and
">2" it is asserted that a clip's first frame is such a unit ("1-2" has only its 5 - XCD map: 7 - second units to offer).

Operands and reference.  x and w are rounded to the storage type on both sides; scale and shift are written here as fp32: odd
channels have a negative scale, channel 4 scale 0 with a positive shift, channel 9 a shift that leaves the whole channel zero
behind the ReLU (both fused kernels use 0 as the pool's -inf).  Reference: F.conv3d on doubles, affine map, ReLU, F.max_pool3d.

Bound, per element (check()).  A = conv(|x|, |w|) in fp64, K = 147 kT (3 kT for the temporal stems).  Before the pool
b = 4 (K + 2) 2^-24 (A |scale| + |shift|): at most K + 2 fp32 roundings of partial sums bounded by that quantity, the factor 4 is
margin for the MFMA's internal add order and rounding mode.  ReLU and max are 1-Lipschitz, so the pooled bound is max_pool3d(b)
over the same window.  The single output rounding adds u |want|, u = 2^-8 (bf16), 2^-11 (f16), 2^-24 (f32), f16 also 2^-25 absolute
for subnormals.  |got - want| <= bound everywhere; tests/test_stem_matrix_host.py shows on the CPU that torch's own fp32 result
stays inside the bound and that a single zeroed tap out of 147 kT does not.

Non-finite values.  Both layouts multiply an eighth, zero-weight column of real pixels into every output (af_stem3.hip: fragment
elements 21..23 and the clamped fragments beyond the kernel; af_stem.hip / af_stem_pool.hip: the eighth tap), so 0 x NaN reaches
outputs that ATen leaves finite.  What is asserted for one NaN pixel in a unit that is not the first of its workgroup:
nan_aten <= nan_got <= nan_wide, where nan_wide is the pooled mask of a conv whose column window is dw = 0..7, one column wider
than ATen's; the bound holds outside nan_got.  An f16 channel whose scale drives values beyond 65504 must come out +inf where the
reference does (decided by the bound at the rounding edge 65520) and survive the u16 max of the pool.

Guards.  Every launch writes into a view of a buffer prefilled with 7.0: 64 guard rows before and after, and in the `ld` form
(out_ld = 80, as SlowFast ships its Slow stem) 8 guard channels left and right; all of them must still be 7.0.

Largest measured max(|got - want| / bound) per kernel and dtype on an MI355X (each test prints its own; MEASURED keeps the run's
largest).  The 16-bit figures are the output rounding: an error of almost half an ulp on a value just above a power of two is
almost u |want|; f32 shows what the accumulation itself uses of b:
    stem3_pool  f16 0.896  bf16 0.976          stem_pool    f16 0.896  bf16 0.965
    stem        f32 0.005  f16 0.827  bf16 0.930   stem_rows  f16 0.801  bf16 0.926
    tstem       f32 0.075  f16 0.990  bf16 0.994   tstem_pool3  f16 0.987  bf16 0.995
    (the NaN cases 0.407 f16 / 0.791 bf16 outside the NaN set, the +inf cases 0.422)

CASES / STEM_CASES are plain data (no device needed): tests/test_host_cpu.py::test_stem_matrix_covers_what_ships compares
case_key() of every case with what the three networks ship."""
import collections
import ctypes as C
import os
import sys

import pytest
import torch
import torch.nn.functional as F

from conftest import ROOT

sys.path.insert(0, os.path.join(ROOT, "tests"))
import hip_helpers as hh  # noqa: E402
from af_mi355x import synth  # noqa: E402

pytestmark = pytest.mark.gpu
GUARD = 64
CUS = 256                                            # the device the cases are written for
UNIT_ROUNDOFF = {"bf16": 2.0 ** -8, "f16": 2.0 ** -11, "f32": 2.0 ** -24}
DT16 = ("f16", "bf16")
DT_ALL = ("f32", "f16", "bf16")
POOL = ((1, 3, 3), (1, 2, 2), (0, 1, 1))
MEASURED = {}                                        # (kernel, dtype) -> largest |got - want| / bound of this run

# kind: stem3_pool / stem_pool; hw: the frame; clips: (n, t), or None = sized for the rounds class; rounds / bands / onerow (a last
# band of one pooled row) / umap: the class the case must run in; out: 0 (the entry point without a row stride), 64 or 80 (the _ld
# entry point); inp: f32 or u8 (the uint8 pack); special: None, "nan" or "inf" (f16 only)
Case = collections.namedtuple("Case", "name kind kt hw clips rounds bands onerow umap out inp special")


def _build_cases():
    cases = []

    def add(kind, kt, hw, clips, rounds="1", bands=1, onerow=False, umap=None, out=0, inp="f32", special=None):
        if umap is None:
            umap = "xcd" if kind == "stem3_pool" and clips is None else "plain"
        name = "%s-kt%d-%dx%d-%s-r%s-b%d%s-%s-ld%d%s%s" % (kind, kt, hw[0], hw[1], "x".join(map(str, clips)) if clips else "sized", rounds,
                                                         bands, "one" if onerow else "", umap, out, "-u8" if inp == "u8" else "",
                                                         "-" + special if special else "")
        cases.append(Case(name, kind, kt, tuple(hw), clips, rounds, bands, onerow, umap, out, inp, special))

    for kind in ("stem3_pool", "stem_pool"):
        s3 = kind == "stem3_pool"
        xcd = "xcd" if s3 else "plain"
        # ---- rounds of units per workgroup, kT = 5 (I3D ships "1", "1-2", "2", ">2"); no bands (frames >= W)
        add(kind, 5, (18, 20), None, "1")
        add(kind, 5, (18, 20), None, "1-2")
        add(kind, 5, (10, 12), None, "2")
        add(kind, 5, (10, 12), None, ">2")
        add(kind, 5, (10, 12), None, "2", special="nan")
        add(kind, 5, (18, 20), None, "1-2", special="inf")
        # ---- kT = 1 and 3 (other prefetch group sizes), several units per workgroup and a few frames on the plain map
        add(kind, 1, (18, 20), None, "1-2")
        add(kind, 3, (10, 12), None, ">2")
        add(kind, 1, (18, 20), (1, 5))
        add(kind, 3, (18, 20), (1, 5))
        add(kind, 5, (18, 20), (1, 5))
        # ---- bands: 4 even ones of 4 pooled rows (Hq = 16); Hq = 21 on 5 bands: a one-row last band (51 frames: 255 units, plain map;
        # 48 frames: 240 units, a multiple of 8)
        add(kind, 5, (64, 20), (2, 32), bands=4, umap=xcd)
        add(kind, 5, (82, 20), (3, 17), bands=5, onerow=True, umap="plain")
        add(kind, 1, (83, 20), (2, 24), bands=5, onerow=True, umap=xcd)
        # ---- 8 column tiles (conv width 113..128): the plain form of stem3_pool, without and with bands (Hq = 8: two of 4 rows)
        add(kind, 1, (6, 230), (1, 3))
        add(kind, 5, (6, 230), (1, 3))
        add(kind, 5, (29, 226), (1, 16), bands=2, umap=xcd)
        if s3:
            add(kind, 1, (29, 226), (1, 16), bands=2, umap=xcd)
        # ---- edge sizes: Ho <= 2 (Hq = 1, one row pair, no odd row); odd Ho and Wo (2-wide last window; Hq = 9: bands of 5 + 4);
        # conv widths 16, 17 and 112
        for hw in ((1, 1), (2, 3), (4, 5)):
            add(kind, 5, hw, (1, 3))
        add(kind, 1, (1, 1), (1, 3))
        add(kind, 5, (33, 37), (1, 3), bands=2)
        for w in (32, 33, 224):
            add(kind, 5, (8, w), (1, 3))
        if not s3:
            continue
        # ---- stem3_pool only: the row stride of the output, the uint8 pack, kT = 3 on bands
        add(kind, 5, (18, 20), None, "1-2", out=64)
        add(kind, 5, (18, 20), None, "1-2", out=80)
        add(kind, 1, (10, 12), None, ">2", out=80)
        add(kind, 1, (64, 20), (2, 32), bands=4, umap="xcd", out=80)         # SlowFast's Slow stem: kT = 1, bands, rows of 80
        add(kind, 1, (82, 20), (3, 17), bands=5, onerow=True, umap="plain", out=80)
        add(kind, 3, (64, 20), (2, 32), bands=4, umap="xcd")
        add(kind, 5, (18, 20), (1, 5), inp="u8")
        add(kind, 5, (33, 37), (1, 3), bands=2, out=80)
    assert len({c.name for c in cases}) == len(cases)
    return cases


CASES = _build_cases()

# the unfused stem: (cout, kt, (n, t, h, w), dtypes); M = n t Ho Wo is no multiple of 64 (the clamped tail lanes)
StemCase = collections.namedtuple("StemCase", "cout kt dims dtypes")
STEM_CASES = [StemCase(64, 5, (1, 3, 18, 22), DT_ALL),        # M = 297
              StemCase(64, 1, (2, 2, 10, 14), DT_ALL),        # M = 140
              StemCase(16, 1, (1, 2, 18, 40), DT_ALL),        # M = 360
              StemCase(8, 5, (2, 6, 50, 70), DT_ALL),         # SlowFast's Fast stem: conv out 25 x 35 - a ragged last 8-row block and 16-column tile
              StemCase(8, 3, (1, 3, 14, 38), DT_ALL),         # fewer rows than a block, 19 columns
              StemCase(4, 3, (1, 4, 14, 14), DT_ALL)]         # M = 196
# the temporal stems: (kind, kt, dtypes) - the existing cases of tests/test_hip_ftcn.py, here with guards, and a launch whose grid is capped
TSTEM_CASES = [("tstem", 5, DT_ALL), ("tstem_pool3", 5, DT16)]


def rounds_class(units, workgroups):
    """the class of a launch of `units` work units on `workgroups` persistent workgroups, as the closure test keys shipped launches"""
    return "1" if units <= workgroups else "1-2" if units < 2 * workgroups else "2" if units == 2 * workgroups else ">2"


def tiles8(w):
    """the conv output of a w-pixel row takes 8 column tiles: stem3_pool runs in the plain form (no free wave for the pooling)"""
    return ((w - 1) // 2 + 1 + 15) // 16 == 8


def launch_key(kind, dtype, kt, w, hq, bands, units, workgroups, ld):
    """what the closure test compares for a fused stem launch: (kind, dtype, kT, 8-tile form, bands > 1, one-row last band, rounds
    class, unit map, out_ld != 64)"""
    band_rows = -(-hq // bands)
    umap = "xcd" if kind == "stem3_pool" and workgroups % 8 == 0 else "plain"
    return (kind, dtype, kt, tiles8(w), bands > 1, bands > 1 and hq - (bands - 1) * band_rows == 1, rounds_class(units, workgroups), umap,
            ld != 64)


def case_key(case, dtype):
    return (case.kind, dtype, case.kt, tiles8(case.hw[1]), case.bands > 1, case.onerow, case.rounds, case.umap, (case.out or 64) != 64)


def stem_case_key(kind, dtype, kt, cout):
    """stem / tstem / tstem_pool3 launches: (kind, dtype, kT, cout)"""
    return (kind, dtype, kt, cout)


def covered_keys():
    keys = {case_key(c, dt) for c in CASES for dt in DT16 if c.special is None}
    keys |= {stem_case_key("stem", dt, c.kt, c.cout) for c in STEM_CASES for dt in c.dtypes}
    keys |= {stem_case_key(kind, dt, kt, 64) for kind, kt, dts in TSTEM_CASES for dt in dts}
    return keys


# ---------------------------------------------------------------- operands, reference, comparator (no device needed)

def operands(kt, dtype, dims, seed, cout=64, special=None, kernel_hw=(7, 7), wscale=0.05):
    """x (n, 3, t, h, w) and w (cout, 3, kt, kh, kw) rounded to the storage type (held as fp32), scale and shift in fp32: odd channels a
    negative scale, channel 4 scale 0 and a positive shift, channel 9 a shift that leaves it zero behind a ReLU; special = "inf":
    channel 6 scaled beyond the largest f16"""
    n, t, h, w = dims
    g = torch.Generator().manual_seed(seed)
    tdt = hh.TORCH_DT[dtype]
    x = torch.randn((n, 3, t, h, w), generator=g).to(tdt).float()
    wt = (torch.randn((cout, 3, kt) + tuple(kernel_hw), generator=g) * wscale).to(tdt).float()
    scale = 0.5 + torch.rand(cout, generator=g)
    scale[1::2] *= -1.0
    shift = torch.randn(cout, generator=g) * 0.5
    if cout > 4:
        scale[4], shift[4] = 0.0, 0.375
    if cout > 9:
        shift[9] = -64.0
    if special == "inf":
        scale[6] = 3.0e4
    return x, wt, scale.contiguous(), shift.contiguous()


def reference(x, w, scale, shift, stride=(1, 2, 2), pad=None, pools=(POOL,), relu_first=True):
    """(want, b) in fp64: conv, affine map, ReLU and the max-pools `pools` (relu_first False: the ReLU behind the first pool, as the
    temporal stem has it); b = the bound on what fp32 accumulation may differ by, before the output rounding (module docstring)"""
    kt, kh, kw = w.shape[2:]
    pad = (kt // 2, kh // 2, kw // 2) if pad is None else pad
    sc, sh = scale.double().view(1, -1, 1, 1, 1), shift.double().view(1, -1, 1, 1, 1)
    y = F.conv3d(x.double(), w.double(), None, stride, pad) * sc + sh
    a = F.conv3d(x.double().abs(), w.double().abs(), None, stride, pad)
    k = 3 * kt * kh * kw
    b = 4.0 * (k + 2) * 2.0 ** -24 * (a * sc.abs() + sh.abs())
    if relu_first:
        y = F.relu(y)
    for i, p in enumerate(pools):
        y, b = F.max_pool3d(y, *p), F.max_pool3d(b, *p)
        if i == 0 and not relu_first:
            y = F.relu(y)
    return y, b


def check(got, want, b, dtype, what, nan_sets=None):
    """|got - want| <= b + u |want| (+ 2^-25, f16) on every element; returns max(|got - want| / bound).  No NaN in `got`, or with
    nan_sets = (nan_aten, nan_wide): nan_aten <= isnan(got) <= nan_wide and the bound outside.  An infinity in `got` is +inf and
    stands where the reference, within the bound, passes the storage type's rounding edge."""
    got, want = got.double(), want.double()
    assert got.shape == want.shape, (got.shape, want.shape)
    bound = b + UNIT_ROUNDOFF[dtype] * want.abs() + (2.0 ** -25 if dtype == "f16" else 0.0)
    nan_got = torch.isnan(got)
    if nan_sets is None:
        assert not nan_got.any(), "%s: %d NaN in the output" % (what, int(nan_got.sum()))
    else:
        nan_aten, nan_wide = nan_sets
        assert not (nan_aten & ~nan_got).any(), "%s: %d outputs are finite where ATen's are NaN" % (what, int((nan_aten & ~nan_got).sum()))
        assert not (nan_got & ~nan_wide).any(), "%s: %d NaN outside the 8-column window" % (what, int((nan_got & ~nan_wide).sum()))
    inf_got = torch.isinf(got)
    if dtype != "f32":
        edge = 65520.0 if dtype == "f16" else 2.0 ** 128 * (1.0 - 2.0 ** -9)       # halfway from the largest finite value to the next power of two
        must, may = ~nan_got & (want - bound > edge), want + bound >= edge
        assert not (must & ~inf_got).any(), "%s: %d outputs finite where the reference is beyond %g" % (what, int((must & ~inf_got).sum()), edge)
        assert not (inf_got & ~may).any() and (got[inf_got] > 0).all(), "%s: infinities where the reference has none" % what
    else:
        assert not inf_got.any(), "%s: infinities in the output" % what
    fin = ~(nan_got | inf_got)
    err = (got - want).abs()[fin]
    ratio = float((err / bound[fin].clamp_min(1e-300)).max()) if err.numel() else 0.0
    print("%s [%s]: max |got - want| / bound = %.3f over %d elements" % (what, dtype, ratio, err.numel()))
    bad = err > bound[fin]
    assert not bad.any(), "%s [%s]: %d elements beyond the bound, max |got - want| / bound = %.3f" % (what, dtype, int(bad.sum()), ratio)
    return ratio


def nan_wide_mask(x, kt, pools=(POOL,)):
    """the pooled mask of a conv whose window is dw = 0..7 (one column wider than the 7 x 7 kernel): where 0 x NaN may reach"""
    m = F.pad(torch.isnan(x).any(1, keepdim=True).double(), (3, 4, 3, 3, kt // 2, kt // 2))
    m = F.conv3d(m, torch.ones(1, 1, kt, 7, 8, dtype=torch.float64), None, (1, 2, 2))
    for p in pools:
        m = F.max_pool3d(m, *p)
    return m > 0


# ---------------------------------------------------------------- sizing and class checks

def stem_work_units(dims, kt, dtype, fused):
    """(units, bands, workgroups) of the fused stem launch over (n, t, h, w): af_stem_work_units, no tensor needed"""
    L = hh.lib()
    n, t, h, w = dims
    d = hh._desc((n, t, h, w, 3), 64, (kt, 7, 7), dtype, stride=(1, 2, 2), pad=(kt // 2, 3, 3), dout=(t, (h - 1) // 2 + 1, (w - 1) // 2 + 1))
    units, bands, groups = C.c_int64(0), C.c_int(0), C.c_int(0)
    L.check(L.lib.af_stem_work_units(C.byref(d), fused, C.byref(units), C.byref(bands), C.byref(groups)), "stem_work_units")
    return units.value, bands.value, groups.value


def clips_for(target, W):
    """`target` frames as n >= 2 clips of t <= 40 frames, t no divisor of W where there is such a t"""
    fits = [t for t in range(40, 1, -1) if target % t == 0 and target // t >= 2]
    assert fits, target
    odd = [t for t in fits if W % t != 0]
    t = (odd or fits)[0]
    return target // t, t


def is_first(unit, units, workgroups, umap):
    """unit is the first one its workgroup runs"""
    if umap == "plain":
        return unit < workgroups
    upx = (units + 7) // 8
    return unit % upx < workgroups // 8


def plan(case, dtype):
    """((n, t, h, w), units, bands, workgroups) of the case on this device; asserts the class (change the shape, not this)"""
    fused = 2 if case.kind == "stem3_pool" else 1
    _, _, W = stem_work_units((64, 64) + case.hw, case.kt, dtype, fused)            # 4096 frames: a launch that fills the device
    assert W == CUS, "these cases are written for %d CUs; the library plans for %d" % (CUS, W)
    if case.clips:
        n, t = case.clips
    else:
        n, t = clips_for({"1": W, "1-2": W + 5, "2": 2 * W, ">2": 3 * W + 37}[case.rounds], W)
    dims = (n, t) + case.hw
    units, bands, groups = stem_work_units(dims, case.kt, dtype, fused)
    hq = ((case.hw[0] - 1) // 2) // 2 + 1
    what = "%s: %d units (%d bands) on %d workgroups (change the shape, not this)" % (case.name, units, bands, groups)
    assert groups == min(units, W) and units == n * t * bands and bands == case.bands, what
    assert launch_key(case.kind, dtype, case.kt, case.hw[1], hq, bands, units, groups, case.out or 64) == case_key(case, dtype), what
    if case.clips is None:
        assert units == {"1": W, "1-2": W + 5, "2": 2 * W, ">2": 3 * W + 37}[case.rounds] and groups == W, what
        if case.rounds == "1-2":
            assert units % 8 != 0 and groups % 8 == 0, what
        if case.rounds != "1":            # several clips, t no divisor of W (2 W has no such t) ...
            assert n >= 2 and (W % t != 0 or case.rounds == "2"), what
        if case.rounds in ("2", ">2"):    # ... and a clip's first frame in a unit that is not the first of its workgroup
            assert any(not is_first(b * t, units, groups, case.umap) for b in range(1, n)), what
    return dims, units, bands, groups


# ---------------------------------------------------------------- launches into guarded buffers

def _guarded(rows, width, ldw, off, tdt):
    buf = torch.full((GUARD + rows + GUARD, ldw), 7.0, dtype=tdt, device="cuda")
    ptr = buf.data_ptr() + (GUARD * ldw + off) * buf.element_size()
    assert ptr % 16 == 0
    return buf, C.c_void_p(ptr)


def _collect(buf, rows, width, off, what):
    """the output view as fp64 on the host; every other element of the buffer must still be 7.0"""
    host = buf.cpu()
    got = host[GUARD:GUARD + rows, off:off + width].double().clone()
    host[GUARD:GUARD + rows, off:off + width] = 7.0
    assert torch.all(host == 7.0), "%s: %d guard elements around the output were written" % (what, int((host != 7.0).sum()))
    return got


def run_fused(kind, x, w, scale, shift, dtype, out_ld=0, u8=None, what=""):
    """the fused stem of `kind` -> (n, 64, t, Hq, Wq) fp64; x: (n, 3, t, h, w) fp32 on the host (u8: the uint8 clips packed instead)"""
    L = hh.lib()
    code, tdt = L.DTYPE_CODES[dtype], hh.TORCH_DT[dtype]
    n, _, t, h, wd = x.shape
    kt = w.shape[2]
    d = hh._stem_desc((n, t, h, wd), w, dtype)
    hq, wq = (d.ho - 1) // 2 + 1, (d.wo - 1) // 2 + 1
    xd, wsrc, sc, sf = x.cuda(), w.float().cuda().contiguous(), scale.cuda(), shift.cuda()
    if kind == "stem3_pool":
        sin = torch.zeros(L.lib.af_stem_input_bytes_rgb3(n, t, h, wd, code) // 2, dtype=tdt, device="cuda")
        if u8 is None:
            s = xd.stride()
            L.check(L.lib.af_pack_input_f32_rgb3(hh._p(xd), n, t, h, wd, s[0], s[1], s[2], s[3], s[4], code, hh._p(sin), hh._stream()), "pack_input_f32_rgb3")
        else:
            u8d = u8.cuda()
            mean, std = synth.pixel_mean_std_f32()
            L.check(L.lib.af_pack_input_u8_rgb3(hh._p(u8d), n, t, h, wd, (C.c_float * 3)(*mean.tolist()), (C.c_float * 3)(*std.tolist()), code,
                                                hh._p(sin), hh._stream()), "pack_input_u8_rgb3")
        packed = torch.empty(L.lib.af_packed_stem_weight_bytes_rgb3(kt, code) // 2, dtype=tdt, device="cuda")
        L.check(L.lib.af_pack_stem_weight_rgb3(hh._p(wsrc), 64, kt, code, hh._p(packed), hh._stream()), "pack_stem_weight_rgb3")
    else:
        assert u8 is None and out_ld == 0
        sin = hh.pack_input_f32(xd, dtype)
        packed = torch.empty(L.lib.af_packed_stem_weight_bytes(64, kt, 7, code) // 2, dtype=tdt, device="cuda")
        L.check(L.lib.af_pack_stem_weight(hh._p(wsrc), 64, kt, 7, 7, code, hh._p(packed), hh._stream()), "pack_stem_weight")
    rows = n * t * hq * wq
    ldw, off = (80, 8) if out_ld == 80 else (64, 0)
    assert out_ld in (0, 64, 80)
    buf, out = _guarded(rows, 64, ldw, off, tdt)
    args = (C.byref(d), hh._p(sin), hh._p(packed), hh._p(sc), hh._p(sf), out)
    if kind == "stem_pool":
        L.check(L.lib.af_stem_conv_bn_relu_maxpool(*args, hh._stream()), "stem_conv_bn_relu_maxpool")
    elif out_ld == 0:
        L.check(L.lib.af_stem_conv_bn_relu_maxpool_rgb3(*args, hh._stream()), "stem_conv_bn_relu_maxpool_rgb3")
    else:
        L.check(L.lib.af_stem_conv_bn_relu_maxpool_rgb3_ld(*args, out_ld, hh._stream()), "stem_conv_bn_relu_maxpool_rgb3_ld")
    torch.cuda.current_stream().synchronize()
    return _collect(buf, rows, 64, off, what).reshape(n, t, hq, wq, 64).permute(0, 4, 1, 2, 3)


def _measured(kernel, dtype, ratio):
    MEASURED[(kernel, dtype)] = max(MEASURED.get((kernel, dtype), 0.0), ratio)
    print("largest so far for %s [%s]: %.3f" % (kernel, dtype, MEASURED[(kernel, dtype)]))


# the operands and the fp64 reference of the last few geometries: the two fused kernels and the output forms share them
_refs = collections.OrderedDict()


def _operands_and_reference(case, dtype, dims, poison):
    key = (case.kt, dtype, dims, case.inp, case.special, poison)
    if key not in _refs:
        seed = 7000 + 13 * case.kt + 101 * dims[2] + dims[3] + 7 * dims[0] * dims[1]
        x, w, scale, shift = operands(case.kt, dtype, dims, seed, special=case.special)
        u8 = None
        if case.inp == "u8":
            n, t, h, wd = dims
            u8 = torch.randint(0, 256, (n, t, h, wd, 3), dtype=torch.uint8, generator=torch.Generator().manual_seed(seed))
            x = synth.normalize_like_callers(u8).to(hh.TORCH_DT[dtype]).float().contiguous()
        if poison is not None:
            frame, c, y, col = poison
            x[frame // dims[1], c, frame % dims[1], y, col] = float("nan")
        _refs[key] = (x, w, scale, shift, u8) + reference(x, w, scale, shift)
        while len(_refs) > 3:
            _refs.popitem(last=False)
    return _refs[key]


FUSED_PARAMS = sorted(((dt, c) for c in CASES for dt in DT16 if c.special != "inf" or dt == "f16"),
                      key=lambda p: (p[1].kt, p[1].hw, p[1].clips or (0, 0), p[1].rounds, p[1].inp, p[1].special or "", p[0], p[1].kind, p[1].out))


@pytest.mark.parametrize("dtype,case", FUSED_PARAMS, ids=["%s-%s" % (dt, c.name) for dt, c in FUSED_PARAMS])
def test_fused_stem_vs_fp64(dtype, case):
    dims, units, bands, groups = plan(case, dtype)
    n, t, h, wd = dims
    poison = None
    if case.special == "nan":
        # one NaN pixel in a frame (= unit: no bands) that is not the first unit of its workgroup on either map
        frame = next(f for f in range(groups + 40, units) if not is_first(f, units, groups, "xcd") and not is_first(f, units, groups, "plain"))
        assert case.bands == 1 and not is_first(frame, units, groups, case.umap)
        poison = (frame, 1, h // 2, 6)              # column 2 (mod 4): the eighth column reaches one pooled column further than ATen's window
    x, w, scale, shift, u8, want, b = _operands_and_reference(case, dtype, dims, poison)
    what = "%s: %d units on %d workgroups" % (case.name, units, groups)
    got = run_fused(case.kind, x, w, scale, shift, dtype, case.out, u8, what)
    clean = ~torch.isnan(want)
    assert (want[:, 9][clean[:, 9]] == 0).all() and (want[:, 4][clean[:, 4]] > 0).all()
    nan_sets = None
    if case.special == "nan":
        nan_sets = (torch.isnan(want), nan_wide_mask(x, case.kt))
        assert nan_sets[0].any() and not (nan_sets[0] & ~nan_sets[1]).any() and (nan_sets[1] & ~nan_sets[0]).any()
    if case.special == "inf":
        assert (want[:, 6] > 2 * 65520.0).any() and (want[:, 6] < 60000.0).any()
    _measured(case.kind, dtype, check(got, want, b, dtype, what, nan_sets))
    if case.special == "inf":
        assert torch.isinf(got[:, 6]).any()


STEM_PARAMS = [(dt, c) for c in STEM_CASES for dt in c.dtypes]


@pytest.mark.parametrize("dtype,case", STEM_PARAMS, ids=["%s-c%d-kt%d-%s" % (dt, c.cout, c.kt, "x".join(map(str, c.dims))) for dt, c in STEM_PARAMS])
def test_unfused_stem_and_pool_vs_fp64(dtype, case):
    """af_stem_conv_bn_relu into a guarded buffer against fp64 with the bound; then af_maxpool3d (channels 8 and 64, with and without
    out_ld) of what the kernel wrote against F.max_pool3d of the same values, exactly: the pool of rounded values is exact"""
    L = hh.lib()
    code, tdt = L.DTYPE_CODES[dtype], hh.TORCH_DT[dtype]
    n, t, h, wd = case.dims
    cout, kt = case.cout, case.kt
    x, w, scale, shift = operands(kt, dtype, case.dims, 8100 + cout + kt, cout=cout)
    want, b = reference(x, w, scale, shift, pools=())
    d = hh._stem_desc(case.dims, w, dtype)
    rows = n * t * d.ho * d.wo
    assert rows % 64 != 0
    sin = hh.pack_input_f32(x.cuda(), dtype)
    wsrc = w.cuda().contiguous()
    packed = torch.empty(L.lib.af_packed_stem_weight_bytes(cout, kt, 7, code) // tdt.itemsize, dtype=tdt, device="cuda")
    L.check(L.lib.af_pack_stem_weight(hh._p(wsrc), cout, kt, 7, 7, code, hh._p(packed), hh._stream()), "pack_stem_weight")
    cpad = L.lib.af_padded_channels(cout)                # the kernels read scale / shift over their channel tile
    sc, sf = torch.zeros(cpad, device="cuda"), torch.zeros(cpad, device="cuda")
    sc[:cout], sf[:cout] = scale.cuda(), shift.cuda()
    buf, out = _guarded(rows, cout, cout, 0, tdt)
    L.check(L.lib.af_stem_conv_bn_relu(C.byref(d), hh._p(sin), hh._p(packed), hh._p(sc), hh._p(sf), out, hh._stream()), "stem_conv_bn_relu")
    torch.cuda.current_stream().synchronize()
    what = "stem %d channels kt %d %s" % (cout, kt, case.dims)
    got = _collect(buf, rows, cout, 0, what)
    kernel = "stem_rows" if cout <= 16 and dtype != "f32" else "stem"
    _measured(kernel, dtype, check(got.reshape(n, t, d.ho, d.wo, cout).permute(0, 4, 1, 2, 3), want, b, dtype, what))
    if cout not in (8, 64):
        return
    y = buf[GUARD:GUARD + rows].reshape(n, t, d.ho, d.wo, cout).contiguous()
    pooled_want = F.max_pool3d(y.float().cpu().permute(0, 4, 1, 2, 3), *POOL).permute(0, 2, 3, 4, 1)
    for ld in (0, cout + 16):
        pd = L.pool_desc(n, (t, d.ho, d.wo), cout, *POOL, code, None, ld)
        prow = n * pd.to * pd.ho * pd.wo
        pbuf, pout = _guarded(prow, cout, ld or cout, 8 if ld else 0, tdt)
        L.check(L.lib.af_maxpool3d(C.byref(pd), hh._p(y), pout, hh._stream()), "maxpool3d")
        torch.cuda.current_stream().synchronize()
        pgot = _collect(pbuf, prow, cout, 8 if ld else 0, what + " pool ld %d" % ld)
        assert torch.equal(pgot.reshape(pooled_want.shape), pooled_want.double()), "%s: af_maxpool3d (out_ld %d) differs from F.max_pool3d" % (what, ld)


TSTEM_PARAMS = [(kind, dt, dims) for kind, kt, dts in TSTEM_CASES for dt in dts
                for dims in (((2, 3, 16, 72), (1, 6, 20, 28)) + (((1, 262200, 2, 2),) if kind == "tstem" else ((1, 131100, 4, 4),)))]


@pytest.mark.parametrize("kind,dtype,dims", TSTEM_PARAMS, ids=["%s-%s-%s" % (k, dt, "x".join(map(str, dm))) for k, dt, dm in TSTEM_PARAMS])
def test_temporal_stems_guards_and_capped_grid(kind, dtype, dims):
    """what tests/test_hip_ftcn.py lacks for af_tstem_conv_bn_pool_relu[_maxpool]: the guard rows around the output, and a launch of
    more tiles than 16 x blocks (the grid is capped at 256 x 64 / 256 x 32 blocks), where the waves' grid-stride loops run unevenly
    (262200 / 131100 tiles of one pooled pixel on 65536 / 32768 waves)"""
    L = hh.lib()
    code, tdt = L.DTYPE_CODES[dtype], hh.TORCH_DT[dtype]
    n, t, h, wd = dims
    kt = 5
    x, w, scale, shift = operands(kt, dtype, dims, 8800 + h + wd, kernel_hw=(1, 1), wscale=0.5)
    pools = (((1, 2, 2), (1, 2, 2), (0, 0, 0)),) + ((POOL,) if kind == "tstem_pool3" else ())
    want, b = reference(x, w, scale, shift, stride=(1, 1, 1), pad=(kt // 2, 0, 0), pools=pools, relu_first=False)
    tiles = n * t * want.shape[3] * (-(-want.shape[4] // 16))
    cap = 256 * (64 if kind == "tstem" else 32)
    assert (t > 1000) == (tiles > 16 * cap)
    sin = hh.pack_input_f32(x.cuda(), dtype)
    wsrc = w.cuda().contiguous()
    packed = torch.empty(L.lib.af_packed_tstem_weight_bytes(code) // tdt.itemsize, dtype=tdt, device="cuda")
    L.check(L.lib.af_pack_tstem_weight(hh._p(wsrc), 64, kt, code, hh._p(packed), hh._stream()), "pack_tstem_weight")
    d = L.ConvDesc()
    d.n, d.t, d.h, d.w, d.cin, d.cout = n, t, h, wd, 3, 64
    d.kt, d.kh, d.kw, d.st, d.sh, d.sw, d.pt, d.ph, d.pw = kt, 1, 1, 1, 1, 1, kt // 2, 0, 0
    d.to, d.ho, d.wo, d.relu, d.dtype = t, h // 2, wd // 2, 1, code
    rows = n * t * want.shape[3] * want.shape[4]
    sc, sf = scale.cuda(), shift.cuda()
    buf, out = _guarded(rows, 64, 64, 0, tdt)
    fn = L.lib.af_tstem_conv_bn_pool_relu if kind == "tstem" else L.lib.af_tstem_conv_bn_pool_relu_maxpool
    L.check(fn(C.byref(d), hh._p(sin), hh._p(packed), hh._p(sc), hh._p(sf), out, hh._stream()), kind)
    torch.cuda.current_stream().synchronize()
    what = "%s %s, %d tiles" % (kind, dims, tiles)
    got = _collect(buf, rows, 64, 0, what).reshape(n, t, want.shape[3], want.shape[4], 64).permute(0, 4, 1, 2, 3)
    _measured(kind, dtype, check(got, want, b, dtype, what))


# ---------------------------------------------------------------- the input packs, byte for byte

SENTINEL = 0x5AC3          # a 16-bit pattern (a finite, odd value in both 16-bit types) no pack writes by accident


def _strided_source(kind, n, t, h, w, seed):
    """a logical (n, 3, t, h, w) fp32 view on the device: a permuted NTHWC tensor, or a view with a storage offset and a row stride
    larger than w"""
    g = torch.Generator().manual_seed(seed)
    if kind == "nthwc":
        return torch.randn((n, t, h, w, 3), generator=g).cuda().permute(0, 4, 1, 2, 3)
    big = torch.randn((n, 3, t, h + 1, w + 5), generator=g).cuda()
    view = big[:, :, :, 1:, 2:2 + w]
    assert view.storage_offset() > 0 and view.stride(3) > w and not view.is_contiguous()
    return view


@pytest.mark.parametrize("source", ["nthwc", "offset"])
@pytest.mark.parametrize("layout,dtype", [("c4", "f32"), ("c4", "f16"), ("c4", "bf16"), ("rgb3", "f16"), ("rgb3", "bf16")])
def test_pack_f32_from_strided_sources_byte_for_byte(layout, dtype, source):
    """af_pack_input_f32 / af_pack_input_f32_rgb3 from strided sources into a buffer prefilled with a 16-bit sentinel, compared whole
    with a host-built image of the documented layout (af_hip.h): the interior cells written - in the 4-channel layout with their
    zero fourth channel, which the pack writes -, every halo, padding and slack byte still the sentinel; widths 1, 7, 8, 9"""
    L = hh.lib()
    code, tdt = L.DTYPE_CODES[dtype], hh.TORCH_DT[dtype]
    n, t, h = 2, 3, 4
    for w in (1, 7, 8, 9):
        x = _strided_source(source, n, t, h, w, 300 + w)
        s = x.stride()
        if layout == "c4":
            nbytes = L.lib.af_stem_input_bytes(n, t, h, w, code)
            fn = L.lib.af_pack_input_f32
        else:
            nbytes = L.lib.af_stem_input_bytes_rgb3(n, t, h, w, code)
            fn = L.lib.af_pack_input_f32_rgb3
        assert nbytes % 2 == 0
        dst = torch.full((nbytes // 2,), SENTINEL, dtype=torch.int16, device="cuda")
        L.check(fn(hh._p(x), n, t, h, w, s[0], s[1], s[2], s[3], s[4], code, hh._p(dst), hh._stream()), "pack_input_f32 " + layout)
        torch.cuda.current_stream().synchronize()
        image = torch.full((nbytes // 2,), SENTINEL, dtype=torch.int16)
        cells = x.cpu().permute(0, 2, 3, 4, 1).to(tdt)                             # (n, t, h, w, 3), one rounding
        if layout == "c4":
            img = image.view(tdt).view(n, t + 4, h + 6, w + 8, 4)
            img[:, 2:2 + t, 3:3 + h, 3:3 + w, :3] = cells
            img[:, 2:2 + t, 3:3 + h, 3:3 + w, 3] = 0
        else:
            row = ((w + 8) * 6 + 15) // 16 * 16 // 2                               # 16-bit elements per row
            assert nbytes // 2 == (n * (t + 4) * (h + 6) + 8) * row
            img = image.view(tdt)[:n * (t + 4) * (h + 6) * row].view(n, t + 4, h + 6, row)
            img[:, 2:2 + t, 3:3 + h, 9:9 + 3 * w] = cells.reshape(n, t, h, 3 * w)
        got = dst.cpu()
        assert torch.equal(got, image), "%s %s w = %d: %d of %d 16-bit words differ from the documented layout" % (
            layout, dtype, w, int((got != image).sum()), image.numel())


@pytest.mark.parametrize("path,shape", [("scalar", (1, 4, 131, 1001, 2)), ("vector", (1, 4, 257, 4096, 2))])
def test_pathways_pack_loops_more_than_once_per_thread(path, shape):
    """af_pack_input_u8_pathways caps its grid at 8 x CUs blocks of 256 threads: just above that many pixels (scalar path, odd w) and
    just above that many 8-pixel runs (vector path, w % 8 == 0) some threads loop twice; the outputs must equal the two single packs
    byte for byte (as tests/test_hip_u8_networks.py checks the small shapes)"""
    import test_hip_u8_networks as u8n
    L = hh.lib()
    n, t, h, w, alpha = shape
    cus = torch.cuda.get_device_properties(torch.cuda.current_device()).multi_processor_count
    work = n * t * h * (w // 8 if path == "vector" else w)
    assert (w % 8 == 0) == (path == "vector") and 8 * cus * 256 < work < 2 * 8 * cus * 256, (work, cus)
    clip = u8n._random_clip(n, t, h, w, seed=77).cuda()
    assert clip.data_ptr() % 8 == 0
    u8n._check_pathways(clip, alpha, "bf16", L.AF_PACK_RGB3, L.AF_PACK_C4)
