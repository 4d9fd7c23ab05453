"""Host side of the HIP forward: turns a network spec + checkpoint tensors into a flat list of
libafhip ops over caller-owned HBM buffers, and runs it with ONE C call per forward.

What this orchestrates is the reference's ``ResNet.forward`` / ``SlowFast.forward``
(altfreezing/slowfast/models/video_model_builder.py:561-578, :370-387): stem(s) -> [lateral] -> s2 -> [lateral] ->
pool -> s3 -> ... -> head, with every Conv3d+BatchNorm3d(+add)(+ReLU)(+pool) group collapsed into one kernel
launch.  PyTorch is used only to own device memory and the stream.
"""
import collections
import ctypes as C
import dataclasses
import os
from typing import Dict, List, Optional

import torch

from . import _lib
from ._lib import Op, check, lib
from .arch import BN_EPS, ConvSpec, FtcnTTSpec, NetSpec, PoolSpec, SlowFastSpec

_TORCH_DTYPE = {"f32": torch.float32, "bf16": torch.bfloat16, "f16": torch.float16}
_ELEM_SIZE = {"f32": 4, "bf16": 2, "f16": 2}

# op tags (echoed by the timed runner; used by bench.py to attribute device time to kernel classes)
TAG_PACK, TAG_STEM, TAG_POOL, TAG_HEAD = 0, 1, 2, 3
TAG_CONV_1x1x1, TAG_CONV_Tx1x1, TAG_CONV_1x3x3, TAG_CONV_OTHER, TAG_CONV_BC, TAG_CONV_CA, TAG_BLOCK_ABC = 10, 11, 12, 13, 14, 15, 16
TAG_NAMES = {TAG_PACK: "input_pack", TAG_STEM: "stem", TAG_POOL: "maxpool", TAG_HEAD: "head",
             TAG_CONV_1x1x1: "conv_1x1x1", TAG_CONV_Tx1x1: "conv_3x1x1", TAG_CONV_1x3x3: "conv_1x3x3",
             TAG_CONV_OTHER: "conv_other", TAG_CONV_BC: "conv_1x3x3+1x1x1_fused", TAG_CONV_CA: "conv_1x1x1+3x1x1_fused",
             TAG_BLOCK_ABC: "bottleneck_block_fused"}


def _conv_tag(cv: ConvSpec) -> int:
    k = tuple(cv.kernel)
    if k == (1, 1, 1):
        return TAG_CONV_1x1x1
    if k[1:] == (1, 1):
        return TAG_CONV_Tx1x1
    if k[0] == 1 and k[1:] == (3, 3):
        return TAG_CONV_1x3x3
    return TAG_CONV_OTHER


def _ptr(t: Optional[torch.Tensor]):
    return None if t is None else C.c_void_p(t.data_ptr())


def _stream_ptr(device):
    return C.c_void_p(torch.cuda.current_stream(device).cuda_stream)


def _pool_out(dims, p: PoolSpec):
    return tuple((d + 2 * pp - k) // s + 1 for d, k, s, pp in zip(dims, p.kernel, p.stride, p.pad))


def _is_pool(p: PoolSpec, k, s, pad):
    return (tuple(p.kernel), tuple(p.stride), tuple(p.pad)) == (k, s, pad)


def _stages_of(spec):
    if isinstance(spec, SlowFastSpec):
        return [st for pair in spec.stages for st in pair]
    return list(spec.stages)


class PackedWeights:
    """Device-resident, kernel-ready copy of a checkpoint: per conv a packed weight in the compute
    dtype plus fp32 BatchNorm scale/shift; fp32 head.  Built with HIP kernels (af_pack.hip)."""

    def __init__(self, spec, state: Dict[str, torch.Tensor], dtype: str, device):
        self.dtype, self.device = dtype, device
        code = _lib.DTYPE_CODES[dtype]
        st = self._stream = _stream_ptr(device)
        f32 = lambda k: state[k].detach().to(device=device, dtype=torch.float32).contiguous()
        stems = set(c.conv for c in (spec.stems if isinstance(spec, SlowFastSpec) else (spec.stem,)))
        self.w, self.scale, self.shift = {}, {}, {}
        self.w3 = {}             # stem conv -> the K-packed image of the same weights (fused 16-bit stem, af_stem3.hip); may be empty
        for cv in spec.convs():
            w = f32(cv.conv + ".weight")
            assert tuple(w.shape) == cv.weight_shape, (cv.conv, tuple(w.shape), cv.weight_shape)
            bn = [f32(cv.bn_key + s) for s in (".weight", ".bias", ".running_mean", ".running_var")]
            cpad = lib.af_padded_channels(cv.cout)           # kernels read scale/shift over the padded channel tile
            scale = torch.zeros(cpad, dtype=torch.float32, device=device)
            shift = torch.zeros(cpad, dtype=torch.float32, device=device)
            check(lib.af_fold_bn(_ptr(bn[0]), _ptr(bn[1]), _ptr(bn[2]), _ptr(bn[3]), BN_EPS, cv.cout,
                                 _ptr(scale), _ptr(shift), st), "af_fold_bn")
            kt, kh, kw = cv.kernel
            if cv.conv in stems and isinstance(spec, FtcnTTSpec):        # temporal stem: MFMA A-fragment image
                packed = self._pack(lib.af_pack_tstem_weight, lib.af_packed_tstem_weight_bytes(code), _ptr(w), cv.cout, kt, code)
            elif cv.conv in stems:
                packed = self._pack(lib.af_pack_stem_weight, lib.af_packed_stem_weight_bytes(cv.cout, kt, kh, code),
                                    _ptr(w), cv.cout, kt, kh, kw, code)
            else:
                packed = self._pack_conv(w, code)
            self.w[cv.conv], self.scale[cv.conv], self.shift[cv.conv] = packed, scale, shift
            if (cv.conv in stems and not isinstance(spec, FtcnTTSpec) and dtype != "f32" and cv.cout == 64
                    and (kh, kw) == (7, 7)):
                self.w3[cv.conv] = self._pack(lib.af_pack_stem_weight_rgb3, lib.af_packed_stem_weight_bytes_rgb3(kt, code),
                                              _ptr(w), cv.cout, kt, code)
        # block 0 of every stage: last 1x1x1 + projection shortcut share one accumulator (af_conv3d_dual_bn_act):
        # both weights get their BN scale folded in (fp32, before the rounding), shifts are summed
        self.w_folded, self.shift_sum, self.ones = {}, {}, {}
        for stage in _stages_of(spec):
            for blk in stage.blocks:
                if blk.branch1 is None or blk.branch1.pool_after_bn is not None:
                    continue                 # (FTCN: a pooled shortcut cannot share the c conv's accumulator)
                for cv in (blk.c, blk.branch1):
                    self.w_folded[cv.conv] = self._pack_conv(f32(cv.conv + ".weight"), code, self.scale[cv.conv])
                self.shift_sum[blk.c.conv] = (self.shift[blk.c.conv] + self.shift[blk.branch1.conv]).contiguous()
                self.ones[blk.c.conv] = torch.ones(lib.af_padded_channels(blk.c.cout), dtype=torch.float32, device=device)
        if isinstance(spec, FtcnTTSpec):
            # transformer head, fp32 whatever the trunk's dtype: Linear weights packed for the fp32 conv kernel,
            # bias as its `shift` (scale = ones), LayerNorm / token parameters as they are
            h = spec.head
            l0, l1 = h + ".transformer.layers.0.0.fn", h + ".transformer.layers.0.1.fn"
            self.lin = {}
            for name, wkey, bkey in (("qkv", l0 + ".fn.to_qkv.weight", None),
                                     ("out", l0 + ".fn.to_out.0.weight", l0 + ".fn.to_out.0.bias"),
                                     ("ff1", l1 + ".fn.net.0.weight", l1 + ".fn.net.0.bias"),
                                     ("ff2", l1 + ".fn.net.3.weight", l1 + ".fn.net.3.bias")):
                w = f32(wkey)
                cout, cin = w.shape
                packed = self._pack_conv(w.reshape(cout, cin, 1, 1, 1), _lib.AF_F32, dtype="f32")
                cpad = lib.af_padded_channels(cout)
                bias = torch.zeros(cpad, dtype=torch.float32, device=device)
                if bkey is not None:
                    bias[:cout] = f32(bkey)
                self.lin[name] = (packed, torch.ones(cpad, dtype=torch.float32, device=device), bias, cin, cout)
            self.ln = {"attn": (f32(l0 + ".norm.weight"), f32(l0 + ".norm.bias")),
                       "ff": (f32(l1 + ".norm.weight"), f32(l1 + ".norm.bias")),
                       "head": (f32(h + ".mlp_head.0.weight"), f32(h + ".mlp_head.0.bias"))}
            self.cls_token = f32(h + ".cls_token").reshape(-1)
            self.pos_embedding = f32(h + ".pos_embedding").reshape(spec.tokens + 1, spec.dim)
            self.fc_w, self.fc_b = f32(h + ".mlp_head.1.weight"), f32(h + ".mlp_head.1.bias")
        else:
            self.fc_w, self.fc_b = f32(spec.head + ".weight"), f32(spec.head + ".bias")
        torch.cuda.current_stream(device).synchronize()      # sources may be freed by the caller

    def _pack(self, fn, nbytes, *args, dtype=None):
        """One pack call of the library: a buffer of the size it asks for, the call, its status."""
        dtype = dtype or self.dtype
        packed = torch.empty(nbytes // _ELEM_SIZE[dtype], dtype=_TORCH_DTYPE[dtype], device=self.device)
        check(fn(*args, _ptr(packed), self._stream), fn.__name__)
        return packed

    def _pack_conv(self, w, code, scale=None, dtype=None):
        """(Cout, Cin, kT, kH, kW) fp32 weights in the conv kernels' layout; ``scale``: folded into the rows before the rounding."""
        shape = tuple(w.shape)
        nbytes = lib.af_packed_conv_weight_bytes(*shape, code)
        if scale is None:
            return self._pack(lib.af_pack_conv_weight, nbytes, _ptr(w), *shape, code, dtype=dtype)
        return self._pack(lib.af_pack_conv_weight_scaled, nbytes, _ptr(w), _ptr(scale), *shape, code, dtype=dtype)

    def bn(self, cv: ConvSpec):
        """(weight, scale, shift) device pointers of a conv with its own BatchNorm."""
        return self.w[cv.conv].data_ptr(), self.scale[cv.conv].data_ptr(), self.shift[cv.conv].data_ptr()

    def folded(self, c: ConvSpec, branch1: ConvSpec):
        """(w_c, w_1, ones, shift_sum) device pointers of a c conv and its projection shortcut sharing one accumulator: both
        weights carry their BN scale, the kernel's scale is ones and its shift the sum of the two shifts."""
        return (self.w_folded[c.conv].data_ptr(), self.w_folded[branch1.conv].data_ptr(), self.ones[c.conv].data_ptr(),
                self.shift_sum[c.conv].data_ptr())


# The plan's switches (A/B runs and tests): name -> on by default.  Read whenever a plan is built; "1" is on, anything else off.
SWITCHES = {"AF_FUSE_BC": False, "AF_FUSE_CA": True, "AF_FUSE_CPA": False, "AF_FUSE_ABC": True, "AF_FUSE_TSTEM_POOL": True,
            "AF_SLOWFAST_STEM3": True}


def _read_switches():
    return {name: os.environ.get(name, "1" if on else "0") == "1" for name, on in SWITCHES.items()}


# The convs of a fused launch by role, in the parameter order of the library entry point it goes to (a lone conv's role: "conv").
_ROLES = {"dual": ("c", "branch1"), "ca": ("c", "branch1", "a_next"), "cpa": ("c", "a_next"), "abc": ("a", "b", "c", "branch1"),
          "bc": ("b", "c")}
# The fused kinds the library is asked about: kind -> (switch, its predicate over the launch's descriptors).
#   bc   a bottleneck's b (1x3x3) and c (1x1x1 + residual) convs (af_conv3d_bc_bn_act).  OFF unless AF_FUSE_BC=1: measured slower
#        than the two launches, whose MFMA-bound b and HBM-bound c overlap across workgroups
#   ca   a block's c conv (+ residual or projection shortcut, + ReLU) and the NEXT block's a conv (af_conv3d_ca_bn_act)
#   cpa  a stage's last c conv (+ residual + ReLU), the temporal max-pool behind the stage and the NEXT stage's first a conv
#        (af_conv3d_cpa_bn_act; the predicate also takes x_sub).  OFF unless AF_FUSE_CPA=1
#   abc  a whole block, a, b, c + identity or stride-1 projection shortcut + ReLU (af_block_abc_bn_act: SlowFast's Fast pathway)
_QUESTIONS = {"bc": ("AF_FUSE_BC", lib.af_conv_bc_fusable), "ca": ("AF_FUSE_CA", lib.af_conv_ca_fusable),
              "cpa": ("AF_FUSE_CPA", lib.af_conv_cpa_fusable), "abc": ("AF_FUSE_ABC", lib.af_block_abc_fusable)}


@dataclasses.dataclass
class Launch:
    """One launch of a plan.  ``convs``: its ConvSpecs by role (_ROLES; None for a conv this launch does not have); ``descs``: their
    af_conv_desc in the same order, built once, by the planner: the library's *_fusable predicate is asked with them, the op is
    filled from them, tools and tests read them.  A lone conv's carries its own ReLU, the convs of a fused launch relu = 1."""
    kind: str
    convs: Dict[str, Optional[ConvSpec]] = dataclasses.field(default_factory=dict)
    descs: tuple = ()
    src: Optional[str] = None            # input
    src2: Optional[str] = None           # what the projection shortcut reads (dual, ca)
    res: Optional[str] = None            # residual
    dst: Optional[str] = None            # output
    dst_a: Optional[str] = None          # output of the a conv behind a c conv (ca, cpa)
    ld: int = 0                          # row stride of the output, in channels
    ch_off: int = 0                      # first channel written in those rows
    x_sub: int = 0                       # cpa: 2 = the pooled trunk is stored at its even (h, w) only, else 1
    pool: Optional[_lib.PoolDesc] = None # the pooling launches (and the token pool of tt_head)

    @property
    def tpool(self) -> int:              # of the conv that writes the output: 1 = the temporal max-pool rides in its epilogue, 2 = a 1x2x2
        return self.descs[0].tpool if self.descs else 0

    def refs(self):                      # ``descs`` as the library takes them
        return [None if d is None else C.byref(d) for d in self.descs]

    def macs(self) -> int:
        return sum(cv.macs(d.t, d.h, d.w) for cv, d in zip(self.convs.values(), self.descs) if cv is not None)


# What a block hands the next (a stage's last: the next stage's first): the launch of its c conv already ran that block's a conv;
# it stored the trunk only where a stride-(1,2,2) projection shortcut reads it.
_Handoff = collections.namedtuple("_Handoff", "a_done sub", defaults=(False, False))


class _Plan:
    """Accumulates ``launches`` and the element count every named activation buffer must hold (``sizes``), and keeps what the
    library was ``asked``: (switch, answer, candidate Launch) per question, in order.  The network planners add what the engine
    needs besides: ``inputs`` [(stem-input buffer, dims, temporal stride)], ``rgb3`` (the single input feeds a K-packed stem),
    ``rgb3_inputs`` (SlowFast: the inputs that do), ``head_dims`` and ``head_width``."""

    def __init__(self, batch, dtype):
        self.batch, self.dtype, self.code = batch, dtype, _lib.DTYPE_CODES[dtype]
        self.launches, self.asked, self.sizes, self.switch = [], [], {}, _read_switches()
        self.handoff = _Handoff()            # of the block planned last
        self.inputs, self.rgb3, self.rgb3_inputs, self.head_dims, self.head_width = [], False, set(), None, None

    def need(self, buf, dims, width):
        self.sizes[buf] = max(self.sizes.get(buf, 0), self.batch * dims[0] * dims[1] * dims[2] * width)

    def make(self, kind, convs, **where) -> Launch:
        """A launch of ``kind`` over ``convs``: (role, ConvSpec or None, din, dout[, tpool]) each, in the order of _ROLES.  ``ld``
        defaults to the channels of the conv that writes the output."""
        assert tuple(c[0] for c in convs) == _ROLES.get(kind, ("conv",)), (kind, convs)
        # lone: a, b, stems and laterals carry their own ReLU; c (final_bn) takes the block's add + ReLU; the projection shortcut
        # has neither (resnet_helper.py:311-326, 438-444; video_model_builder.py:136-143)
        descs = tuple(cv and _lib.conv_desc(self.batch, din, cv.cin, cv.cout, cv.kernel, cv.stride, cv.pad,
                                            len(convs) > 1 or cv.relu or cv.final_bn, self.code, dout, *tpool)
                      for _, cv, din, dout, *tpool in convs)
        specs = {c[0]: c[1] for c in convs}
        where.setdefault("ld", (specs.get("c") or specs.get("conv")).cout)
        return Launch(kind, specs, descs, **where)

    def conv(self, cv: ConvSpec, din, dout, src, dst, kind="conv", tpool=0, **where):
        """a conv (or stem) launch of its own"""
        self.launches.append(self.make(kind, [("conv", cv, din, dout, tpool)], src=src, dst=dst, **where))

    def pool(self, kind, p, ch, din, dout, src, **where):
        """a pooling launch: ``p`` a PoolSpec, or the kernel alone (stride 1, no padding); ``ld`` goes into its descriptor"""
        kernel, stride, pad = (p.kernel, p.stride, p.pad) if isinstance(p, PoolSpec) else (p, (1, 1, 1), (0, 0, 0))
        desc = _lib.pool_desc(self.batch, din, ch, kernel, stride, pad, self.code, dout, where.pop("ld", 0))
        self.launches.append(Launch(kind, src=src, pool=desc, **where))

    def ask(self, cand: Launch) -> Optional[Launch]:
        """The candidate, if its switch is on (else no question reaches the library) and the library runs its descriptors as one launch."""
        switch, question = _QUESTIONS[cand.kind]
        if not self.switch[switch]:
            return None
        yes = bool(question(*cand.refs(), *((cand.x_sub,) if cand.kind == "cpa" else ())))
        self.asked.append((switch, yes, cand))
        return cand if yes else None

    def stage(self, stage, d, cur, nxt, a_buf, b_buf, last_ld=None, tpool_last=False, next_stage=None):
        """One pathway's ResStage.  ``last_ld``: row stride of the stage's final output (room for the lateral's channels);
        ``next_stage`` (with ``tpool_last``): the stage behind the temporal pool, whose first a conv may ride in this stage's last launch.
        Returns (dims, channels, buffer holding the output, the other trunk buffer, whether the temporal pool rode in the last launch)."""
        c, tpooled = None, False
        for bi, blk in enumerate(stage.blocks):
            last = bi == len(stage.blocks) - 1
            nxa = None if last else stage.blocks[bi + 1].a
            ld = last_ld if (last and last_ld) else blk.c.cout
            tpool_here = tpool_last and last
            hand, self.handoff = self.handoff, _Handoff()
            dout = None if (hand.a_done or tpool_here) else self._whole_block(blk, d, cur, nxt, ld)
            if dout is None:
                da = blk.a.out_dims(*d)
                if not hand.a_done:
                    self.conv(blk.a, d, da, cur, a_buf)
                self.need(a_buf, da, blk.a.cout)
                dout, c_src = self._b_side(blk, da, cur, nxt, a_buf, b_buf, ld, with_c=not tpool_here)
                if c_src is not None:
                    res = cur
                    if blk.branch1 is not None and blk.branch1.pool_after_bn is not None:
                        # pooled projection shortcut: conv + BN, pool, then it is the residual of the c conv
                        _, res = self._conv_maxpool(blk.branch1, d, cur, "R1", "R0", "R1")
                    dout, self.handoff, tpooled = self._c_side(blk, nxa, d, dout, c_src, res, cur, nxt, a_buf, ld, hand.sub, tpool_here,
                                                               next_stage)
            d, cur, nxt, c = dout, nxt, cur, blk.c.cout
        return d, c, cur, nxt, tpooled

    def _whole_block(self, blk, d, cur, nxt, ld):
        """The whole block as one launch (narrow pathway): trunk in, trunk out, a and b stay on the CU.  Returns the output dims,
        or None where the library does not run it so."""
        da = blk.a.out_dims(*d)
        db = blk.b.out_dims(*da)
        dc = blk.c.out_dims(*db)
        if (any(cv is not None and cv.pool_after_bn is not None for cv in (blk.a, blk.b, blk.c, blk.branch1))
                or (blk.branch1 is not None and blk.branch1.out_dims(*d) != dc)):
            return None
        launch = self.ask(self.make("abc", [("a", blk.a, d, da), ("b", blk.b, da, db), ("c", blk.c, db, dc), ("branch1", blk.branch1, d, dc)],
                                    src=cur, dst=nxt, ld=ld))
        if launch is not None:
            self.launches.append(launch); self.need(nxt, dc, ld)
            return dc

    def _b_side(self, blk, da, cur, nxt, a_buf, b_buf, ld, with_c):
        """The b conv.  Returns (dims, buffer) of what the c conv reads; or, where b, c, the residual add and the ReLU went as one
        launch (``with_c`` allows it), (the block's output dims, None)."""
        if blk.b.pool_after_bn is not None:
            return self._conv_maxpool(blk.b, da, a_buf, b_buf, b_buf, a_buf)       # the pool of its own goes into the free a buffer
        db = blk.b.out_dims(*da)
        if blk.branch1 is None and with_c:
            # b + c + residual + ReLU in one launch: the b output of a frame stays in LDS (s3 / s4 at bench batch sizes)
            dc = blk.c.out_dims(*db)
            launch = self.ask(self.make("bc", [("b", blk.b, da, db), ("c", blk.c, db, dc)], src=a_buf, res=cur, dst=nxt, ld=ld))
            if launch is not None:
                self.launches.append(launch); self.need(nxt, dc, ld)
                return dc, None
        self.conv(blk.b, da, db, a_buf, b_buf); self.need(b_buf, db, blk.b.cout)
        return db, b_buf

    def _conv_maxpool(self, cv: ConvSpec, din, src, fused_dst, conv_dst, pool_dst):
        """FTCN's conv -> BN -> MaxPool3d -> ReLU.  A 1x2x2 pool over even sizes rides in the conv's launch, into ``fused_dst`` (max
        and ReLU commute: the tile rows are ordered so that a 2x2 window is 4 adjacent rows and the epilogue stores their max); else
        the conv goes into ``conv_dst`` and the pool, a launch of its own, into ``pool_dst``.  Returns (pooled dims, their buffer)."""
        p, dout = cv.pool_after_bn, cv.out_dims(*din)
        dp = _pool_out(dout, p)
        if _is_pool(p, (1, 2, 2), (1, 2, 2), (0, 0, 0)) and dout[1] % 2 == 0 and dout[2] % 2 == 0:
            self.conv(cv, din, dout, src, fused_dst, tpool=2); self.need(fused_dst, dp, cv.cout)
            return dp, fused_dst
        self.conv(cv, din, dout, src, conv_dst); self.need(conv_dst, dout, cv.cout)
        self.pool("pool", p, cv.cout, dout, dp, conv_dst, dst=pool_dst); self.need(pool_dst, dp, cv.cout)
        return dp, pool_dst

    def _c_side(self, blk, nxa, d, db, c_src, res, cur, nxt, a_buf, ld, sub, tpool_here, next_stage):
        """The c conv with the block's shortcut, add and ReLU, as the first of these that applies: dual on a subsampled trunk (``sub``:
        a cpa launch with x_sub = 2 stored ``cur``), ca with projection, dual, ca, cpa, conv.  ``nxa``: the next block's a conv, None
        behind the last block.  Returns (the dims stored, what the next block is handed, whether the temporal pool rode along)."""
        dc = blk.c.out_dims(*db)
        proj = blk.branch1 if (blk.branch1 is not None and blk.branch1.pool_after_bn is None) else None
        # the temporal max-pool after s2 rides in the epilogue of s2's last conv when it can
        tp = bool(tpool_here and blk.branch1 is None and dc[0] % 2 == 0)
        c = ("c", blk.c, db, dc)
        a_next = lambda: ("a_next", nxa, dc, nxa.out_dims(*dc))
        may_ca = nxa is not None and ld == blk.c.cout and nxa.pool_after_bn is None
        launch = None
        if proj is not None and sub:
            # the previous stage's last launch stored the trunk only where this stride-(1,2,2) shortcut reads it, packed:
            # the same weights as a stride-1 convolution over that tensor
            b1 = dataclasses.replace(proj, stride=(1, 1, 1))
            dsub = (d[0], d[1] // 2, d[2] // 2)
            assert b1.out_dims(*dsub) == dc
            launch = self.make("dual", [c, ("branch1", b1, dsub, dc)], src=c_src, src2=cur, dst=nxt, ld=ld)
        elif proj is not None:
            # c conv + projection shortcut in one launch, no shortcut tensor; and the next block's a conv behind them (s2) where
            # the library takes it: the trunk slab never comes back from HBM
            assert proj.out_dims(*d) == dc
            b1 = ("branch1", proj, d, dc)
            launch = may_ca and self.ask(self.make("ca", [c, b1, a_next()], src=c_src, src2=cur, dst=nxt, dst_a=a_buf))
            launch = launch or self.make("dual", [c, b1], src=c_src, src2=cur, dst=nxt, ld=ld)
        elif may_ca and not tp and res == cur:
            # c + residual + ReLU of this block and the a conv of the next one in one launch (s2): the trunk slab is
            # produced in LDS, stored once, and multiplied by the temporal taps without being read back
            launch = self.ask(self.make("ca", [c, ("branch1", None, d, dc), a_next()], src=c_src, res=res, dst=nxt, dst_a=a_buf))
        elif tp and next_stage is not None and res == cur and ld == blk.c.cout:
            # s2 -> s3: c + residual + ReLU, the temporal pool and the next stage's first a conv in one launch; the pooled trunk
            # is stored only where the next stage's projection shortcut reads it
            launch = self._boundary(blk.c, next_stage.blocks[0], db, dc, c_src, res, nxt, a_buf)
        launch = launch or self.make("conv", [("conv", blk.c, db, dc, int(tp))], src=c_src, res=res, dst=nxt, ld=ld)
        self.launches.append(launch)
        if launch.dst_a:
            a = launch.descs[-1]
            self.need(a_buf, (a.to, a.ho, a.wo), a.cout)
        dstore = (dc[0] // 2,) + tuple(dc[1:]) if tp else dc
        self.need(nxt, dstore, ld)
        return dstore, _Handoff(bool(launch.dst_a), launch.x_sub == 2), launch.tpool == 1

    def _boundary(self, c: ConvSpec, nb, db, dc, c_src, res, nxt, a_buf) -> Optional[Launch]:
        """The fused stage-boundary launch (cpa) into block ``nb`` of the next stage, or None.  x_sub = 2 when ``nb`` reads the
        pooled trunk only through a 1x1x1 projection shortcut of stride (1,2,2) (and its a conv, which runs inside the launch)."""
        b1 = nb.branch1
        if nb.a.pool_after_bn is not None or dc[0] % 2 or b1 is None:
            return None                    # (an identity shortcut would need the whole trunk AND block 0's residual add: not this launch)
        sub = 2 if (b1.pool_after_bn is None and tuple(b1.kernel) == (1, 1, 1) and tuple(b1.stride) == (1, 2, 2)
                    and tuple(b1.pad) == (0, 0, 0) and dc[1] % 2 == 0 and dc[2] % 2 == 0) else 1
        dp = (dc[0] // 2,) + tuple(dc[1:])
        return self.ask(self.make("cpa", [("c", c, db, dc, 1), ("a_next", nb.a, dp, nb.a.out_dims(*dp))],
                                  src=c_src, res=res, dst=nxt, dst_a=a_buf, x_sub=sub))


def _plan_i3d(plan: _Plan, spec: NetSpec, T, H, W, has_rgb3):
    plan.inputs = [("IN", (T, H, W), 1)]                       # (stem-input buffer, dims, temporal stride)
    cur, nxt = "P0", "P1"
    d = spec.stem.out_dims(T, H, W)
    d2 = _pool_out(d, spec.stem_pool)
    fuse_stem_pool = (plan.dtype != "f32" and d[2] <= 128 and spec.stem.cout == 64 and
                      _is_pool(spec.stem_pool, (1, 3, 3), (1, 2, 2), (0, 1, 1)))
    plan.rgb3 = bool(fuse_stem_pool and spec.stem.conv in has_rgb3)
    if fuse_stem_pool:        # conv + BN + ReLU + max-pool in one launch; the conv output never reaches HBM
        plan.conv(spec.stem, (T, H, W), d, "IN", cur, kind="stem3_pool" if plan.rgb3 else "stem_pool"); plan.need(cur, d2, spec.stem.cout)
    else:
        plan.conv(spec.stem, (T, H, W), d, "IN", cur, kind="stem"); plan.need(cur, d, spec.stem.cout)
        plan.pool("pool", spec.stem_pool, spec.stem.cout, d, d2, cur, dst=nxt); plan.need(nxt, d2, spec.stem.cout)
        cur, nxt = nxt, cur
    d = d2
    fuse_tpool = _is_pool(spec.pool_after_s2, (2, 1, 1), (2, 1, 1), (0, 0, 0))
    c = spec.stem.cout
    for si, stage in enumerate(spec.stages):
        d, c, cur, nxt, tpooled = plan.stage(stage, d, cur, nxt, "A", "B", tpool_last=(fuse_tpool and si == 0),
                                             next_stage=spec.stages[1] if (si == 0 and len(spec.stages) > 1) else None)
        if si == 0 and not tpooled:
            # pathway0_pool as its own launch (odd frame counts / other pool shapes)
            d2 = _pool_out(d, spec.pool_after_s2)
            plan.pool("pool", spec.pool_after_s2, c, d, d2, cur, dst=nxt); plan.need(nxt, d2, c)
            cur, nxt = nxt, cur
            d = d2
    hp = tuple(spec.head_pool)
    dh = tuple(di - k + 1 for di, k in zip(d, hp))
    if min(dh) < 1:
        raise ValueError("input %s too small for the head pool %s" % ((T, H, W), hp))
    plan.head_dims, plan.head_width = dh, c
    plan.pool("head", hp, c, d, dh, cur)


def _plan_ftcn(plan: _Plan, spec: FtcnTTSpec, T, H, W, has_rgb3):
    """FTCN-TT (reference i3d_temporal_var_fix_dropout_tt_cfg.py:290-359): temporal stem, s2..s4 with every spatial
    kernel 1x1, per-frame average-pooled tokens, one pre-norm transformer layer, LayerNorm + Linear on the class
    token (time_transformer.py:268-281)."""
    plan.inputs = [("IN", (T, H, W), 1)]
    cur, nxt = "P0", "P1"
    d = _pool_out(spec.stem.out_dims(T, H, W), spec.stem.pool_after_bn)
    d2 = _pool_out(d, spec.stem_pool)
    if (plan.dtype != "f32" and plan.switch["AF_FUSE_TSTEM_POOL"]
            and _is_pool(spec.stem_pool, (1, 3, 3), (1, 2, 2), (0, 1, 1))):
        # 16-bit: the stem's own 1x3x3 / stride-2 max-pool rides behind the temporal stem (the half-resolution tensor -
        # 822 MB at 16 clips - is neither written nor read back)
        plan.conv(spec.stem, (T, H, W), d, "IN", cur, kind="tstem_pool3"); plan.need(cur, d2, spec.stem.cout)
        d = d2
    else:
        plan.conv(spec.stem, (T, H, W), d, "IN", cur, kind="tstem"); plan.need(cur, d, spec.stem.cout)
        plan.pool("pool", spec.stem_pool, spec.stem.cout, d, d2, cur, dst=nxt); plan.need(nxt, d2, spec.stem.cout)
        cur, nxt, d = nxt, cur, d2
    fuse_tpool = _is_pool(spec.pool_after_s2, (2, 1, 1), (2, 1, 1), (0, 0, 0))
    c = spec.stem.cout
    for si, stage in enumerate(spec.stages):
        d, c, cur, nxt, tpooled = plan.stage(stage, d, cur, nxt, "A", "B", tpool_last=(fuse_tpool and si == 0))
        if si == 0 and not tpooled:
            dp = _pool_out(d, spec.pool_after_s2)
            plan.pool("pool", spec.pool_after_s2, c, d, dp, cur, dst=nxt); plan.need(nxt, dp, c)
            cur, nxt, d = nxt, cur, dp
    # TransformerHead 'time' patches (:133-135): AvgPool3d((1, S, S)) sized from the crop, one token per frame
    if tuple(d[1:]) != tuple(spec.token_pool[1:]) or d[0] != spec.tokens or c != spec.dim:
        raise ValueError("FTCN-TT head expects a (%d,%d,%d)x%d feature map, got %s x %d"
                         % (spec.tokens, spec.token_pool[1], spec.token_pool[2], spec.dim, d, c))
    plan.head_dims, plan.head_width = (1, 1, 1), spec.dim
    plan.pool("tt_head", spec.token_pool, c, d, (d[0], 1, 1), cur)           # its first op: one token per frame


def _plan_slowfast(plan: _Plan, spec: SlowFastSpec, T, H, W, has_rgb3):
    if T % spec.alpha:
        raise ValueError("SlowFast needs a frame count divisible by alpha=%d (got %d)" % (spec.alpha, T))
    Ts = T // spec.alpha
    plan.inputs = [("IN_S", (Ts, H, W), spec.alpha), ("IN_F", (T, H, W), 1)]
    fuse_w = [f.cout for f in spec.fuses]                         # channels each lateral adds to the Slow tensor
    # stems (+ max-pool); the Slow pool writes at the widened row stride so the lateral can append its channels
    ds = spec.stems[0].out_dims(Ts, H, W); ds2 = _pool_out(ds, spec.stem_pool)
    df = spec.stems[1].out_dims(T, H, W); df2 = _pool_out(df, spec.stem_pool)
    ld0 = spec.stems[0].cout + fuse_w[0]
    if (spec.stems[0].conv in has_rgb3 and plan.switch["AF_SLOWFAST_STEM3"]
            and _is_pool(spec.stem_pool, (1, 3, 3), (1, 2, 2), (0, 1, 1)) and ds[2] <= 128):
        # 16-bit: the Slow stem + its max-pool as the K-packed fused stem (3-channel input layout), pooled rows at the widened stride
        plan.rgb3_inputs.add("IN_S")
        plan.conv(spec.stems[0], (Ts, H, W), ds, "IN_S", "S0", kind="stem3_pool", ld=ld0)
        plan.need("S1", ds2, spec.stems[0].cout)
    else:
        plan.conv(spec.stems[0], (Ts, H, W), ds, "IN_S", "S1", kind="stem"); plan.need("S1", ds, spec.stems[0].cout)
        plan.pool("pool", spec.stem_pool, spec.stems[0].cout, ds, ds2, "S1", dst="S0", ld=ld0)
    plan.need("S0", ds2, ld0)
    plan.conv(spec.stems[1], (T, H, W), df, "IN_F", "F1", kind="stem"); plan.need("F1", df, spec.stems[1].cout)
    plan.pool("pool", spec.stem_pool, spec.stems[1].cout, df, df2, "F1", dst="F0")
    plan.need("F0", df2, spec.stems[1].cout)
    scur, snxt, fcur, fnxt = "S0", "S1", "F0", "F1"
    ds, df, cs = ds2, df2, spec.stems[0].cout

    def lateral(fz: ConvSpec, dfast, fbuf, sbuf, c_slow, ld):
        do = fz.out_dims(*dfast)                                   # FuseFastToSlow: conv + BN + ReLU into the Slow rows
        plan.conv(fz, dfast, do, fbuf, sbuf, ld=ld, ch_off=c_slow)
        return do

    if lateral(spec.fuses[0], df, fcur, scur, cs, ld0) != ds:
        raise ValueError("the Fast->Slow lateral does not land on the Slow grid")
    cf = spec.stems[1].cout
    for si, (slow, fast) in enumerate(spec.stages):
        has_fuse = si + 1 < len(spec.fuses)
        ld = slow.blocks[-1].c.cout + (fuse_w[si + 1] if has_fuse else 0)
        ds, cs, scur, snxt, _ = plan.stage(slow, ds, scur, snxt, "A_S", "B_S", last_ld=ld)
        df, cf, fcur, fnxt, _ = plan.stage(fast, df, fcur, fnxt, "A_F", "B_F")
        if has_fuse and lateral(spec.fuses[si + 1], df, fcur, scur, cs, ld) != ds:
            raise ValueError("the Fast->Slow lateral does not land on the Slow grid")
    hs, hf = (tuple(p) for p in spec.head_pools)
    dhs = tuple(di - k + 1 for di, k in zip(ds, hs))
    dhf = tuple(di - k + 1 for di, k in zip(df, hf))
    if min(dhs) < 1 or dhs != dhf:
        raise ValueError("input %s does not fit the SlowFast head pools %s / %s" % ((T, H, W), hs, hf))
    plan.head_dims, plan.head_width = dhs, cs + cf
    plan.pool("avgpool", hs, cs, ds, dhs, scur, ch_off=0)
    plan.pool("avgpool", hf, cf, df, dhf, fcur, ch_off=cs)
    plan.launches.append(Launch("linear"))


def plan_network(spec, dtype: str, batch: int, dims, has_rgb3=()) -> _Plan:
    """The launch plan of one (network, dtype, batch, input dims); needs no device.  ``has_rgb3``: the stem convs whose weights
    also exist as the K-packed image of the fused 16-bit stem (PackedWeights.w3)."""
    plan = _Plan(batch, dtype)
    planner = _plan_slowfast if isinstance(spec, SlowFastSpec) else _plan_ftcn if isinstance(spec, FtcnTTSpec) else _plan_i3d
    planner(plan, spec, *dims, has_rgb3)
    return plan


class Engine:
    """Op list + activation buffers for one (batch, dtype).  ``run_*`` enqueue the whole forward on
    the current torch stream and return the engine-owned logits / pooled-feature tensors."""

    def __init__(self, spec, weights: PackedWeights, batch: int, device, dims=None):
        self.spec, self.weights, self.batch, self.device = spec, weights, batch, device
        self.dtype = weights.dtype
        self.code = _lib.DTYPE_CODES[self.dtype]
        self.in_dims = tuple(dims or (spec.num_frames, spec.crop, spec.crop))
        plan = plan_network(spec, self.dtype, batch, self.in_dims, weights.w3)
        self.inputs, self.rgb3, self.head_dims, self.head_width = plan.inputs, plan.rgb3, plan.head_dims, plan.head_width
        self._materialise(plan)

    # -- buffers + op list ------------------------------------------------------------------------------
    def _materialise(self, plan: _Plan):
        batch, device, spec = self.batch, self.device, self.spec
        tdt = _TORCH_DTYPE[self.dtype]
        es = _ELEM_SIZE[self.dtype]
        self.buf = {k: torch.empty(max(v, 8), dtype=tdt, device=device) for k, v in plan.sizes.items()}
        # inputs that feed a K-packed stem take the 3-channel layout (the single input of the i3d engine; SlowFast: the Slow one)
        r3 = plan.rgb3_inputs | ({self.inputs[0][0]} if self.rgb3 else set())
        self.k_pack_f32 = [_lib.AF_OP_PACK3_F32 if name in r3 else _lib.AF_OP_PACK_F32 for name, _, _ in self.inputs]
        # a uint8 run: the one input's pack op, or (SlowFast) one launch that writes both inputs in slot 0 and nothing in slot 1
        self.k_pack_u8 = ([_lib.AF_OP_PACK3_U8 if self.rgb3 else _lib.AF_OP_PACK_U8] if len(self.inputs) == 1
                          else [_lib.AF_OP_PACK_PATHWAYS_U8, _lib.AF_OP_NOP])
        for name, dims, _ in self.inputs:                           # padded stem inputs: halos stay zero forever
            nbytes = (lib.af_stem_input_bytes_rgb3 if name in r3 else lib.af_stem_input_bytes)(batch, dims[0], dims[1], dims[2], self.code)
            self.buf[name] = torch.zeros(nbytes // es, dtype=tdt, device=device)
        self.head_positions = self.head_dims[0] * self.head_dims[1] * self.head_dims[2]
        self.pooled = torch.empty((batch, self.head_positions, self.head_width), dtype=torch.float32, device=device)
        self.logits = torch.empty((batch, self.head_positions * spec.num_classes), dtype=torch.float32, device=device)
        # the callers' score epilogue (sigmoid / softmax[:,1], test/af_realtime.py:88-95) rides behind the head's Linear
        self.scores = (torch.empty((batch, self.head_positions), dtype=torch.float32, device=device)
                       if spec.num_classes in (1, 2) else None)

        n_pack = len(self.inputs)
        self.launches = plan.launches        # launch k is ops[n_pack + k] (a tt_head launch: TT_HEAD_OPS ops from there)
        self.n_ops = n_pack + len(plan.launches) + (self.TT_HEAD_OPS - 1 if isinstance(spec, FtcnTTSpec) else 0)
        self.ops = (Op * self.n_ops)()
        self.op_names: List[str] = []
        self.op_macs: List[int] = []
        self.op_dst: List[Optional[str]] = [name for name, _, _ in self.inputs] + [launch.dst for launch in plan.launches]
        for i, (name, dims, _) in enumerate(self.inputs):
            pk = self.ops[i]
            pk.kind, pk.tag = self.k_pack_f32[i], TAG_PACK
            pk.conv.n, (pk.conv.t, pk.conv.h, pk.conv.w), pk.conv.dtype = batch, dims, self.code
            pk.out = self.buf[name].data_ptr()
            self.op_names.append("input_pack" if n_pack == 1 else "input_pack_" + name)
            self.op_macs.append(0)
        if n_pack == 2:                      # what PACK_PATHWAYS_U8 reads besides the pack fields; the fp32 pack ops ignore them
            pk = self.ops[0]
            pk.aux, pk.x_sub = self.buf[self.inputs[1][0]].data_ptr(), self.inputs[0][2]
            pk.pack_rgb3 = sum(1 << i for i, (name, _, _) in enumerate(self.inputs) if name in r3)
        for k, launch in enumerate(plan.launches):
            op = self.ops[n_pack + k]
            op.in_, op.residual, op.aux = self._at(launch.src), self._at(launch.res), self._at(launch.dst_a)
            op.out_ld, op.x_sub = launch.ld, launch.x_sub
            if launch.pool is not None:
                op.pool = launch.pool
            if launch.dst:
                op.out = self._at(launch.dst) + launch.ch_off * es
            if launch.kind == "tt_head":
                self._materialise_tt_head(n_pack + k, launch)
                continue
            name, macs = self._EMIT[launch.kind](self, op, launch)
            self.op_names.append(name)
            self.op_macs.append(batch * macs)
        # split-K scratch (small batches, long-K layers): sized by the library, owned by this engine (one per engine =
        # one per device and per stream of work, since an engine enqueues its forward on one stream); consecutive
        # launches of one forward reuse it in stream order
        need = 0
        for i in range(self.n_ops):
            if self.ops[i].kind == _lib.AF_OP_CONV:
                need = max(need, int(lib.af_conv_workspace_bytes(C.byref(self.ops[i].conv))))
        self.workspace = torch.empty(need // 4, dtype=torch.float32, device=device) if need else None
        for i in range(self.n_ops):
            if self.ops[i].kind == _lib.AF_OP_CONV and need:
                self.ops[i].workspace = self.workspace.data_ptr()
                self.ops[i].workspace_bytes = need

    # One function per launch kind: fills ``op`` (in_, out, residual, aux, out_ld, x_sub and pool are already bound) and returns (op
    # name, MACs per clip).  The descriptors are the launch's own, copied: what the library's *_fusable predicate was asked with.
    def _at(self, buf: Optional[str]):
        return self.buf[buf].data_ptr() if buf else None

    _CONV_KINDS = {"stem": _lib.AF_OP_STEM, "stem_pool": _lib.AF_OP_STEM_POOL, "stem3_pool": _lib.AF_OP_STEM3_POOL,
                   "tstem": _lib.AF_OP_TSTEM, "tstem_pool3": _lib.AF_OP_TSTEM_POOL3, "conv": _lib.AF_OP_CONV}

    def _emit_conv(self, op, launch):
        cv = launch.convs["conv"]
        op.kind, op.tag = self._CONV_KINDS[launch.kind], TAG_STEM if launch.kind != "conv" else _conv_tag(cv)
        op.conv, = launch.descs
        op.weight, op.scale, op.shift = self.weights.bn(cv)
        if launch.kind == "stem3_pool":
            op.weight = self.weights.w3[cv.conv].data_ptr()
        return cv.conv, launch.macs()

    def _emit_ca(self, op, launch):
        cvc, cv1, cva = launch.convs.values()
        op.kind, op.tag = _lib.AF_OP_CONV_CA, TAG_CONV_CA
        op.conv, d1, op.conv2 = launch.descs
        op.weight2, op.scale2, op.shift2 = self.weights.bn(cva)
        if cv1 is not None:                          # projection block: no residual tensor
            op.conv3 = d1
            op.weight, op.weight3, op.scale, op.shift = self.weights.folded(cvc, cv1)
            op.in3 = self._at(launch.src2)
        else:
            op.weight, op.scale, op.shift = self.weights.bn(cvc)
        return cvc.conv + ("+branch1" if cv1 is not None else "") + "->" + cva.conv.split("resnet.")[-1], launch.macs()

    def _emit_cpa(self, op, launch):
        cvc, cva = launch.convs.values()
        op.kind, op.tag = _lib.AF_OP_CONV_CPA, TAG_CONV_CA
        op.conv, op.conv2 = launch.descs
        op.weight, op.scale, op.shift = self.weights.bn(cvc)
        op.weight2, op.scale2, op.shift2 = self.weights.bn(cva)
        return cvc.conv + "+pool->" + cva.conv.split("resnet.")[-1], launch.macs()

    def _emit_abc(self, op, launch):
        cva, cvb, cvc, cv1 = launch.convs.values()
        op.kind, op.tag = _lib.AF_OP_BLOCK_ABC, TAG_BLOCK_ABC
        op.conv, op.conv2, op.conv3, d1 = launch.descs
        op.weight, op.scale, op.shift = self.weights.bn(cva)
        op.weight2, op.scale2, op.shift2 = self.weights.bn(cvb)
        if cv1 is not None:                          # projection block
            op.conv4 = d1
            op.weight3, op.weight4, op.scale3, op.shift3 = self.weights.folded(cvc, cv1)
        else:
            op.weight3, op.scale3, op.shift3 = self.weights.bn(cvc)
        return cva.conv.rsplit(".", 1)[0] + ".a+b+c" + ("+branch1" if cv1 is not None else ""), launch.macs()

    def _emit_bc(self, op, launch):
        cvb, cvc = launch.convs.values()
        op.kind, op.tag = _lib.AF_OP_CONV_BC, TAG_CONV_BC
        op.conv, op.conv2 = launch.descs
        op.weight, op.scale, op.shift = self.weights.bn(cvb)
        op.weight2, op.scale2, op.shift2 = self.weights.bn(cvc)
        return cvb.conv + "+c", launch.macs()

    def _emit_dual(self, op, launch):
        cvc, cv1 = launch.convs.values()
        op.kind, op.tag = _lib.AF_OP_CONV_DUAL, _conv_tag(cvc)
        op.conv, op.conv2 = launch.descs
        op.weight, op.weight2, op.scale, op.shift = self.weights.folded(cvc, cv1)
        op.in2 = self._at(launch.src2)
        return cvc.conv + "+branch1", launch.macs()

    def _emit_pool(self, op, launch):
        op.kind, op.tag = _lib.AF_OP_MAXPOOL, TAG_POOL
        return "maxpool_%dx%dx%d" % (op.pool.kt, op.pool.kh, op.pool.kw), 0

    def _bind_fc(self, op):
        """the head's Linear (+ the score epilogue) into ``logits`` / ``scores``"""
        op.tag = TAG_HEAD
        op.weight, op.scale = self.weights.fc_w.data_ptr(), self.weights.fc_b.data_ptr()
        op.num_classes = self.spec.num_classes
        op.out = self.logits.data_ptr()
        op.scores = self.scores.data_ptr() if self.scores is not None else None

    def _emit_head(self, op, launch):
        op.kind = _lib.AF_OP_HEAD
        op.aux = self.pooled.data_ptr()
        self._bind_fc(op)
        return "head", 0

    def _emit_linear(self, op, launch):
        op.kind = _lib.AF_OP_LINEAR
        op.in_ = self.pooled.data_ptr()
        op.pool.n, op.pool.c = self.batch * self.head_positions, self.head_width
        self._bind_fc(op)
        return "head_linear", 0

    def _emit_avgpool(self, op, launch):
        op.kind, op.tag = _lib.AF_OP_AVGPOOL, TAG_HEAD
        op.out = self.pooled.data_ptr() + launch.ch_off * 4
        op.out_ld = self.head_width
        return "head_avgpool_%d" % launch.ch_off, 0

    _EMIT = {"stem": _emit_conv, "stem_pool": _emit_conv, "stem3_pool": _emit_conv, "tstem": _emit_conv, "tstem_pool3": _emit_conv,
             "conv": _emit_conv, "ca": _emit_ca, "cpa": _emit_cpa, "abc": _emit_abc, "bc": _emit_bc, "dual": _emit_dual,
             "pool": _emit_pool, "head": _emit_head, "avgpool": _emit_avgpool, "linear": _emit_linear}

    TT_HEAD_OPS = 12

    def _materialise_tt_head(self, first: int, launch):
        """The FTCN-TT head as TT_HEAD_OPS ops starting at ops[first] (fp32 buffers of its own)."""
        spec, w, batch, dev = self.spec, self.weights, self.batch, self.device
        n1, dim, inner = spec.tokens + 1, spec.dim, spec.heads * spec.dim_head
        rows = batch * n1
        fb = lambda *shape: torch.empty(shape, dtype=torch.float32, device=dev)
        self.tokens_pooled = fb(batch, spec.tokens, dim)
        self.fbuf = {"x": fb(rows, dim), "h": fb(rows, dim), "qkv": fb(rows, 3 * inner), "att": fb(rows, inner),
                     "x2": fb(rows, dim), "ff": fb(rows, spec.mlp_dim), "x3": fb(rows, dim)}
        i = [first]

        def nxt(name, tag=TAG_HEAD, macs=0):
            op = self.ops[i[0]]
            i[0] += 1
            op.tag = tag
            self.op_names.append("tt_head." + name)
            self.op_macs.append(macs)
            if len(self.op_dst) < len(self.op_names):
                self.op_dst.append(None)
            return op

        def linear(name, key, src, dst, res=None):
            packed, ones, bias, cin, cout = w.lin[key]
            op = nxt(name, TAG_CONV_1x1x1, rows * cin * cout)
            op.kind = _lib.AF_OP_CONV
            op.conv = _lib.conv_desc(1, (1, 1, rows), cin, cout, (1, 1, 1), (1, 1, 1), (0, 0, 0), False, _lib.AF_F32)
            op.in_, op.out = self.fbuf[src].data_ptr(), self.fbuf[dst].data_ptr()
            op.weight, op.scale, op.shift = packed.data_ptr(), ones.data_ptr(), bias.data_ptr()
            op.residual = self.fbuf[res].data_ptr() if res else None
            op.out_ld = cout

        def layernorm(name, key, src, dst, n_rows, x_stride, y_stride):
            op = nxt(name)
            op.kind = _lib.AF_OP_LAYERNORM
            op.in_, op.out = src.data_ptr(), dst.data_ptr()
            op.scale, op.shift = w.ln[key][0].data_ptr(), w.ln[key][1].data_ptr()
            op.pool.n, op.pool.c, op.pool.h, op.pool.w = n_rows, dim, x_stride, y_stride

        op = nxt("avgpool_tokens")                                         # (B, T/2, dim) per-frame tokens
        op.kind = _lib.AF_OP_AVGPOOL
        op.in_, op.out, op.out_ld = self.buf[launch.src].data_ptr(), self.tokens_pooled.data_ptr(), dim
        op = nxt("tokens")                                                 # class token + position embedding
        op.kind = _lib.AF_OP_TOKENS
        op.in_, op.weight, op.scale = self.tokens_pooled.data_ptr(), w.cls_token.data_ptr(), w.pos_embedding.data_ptr()
        op.pool.n, op.pool.t, op.pool.c = batch, spec.tokens, dim
        op.out = self.fbuf["x"].data_ptr()
        layernorm("attn_norm", "attn", self.fbuf["x"], self.fbuf["h"], rows, dim, dim)
        linear("to_qkv", "qkv", "h", "qkv")
        op = nxt("attention")
        op.kind = _lib.AF_OP_ATTENTION
        op.in_, op.out = self.fbuf["qkv"].data_ptr(), self.fbuf["att"].data_ptr()
        op.pool.n, op.pool.t, op.pool.h, op.pool.w = batch, n1, spec.heads, spec.dim_head
        linear("to_out", "out", "att", "x2", res="x")                      # Residual(PreNorm(Attention))
        layernorm("ff_norm", "ff", self.fbuf["x2"], self.fbuf["h"], rows, dim, dim)
        linear("ff1", "ff1", "h", "ff")
        op = nxt("gelu")
        op.kind = _lib.AF_OP_GELU
        op.out = self.fbuf["ff"].data_ptr()
        op.pool.n, op.pool.c = rows, spec.mlp_dim
        linear("ff2", "ff2", "ff", "x3", res="x2")                         # Residual(PreNorm(FeedForward))
        # mlp_head on the class token (row 0 of every clip): LayerNorm -> Linear; `pooled` = the Linear's input
        layernorm("head_norm", "head", self.fbuf["x3"], self.pooled, batch, n1 * dim, dim)
        op = nxt("head_linear")
        op.kind = _lib.AF_OP_LINEAR
        op.in_ = self.pooled.data_ptr()
        op.pool.n, op.pool.c = batch, dim
        self._bind_fc(op)
        assert i[0] - first == self.TT_HEAD_OPS

    # -- input binding -------------------------------------------------------------------------------------
    def _bind_f32(self, i: int, x: torch.Tensor, tstride: int = 1):
        """Binds network input i to x.  ``tstride`` > 1 takes every tstride-th frame of x (the Slow pathway of a
        single-clip SlowFast call): only the element stride handed to the pack kernel changes, nothing is copied."""
        name, dims, _ = self.inputs[i]
        B, Cc, T, H, W = x.shape
        if (B, Cc, H, W) != (self.batch, 3, dims[1], dims[2]) or T != dims[0] * tstride:
            raise ValueError("expected input (%d,3,%d,%d,%d), got %s"
                             % (self.batch, dims[0] * tstride, dims[1], dims[2], tuple(x.shape)))
        if x.dtype != torch.float32 or not x.is_cuda:
            raise ValueError("inputs must be fp32 HIP tensors")
        pk = self.ops[i]
        pk.kind = self.k_pack_f32[i]
        (pk.conv.t, pk.conv.h, pk.conv.w) = dims
        pk.in_ = x.data_ptr()
        st = list(x.stride())
        st[2] *= tstride
        for k, s in enumerate(st):
            pk.in_strides[k] = s

    def run_f32(self, *xs: torch.Tensor):
        """One (B,3,T,H,W) fp32 device tensor per network input, any strides (the callers' normalised clip; SlowFast:
        slow, fast).  A single tensor given to a two-input network is split by frame striding."""
        if len(xs) == 1 and len(self.inputs) > 1:
            for i, (_, _, ts) in enumerate(self.inputs):
                self._bind_f32(i, xs[0], ts)
        else:
            if len(xs) != len(self.inputs):
                raise ValueError("network takes %d inputs, got %d" % (len(self.inputs), len(xs)))
            for i, x in enumerate(xs):
                self._bind_f32(i, x)
        check(lib.af_run_ops(self.ops, self.n_ops, _stream_ptr(self.device)), "af_run_ops")
        return self.logits, self.pooled

    def run_u8(self, clips: torch.Tensor, mean, std):
        """clips: (B,T,H,W,3) uint8 device tensor in caller layout; normalisation fused into the prologue.  SlowFast: one
        full-rate clip; the Slow input is every alpha-th frame of it, written by the same launch as the Fast input."""
        assert clips.dtype == torch.uint8 and clips.is_cuda
        B, T, H, W, Cc = clips.shape
        if (B, T, H, W, Cc) != (self.batch,) + self.in_dims + (3,) or not clips.is_contiguous():
            raise ValueError("expected contiguous uint8 clips (%d,%d,%d,%d,3)" % ((self.batch,) + self.in_dims))
        for i, kind in enumerate(self.k_pack_u8):
            self.ops[i].kind = kind
        pk = self.ops[0]
        pk.in_ = clips.data_ptr()
        (pk.conv.t, pk.conv.h, pk.conv.w) = self.in_dims          # SlowFast: slot 0 describes the Slow input in an fp32 run
        for i in range(3):
            pk.mean[i], pk.std_[i] = float(mean[i]), float(std[i])
        check(lib.af_run_ops(self.ops, self.n_ops, _stream_ptr(self.device)), "af_run_ops")
        return self.logits, self.pooled

    def run_prefix(self, n_ops: int):
        """Runs ops[0:n_ops] of the currently bound forward (tests read intermediate activations)."""
        check(lib.af_run_ops(self.ops, n_ops, _stream_ptr(self.device)), "af_run_ops")

    def run_ops(self, first: int, count: int):
        """Runs ops[first:first + count] of the currently bound forward (tests step a forward launch by launch)."""
        assert 0 <= first and count >= 1 and first + count <= self.n_ops, (first, count, self.n_ops)
        ops = C.cast(C.addressof(self.ops) + first * C.sizeof(Op), C.POINTER(Op))
        check(lib.af_run_ops(ops, count, _stream_ptr(self.device)), "af_run_ops")

    def run_timed(self, first_op: int = 0):
        """Re-runs the currently bound forward with hipEvents around every op; returns ms per op."""
        ms = (C.c_float * self.n_ops)()
        n = self.n_ops - first_op
        ops = C.cast(C.addressof(self.ops) + first_op * C.sizeof(Op), C.POINTER(Op))
        msp = C.cast(C.addressof(ms) + first_op * C.sizeof(C.c_float), C.POINTER(C.c_float))
        check(lib.af_run_ops_timed(ops, n, _stream_ptr(self.device), msp), "af_run_ops_timed")
        return [float(v) for v in ms]

    def activation(self, op_index: int) -> torch.Tensor:
        """Output of op ``op_index`` as an (N,T,H,W,C) view of its buffer (valid until overwritten; ops that write
        into a wider, concatenated row return the full-width rows)."""
        op = self.ops[op_index]
        if op.kind in (_lib.AF_OP_STEM_POOL, _lib.AF_OP_STEM3_POOL, _lib.AF_OP_TSTEM_POOL3):
            shape = (op.conv.n, op.conv.to, (op.conv.ho - 1) // 2 + 1, (op.conv.wo - 1) // 2 + 1, op.out_ld or op.conv.cout)
        elif op.kind == _lib.AF_OP_CONV_BC:
            shape = (op.conv2.n, op.conv2.to, op.conv2.ho, op.conv2.wo, op.out_ld or op.conv2.cout)
        elif op.kind == _lib.AF_OP_BLOCK_ABC:
            shape = (op.conv3.n, op.conv3.to, op.conv3.ho, op.conv3.wo, op.out_ld or op.conv3.cout)
        elif op.kind == _lib.AF_OP_CONV_CPA:       # the pooled trunk, or (x_sub == 2) its even (h, w) positions
            shape = (op.conv.n, op.conv.to // 2, op.conv.ho // op.x_sub, op.conv.wo // op.x_sub, op.conv.cout)
        elif op.kind == _lib.AF_OP_CONV_CA:        # the trunk
            shape = (op.conv.n, op.conv.to, op.conv.ho, op.conv.wo, op.conv.cout)
        elif op.kind in (_lib.AF_OP_STEM, _lib.AF_OP_CONV, _lib.AF_OP_CONV_DUAL, _lib.AF_OP_TSTEM):
            ld = op.out_ld or op.conv.cout
            q = 2 if op.conv.tpool == 2 else 1
            shape = (op.conv.n, op.conv.to // 2 if op.conv.tpool == 1 else op.conv.to, op.conv.ho // q, op.conv.wo // q, ld)
        elif op.kind == _lib.AF_OP_MAXPOOL:
            shape = (op.pool.n, op.pool.to, op.pool.ho, op.pool.wo, op.pool.out_ld or op.pool.c)
        else:
            raise ValueError("op %d has no NDHWC output" % op_index)
        numel = 1
        for s in shape:
            numel *= s
        return self.buf[self.op_dst[op_index]][:numel].view(shape)      # rows from channel 0 of the destination buffer
