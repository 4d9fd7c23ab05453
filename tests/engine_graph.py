"""The dataflow of the three networks as plain data, stated apart from the planner: an ordered list of named tensors with their
producer, the names they read, their dims (t, h, w) and channel count for given input dims.  Derived from arch.py alone (NetSpec,
SlowFastSpec, FtcnTTSpec) along the structure of the CPU oracle (oracle/i3d_oracle.py: forward, ftcn_forward, slowfast_forward);
engine.py is not imported.  test_plan_dataflow_host.py holds every launch plan to this graph, test_hip_engine_replay.py computes
each launch's fp64 reference from tensors looked up here by name.

Names:
  "input" (SlowFast: "input_slow", "input_fast")    the normalised clip(s)
  <conv prefix>         a conv's output after BN, pool_after_bn and ReLU ("resnet.s2.pathway0_res0.branch2.a"); a c conv's is
                        BN(conv) alone, before the block's add, and the projection shortcut's has no ReLU
  "stem_pool" (SlowFast: "stem_pool0", "stem_pool1")   the 1x3x3 / stride-2 max-pool behind a stem
  <block name>          relu(shortcut + c)             ("resnet.s2.pathway0_res0")
  "pool_after_s2"       the temporal max-pool behind s2 (I3D, FTCN-TT)
  <fuse prefix>         the Slow rows after a lateral: [stage output | lateral channels]   ("resnet.s1_fuse")
  "pooled"              the head's pooled features (SlowFast: [slow | fast])
  "tokens"              FTCN-TT's per-frame tokens
  "logits"
"""
import dataclasses
from typing import Optional, Tuple

from af_mi355x.arch import ConvSpec, FtcnTTSpec, PoolSpec, SlowFastSpec


@dataclasses.dataclass(frozen=True)
class Node:
    name: str
    op: str                        # input | conv | pool | add | concat | avgpool | tokens | linear | transformer
    reads: Tuple[str, ...]         # add: (shortcut, c); concat: the parts in channel order
    dims: Tuple[int, int, int]
    ch: int
    conv: Optional[ConvSpec] = None        # op == "conv"
    pool: Optional[PoolSpec] = None        # op == "pool"; avgpool / tokens: the window, stride 1


class Graph:
    def __init__(self):
        self.nodes = {}                    # name -> Node, in order

    def add(self, name, op, reads, dims, ch, **kw):
        assert name not in self.nodes, name
        assert all(r in self.nodes for r in reads), (name, reads)
        self.nodes[name] = Node(name, op, tuple(reads), tuple(dims), ch, **kw)
        return name

    def __getitem__(self, name):
        return self.nodes[name]

    def consumers(self):
        """name -> the names that read it, in graph order"""
        out = {name: [] for name in self.nodes}
        for node in self.nodes.values():
            for r in node.reads:
                out[r].append(node.name)
        return out

    # -- building blocks -------------------------------------------------------------------------------
    def conv(self, cv: ConvSpec, src):
        x = self[src]
        assert x.ch == cv.cin, (cv.conv, x.ch, cv.cin)
        d = cv.out_dims(*x.dims)
        if cv.pool_after_bn is not None:
            d = pool_dims(d, cv.pool_after_bn)
        return self.add(cv.conv, "conv", [src], d, cv.cout, conv=cv)

    def maxpool(self, name, p: PoolSpec, src):
        x = self[src]
        return self.add(name, "pool", [src], pool_dims(x.dims, p), x.ch, pool=p)

    def block(self, blk, src):
        """ResBlock (oracle.res_block / ftcn_block): relu(shortcut(x) + c_bn(c(b(a(x)))))"""
        sc = self.conv(blk.branch1, src) if blk.branch1 is not None else src
        c = self.conv(blk.c, self.conv(blk.b, self.conv(blk.a, src)))
        assert self[sc].dims == self[c].dims and self[sc].ch == self[c].ch, blk.name
        return self.add(blk.name, "add", [sc, c], self[c].dims, self[c].ch)

    def stage(self, stage, src):
        for blk in stage.blocks:
            src = self.block(blk, src)
        return src


def pool_dims(dims, p: PoolSpec):
    return tuple((d + 2 * pp - k) // s + 1 for d, k, s, pp in zip(dims, p.kernel, p.stride, p.pad))


def fuse_name(fz: ConvSpec):
    return fz.conv.rsplit(".", 1)[0]           # "resnet.s1_fuse.conv_f2s" -> "resnet.s1_fuse"


def build(spec, dims=None) -> Graph:
    """The graph of ``spec`` over an input of ``dims`` = (T, H, W) (default: the spec's own clip)."""
    T, H, W = dims or (spec.num_frames, spec.crop, spec.crop)
    g = Graph()
    if isinstance(spec, SlowFastSpec):
        xs = g.add("input_slow", "input", [], (T // spec.alpha, H, W), 3)
        xf = g.add("input_fast", "input", [], (T, H, W), 3)
        xs = g.maxpool("stem_pool0", spec.stem_pool, g.conv(spec.stems[0], xs))
        xf = g.maxpool("stem_pool1", spec.stem_pool, g.conv(spec.stems[1], xf))

        def fuse(fz, xs, xf):                  # oracle.fuse_fast_to_slow
            lat = g.conv(fz, xf)
            assert g[lat].dims == g[xs].dims, fz.conv
            return g.add(fuse_name(fz), "concat", [xs, lat], g[xs].dims, g[xs].ch + g[lat].ch)

        xs = fuse(spec.fuses[0], xs, xf)
        for si, (slow, fast) in enumerate(spec.stages):
            xs, xf = g.stage(slow, xs), g.stage(fast, xf)
            if si + 1 < len(spec.fuses):
                xs = fuse(spec.fuses[si + 1], xs, xf)
        ps = g.add("pooled_slow", "avgpool", [xs], tuple(d - k + 1 for d, k in zip(g[xs].dims, spec.head_pools[0])), g[xs].ch,
                   pool=PoolSpec(tuple(spec.head_pools[0]), (1, 1, 1), (0, 0, 0)))
        pf = g.add("pooled_fast", "avgpool", [xf], tuple(d - k + 1 for d, k in zip(g[xf].dims, spec.head_pools[1])), g[xf].ch,
                   pool=PoolSpec(tuple(spec.head_pools[1]), (1, 1, 1), (0, 0, 0)))
        assert g[ps].dims == g[pf].dims
        g.add("pooled", "concat", [ps, pf], g[ps].dims, g[ps].ch + g[pf].ch)
        g.add("logits", "linear", ["pooled"], g[ps].dims, spec.num_classes)
        return g
    x = g.add("input", "input", [], (T, H, W), 3)
    x = g.maxpool("stem_pool", spec.stem_pool, g.conv(spec.stem, x))
    for si, stage in enumerate(spec.stages):
        x = g.stage(stage, x)
        if si == 0:
            x = g.maxpool("pool_after_s2", spec.pool_after_s2, x)
    if isinstance(spec, FtcnTTSpec):
        d = g[x].dims
        assert tuple(d[1:]) == tuple(spec.token_pool[1:]) and d[0] == spec.tokens and g[x].ch == spec.dim, (d, g[x].ch)
        g.add("tokens", "tokens", [x], (d[0], 1, 1), spec.dim, pool=PoolSpec(tuple(spec.token_pool), (1, 1, 1), (0, 0, 0)))
        g.add("logits", "transformer", ["tokens"], (1, 1, 1), spec.num_classes)
        return g
    hp = tuple(spec.head_pool)
    g.add("pooled", "avgpool", [x], tuple(d - k + 1 for d, k in zip(g[x].dims, hp)), g[x].ch, pool=PoolSpec(hp, (1, 1, 1), (0, 0, 0)))
    g.add("logits", "linear", ["pooled"], g["pooled"].dims, spec.num_classes)
    return g
