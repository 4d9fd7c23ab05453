"""Holds a launch plan (engine.plan_network) to the network's dataflow graph (engine_graph.py).

``launch_io`` maps one launch, through the names and roles of its ConvSpecs, onto the graph tensors it computes, the ones it stores
(dst, dst_a, x_sub) and the ones it must find in memory (src, src2, res), with the dims and channels its descriptors state.
``walk`` runs the launches in order over a table "buffer -> what was written there last" and returns [(launch index, message)] for
everything that contradicts the graph: coverage, reads, writes and extents.  A plan is duck-typed here: engine.py is not imported.
"""
import dataclasses
from typing import List, Tuple

STEM_KINDS = ("stem", "stem_pool", "stem3_pool", "tstem", "tstem_pool3")
HEAD_KINDS = ("head", "avgpool", "linear", "tt_head")
PREPOOL = "@prepool"           # a conv with pool_after_bn whose pool is a launch of its own: what the conv launch stores
# which operand holds what a conv of a role (or the block's add: its shortcut) reads from memory, per launch kind
OPERANDS = {"conv": {"conv": "src", "add": "res"}, "dual": {"c": "src", "branch1": "src2"},
            "ca": {"c": "src", "branch1": "src2", "add": "res"}, "cpa": {"c": "src", "add": "res"},
            "abc": {"a": "src", "branch1": "src", "add": "src"}, "bc": {"b": "src", "add": "res"}}


class Mismatch(Exception):
    pass


@dataclasses.dataclass
class Read:
    operand: str               # src | src2 | res
    name: str                  # graph tensor
    dims: Tuple[int, int, int] # as the descriptor states them
    ch: int
    sub: int = 1               # 2: the even-(h, w) restriction


@dataclasses.dataclass
class Store:
    operand: str               # dst | dst_a | pooled | logits | tokens
    name: str
    dims: Tuple[int, int, int]
    ch: int
    ld: int
    ch_off: int = 0
    sub: int = 1


@dataclasses.dataclass
class LaunchIO:
    made: List[str]            # every graph tensor the launch computes, stored or not, in graph order
    reads: List[Read]
    stores: List[Store]


def _block_of(c_conv: str) -> str:
    assert c_conv.endswith(".branch2.c"), c_conv
    return c_conv[:-len(".branch2.c")]


def _consumer(g, cons, name, op):
    got = [c for c in cons[name] if g[c].op == op]
    if len(got) != 1:
        raise Mismatch("graph has %d %s nodes behind %s" % (len(got), op, name))
    return got[0]


def _check_conv(g, role, cv, d, lone, pooled_out):
    """the descriptor of one conv of a launch against its graph node; returns (the node read, sub).  ``lone``: a launch of its own,
    which carries the conv's own ReLU; ``pooled_out``: the descriptor's output dims are those behind pool_after_bn (tstem)"""
    if cv.conv not in g.nodes or g[cv.conv].op != "conv":
        raise Mismatch("%s: %s is no conv of the graph" % (role, cv.conv))
    node, sub = g[cv.conv], 1
    if cv != node.conv:
        # the one restatement a plan makes: a stride-(1,2,2) 1x1x1 shortcut as a stride-1 conv over the even-(h, w) restriction
        if (dataclasses.replace(cv, stride=node.conv.stride) == node.conv and tuple(node.conv.stride) == (1, 2, 2)
                and tuple(cv.stride) == (1, 1, 1) and tuple(cv.kernel) == (1, 1, 1) and tuple(cv.pad) == (0, 0, 0) and role == "branch1"):
            sub = 2
        else:
            raise Mismatch("%s: the launch's ConvSpec of %s is not the graph's" % (role, cv.conv))
    src = g[node.reads[0]]
    want_in = src.dims if sub == 1 else (src.dims[0], src.dims[1] // 2, src.dims[2] // 2)
    if sub == 2 and (src.dims[1] % 2 or src.dims[2] % 2):
        raise Mismatch("%s: even-(h, w) restriction of odd dims %s" % (role, src.dims))
    if (d.t, d.h, d.w) != tuple(want_in) or d.cin != src.ch:
        raise Mismatch("%s %s: descriptor reads %s x %d, the graph's %s is %s x %d" % (role, cv.conv, (d.t, d.h, d.w), d.cin, src.name,
                                                                                      tuple(want_in), src.ch))
    if ((d.kt, d.kh, d.kw), (d.st, d.sh, d.sw), (d.pt, d.ph, d.pw)) != (tuple(cv.kernel), tuple(cv.stride), tuple(cv.pad)):
        raise Mismatch("%s %s: kernel / stride / pad of the descriptor differ from the ConvSpec" % (role, cv.conv))
    out = cv.out_dims(d.t, d.h, d.w)
    if pooled_out:
        p = cv.pool_after_bn
        out = tuple((x + 2 * pp - k) // s + 1 for x, k, s, pp in zip(out, p.kernel, p.stride, p.pad))
    if d.relu != int(not lone or cv.relu or cv.final_bn):
        raise Mismatch("%s %s: relu = %d in the descriptor" % (role, cv.conv, d.relu))
    if (d.to, d.ho, d.wo) != out or d.cout != node.ch or d.n <= 0:
        raise Mismatch("%s %s: descriptor writes %s x %d, the conv gives %s x %d" % (role, cv.conv, (d.to, d.ho, d.wo), d.cout, out, node.ch))
    return src.name, sub


def launch_io(g, cons, launch, held=None) -> LaunchIO:
    """What ``launch`` computes, reads and stores in terms of graph ``g`` (``cons`` = g.consumers()).  ``held``: buffer -> name of the
    tensor there, which names what a pooling launch pools.  Raises Mismatch where the launch is no part of the graph."""
    kind = launch.kind
    if kind in HEAD_KINDS:
        return _head_io(g, cons, launch, held or {})
    if kind == "pool":
        p = launch.pool
        src = (held or {}).get(launch.src)
        if src is None:
            raise Mismatch("pools %s, which holds nothing" % launch.src)
        if src.endswith(PREPOOL):
            name, pool = src[:-len(PREPOOL)], g[src[:-len(PREPOOL)]].conv.pool_after_bn
        else:
            name = _consumer(g, cons, src, "pool")
            pool = g[name].pool
        if ((p.kt, p.kh, p.kw), (p.st, p.sh, p.sw), (p.pt, p.ph, p.pw)) != (tuple(pool.kernel), tuple(pool.stride), tuple(pool.pad)):
            raise Mismatch("pool descriptor is not the graph's pool behind %s" % src)
        return LaunchIO([name], [Read("src", src, (p.t, p.h, p.w), p.c)],
                        [Store("dst", name, (p.to, p.ho, p.wo), p.c, p.out_ld or p.c, launch.ch_off)])
    roles = OPERANDS.get("conv" if kind in STEM_KINDS else kind)
    if roles is None:
        raise Mismatch("launch kind %r has no place in the graph" % kind)
    convs = [(role, cv, d) for (role, cv), d in zip(launch.convs.items(), launch.descs) if cv is not None]
    if sum(d is not None for d in launch.descs) != len(convs) or len(launch.descs) != len(launch.convs) or not convs:
        raise Mismatch("ConvSpecs and descriptors of the launch do not pair up")
    made, reads_of, dsc = [], {}, {}
    for role, cv, d in convs:
        src, sub = _check_conv(g, role, cv, d, len(launch.convs) == 1, kind in ("tstem", "tstem_pool3"))
        made.append(cv.conv); reads_of[cv.conv] = (role, src, sub); dsc[role] = d
    # the block's add rides behind a c conv
    c_role = "c" if "c" in dsc else ("conv" if convs[0][1].final_bn else None)
    block = None
    if c_role is not None:
        cvc = launch.convs[c_role]
        block = _block_of(cvc.conv)
        if g[block].op != "add" or g[block].reads[1] != cvc.conv:
            raise Mismatch("%s is not the c conv of block %s" % (cvc.conv, block))
        made.append(block)
    out_desc = dsc[c_role] if c_role else convs[0][2]
    to, ho, wo = out_desc.to, out_desc.ho, out_desc.wo
    stores = []
    last = block or convs[0][1].conv
    dims, sub_out = (to, ho, wo), 1
    if kind in ("stem_pool", "stem3_pool", "tstem_pool3"):          # the stem's 1x3x3 / stride-2 pool behind it
        last = _consumer(g, cons, last, "pool"); made.append(last)
        if (tuple(g[last].pool.kernel), tuple(g[last].pool.stride), tuple(g[last].pool.pad)) != ((1, 3, 3), (1, 2, 2), (0, 1, 1)):
            raise Mismatch("%s fuses a pool the graph does not have" % kind)
        dims = (to, (ho - 1) // 2 + 1, (wo - 1) // 2 + 1)
    cv0 = convs[0][1]
    if kind == "tstem":                                              # its descriptor's output dims are the pooled ones
        pass
    elif kind == "conv" and cv0.pool_after_bn is not None:
        p = cv0.pool_after_bn
        if launch.tpool == 2:
            if (tuple(p.kernel), tuple(p.stride), tuple(p.pad)) != ((1, 2, 2), (1, 2, 2), (0, 0, 0)) or ho % 2 or wo % 2:
                raise Mismatch("tpool = 2 is not the pool_after_bn of %s" % cv0.conv)
            dims = (to, ho // 2, wo // 2)
        elif launch.tpool == 0:
            made[made.index(cv0.conv)] = last = cv0.conv + PREPOOL
        else:
            raise Mismatch("tpool = %d on %s" % (launch.tpool, cv0.conv))
    elif launch.tpool == 1:                                          # the temporal pool behind s2 rides behind the add
        if block is None or kind not in ("conv", "cpa") or to % 2:
            raise Mismatch("tpool = 1 on a launch without a block add")
        last = _consumer(g, cons, block, "pool"); made.append(last)
        if (tuple(g[last].pool.kernel), tuple(g[last].pool.stride), tuple(g[last].pool.pad)) != ((2, 1, 1), (2, 1, 1), (0, 0, 0)):
            raise Mismatch("tpool = 1 is not the graph's pool behind %s" % block)
        dims = (to // 2, ho, wo)
    elif launch.tpool != 0:
        raise Mismatch("tpool = %d on a %s launch" % (launch.tpool, kind))
    if kind == "cpa":
        if launch.tpool != 1 or launch.x_sub not in (1, 2):
            raise Mismatch("cpa with tpool = %d, x_sub = %d" % (launch.tpool, launch.x_sub))
        if launch.x_sub == 2:
            if ho % 2 or wo % 2:
                raise Mismatch("x_sub = 2 over odd dims")
            dims, sub_out = (dims[0], ho // 2, wo // 2), 2
    elif launch.x_sub not in (0, 1):
        raise Mismatch("x_sub = %d on a %s launch" % (launch.x_sub, kind))
    ch = out_desc.cout
    stores.append(Store("dst", last, dims, ch, launch.ld or ch, launch.ch_off, sub_out))
    if "a_next" in dsc:
        da, cva = dsc["a_next"], launch.convs["a_next"]
        made.remove(cva.conv); made.append(cva.conv)                 # graph order: behind what it reads
        stores.append(Store("dst_a", cva.conv, (da.to, da.ho, da.wo), da.cout, da.cout))
    # what the launch must find in memory
    reads = {}

    def need(operand, r):
        if operand in reads and (reads[operand].name, reads[operand].dims, reads[operand].ch, reads[operand].sub) != (r.name, r.dims, r.ch, r.sub):
            raise Mismatch("%s would have to hold both %s and %s" % (operand, reads[operand].name, r.name))
        reads[operand] = r
    inside = set(made) | ({cv0.conv} if last.endswith(PREPOOL) else set())
    for role, cv, d in convs:
        _, src, sub = reads_of[cv.conv]
        if src in inside:
            if sub != 1:
                raise Mismatch("%s: subsampled read of a tensor made in the same launch" % cv.conv)
            continue
        if role not in roles:
            raise Mismatch("a %s launch reads nothing from memory for its %s conv, the graph has %s read %s" % (kind, role, cv.conv, src))
        need(roles[role], Read(roles[role], src, (d.t, d.h, d.w), d.cin, sub))
    if block is not None:
        sc = g[block].reads[0]
        if sc not in inside:
            need(roles["add"], Read(roles["add"], sc, (to, ho, wo), ch))
    for name in made:                                                 # nothing else of the graph may be read
        if name.endswith(PREPOOL):
            continue
        for r in g[name].reads:
            if r not in inside and r not in [x.name for x in reads.values()]:
                raise Mismatch("%s reads %s, which this launch neither makes nor binds" % (name, r))
    return LaunchIO(made, list(reads.values()), stores)


def _head_io(g, cons, launch, held):
    p = launch.pool
    if launch.kind == "linear":
        return LaunchIO(["logits"], [], [Store("logits", "logits", g["logits"].dims, g["logits"].ch, g["logits"].ch)])
    src = held.get(launch.src)
    if src is None:
        raise Mismatch("the head reads %s, which holds nothing" % launch.src)
    op = "tokens" if launch.kind == "tt_head" else "avgpool"
    name = _consumer(g, cons, src, op)
    node = g[name]
    if (p.kt, p.kh, p.kw) != tuple(node.pool.kernel) or (p.st, p.sh, p.sw, p.pt, p.ph, p.pw) != (1, 1, 1, 0, 0, 0):
        raise Mismatch("head pool window %s is not the graph's %s" % ((p.kt, p.kh, p.kw), tuple(node.pool.kernel)))
    read = Read("src", src, (p.t, p.h, p.w), p.c)
    dims = (p.to, p.ho, p.wo)
    if launch.kind == "tt_head":
        return LaunchIO([name, "logits"], [read], [Store("tokens", name, dims, p.c, p.c), Store("logits", "logits", (1, 1, 1), g["logits"].ch, g["logits"].ch)])
    if launch.kind == "head":
        if name != "pooled":
            raise Mismatch("head pools %s, not the last trunk" % src)
        return LaunchIO([name, "logits"], [read], [Store("pooled", name, dims, p.c, p.c),
                                                   Store("logits", "logits", g["logits"].dims, g["logits"].ch, g["logits"].ch)])
    cc = _consumer(g, cons, name, "concat")                          # SlowFast: one pathway's share of the pooled row
    off = sum(g[r].ch for r in g[cc].reads[:g[cc].reads.index(name)])
    if launch.ch_off != off:
        raise Mismatch("%s goes to channel %d of the pooled row, the graph has it at %d" % (name, launch.ch_off, off))
    return LaunchIO([name], [read], [Store("pooled", name, dims, p.c, g[cc].ch, launch.ch_off)])


@dataclasses.dataclass
class Held:
    dims: Tuple[int, int, int]
    ld: int
    segs: List[Tuple[int, int, str]]           # (first channel, channels, graph tensor), by first channel
    sub: int = 1


def input_names(plan):
    return ["input"] if len(plan.inputs) == 1 else ["input_slow", "input_fast"]


def walk(plan, g, on_launch=None):
    """[(launch index, message)]; empty when every launch of ``plan`` executes graph ``g``.  What the graph lacks at the end is
    reported at index len(plan.launches).  ``on_launch(i, launch, io, table)`` sees every launch that maps (the replay's hook)."""
    cons = g.consumers()
    errors = []
    table = {buf: Held(tuple(dims), 3, [(0, 3, name)]) for (buf, dims, _), name in zip(plan.inputs, input_names(plan))}
    for (buf, dims, _), name in zip(plan.inputs, input_names(plan)):
        if tuple(dims) != g[name].dims:
            errors.append((0, "input %s has dims %s, the graph %s" % (buf, dims, g[name].dims)))
    done = {name: -1 for name in input_names(plan)}                   # graph tensor -> the launch that computed it

    def alive(name, after):
        """some graph reader of ``name`` is still to come"""
        for c in cons.get(name, ()) if not name.endswith(PREPOOL) else [name[:-len(PREPOOL)]]:
            if c not in after or (g[c].op == "concat" and alive(c, after)):
                return True
        return False

    for i, launch in enumerate(plan.launches):
        err = lambda msg: errors.append((i, "%s launch %d: %s" % (launch.kind, i, msg)))      # noqa: E731
        try:
            io = launch_io(g, cons, launch, {b: h.segs[0][2] for b, h in table.items() if len(h.segs) == 1})
        except Mismatch as e:
            err(str(e))
            continue
        # reads: the operand holds, as the last thing written there, exactly the tensor the graph has this launch read
        want = {r.operand: r for r in io.reads}
        read_bufs = set()
        for operand in ("src", "src2", "res"):
            buf, r = getattr(launch, operand), want.get(operand)
            if buf is None and r is None:
                continue
            if r is None:
                err("binds %s = %s, the graph has nothing read there" % (operand, buf)); read_bufs.add(buf)
                continue
            if buf is None:
                err("binds no %s, the graph reads %s there" % (operand, r.name))
                continue
            read_bufs.add(buf)
            node = g[r.name] if not r.name.endswith(PREPOOL) else None
            parts = [(q, g[q].ch) for q in node.reads] if node is not None and node.op == "concat" else [(r.name, r.ch)]
            segs, off = [], 0
            for q, c in parts:
                segs.append((off, c, q)); off += c
            gdims = node.dims if node is not None else None
            if r.sub == 2:
                gdims = (gdims[0], gdims[1] // 2, gdims[2] // 2)
            if node is not None and (tuple(r.dims) != tuple(gdims) or r.ch != node.ch):
                err("%s: the descriptor takes %s as %s x %d, the graph has %s x %d" % (operand, r.name, r.dims, r.ch, gdims, node.ch))
            h = table.get(buf)
            if h is None:
                err("%s = %s holds nothing yet, the graph reads %s" % (operand, buf, r.name))
            elif (h.segs, tuple(h.dims), h.ld, h.sub) != (segs, tuple(r.dims), r.ch, r.sub):
                err("%s = %s holds %s dims %s row stride %d sub %d; the graph reads %s as dims %s x %d channels sub %d"
                    % (operand, buf, [s[2] for s in h.segs], h.dims, h.ld, h.sub, r.name, r.dims, r.ch, r.sub))
            rows = plan.batch * r.dims[0] * r.dims[1] * r.dims[2]
            if buf in plan.sizes and rows * r.ch > plan.sizes[buf]:
                err("reads %d elements of %s, sized %d" % (rows * r.ch, buf, plan.sizes[buf]))
            elif buf not in plan.sizes and done.get(r.name) != -1:
                err("%s = %s has no size in the plan" % (operand, buf))
        for name in io.made:
            for q in (g[name].reads if not name.endswith(PREPOOL) else ()):
                if q not in done and q not in io.made:
                    err("%s needs %s, which no earlier launch computed" % (name, q))
        # coverage: every graph tensor is computed once
        after = set(done) | set(io.made)
        for name in io.made:
            if name in done:
                err("computes %s again (launch %d did)" % (name, done[name]))
            done[name] = i
        # writes
        for s in io.stores:
            if s.operand not in ("dst", "dst_a"):
                continue
            buf = getattr(launch, s.operand)
            if buf is None:
                err("stores %s but binds no %s" % (s.name, s.operand))
                continue
            if buf in read_bufs:
                err("%s = %s is a buffer the launch reads" % (s.operand, buf))
            if s.operand == "dst_a" and buf == launch.dst:
                err("dst and dst_a are both %s" % buf)
            rows = plan.batch * s.dims[0] * s.dims[1] * s.dims[2]
            if buf not in plan.sizes:
                err("%s = %s has no size in the plan" % (s.operand, buf))
            elif (rows - 1) * s.ld + s.ch_off + s.ch > plan.sizes[buf]:
                err("writes up to element %d of %s, sized %d" % ((rows - 1) * s.ld + s.ch_off + s.ch, buf, plan.sizes[buf]))
            if s.ch_off + s.ch > s.ld:
                err("channels %d..%d do not fit the row stride %d" % (s.ch_off, s.ch_off + s.ch, s.ld))
            node = g[s.name] if not s.name.endswith(PREPOOL) else None
            if node is not None:
                gd = node.dims if s.sub == 1 else (node.dims[0], node.dims[1] // 2, node.dims[2] // 2)
                if tuple(s.dims) != tuple(gd) or s.ch != node.ch:
                    err("stores %s as %s x %d, the graph has %s x %d" % (s.name, s.dims, s.ch, gd, node.ch))
            h = table.get(buf)
            if s.ch_off == 0:
                for _, _, old in (h.segs if h is not None else ()):
                    if alive(old, after):
                        err("overwrites %s in %s, which a later launch still reads" % (old, buf))
                table[buf] = Held(tuple(s.dims), s.ld, [(0, s.ch, s.name)], s.sub)
                continue
            # a lateral: channels behind what the rows already hold, which completes the graph's concat
            cc = [c for c in cons[s.name] if g[c].op == "concat"] if node is not None else []
            if len(cc) != 1:
                err("writes %s at channel %d, the graph has no concat for it" % (s.name, s.ch_off))
                continue
            parts, off, segs = g[cc[0]].reads, 0, []
            for q in parts:
                segs.append((off, g[q].ch, q)); off += g[q].ch
            mine = [x for x in segs if x[2] == s.name]
            if h is None or (tuple(h.dims), h.ld, h.sub) != (tuple(s.dims), s.ld, 1) or mine != [(s.ch_off, s.ch, s.name)] or \
                    h.segs != [x for x in segs if x[2] != s.name] or off != s.ld:
                err("writes %s at channel %d of %s (row stride %d), which holds %s: not the graph's %s = %s"
                    % (s.name, s.ch_off, buf, s.ld, None if h is None else ([x[2] for x in h.segs], h.dims, h.ld), cc[0], list(parts)))
                continue
            h.segs = segs
            if cc[0] in done:
                err("completes %s again" % cc[0])
            done[cc[0]] = i
        # the pooled row of a two-pathway head is complete once both pathways have been pooled
        for s in io.stores:
            if s.operand == "pooled" and s.name != "pooled" and all(q in done for q in g["pooled"].reads) and "pooled" not in done:
                done["pooled"] = i
        if launch.kind == "linear" and "pooled" not in done:
            err("the head's Linear runs before the pooled row is complete")
        if on_launch is not None:
            on_launch(i, launch, io, table)
    n = len(plan.launches)
    for name in g.nodes:
        if name not in done:
            errors.append((n, "the plan never computes %s" % name))
    return errors
