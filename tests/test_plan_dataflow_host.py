"""No GPU: every launch plan executes the network's dataflow graph.

The plan digests (tests/golden/plan_launches.json) say that a plan has not changed; this says that it is right.  engine_graph.py
states the three networks' dataflow from arch.py alone; plan_dataflow.walk runs each plan's launches in order over a table of what
every buffer holds and reports whatever contradicts the graph:
  coverage  each launch maps, by the names and roles of its ConvSpecs, onto the graph tensors it stores; every graph tensor is
            computed exactly once, before its first reader; the head is reached
  reads     src / src2 / res hold, as the last thing written there, the tensor the graph has that conv read, with the descriptor's
            dims, at a row stride and channel range that make the descriptor's cin channels the right ones (the Slow convs behind a
            lateral read [stage output | lateral] at the widened stride); x_sub == 2: the even-(h, w) restriction, read by the
            stride-1 restatement of the stride-(1,2,2) shortcut
  writes    dst / dst_a is none of the buffers the launch reads; no write destroys a tensor a later launch still reads
  extents   every read and write ends inside plan.sizes[buffer]
over three networks x f32 / bf16 / f16 x plan_cases.BATCHES x the switch settings of gen_conv_paths_golden.LAUNCH_CONFIGS plus every
engine switch flipped (720 plans, ~3 s).  The mutation tests show that the walk can fail: hand-made corruptions of the I3D bf16 batch-16
plan (the lateral one: of SlowFast's, I3D has no lateral) are each reported at the launch they were made in - a buffer that is too
short at the first launch that needs the missing elements.  The walk found no defect in a shipped plan.
"""
import copy
import dataclasses

import pytest

import engine_graph
import plan_cases
import plan_dataflow
from af_mi355x import engine

SETTINGS = [{}, plan_cases.UNFUSED] + [{name: "0" if on else "1"} for name, on in engine.SWITCHES.items()]
GRAPHS = {net: engine_graph.build(spec) for net, spec in plan_cases.SPECS.items()}


def test_graph_holds_every_conv_once_with_the_oracles_shapes():
    """the graph itself: every conv of the spec, the shapes the oracle's forward gives (f2_stages / the head widths)"""
    for net, spec in plan_cases.SPECS.items():
        g = GRAPHS[net]
        convs = [n.conv for n in g.nodes.values() if n.op == "conv"]
        assert sorted(c.conv for c in convs) == sorted(c.conv for c in spec.convs()), net
        assert all(n.reads for n in g.nodes.values() if n.op != "input")
    g = GRAPHS["i3d_r50"]
    assert (g["stem_pool"].dims, g["stem_pool"].ch) == ((32, 56, 56), 64)
    assert (g["pool_after_s2"].dims, g["pool_after_s2"].ch) == ((16, 56, 56), 256)
    assert (g["resnet.s5.pathway0_res2"].dims, g["resnet.s5.pathway0_res2"].ch) == ((16, 7, 7), 2048)
    assert (g["pooled"].dims, g["pooled"].ch) == ((1, 1, 1), 2048)
    g = GRAPHS["ftcn_tt"]
    assert (g["resnet.s1.pathway0_stem.conv"].dims, g["stem_pool"].dims) == ((32, 112, 112), (32, 56, 56))
    assert (g["resnet.s4.pathway0_res5"].dims, g["resnet.s4.pathway0_res5"].ch) == ((16, 14, 14), 1024)
    assert (g["tokens"].dims, g["tokens"].ch) == ((16, 1, 1), 1024)
    g = GRAPHS["slowfast_r50"]
    assert (g["resnet.s1_fuse"].dims, g["resnet.s1_fuse"].ch) == ((4, 56, 56), 80)
    assert g["resnet.s1_fuse"].reads == ("stem_pool0", "resnet.s1_fuse.conv_f2s")
    assert g["resnet.s3.pathway0_res0.branch2.a"].reads == ("resnet.s2_fuse",) and g["resnet.s2_fuse"].ch == 320
    assert (g["resnet.s5.pathway1_res2"].dims, g["resnet.s5.pathway1_res2"].ch) == ((32, 7, 7), 256)
    assert (g["pooled"].ch, g["pooled"].reads) == (2304, ("pooled_slow", "pooled_fast"))


def test_every_plan_executes_the_graph(monkeypatch):
    n = 0
    for net, dtype, batch, what, plan in plan_cases.plans(monkeypatch, SETTINGS):
        errors = plan_dataflow.walk(plan, GRAPHS[net])
        assert not errors, "%s %s batch %d%s: %s" % (net, dtype, batch, what, errors[:3])
        n += 1
    assert n == 3 * 3 * len(plan_cases.BATCHES) * len(SETTINGS)


def test_odd_sizes_execute_the_graph_too(monkeypatch):
    """input sizes at which the pools cannot ride in their convs (odd frame counts and maps): pools as launches of their own"""
    from af_mi355x import arch
    plan_cases.set_switches(monkeypatch, {})
    for spec, dims in ((arch.i3d_r50_spec(30, 160), (30, 160, 160)), (arch.i3d_r50_spec(10, 96), (10, 96, 96)),
                       (arch.ftcn_tt_spec(10, 96), (10, 96, 96)), (arch.slowfast_r50_spec(16, 96), (16, 96, 96))):
        for dtype in ("f32", "bf16"):
            for batch in (1, 5):
                plan = engine.plan_network(spec, dtype, batch, dims, set())
                errors = plan_dataflow.walk(plan, engine_graph.build(spec, dims))
                assert not errors, (type(spec).__name__, dims, dtype, batch, errors[:3])


# -- the walk can fail --------------------------------------------------------------------------------------------------------------
def _mutable(plan):
    p = copy.copy(plan)
    p.launches, p.sizes = list(plan.launches), dict(plan.sizes)
    return p


def _first_error(plan, net):
    errors = plan_dataflow.walk(plan, GRAPHS[net])
    assert errors, "the corrupted plan passed"
    print(errors[0])
    return errors[0][0]


@pytest.fixture
def i3d(monkeypatch):
    plan_cases.set_switches(monkeypatch, {})
    plan = plan_cases.plan("i3d_r50", "bf16", 16)
    assert not plan_dataflow.walk(plan, GRAPHS["i3d_r50"])
    return plan


def _is_c(launch):
    return launch.kind == "conv" and launch.convs["conv"].final_bn


def test_mutation_residual_from_the_other_trunk_buffer(i3d):
    for i, l in enumerate(i3d.launches):
        if _is_c(l) and l.res in ("P0", "P1"):
            p = _mutable(i3d)
            p.launches[i] = dataclasses.replace(l, res="P1" if l.res == "P0" else "P0")
            assert _first_error(p, "i3d_r50") == i
            break
    else:
        raise AssertionError("no c launch with a residual")


def test_mutation_buffer_one_row_short(i3d):
    extents = []           # (launch, buffer, elements it needs there) of the clean plan

    def see(i, launch, io, table):
        for s in io.stores:
            if s.operand in ("dst", "dst_a"):
                extents.append((i, getattr(launch, s.operand), (i3d.batch * s.dims[0] * s.dims[1] * s.dims[2] - 1) * s.ld + s.ch_off + s.ch))
        for r in io.reads:
            extents.append((i, getattr(launch, r.operand), i3d.batch * r.dims[0] * r.dims[1] * r.dims[2] * r.ch))
    assert not plan_dataflow.walk(i3d, GRAPHS["i3d_r50"], see)
    for buf, size in i3d.sizes.items():
        # the planner sizes every buffer by its largest tenant exactly: no row to spare
        assert max(e for _, b, e in extents if b == buf) == size, buf
        row = 64               # the narrowest row any of these buffers holds
        p = _mutable(i3d)
        p.sizes[buf] = size - row
        assert _first_error(p, "i3d_r50") == min(i for i, b, e in extents if b == buf and e > size - row), buf


def test_mutation_two_adjacent_launches_swapped(i3d):
    swapped = 0
    for i in range(len(i3d.launches) - 1):
        a, b = i3d.launches[i], i3d.launches[i + 1]
        if a.dst is None or b.kind in plan_dataflow.HEAD_KINDS:
            continue
        p = _mutable(i3d)
        p.launches[i], p.launches[i + 1] = b, a
        assert _first_error(p, "i3d_r50") == i, (i, a.kind, b.kind)
        swapped += 1
    assert swapped >= 40           # a chain: every launch reads what the one before it stored


def test_mutation_lateral_at_channel_zero(monkeypatch):
    plan_cases.set_switches(monkeypatch, {})
    plan = plan_cases.plan("slowfast_r50", "bf16", 16)
    laterals = [i for i, l in enumerate(plan.launches) if l.ch_off > 0 and l.kind == "conv"]
    assert len(laterals) == 4
    for i in laterals:
        p = _mutable(plan)
        p.launches[i] = dataclasses.replace(plan.launches[i], ch_off=0)
        assert _first_error(p, "slowfast_r50") == i


def test_mutation_b_conv_into_the_live_trunk(i3d):
    for i, l in enumerate(i3d.launches[:-2]):
        b, c = i3d.launches[i + 1], i3d.launches[i + 2]
        if l.kind == "conv" and l.dst == "A" and (b.kind, b.src, b.dst) == ("conv", "A", "B") and c.res == l.src:
            p = _mutable(i3d)
            p.launches[i + 1] = dataclasses.replace(b, dst=l.src)            # the block's input, which the c conv still adds
            assert _first_error(p, "i3d_r50") == i + 1
            p = _mutable(i3d)
            p.launches[i] = dataclasses.replace(l, dst="B")
            p.launches[i + 1] = dataclasses.replace(b, src="B", dst="A")
            p.launches[i + 2] = dataclasses.replace(c, src="A")
            assert not plan_dataflow.walk(p, GRAPHS["i3d_r50"])              # A and B exchanged: still the graph
            break
    else:
        raise AssertionError("no a, b, c launches in a row")


def test_mutation_neighbours_conv(i3d):
    """a launch bound to the next block's conv of the same shape"""
    blocks = {b.name: b for st in plan_cases.SPECS["i3d_r50"].stages for b in st.blocks}
    for i, l in enumerate(i3d.launches):
        if l.kind == "conv" and l.convs["conv"].conv == "resnet.s4.pathway0_res2.branch2.b":
            other = blocks["resnet.s4.pathway0_res3"].b
            assert dataclasses.replace(other, conv=l.convs["conv"].conv, bn=l.convs["conv"].bn) == l.convs["conv"]
            p = _mutable(i3d)
            p.launches[i] = dataclasses.replace(l, convs={"conv": other})
            assert _first_error(p, "i3d_r50") == i
            return
    raise AssertionError("no such launch")
