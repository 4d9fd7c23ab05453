"""Generates tests/golden/conv_paths.json and tests/golden/conv_work_units.json: the host-side decisions of libafhip.so for every
conv of the three networks; with --launches, tests/golden/plan_launches.json: a digest of every launch plan.

    AF_HIP_LIB=<libafhip.so of the commit to record> python tools/gen_conv_paths_golden.py [--launches]

No GPU is needed: af_conv_variant, af_conv_workspace_bytes, the *_work_units functions and the *_fusable predicates are host logic
(a machine without a device counts 256 compute units, as an MI355X has).  Record from the library whose decisions are to be kept -
for a refactor of the launchers that is the PARENT commit's build (check the parent out into a scratch directory, run its
build.py there and name that libafhip.so) - and let tests/test_host_cpu.py compare the library under test with it.  Every
descriptor is the plan's own (engine.Launch.descs): what the engine launches with is what is recorded.

Per network (i3d_r50, slowfast_r50, ftcn_tt), precision (f32, bf16, f16) and batch (1, 8, 16):
  convs    the plan with every fusion switched off, so that each conv is a launch of its own ("conv") or one with its
           projection shortcut ("dual"): [kind, af_conv_variant id, its af_conv_variant_name, af_conv_workspace_bytes] per launch,
           in plan order
  fusable  the plan with every fusion switched on: [switch, answer] for each question the engine asks the library's four
           *_fusable predicates (bc, ca, cpa, abc), in the order asked (engine._Plan.asked)
conv_work_units.json, same keys:
  convs    per launch of `convs` above what af_conv_work_units returns: [rc, units, workgroups], or [rc, af_last_error] where it refuses
  fused    per question of `fusable` answered yes, in the same order: [switch, ...] with what af_conv_ca_work_units (tiles,
           workgroups, form, pixels), af_conv_cpa_work_units (tiles, workgroups) or af_block_abc_work_units (patch rows, time
           segments, units) says; a bc pair has no such function: [switch]
plan_launches.json: per switch setting of LAUNCH_CONFIGS and per network / precision / batch (1 .. 32) the first 16 hex digits of
the SHA-256 of plan_text(), the whole plan as text.  A refactor of the planner leaves every digest as it is.
"""
import contextlib
import ctypes as C
import hashlib
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden", "conv_paths.json")
GOLDEN_WORK = os.path.join(ROOT, "tests", "golden", "conv_work_units.json")
GOLDEN_LAUNCHES = os.path.join(ROOT, "tests", "golden", "plan_launches.json")
BATCHES, PRECISIONS = (1, 8, 16), ("f32", "bf16", "f16")
FUSIONS = ("AF_FUSE_BC", "AF_FUSE_CA", "AF_FUSE_CPA", "AF_FUSE_ABC")
LAUNCH_BATCHES = (1, 2, 3, 4, 6, 8, 12, 16, 24, 32)
LAUNCH_CONFIGS = {"default": {}, "unfused": {name: "0" for name in FUSIONS}, "AF_FUSE_CPA=1": {"AF_FUSE_CPA": "1"},
                  "AF_FUSE_BC=1": {"AF_FUSE_BC": "1"}, "AF_FUSE_TSTEM_POOL=0": {"AF_FUSE_TSTEM_POOL": "0"},
                  "AF_SLOWFAST_STEM3=0": {"AF_SLOWFAST_STEM3": "0"}}


if ROOT not in sys.path:
    sys.path.insert(0, ROOT)
from af_mi355x import arch, engine  # noqa: E402
from af_mi355x._lib import lib  # noqa: E402

SPECS = {"i3d_r50": arch.i3d_r50_spec(), "slowfast_r50": arch.slowfast_r50_spec(), "ftcn_tt": arch.ftcn_tt_spec()}
RGB3 = {"i3d_r50": {SPECS["i3d_r50"].stem.conv}, "slowfast_r50": {SPECS["slowfast_r50"].stems[0].conv}, "ftcn_tt": set()}


def plan(net, dtype, batch):
    spec = SPECS[net]
    return engine.plan_network(spec, dtype, batch, (spec.num_frames, spec.crop, spec.crop), RGB3[net] if dtype != "f32" else set())


@contextlib.contextmanager
def _switches(env):
    """the engine's switches as ``env`` sets them, every other one at its default; the caller's environment is put back"""
    saved = {name: os.environ.pop(name, None) for name in engine.SWITCHES}
    os.environ.update(env)
    try:
        yield
    finally:
        for name, v in saved.items():
            os.environ.pop(name, None)
            os.environ.update({} if v is None else {name: v})


def _ints(desc):
    return "-" if desc is None else ",".join(str(getattr(desc, name)) for name, _ in desc._fields_)


def plan_text(p):
    """The canonical text of a plan: its buffer sizes, inputs, head and the questions asked with their answers; per launch the kind,
    the 21 integers of every conv descriptor, the buffers, row stride, channel offset, x_sub and the pool descriptor."""
    out = ["sizes=%s" % sorted(p.sizes.items()), "inputs=%s" % (p.inputs,), "rgb3=%s" % p.rgb3,
           "rgb3_inputs=%s" % sorted(p.rgb3_inputs), "head_dims=%s head_width=%s" % (p.head_dims, p.head_width),
           "asked=%s" % [(switch, int(yes)) for switch, yes, _ in p.asked]]
    for l in p.launches:
        out.append("%s descs=[%s] src=%s src2=%s res=%s dst=%s dst_a=%s ld=%d ch_off=%d x_sub=%d pool=%s" % (
            l.kind, " ".join("%s:%s" % (role, _ints(d)) for role, d in zip(l.convs, l.descs)), l.src, l.src2, l.res, l.dst, l.dst_a,
            l.ld, l.ch_off, l.x_sub, _ints(l.pool)))
    return "\n".join(out) + "\n"


def collect_launches():
    """the content of plan_launches.json"""
    out = {}
    for config, env in LAUNCH_CONFIGS.items():
        with _switches(env):
            out[config] = {"%s/%s/%d" % (net, dtype, batch): hashlib.sha256(plan_text(plan(net, dtype, batch)).encode()).hexdigest()[:16]
                           for net in SPECS for dtype in PRECISIONS for batch in LAUNCH_BATCHES}
    return out


def collect(work=None):
    """the content of conv_paths.json; with `work` (a dict) also that of conv_work_units.json into it"""
    def fused_work(switch, launch):
        n, i, j, k = C.c_int64(0), C.c_int(0), C.c_int(0), C.c_int(0)
        if launch.kind == "ca":
            rc, got = lib.af_conv_ca_work_units(*launch.refs(), C.byref(n), C.byref(i), C.byref(j), C.byref(k)), [n, i, j, k]
        elif launch.kind == "cpa":
            rc, got = lib.af_conv_cpa_work_units(*launch.refs(), launch.x_sub, C.byref(n), C.byref(i)), [n, i]
        elif launch.kind == "abc":
            rc, got = lib.af_block_abc_work_units(*launch.refs(), C.byref(i), C.byref(j), C.byref(n)), [i, j, n]
        else:
            return [switch]
        assert rc == 1, (switch, rc)
        return [switch] + [int(x.value) for x in got]

    def conv_work(refs):
        units, groups = C.c_int64(0), C.c_int(0)
        rc = int(lib.af_conv_work_units(*refs, C.byref(units), C.byref(groups)))
        return [rc, int(units.value), int(groups.value)] if rc >= 0 else [rc, lib.af_last_error().decode()]

    out = {}
    for net in SPECS:
        for dtype in PRECISIONS:
            for batch in BATCHES:
                convs, units = [], []
                with _switches({name: "0" for name in FUSIONS}):
                    launches = [l for l in plan(net, dtype, batch).launches if l.kind in ("conv", "dual")]
                for l in launches:
                    refs = (l.refs() + [None])[:2]
                    v = lib.af_conv_variant(*refs)
                    convs.append([l.kind, int(v), lib.af_conv_variant_name(v).decode(), int(lib.af_conv_workspace_bytes(refs[0]))])
                    units.append(conv_work(refs))
                with _switches({name: "1" for name in FUSIONS}):
                    asked = plan(net, dtype, batch).asked
                out["%s/%s/%d" % (net, dtype, batch)] = {"convs": convs, "fusable": [[switch, int(yes)] for switch, yes, _ in asked]}
                if work is not None:
                    work["%s/%s/%d" % (net, dtype, batch)] = {"convs": units, "fused": [fused_work(s, l) for s, yes, l in asked if yes]}
    return out


def _write(path, what):
    with open(path, "w") as f:
        json.dump(what, f, separators=(",", ":"), sort_keys=True)
        f.write("\n")


if __name__ == "__main__":
    if "--launches" in sys.argv:
        got = collect_launches()
        _write(GOLDEN_LAUNCHES, got)
        print("wrote", GOLDEN_LAUNCHES, sum(len(v) for v in got.values()), "plans")
        sys.exit(0)
    work = {}
    got = collect(work)
    _write(GOLDEN, got)
    _write(GOLDEN_WORK, work)
    print("wrote", GOLDEN, sum(len(v["convs"]) for v in got.values()), "convs,",
          sum(len(v["fusable"]) for v in got.values()), "fusable answers")
    print("wrote", GOLDEN_WORK, sum(len(v["convs"]) for v in work.values()), "conv work units,",
          sum(len(v["fused"]) for v in work.values()), "fused pairs")
