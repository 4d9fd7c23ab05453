"""Generates tests/golden/conv_paths.json and tests/golden/conv_work_units.json: the host-side decisions of libafhip.so for every
conv of the three networks.

    AF_HIP_LIB=<libafhip.so of the commit to record> python tools/gen_conv_paths_golden.py

No GPU is needed: af_conv_variant, af_conv_workspace_bytes, the *_work_units functions and the *_fusable predicates are host logic
(a machine without a device counts 256 compute units, as an MI355X has).  Record from the library whose decisions are to be kept -
for a refactor of the launchers that is the PARENT commit's build (check the parent out into a scratch directory, run its
build.py there and name that libafhip.so) - and let tests/test_host_cpu.py compare the library under test with it.

Per network (i3d_r50, slowfast_r50, ftcn_tt), precision (f32, bf16, f16) and batch (1, 8, 16):
  convs    the plan with every fusion switched off, so that each conv is a launch of its own ("conv") or one with its
           projection shortcut ("dual"): [kind, af_conv_variant id, its af_conv_variant_name, af_conv_workspace_bytes] per launch,
           in plan order
  fusable  the plan with every fusion switched on: [switch, answer] for each question the engine asks the library's four
           *_fusable predicates (bc, ca, cpa, abc), in the order asked
conv_work_units.json, same keys:
  convs    per launch of `convs` above what af_conv_work_units returns: [rc, units, workgroups], or [rc, af_last_error] where it refuses
  fused    per question of `fusable` answered yes, in the same order: [switch, ...] with what af_conv_ca_work_units (tiles,
           workgroups, form, pixels), af_conv_cpa_work_units (tiles, workgroups) or af_block_abc_work_units (patch rows, time
           segments, units) says; a bc pair has no such function: [switch]
"""
import ctypes as C
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden", "conv_paths.json")
GOLDEN_WORK = os.path.join(ROOT, "tests", "golden", "conv_work_units.json")
BATCHES, PRECISIONS = (1, 8, 16), ("f32", "bf16", "f16")
FUSIONS = ("AF_FUSE_BC", "AF_FUSE_CA", "AF_FUSE_CPA", "AF_FUSE_ABC")


def collect(work=None):
    """the content of conv_paths.json; with `work` (a dict) also that of conv_work_units.json into it"""
    if ROOT not in sys.path:
        sys.path.insert(0, ROOT)
    from af_mi355x import arch, engine
    from af_mi355x._lib import lib
    lib.af_conv_variant_name.restype = C.c_char_p
    specs = {"i3d_r50": arch.i3d_r50_spec(), "slowfast_r50": arch.slowfast_r50_spec(), "ftcn_tt": arch.ftcn_tt_spec()}
    rgb3 = {"i3d_r50": {specs["i3d_r50"].stem.conv}, "slowfast_r50": {specs["slowfast_r50"].stems[0].conv}, "ftcn_tt": set()}
    asked, fused = [], []
    plain_fusable = engine._Plan._fusable

    def pair_work(self, switch, convs, more):
        ds = [None if c is None else C.byref(self.desc(*c)) for c in convs]
        n, i, j, k = C.c_int64(0), C.c_int(0), C.c_int(0), C.c_int(0)
        if switch == "AF_FUSE_CA":
            rc, got = lib.af_conv_ca_work_units(*ds, C.byref(n), C.byref(i), C.byref(j), C.byref(k)), [n, i, j, k]
        elif switch == "AF_FUSE_CPA":
            rc, got = lib.af_conv_cpa_work_units(*ds, *more, C.byref(n), C.byref(i)), [n, i]
        elif switch == "AF_FUSE_ABC":
            rc, got = lib.af_block_abc_work_units(*ds, C.byref(i), C.byref(j), C.byref(n)), [i, j, n]
        else:
            return [switch]
        assert rc == 1, (switch, rc)
        return [switch] + [int(x.value) for x in got]

    def recording_fusable(self, switch, ask, convs, *more):
        answer = plain_fusable(self, switch, ask, convs, *more)
        asked.append([switch, int(answer)])
        if answer and work is not None:
            fused.append(pair_work(self, switch, convs, more))
        return answer

    def conv_work(d, d2):
        units, groups = C.c_int64(0), C.c_int(0)
        rc = int(lib.af_conv_work_units(C.byref(d), C.byref(d2) if d2 is not None else None, C.byref(units), C.byref(groups)))
        return [rc, int(units.value), int(groups.value)] if rc >= 0 else [rc, lib.af_last_error().decode()]

    def plan(net, dtype, batch, fuse):
        spec = specs[net]
        for name in FUSIONS:
            os.environ[name] = "1" if fuse else "0"
        return engine.plan_network(spec, dtype, batch, (spec.num_frames, spec.crop, spec.crop), rgb3[net] if dtype != "f32" else set())

    saved = {name: os.environ.get(name) for name in FUSIONS}
    out = {}
    try:
        engine._Plan._fusable = recording_fusable
        for net in specs:
            for dtype in PRECISIONS:
                for batch in BATCHES:
                    p, convs, units = plan(net, dtype, batch, False), [], []
                    for e in p.entries:
                        if e["kind"] not in ("conv", "dual"):
                            continue
                        d = p.desc(e["cv"], e["din"], e["dout"], int(e.get("tpool") or 0))
                        d2 = p.desc(e["cv2"], e["din2"], e["dout"]) if e["kind"] == "dual" else None
                        v = lib.af_conv_variant(C.byref(d), C.byref(d2) if d2 is not None else None)
                        convs.append([e["kind"], int(v), lib.af_conv_variant_name(v).decode(), int(lib.af_conv_workspace_bytes(C.byref(d)))])
                        if work is not None:
                            units.append(conv_work(d, d2))
                    del asked[:], fused[:]
                    plan(net, dtype, batch, True)
                    out["%s/%s/%d" % (net, dtype, batch)] = {"convs": convs, "fusable": list(asked)}
                    if work is not None:
                        work["%s/%s/%d" % (net, dtype, batch)] = {"convs": units, "fused": list(fused)}
    finally:
        engine._Plan._fusable = plain_fusable
        for name, v in saved.items():
            if v is None:
                os.environ.pop(name, None)
            else:
                os.environ[name] = v
    return out


if __name__ == "__main__":
    work = {}
    got = collect(work)
    for path, what in ((GOLDEN, got), (GOLDEN_WORK, work)):
        with open(path, "w") as f:
            json.dump(what, f, separators=(",", ":"), sort_keys=True)
            f.write("\n")
    print("wrote", GOLDEN, sum(len(v["convs"]) for v in got.values()), "convs,",
          sum(len(v["fusable"]) for v in got.values()), "fusable answers")
    print("wrote", GOLDEN_WORK, sum(len(v["convs"]) for v in work.values()), "conv work units,",
          sum(len(v["fused"]) for v in work.values()), "fused pairs")
