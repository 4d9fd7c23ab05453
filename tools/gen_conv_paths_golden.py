"""Generates tests/golden/conv_paths.json: the host-side decisions of libafhip.so for every conv of the three networks.

    AF_HIP_LIB=<libafhip.so of the commit to record> python tools/gen_conv_paths_golden.py

No GPU is needed: af_conv_variant, af_conv_workspace_bytes and the *_fusable predicates are host logic (a machine without a
device counts 256 compute units, as an MI355X has).  Record from the library whose decisions are to be kept - for a refactor of
the launchers that is the PARENT commit's build - and let tests/test_host_cpu.py compare the library under test with it.

Per network (i3d_r50, slowfast_r50, ftcn_tt), precision (f32, bf16, f16) and batch (1, 8, 16):
  convs    the plan with every fusion switched off, so that each conv is a launch of its own ("conv") or one with its
           projection shortcut ("dual"): [kind, af_conv_variant id, its af_conv_variant_name, af_conv_workspace_bytes] per launch,
           in plan order
  fusable  the plan with every fusion switched on: [switch, answer] for each question the engine asks the library's four
           *_fusable predicates (bc, ca, cpa, abc), in the order asked
"""
import ctypes as C
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden", "conv_paths.json")
BATCHES, PRECISIONS = (1, 8, 16), ("f32", "bf16", "f16")
FUSIONS = ("AF_FUSE_BC", "AF_FUSE_CA", "AF_FUSE_CPA", "AF_FUSE_ABC")


def collect():
    if ROOT not in sys.path:
        sys.path.insert(0, ROOT)
    from af_mi355x import arch, engine
    from af_mi355x._lib import lib
    lib.af_conv_variant_name.restype = C.c_char_p
    specs = {"i3d_r50": arch.i3d_r50_spec(), "slowfast_r50": arch.slowfast_r50_spec(), "ftcn_tt": arch.ftcn_tt_spec()}
    rgb3 = {"i3d_r50": {specs["i3d_r50"].stem.conv}, "slowfast_r50": {specs["slowfast_r50"].stems[0].conv}, "ftcn_tt": set()}
    asked = []
    plain_fusable = engine._Plan._fusable

    def recording_fusable(self, switch, ask, convs, *more):
        answer = plain_fusable(self, switch, ask, convs, *more)
        asked.append([switch, int(answer)])
        return answer

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
                    p, convs = plan(net, dtype, batch, False), []
                    for e in p.entries:
                        if e["kind"] not in ("conv", "dual"):
                            continue
                        d = p.desc(e["cv"], e["din"], e["dout"], int(e.get("tpool") or 0))
                        d2 = p.desc(e["cv2"], e["din2"], e["dout"]) if e["kind"] == "dual" else None
                        v = lib.af_conv_variant(C.byref(d), C.byref(d2) if d2 is not None else None)
                        convs.append([e["kind"], int(v), lib.af_conv_variant_name(v).decode(), int(lib.af_conv_workspace_bytes(C.byref(d)))])
                    del asked[:]
                    plan(net, dtype, batch, True)
                    out["%s/%s/%d" % (net, dtype, batch)] = {"convs": convs, "fusable": list(asked)}
    finally:
        engine._Plan._fusable = plain_fusable
        for name, v in saved.items():
            if v is None:
                os.environ.pop(name, None)
            else:
                os.environ[name] = v
    return out


if __name__ == "__main__":
    got = collect()
    with open(GOLDEN, "w") as f:
        json.dump(got, f, separators=(",", ":"), sort_keys=True)
        f.write("\n")
    print("wrote", GOLDEN, sum(len(v["convs"]) for v in got.values()), "convs,",
          sum(len(v["fusable"]) for v in got.values()), "fusable answers")
