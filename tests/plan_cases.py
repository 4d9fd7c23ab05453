"""The launch plans the plan tests of test_host_cpu.py walk: the three networks at their own input size, with the K-packed stem
weights a 16-bit PackedWeights has (PackedWeights.w3), under given settings of the engine's switches.  Planning needs no device."""
from af_mi355x import arch, engine

FUSIONS = ("AF_FUSE_BC", "AF_FUSE_CA", "AF_FUSE_CPA", "AF_FUSE_ABC")
UNFUSED = {name: "0" for name in FUSIONS}
BATCHES = (1, 2, 3, 4, 6, 8, 12, 16, 24, 32)
SPECS = {"i3d_r50": arch.i3d_r50_spec(), "slowfast_r50": arch.slowfast_r50_spec(), "ftcn_tt": arch.ftcn_tt_spec()}
RGB3 = {"i3d_r50": {SPECS["i3d_r50"].stem.conv}, "slowfast_r50": {SPECS["slowfast_r50"].stems[0].conv}, "ftcn_tt": set()}


def set_switches(monkeypatch, switches):
    """every engine switch at its default, but for ``switches`` (name -> "0" / "1"); they are read when a plan is built"""
    for name in engine.SWITCHES:
        monkeypatch.delenv(name, raising=False)
    for name, value in switches.items():
        monkeypatch.setenv(name, value)


def plan(net, dtype, batch):
    spec = SPECS[net]
    return engine.plan_network(spec, dtype, batch, (spec.num_frames, spec.crop, spec.crop), RGB3[net] if dtype != "f32" else set())


def plans(monkeypatch, settings=({},), dtypes=("f32", "bf16", "f16"), batches=BATCHES):
    """(net, dtype, batch, text naming the setting, plan) for every network, dtype and batch under each setting of the switches"""
    for switches in settings:
        set_switches(monkeypatch, switches)
        what = " unfused" if switches == UNFUSED else "".join(" with %s=%s" % kv for kv in switches.items())
        for net in SPECS:
            for dtype in dtypes:
                for batch in batches:
                    yield net, dtype, batch, what, plan(net, dtype, batch)
