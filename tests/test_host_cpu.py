"""CPU: host-side logic of the drop-in (no compute calls): checkpoint layout, load() behaviour table
generated from the reference's ModelBase.load, error behaviour, and the C ABI surface."""
import os
import re
import tempfile

import pytest
import torch

from conftest import ROOT, load_json
from af_mi355x import arch, synth
from af_mi355x.classifier import Classifier


@pytest.fixture(scope="module")
def clf():
    return Classifier().eval()


def test_state_dict_layout_equals_reference(clf):
    lay = load_json("layout.json")["entries"]
    mine = [[k, list(v.shape), str(v.dtype).replace("torch.", "")] for k, v in clf.network.state_dict().items()]
    assert mine == lay
    both = list(clf.state_dict().keys())
    assert len(both) == 640 and both[0].startswith("network.") and both[320].startswith("_warped_network.")
    assert sum(p.numel() for p in clf.parameters()) == 27225921


def test_slowfast_state_dict_layout():
    from af_mi355x.classifier import SlowFast8x8
    m = SlowFast8x8()
    lay = [(k, tuple(v.shape)) for k, v in m.state_dict().items()]
    assert lay == [(k, tuple(s)) for k, s, d in arch.state_dict_layout(m.spec)]
    assert len(lay) == load_json("f5_slowfast.json")["num_keys"] == 662
    assert sum(p.numel() for p in m.parameters()) == 33560521
    assert m.resnet.s1_fuse.conv_f2s.weight.shape == (16, 8, 5, 1, 1)
    assert m.resnet.s2.pathway0_res0.branch2.a.weight.shape == (64, 80, 1, 1, 1)     # 64 + 2*8 fused channels in
    assert m.resnet.head.projection.in_features == 2304


def test_ftcn_tt_plugin_layout_and_load(tmp_path):
    """FTCN-TT drop-in: the module tree reproduces the reference plugin's 275-key state_dict (BNs followed by a pool
    under `<bn>.0`, `resnet.head.time_T.*`; asserted key-by-key against the reference in oracle/gen_golden.py --ftcn
    and pinned here through the fixture's key / parameter counts), its last nn.Linear is mlp_head.1, and load() has the
    ModelBase semantics (wrapper key + one prefix stripped)."""
    from af_mi355x.classifier import FtcnTTClassifier
    g = load_json("f6_ftcn.json")
    c = FtcnTTClassifier().eval()
    sd = c.network.state_dict()
    lay = arch.state_dict_layout(arch.ftcn_tt_spec())
    assert [k for k, _, _ in lay] == list(sd.keys()) and len(sd) == g["num_keys"] == 275
    assert all(tuple(sd[k].shape) == tuple(sh) for k, sh, _ in lay)
    assert sum(p.numel() for p in c.parameters()) == g["num_params"]
    assert "resnet.s1.pathway0_stem.bn.0.weight" in sd and "resnet.s3.pathway0_res0.branch1_bn.0.running_var" in sd
    last = [m for m in c.network.modules() if isinstance(m, torch.nn.Linear)][-1]
    assert last is getattr(c.network.resnet.head.time_T.mlp_head, "1") and last.in_features == 1024
    w = synth.synthetic_state_dict(arch.ftcn_tt_spec(), seed=g["weights_seed"])
    assert synth.state_dict_sha256(w) == g["weights_sha256"]
    path = os.path.join(tmp_path, "ftcn.pth")
    torch.save({"model_state_dict": {"network." + k: v for k, v in w.items()}}, path)
    assert c.load(path) == (True, -1)
    assert torch.equal(c.network.state_dict()["resnet.head.time_T.pos_embedding"], w["resnet.head.time_T.pos_embedding"])
    assert c.load(os.path.join(tmp_path, "missing.pth")) == (False, -1)
    with pytest.raises(RuntimeError):
        c(torch.zeros(1, 3, 32, 224, 224))               # CPU tensor: no fallback


def test_dualrun_encoder_layout_and_errors():
    """dualrun drop-in: 136-key state_dict in the reference's order (asserted against the reference class in
    oracle/gen_golden.py --dualrun, pinned here by the fixture's counts and the recipe hash); no CPU fallback."""
    from af_mi355x import dualrun
    g = load_json("f7_dualrun.json")
    sp = dualrun.DualSpec()
    net = dualrun.DualEncoderAU_LMK(mlp_ratio=3.0).eval()
    sd = net.state_dict()
    lay = dualrun.dual_state_dict_layout(sp)
    assert [k for k, _ in lay] == list(sd.keys()) and len(sd) == g["num_keys"]
    assert all(tuple(sd[k].shape) == tuple(sh) for k, sh in lay)
    assert sum(p.numel() for p in net.parameters()) == g["num_params"]
    w = dualrun.dual_synthetic_state_dict(sp, seed=g["weights_seed"])
    assert synth.state_dict_sha256(w) == g["weights_sha256"]
    net.load_state_dict(w)
    A, L, lengths = dualrun.synthetic_dual_inputs(2, sp)
    with pytest.raises(RuntimeError):
        net(A, L, lengths)
    with pytest.raises(NotImplementedError):
        dualrun.DualEncoderAU_LMK(use_dat=True, domain_classes=3)


@pytest.mark.parametrize("kw,why", [
    (dict(au_dim=17), "multiple of 4"), (dict(lmk_dim=260), "4..256"), (dict(lmk_dim=0), "4..256"),
    (dict(mlp_ratio=2.0 + 1 / 256), "dim_feedforward"), (dict(mlp_ratio=3.5), "dim_feedforward"),
    (dict(mlp_ratio=0.01), "dim_feedforward"), (dict(heads=3), "heads dividing"), (dict(heads=0), "heads dividing"),
    (dict(d_model=512, mlp_ratio=1.5), "d_model = 256"), (dict(depth=-1), "depth")])
def test_dual_classes_reject_setups_the_kernel_cannot_run(kw, why):
    """af_dual_branch_encoders takes 4..256 input features and dim_feedforward 4..768, each a multiple of 4, and a head
    count that divides 256: both drop-in classes refuse anything else when they are built, not at the first forward"""
    from af_mi355x import dualrun
    with pytest.raises(ValueError, match=re.escape(why)):
        dualrun.DualEncoderAU_LMK(**kw)
    rgb = dict(au_dim=36, lmk_dim=132, vis_dim=2048, ff_dim=3.0)
    rgb.update({"ff_dim" if k == "mlp_ratio" else k: v for k, v in kw.items()})
    with pytest.raises(ValueError, match=re.escape(why)):
        dualrun.DualEncoderRGB(**rgb)


def test_dual_classes_frame_limit_follows_the_head_count():
    """up to 32 heads fit LDS at 16 frames; 64..256 heads only at 8 (af_dual_branch_encoders' LDS check): such a module is
    built, and its forward refuses a longer clip with a ValueError (tests/test_hip_dual_configs.py)"""
    from af_mi355x import dualrun
    for heads, frames in ((1, 16), (4, 16), (32, 16), (64, 8), (256, 8)):
        assert dualrun.DualEncoderAU_LMK(heads=heads).max_frames == frames
        assert dualrun.DualEncoderRGB(36, 132, 2048, heads=heads, ff_dim=2.0).max_frames == frames
        assert dualrun._branch_lds_bytes(frames, heads) <= 160 * 1024
    assert dualrun._branch_lds_bytes(16, 64) > 160 * 1024
    ok = dualrun.DualEncoderAU_LMK(au_dim=4, lmk_dim=256, depth=0, heads=1, mlp_ratio=0.5)
    assert ok.spec.ff == 128 and ok.max_frames == 16


def test_last_linear_is_head_projection(clf):
    lin = [m for m in clf.modules() if isinstance(m, torch.nn.Linear)][-1]
    assert lin is clf.network.resnet.head.projection and lin.in_features == 2048 and lin.out_features == 1


def test_load_behaviour_table(clf):
    """Every row of tests/golden/f4_load.json was produced by the reference's ModelBase.load."""
    rows = {r["case"]: r for r in load_json("f4_load.json")["rows"]}
    base = synth.synthetic_state_dict(seed=3)
    probe, other = "resnet.head.projection.bias", "resnet.s1.pathway0_stem.bn.bias"
    with tempfile.TemporaryDirectory() as td:
        def run(name, obj=None, path=None, **kw):
            clf.load_state_dict({k: torch.zeros_like(v) for k, v in clf.state_dict().items()})
            p = path or os.path.join(td, name + ".pth")
            if obj is not None:
                torch.save(obj, p)
            ret = clf.load(p, **kw)
            cur = clf.network.state_dict()
            want = rows[name]
            assert list(ret) == want["ret"], name
            if "probe_loaded" in want:
                assert bool(torch.equal(cur[probe], base[probe])) == want["probe_loaded"], name
                assert bool(torch.equal(cur[other], base[other])) == want["other_loaded"], name

        run("raw", base)
        run("wrap_state_dict", {"state_dict": base, "epoch": 7})
        run("wrap_classifier_state_dict", {"classifier_state_dict": base})
        run("wrap_model_state_dict", {"model_state_dict": base})
        for pfx in ("module.", "network.", "_warped_network."):
            run("prefix_" + pfx.strip("._"), {pfx + k: v for k, v in base.items()})
        run("prefix_double", {"module.network." + k: v for k, v in base.items()})
        run("extra_key", dict(base, **{"resnet.extra.weight": torch.ones(3)}))
        run("missing_probe", {k: v for k, v in base.items() if k != probe})
        bad = dict(base)
        bad[probe] = torch.ones(5)
        run("shape_mismatch_probe", bad)
        run("missing_file", path=os.path.join(td, "does_not_exist.pth"))
        run("epoch_kw", base, epoch=12)
    assert clf.load() == (False, -1)                        # no path, no model_dir, no pretrained


def test_find_last_picks_highest_epoch():
    with tempfile.TemporaryDirectory() as td:
        c = Classifier(model_dir=td)
        sd = c.network.state_dict()
        for e in (3, 11, 7):
            torch.save(sd, os.path.join(td, "i3d_ori_%d.pth" % e))
        assert c.load() == (True, 11)
        assert c.load(epoch=7) == (True, 7)


def test_forward_contract_errors(clf):
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        clf(torch.zeros(1, 3, 32, 224, 224))
    with pytest.raises(ValueError):
        clf(torch.zeros(3, 32, 224, 224))
    with pytest.raises(AssertionError):
        clf(torch.zeros(1, 3, 32, 224, 224), freeze_backbone=True)


def test_fresh_init_matches_reference_policy():
    c = Classifier()
    n = c.network.resnet
    assert float(n.s2.pathway0_res0.branch2.c_bn.weight.abs().sum()) == 0.0      # ZERO_INIT_FINAL_BN
    assert float(n.s2.pathway0_res0.branch2.a_bn.weight.min()) == 1.0
    assert float(n.head.projection.bias.abs().sum()) == 0.0
    assert abs(float(n.head.projection.weight.std()) - 0.01) < 2e-3


def test_c_abi_exports_every_declared_symbol():
    from af_mi355x import _lib
    hdr = open(os.path.join(ROOT, "include", "af_hip.h")).read()
    hdr = re.sub(r"/\*.*?\*/", "", hdr, flags=re.S)
    declared = set(re.findall(r"\b(af_[a-z0-9_]+)\s*\(", hdr))
    assert declared == set(_lib.ABI), declared ^ set(_lib.ABI)
    for name in declared:
        assert hasattr(_lib.lib, name)
    assert _lib.lib.af_version() == _lib.AF_ABI_VERSION == int(re.search(r"#define AF_ABI_VERSION (\d+)", hdr).group(1))
    import ctypes as C
    assert C.sizeof(_lib.ConvDesc) == 21 * 4 and C.sizeof(_lib.PoolDesc) == 19 * 4


def test_abi_rejects_bad_arguments_without_a_gpu():
    from af_mi355x import _lib
    import ctypes as C
    d = _lib.ConvDesc()
    assert _lib.lib.af_conv3d_bn_act(C.byref(d), None, None, None, None, None, None, 0, None, 0, None) == -1
    assert b"null" in _lib.lib.af_last_error()
    assert _lib.lib.af_conv_workspace_bytes(C.byref(d)) == 0 and _lib.lib.af_conv_workspace_bytes(None) == 0
    assert _lib.lib.af_packed_conv_weight_bytes(64, 64, 1, 3, 3, 1) == 64 * 64 * 9 * 2
    assert _lib.lib.af_stem_input_bytes(1, 32, 224, 224, 0) == 36 * 230 * 232 * 4 * 4


def test_aligner_host_fit_matches_reference():
    """FasterCropAlignXRay's host side (similarity fit over all frames, landmark transform) against the vectors the
    reference's numpy code produced (tests/golden/f8_aligner.npz), incl. the mirrored clip that takes the reflective
    solution; the landmark-only call needs neither GPU nor library."""
    import numpy as np
    from conftest import load_npz
    from af_mi355x import aligner
    g = load_npz("f8_aligner.npz")
    np.testing.assert_allclose(aligner.STD_POINTS_256, g["std_points_256"], rtol=0, atol=1e-12)
    for tag, size in (("t32_224", 224), ("t1_256", 256), ("t8_mirrored", 224)):
        infos = [(None, a.copy(), b.copy(), c.copy()) for a, b, c in zip(g[tag + "_ldm5"], g[tag + "_ldm68"], g[tag + "_boxes"])]
        t5, t68 = aligner.FasterCropAlignXRay(size, return_ldm5=True)(infos)
        np.testing.assert_allclose(t5, g[tag + "_t5"], rtol=1e-10, atol=1e-9)
        np.testing.assert_allclose(t68, g[tag + "_t68"], rtol=1e-10, atol=1e-9)
        only68 = aligner.FasterCropAlignXRay(size)(infos)
        np.testing.assert_allclose(only68, g[tag + "_t68"], rtol=1e-10, atol=1e-9)
        boxes = g[tag + "_boxes"]
        diff = boxes[:, :2] - boxes[:, :2].min(0)[None]
        tfm, trans = aligner.estimate_batch_transform(g[tag + "_ldm5"] + diff[:, None, :], aligner.STD_POINTS_256 * size / 256.0)
        np.testing.assert_allclose(tfm, g[tag + "_tfm"], rtol=1e-10, atol=1e-10)
        np.testing.assert_allclose(trans, g[tag + "_trans"], rtol=1e-10, atol=1e-10)
    with pytest.raises(Exception, match="twoUniquePointsReq"):
        aligner.estimate_batch_transform(g["t1_256_ldm5"], np.zeros((5, 2)))       # rank-deficient targets (cp2tform's error)


def _desc(n, t, h, w, cin, cout, k, s, p, dtype=1, relu=1):
    from af_mi355x import _lib
    d = _lib.ConvDesc()
    d.n, d.t, d.h, d.w, d.cin, d.cout = n, t, h, w, cin, cout
    d.kt, d.kh, d.kw = k
    d.st, d.sh, d.sw = s
    d.pt, d.ph, d.pw = p
    d.to, d.ho, d.wo = [(a + 2 * pp - kk) // ss + 1 for a, pp, kk, ss in zip((t, h, w), p, k, s)]
    d.relu, d.dtype = relu, dtype
    return d


def test_kernel_selection_and_workspace_sizing_are_host_logic():
    """af_conv_variant / af_conv_workspace_bytes / af_conv_bc_fusable run on the host (no GPU): the s3 / s4 `b` convs take the
    frame-resident halo kernel at bench batch sizes and the generic kernel (+ split-K scratch) for a live call's one clip."""
    import ctypes as C
    from af_mi355x import _lib
    L = _lib.lib
    name = lambda d: L.af_conv_variant_name(L.af_conv_variant(C.byref(d), None)).decode()
    s4b = lambda n, dt=1: _desc(n, 16, 14, 14, 256, 256, (1, 3, 3), (1, 1, 1), (0, 1, 1), dt)
    s3b = lambda n: _desc(n, 16, 28, 28, 128, 128, (1, 3, 3), (1, 1, 1), (0, 1, 1))
    assert name(s4b(16)).startswith("conv133g") and name(s3b(16)).startswith("conv133g") and name(s3b(8)).startswith("conv133g")
    assert name(s4b(8)).startswith("conv_igemm") and name(s4b(1)).startswith("conv_igemm")      # 128 / 16 frames: too few units
    assert name(s4b(16, 0)).startswith("conv_igemm")                                            # fp32: generic kernel
    assert name(_desc(16, 16, 28, 28, 128, 128, (1, 3, 3), (1, 2, 2), (0, 1, 1))).startswith("conv_igemm")   # stride 2
    assert name(_desc(16, 32, 56, 56, 64, 64, (1, 3, 3), (1, 1, 1), (0, 1, 1))).startswith("conv133_c64")
    # round 4: the 3x1x1 `a` convs of s3 / s4 take the patch-resident kernel's temporal mode at bench batch sizes (>= 192 units of
    # (clip, P pixels, all frames)); one clip, fp32 and 512 output channels (s5) do not
    t311 = lambda n, hw, cin, cout, dt=1: _desc(n, 16, hw, hw, cin, cout, (3, 1, 1), (1, 1, 1), (1, 0, 0), dt)
    assert name(t311(16, 14, 1024, 256)).startswith("conv311g") and name(t311(16, 28, 512, 128)).startswith("conv311g")
    assert name(t311(16, 56, 256, 128)).startswith("conv311g") and name(t311(16, 28, 512, 256)).startswith("conv311g")
    assert not name(t311(1, 14, 1024, 256)).startswith("conv311g") and not name(t311(16, 14, 1024, 256, 0)).startswith("conv311g")
    assert name(t311(16, 7, 2048, 512)).startswith("conv_igemm")
    # SlowFast's Slow pathway at bench size (T = 4: P = 56, a (4 + 2) x 56 = 336-row patch) is more than the five DMA pieces per wave of
    # the 256-channel instantiation cover: the predicate must say no (round 4: it said yes and the bench's launch failed)
    assert not name(_desc(16, 4, 28, 28, 512, 256, (3, 1, 1), (1, 1, 1), (1, 0, 0))).startswith("conv311g")
    # the long-K 1x1x1 `a` convs of s4 (positions = a multiple of 49: 14x14 frames): 224-row tiles = 224 workgroups instead of 196
    s4a = _desc(16, 16, 14, 14, 1024, 256, (1, 1, 1), (1, 1, 1), (0, 0, 0))
    assert name(s4a) == "conv_igemm<BN=256,BM=224>"
    os.environ["AF_IGEMM_224"] = "0"
    try:
        assert name(s4a) == "conv_igemm<BN=256,BM=256>"
    finally:
        del os.environ["AF_IGEMM_224"]
    assert name(_desc(16, 16, 16, 16, 1024, 256, (1, 1, 1), (1, 1, 1), (0, 0, 0))) == "conv_igemm<BN=256,BM=256>"   # 65 536 positions
    # split-K scratch: one clip in s4 / s5 splits, a full batch does not
    assert L.af_conv_workspace_bytes(C.byref(s4b(1))) > 0 and L.af_conv_workspace_bytes(C.byref(s4b(16))) == 0
    s5b = _desc(1, 16, 7, 7, 512, 512, (1, 3, 3), (1, 1, 1), (0, 1, 1))
    assert L.af_conv_workspace_bytes(C.byref(s5b)) == 4 * 784 * 512 * 4                        # 56 tiles -> 4 K ranges of fp32 partial sums
    # b + c fusion is offered exactly where the halo kernel runs and c is a plain 1x1x1 over b's output
    c4 = lambda n: _desc(n, 16, 14, 14, 256, 1024, (1, 1, 1), (1, 1, 1), (0, 0, 0))
    assert L.af_conv_bc_fusable(C.byref(s4b(16)), C.byref(c4(16))) == 1
    assert L.af_conv_bc_fusable(C.byref(s4b(1)), C.byref(c4(1))) == 0
    assert L.af_conv_bc_fusable(C.byref(s4b(16)), C.byref(_desc(16, 16, 14, 14, 128, 1024, (1, 1, 1), (1, 1, 1), (0, 0, 0)))) == 0


def test_rgb3_stem_sizes():
    from af_mi355x import _lib
    L = _lib.lib
    row = ((224 + 8) * 6 + 15) // 16 * 16
    assert L.af_stem_input_bytes_rgb3(1, 32, 224, 224, 1) == (36 * 230 + 8) * row
    assert L.af_packed_stem_weight_bytes_rgb3(5, 1) == 27 * 4 * 64 * 16 and L.af_packed_stem_weight_bytes_rgb3(1, 2) == 6 * 4 * 64 * 16
    assert L.af_stem_input_bytes_rgb3(1, 32, 224, 224, 0) < 0                                  # fp32 keeps the 4-channel layout


def test_conv_ca_is_not_offered_where_its_lds_does_not_fit():
    """af_conv_ca_fusable must agree with what conv_ca_run can launch: the fused c -> a pair needs 2 a-weight slots + 3 image
    slots (plain) or 1 image slot + both c-side weight sets (projection); with a 512-wide trunk that is > 160 KB and the
    engine has to keep the two launches (it used to plan the fused op and fail every forward with AF_ERR_ARG)."""
    import ctypes as C
    from af_mi355x import _lib
    L = _lib.lib
    c = lambda cout, t=32: _desc(64, t, 56, 56, 64, cout, (1, 1, 1), (1, 1, 1), (0, 0, 0))
    a = lambda cin, t=32: _desc(64, t, 56, 56, cin, 64, (3, 1, 1), (1, 1, 1), (1, 0, 0))
    b1 = lambda cout, t=32: _desc(64, t, 56, 56, 64, cout, (1, 1, 1), (1, 1, 1), (0, 0, 0), relu=0)
    assert L.af_conv_ca_fusable(C.byref(c(256)), None, C.byref(a(256))) == 1                      # s2 as shipped
    assert L.af_conv_ca_fusable(C.byref(c(256)), C.byref(b1(256)), C.byref(a(256))) == 1
    assert L.af_conv_ca_fusable(C.byref(c(512, 16)), None, C.byref(a(512, 16))) == 1              # 160 256 B since the image slots share their padding frames (round 4; 164 352 before)
    assert L.af_conv_ca_fusable(C.byref(c(512)), C.byref(b1(512)), C.byref(a(512))) == 0          # > 217 KB
    assert L.af_conv_ca_fusable(C.byref(c(1024, 16)), None, C.byref(a(1024, 16))) == 0
    assert L.af_conv_ca_fusable(C.byref(c(1024)), None, C.byref(a(1024))) == 1                    # T = 32 (8-pixel tiles): 160 256 B fits


def test_self_launch_returns_quickly_when_a_rank_dies():
    """bench.self_launch polls ALL children: rank 1 dies at start-up (AF_BENCH_FAIL_RANK), rank 0 would wait in the
    rendezvous for the process-group timeout - the parent must terminate it, relay the failure and return 1 in seconds."""
    import subprocess
    import sys
    import time
    env = dict(os.environ, AF_BENCH_FAIL_RANK="1", AF_BENCH_REHEARSAL="1")
    t0 = time.time()
    p = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "2", "--steps", "1", "--warmup", "0", "--cpu-clips", "0",
                        "--no-roofline"], env=env, capture_output=True, timeout=120)
    dt = time.time() - t0
    assert p.returncode == 1, (p.returncode, p.stderr.decode()[-2000:])
    assert b"rank 1 exited with code 3" in p.stderr and p.stdout.strip() == b""
    assert dt < 30.0, dt                                            # (python + torch start-up of the children included)


@pytest.mark.parametrize("args", [["--steps", "0"], ["--model", "aligner", "--dump-outputs", "unused"]])
def test_bench_rejects_arguments_it_cannot_honour(args):
    """bench.py refuses, before it touches a GPU, a run with no timed step and --dump-outputs on a model that does not dump."""
    import subprocess
    import sys
    p = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py")] + args, capture_output=True, timeout=120)
    assert p.returncode == 2 and p.stdout.strip() == b"", p.stderr.decode()[-2000:]
    assert b"error:" in p.stderr


def _device_asm(src):
    """gfx950 assembly of one .hip source (device side only; no GPU needed)"""
    import subprocess
    out = subprocess.run(["/opt/rocm/bin/hipcc", "--offload-arch=gfx950", "-O3", "-std=c++17", "--offload-device-only", "-S", "-o", "-", src],
                         capture_output=True, timeout=600)
    assert out.returncode == 0, out.stderr.decode()[-2000:]
    return out.stdout.decode()


_ASM_CACHE = {}


def _all_device_asm():
    """{file: gfx950 assembly} of every kernel source, compiled once per test session (~1 min on 6 threads)"""
    if not _ASM_CACHE:
        from concurrent.futures import ThreadPoolExecutor
        csrc = os.path.join(ROOT, "spatiotemporal-deepfake-detection-for-live-video-calls_amd", "csrc")
        files = sorted(f for f in os.listdir(csrc) if f.endswith(".hip"))
        with ThreadPoolExecutor(max_workers=6) as ex:
            _ASM_CACHE.update(zip(files, ex.map(lambda f: _device_asm(os.path.join(csrc, f)), files)))
    return _ASM_CACHE


def _regs_of(text):
    regs = set()
    for m in re.finditer(r"\bv\[(\d+):(\d+)\]|\bv(\d+)\b", text):
        if m.group(3) is not None:
            regs.add(int(m.group(3)))
        else:
            regs.update(range(int(m.group(1)), int(m.group(2)) + 1))
    return regs


def test_hand_counted_vmcnt_kernels_have_no_spills_and_no_early_use_of_uncounted_loads():
    """Build-time guard for the kernels whose vector-memory waits are hand counted (LDS-DMA + inline-asm loads that hipcc
    does not see): (1) no kernel of the library spills or uses scratch - a scratch reload's vmcnt(0), or a
    spilled destination of an in-flight load, would break the counts silently; (2) between every inline-asm register load
    (`bload16_nt_uncounted` / `gload16_uncounted`: a buffer / global load inside an ASMSTART block, without `lds`) and the
    next `s_waitcnt vmcnt` in straight-line code, no instruction reads or writes its destination registers (a phi copy or
    v_mov of a pending register would read stale data)."""
    asms = _all_device_asm()
    n_kernels = n_loads = 0
    for f, asm in asms.items():
        names = re.findall(r"^\s*\.name:\s+(\S+)$", asm, re.M)
        spills = [int(v) for v in re.findall(r"\.vgpr_spill_count:\s+(\d+)", asm)]
        scratch = [int(v) for v in re.findall(r"^\s*\.private_segment_fixed_size:\s+(\d+)", asm, re.M)]
        kernels = [n for n in names if n.startswith("_Z")]
        n_kernels += len(spills)
        if not spills:
            continue                                            # a file without kernels (af_api.hip: the op-list runner)
        assert len(spills) == len(scratch), f
        # a spilling kernel is tolerated only if every vector-memory wait in it is a full drain (vmcnt(0)): then a scratch
        # reload cannot be miscounted (conv133g's b + c fused instantiation - off by default - is such a kernel)
        counted = set()
        for seg in re.split(r"^\.Lfunc_end\d+:", asm, flags=re.M):
            lab = re.findall(r"^(_Z\w+):", seg, re.M)
            if lab and re.search(r"s_waitcnt vmcnt\(([1-9]\d*)\)", "\n".join(
                    b for b in re.findall(r";;#ASMSTART(.*?);;#ASMEND", seg, re.S))):
                counted.add(lab[-1])
        bad = [(k, s, p) for k, s, p in zip(kernels, spills, scratch) if (s or p) and k in counted]
        assert not bad, "%s: kernels with hand-counted vmcnt waits AND VGPR spills / scratch: %s" % (f, bad)
        n_counted = locals().get("n_counted", 0) + len(counted)
        lines = asm.splitlines()
        in_asm = False
        for i, ln in enumerate(lines):
            t = ln.strip()
            if t.startswith(";;#ASMSTART"):
                in_asm = True
                continue
            if t.startswith(";;#ASMEND"):
                in_asm = False
                continue
            if not in_asm or " lds" in t or not re.match(r"(buffer|global)_load_dword", t):
                continue
            n_loads += 1
            dest = _regs_of(t.split(",")[0])
            assert dest, t
            for j in range(i + 1, len(lines)):
                u = lines[j].strip()
                if not u or u.startswith(";") or u.startswith("."):
                    continue                                    # (labels: the scan follows the fall-through path across them)
                if u.startswith("s_waitcnt") and "vmcnt" in u:
                    break
                if u.startswith(("s_branch", "s_endpgm", "s_setpc")):
                    break                                       # conditional branches: the not-taken path continues below
                # the address operand of ANOTHER load may reuse no destination register either; any mention counts
                hit = dest & _regs_of(u)
                assert not hit, "%s: v%s is the destination of a pending uncounted load (line %d: %s) but is touched by line %d: %s" % (
                    f, sorted(hit), i + 1, t, j + 1, u)
    assert n_counted >= 10, n_counted                              # ... including the kernels with counted waits
    assert n_kernels >= 40 and n_loads >= 8, (n_kernels, n_loads)   # the lint saw the kernels / loads it is meant for


def test_asm_statement_mfmas_and_lds_reads_are_not_crowded_by_compiler_code():
    """Round 4: the MFMA-bound K loops issue their MFMAs and LDS fragment reads as asm statements (af_common.h: MmaAsm,
    lds_read16_uncounted).  hipcc pads the hazards of its own MFMAs and counts its own LDS reads; around an asm statement it does
    neither, so the generated code is checked instead:
    (1) no vector-ALU instruction writes an operand register of an asm MFMA within the two instructions in front of it (what hipcc
        made of "acc = 0" before acc_live(): v_mov zero, zero, MFMA - whole-network f16 logits moved by 2e-3, run to run);
    (2) between an asm ds_read_b128 and the next s_waitcnt that names lgkmcnt on the fall-through path, nothing mentions its
        destination registers (a copy or a reuse of a fragment register whose data has not landed)."""
    n_mfma = n_reads = 0
    for f, asm in _all_device_asm().items():
        lines = [ln.split(";")[0].strip() if not ln.strip().startswith(";;#") else ln.strip() for ln in asm.splitlines()]
        in_asm = False
        hist = []                                                  # the last instructions: (inside an asm block?, text)
        for i, t in enumerate(lines):
            if t.startswith(";;#ASMSTART"):
                in_asm = True
                continue
            if t.startswith(";;#ASMEND"):
                in_asm = False
                continue
            if not t or t.startswith(".") or t.endswith(":"):
                if t.endswith(":") and t.startswith("_Z"):
                    hist = []
                continue
            if in_asm and t.startswith("v_mfma"):
                n_mfma += 1
                srcs = _regs_of(t.split(None, 1)[1].split(",", 1)[1])         # A, B, C (C = the destination registers)
                for was_asm, u in hist[-2:]:
                    if u.startswith("v_") and not u.startswith(("v_mfma", "v_cmp")):
                        hit = _regs_of(u.split(None, 1)[1].split(",")[0]) & srcs
                        assert not hit, "%s: v%s written by `%s` right in front of the asm MFMA `%s`" % (f, sorted(hit), u, t)
            if in_asm and t.startswith("ds_read_b128"):
                n_reads += 1
                dest = _regs_of(t.split(None, 1)[1].split(",")[0])
                for j in range(i + 1, len(lines)):
                    u = lines[j]
                    if not u or u.startswith((".", ";;#")) or u.endswith(":"):
                        continue
                    if u.startswith("s_waitcnt") and "lgkmcnt" in u:
                        break
                    if u.startswith(("s_branch", "s_endpgm", "s_setpc")):
                        break
                    if u.startswith("ds_read_b128") and not (dest & _regs_of(u)):
                        continue
                    hit = dest & _regs_of(u)
                    assert not hit, "%s: v%s is the destination of a pending asm LDS read (line %d: %s) but line %d touches it: %s" % (
                        f, sorted(hit), i + 1, t, j + 1, u)
            hist.append((in_asm, t))
    assert n_mfma >= 1000 and n_reads >= 500, (n_mfma, n_reads)     # the lint saw the loops it is meant for


def test_kernel_sources_read_exactly_the_three_product_knobs():
    """The shipped library reads three environment names, all in host-side selection code and all flipped by tests: AF_FORCE_VAR,
    AF_IGEMM_224, AF_ABC_INNER32.  A kernel form is not chosen through the environment (two forms are compared as two libraries),
    and the diagnostic build's knobs live in af_common.h under AF_STAMPS - so a new env_int / getenv of an AF_ name in a kernel
    source is a decision to take here, not an accident.  Source text only: no compiler."""
    csrc = os.path.join(ROOT, "spatiotemporal-deepfake-detection-for-live-video-calls_amd", "csrc")
    files = sorted(f for f in os.listdir(csrc) if f.endswith(".hip"))
    assert len(files) >= 20, files
    names = {}
    for f in files:
        with open(os.path.join(csrc, f)) as fh:
            for m in re.finditer(r'\b(?:env_int|getenv)\s*\(\s*"(AF_\w+)"', fh.read()):
                names.setdefault(m.group(1), []).append(f)
    assert set(names) == {"AF_FORCE_VAR", "AF_IGEMM_224", "AF_ABC_INNER32"}, names


def test_stage_rows_host_helper_matches_numpy():
    """af_stage_rows_u8 is host code (the aligner's copy of the sampled crop rows into its pinned staging buffer): contiguous and
    strided rectangles against numpy, a refused rectangle (pitch smaller than the row)."""
    import ctypes as C
    import numpy as np
    from af_mi355x import _lib
    rng = np.random.default_rng(5)
    imgs = [rng.integers(0, 256, size=(h, w, 3), dtype=np.uint8) for h, w in ((37, 53), (64, 64), (5, 301))]
    views = [imgs[0].reshape(37, -1), imgs[1][10:50].reshape(40, -1)[:, 12:150], imgs[2].reshape(5, -1)[:, 3:900]]
    offs, total = [], 0
    for v in views:
        offs.append(total)
        total += (v.size + 15) // 16 * 16
    dst = np.full(total, 7, dtype=np.uint8)
    rects = (_lib.StageRect * len(views))()
    for i, (v, o) in enumerate(zip(views, offs)):
        rects[i] = _lib.StageRect(v.ctypes.data, o, v.strides[0], v.shape[0], v.shape[1])
    _lib.check(_lib.lib.af_stage_rows_u8(C.c_void_p(dst.ctypes.data), rects, len(views)), "stage_rows_u8")
    for v, o in zip(views, offs):
        assert np.array_equal(dst[o:o + v.size].reshape(v.shape), v)
    bad = (_lib.StageRect * 1)(_lib.StageRect(views[1].ctypes.data, 0, 10, 4, 138))
    assert _lib.lib.af_stage_rows_u8(C.c_void_p(dst.ctypes.data), bad, 1) != 0


def _row_cut(images, diff, tfm, size):
    """the rectangle of the canvas the size x size destination can sample (bilinear taps, fixed-point rounding: 3 pixels of margin)
    -> per frame the rows of the crop inside it (a rows x bytes view, no copy), their (h, w, 3) shape and the paste offset moved
    accordingly: the aligner's per-frame planning as Python did it before af_align_plan_u8"""
    import numpy as np
    m = np.asarray(tfm, dtype=np.float64).reshape(2, 3)
    det = m[0, 0] * m[1, 1] - m[0, 1] * m[1, 0]
    if not np.isfinite(det) or abs(det) < 1e-12:
        return images, [im.shape for im in images], diff     # singular map: OpenCV's D = 0 path samples around one point; keep everything
    s = float(size - 1)
    corners = np.array([[0.0, 0.0], [s, 0.0], [0.0, s], [s, s]])
    # dst = M [x y 1]^T  ->  src = M^-1 (dst - t)
    dx, dy = corners[:, 0] - m[0, 2], corners[:, 1] - m[1, 2]
    xs = (m[1, 1] * dx - m[0, 1] * dy) / det
    ys = (-m[1, 0] * dx + m[0, 0] * dy) / det
    if not (np.isfinite(xs).all() and np.isfinite(ys).all()):
        return images, [im.shape for im in images], diff
    ylo, yhi = int(np.floor(ys.min())) - 3, int(np.ceil(ys.max())) + 4
    out_images, shapes, out_diff = [], [], np.array(diff, dtype=np.int64, copy=True)
    for i, im in enumerate(images):
        x0, y0 = int(out_diff[i][0]), int(out_diff[i][1])
        r0, r1, c1 = max(0, ylo - y0), min(im.shape[0], yhi - y0), im.shape[1]
        if r1 <= r0:                                          # the warp never reaches this crop: one pixel keeps the frame table valid
            r0, r1, c1 = 0, 1, 1
        rows = im[r0:r1]
        if rows.flags.c_contiguous:
            out_images.append(rows.reshape(r1 - r0, im.shape[1] * 3)[:, :c1 * 3])
        else:
            out_images.append(np.ascontiguousarray(rows[:, :c1]).reshape(r1 - r0, c1 * 3))
        shapes.append((r1 - r0, c1, 3))
        out_diff[i][0], out_diff[i][1] = x0, y0 + r0
    return out_images, shapes, out_diff


def test_align_plan_host_helper_matches_the_python_path():
    """af_align_plan_u8 is host code (round 4: the aligner's per-frame planning - canvas fit, row cut, staging table, frame table - as
    one C call): same tables as the Python path it replaced (_row_cut below + FasterCropAlignXRay._layout + launch_warps' frame
    table) for a random clip, for a singular transform (nothing is cut), and the reference's ValueError case (a crop that sticks out)."""
    import ctypes as C
    import numpy as np
    from af_mi355x import _lib, aligner
    rng = np.random.default_rng(3)
    n, H, W = 9, 300, 280
    images, diff = [], []
    for i in range(n):
        ih, iw = int(rng.integers(120, 200)), int(rng.integers(100, 180))
        images.append(rng.integers(0, 256, size=(ih, iw, 3), dtype=np.uint8))
        diff.append((int(rng.integers(0, W - iw)), int(rng.integers(0, H - ih))))
    diff = np.array(diff, dtype=np.int64)
    for tfm in (np.array([[0.9, 0.2, -30.0], [-0.2, 0.9, 10.0]]), np.array([[1.0, 2.0, 3.0], [2.0, 4.0, 5.0]])):   # regular, singular
        cut, shapes, d2 = _row_cut(images, diff, tfm, 224)
        offs, total = aligner.FasterCropAlignXRay._layout(cut)
        crops = (_lib.AlignCrop * n)(*[_lib.AlignCrop(im.ctypes.data, im.strides[0], im.shape[0], im.shape[1], int(diff[i][0]), int(diff[i][1]))
                                       for i, im in enumerate(images)])
        rects, frames = (_lib.StageRect * n)(), (_lib.AlignFrame * n)()
        tot, bad = C.c_int64(0), C.c_int32(-1)
        m = (C.c_double * 6)(*tfm.reshape(6).tolist())
        _lib.check(_lib.lib.af_align_plan_u8(crops, n, H, W, m, 224, rects, frames, C.byref(tot), C.byref(bad)), "align_plan_u8")
        assert tot.value == total and bad.value == -1
        for i in range(n):
            assert (frames[i].offset, frames[i].ih, frames[i].iw, frames[i].x, frames[i].y) == (offs[i], shapes[i][0], shapes[i][1], int(d2[i][0]), int(d2[i][1]))
            assert (rects[i].dst_offset, rects[i].rows, rects[i].row_bytes) == (offs[i], shapes[i][0], shapes[i][1] * 3)
            assert rects[i].src == cut[i].ctypes.data
        # ... and the staged bytes are the same picture
        dst = np.zeros(total, dtype=np.uint8)
        _lib.check(_lib.lib.af_stage_rows_u8(C.c_void_p(dst.ctypes.data), rects, n), "stage_rows_u8")
        for i in range(n):
            assert (dst[offs[i]:offs[i] + cut[i].size] == np.ascontiguousarray(cut[i]).reshape(-1)).all()
    crops[4].x = W - images[4].shape[1] + 1                                    # one pixel over the right edge of the canvas
    rc = _lib.lib.af_align_plan_u8(crops, n, H, W, m, 224, rects, frames, C.byref(tot), C.byref(bad))
    assert rc != 0 and bad.value == 4


def _reference_fit(infos, std_points):
    """faster_crop_align_xray.py:21-66 up to the transform, as FasterCropAlignXRay.__call__, StreamingCropAligner.align_last and the
    evaluator's per-window fit each had it written out"""
    import numpy as np
    from af_mi355x import aligner
    boxes = np.array([box for _, _, _, box in infos])
    five = np.array([l5 for _, l5, _, _ in infos])
    left_top = boxes[:, :2].min(0)
    w, h = boxes[:, 2:].max(0) - left_top
    diff = boxes[:, :2] - left_top[None]
    tfm, trans = aligner.estimate_batch_transform(five + diff[:, None, :], std_points)
    return tfm, trans, h, w, diff


def test_fit_window_is_the_arithmetic_its_three_copies_had():
    """aligner.fit_window against that arithmetic: the same float64 operations in the same order, so equality is exact"""
    import numpy as np
    from af_mi355x import aligner
    std = aligner.STD_POINTS_256 * 224 / 256.0
    clips = [aligner.synthetic_clip(8, seed=0)[0], aligner.synthetic_clip(8, seed=1, mirrored=True)[0], aligner.synthetic_clip(1, seed=2)[0]]
    mirrored = []
    for infos in clips:
        want = _reference_fit(infos, std)
        got = aligner.fit_window(np.array([i[3] for i in infos]), np.array([i[1] for i in infos]), std)
        assert len(got) == 5
        for g, w_ in zip(got, want):
            assert np.asarray(g).dtype == np.asarray(w_).dtype and np.array_equal(g, w_)
        assert got[0].dtype == got[1].dtype == np.float64 and got[0].shape == (2, 3) and got[4].shape == (len(infos), 2)
        mirrored.append(bool(np.linalg.det(got[0][:, :2]) < 0))
        # ... and the callers hand on what it gives: the landmarks through `trans`
        t68 = aligner.FasterCropAlignXRay(224)(infos)
        assert np.array_equal(t68, aligner._apply(want[1], np.array([i[2] for i in infos]) + want[4][:, None, :]))
    assert mirrored == [False, True, False]                     # the second clip takes the reflective solution


def test_stage_rects_and_crop_rect_against_numpy(monkeypatch):
    """_staging.crop_rect + stage_rects into numpy memory: packed views are copied from where they are (a column slice keeps its
    larger pitch), a channel-reversed view through a contiguous copy, a one-row crop with pitch = row bytes; once in a single
    call and once with the size threshold down so that the two copy threads each take a part.  Every byte of every crop at its
    offset, and no byte between the crops touched."""
    import ctypes as C
    import numpy as np
    from af_mi355x import _lib, _staging
    rng = np.random.default_rng(17)
    wide = rng.integers(0, 256, size=(70, 140, 3), dtype=np.uint8)
    crops = [rng.integers(0, 256, size=(60, 50, 3), dtype=np.uint8),
             rng.integers(0, 256, size=(66, 58, 3), dtype=np.uint8)[:, :, ::-1],      # channel-reversed view
             wide[:, 30:110],                                                          # packed pixels, larger pitch
             rng.integers(0, 256, size=(90, 70, 3), dtype=np.uint8)[10:11],           # one row
             rng.integers(0, 256, size=(90, 70, 3), dtype=np.uint8)]
    assert [_staging.packed_rgb(c) for c in crops] == [True, False, True, True, True] and not crops[2].flags.c_contiguous
    assert all(_staging.is_crop(c) for c in crops) and not _staging.is_crop(crops[0].astype(np.int8)) and not _staging.is_crop(crops[0][..., 0])
    offs, total = [], 48                                         # gaps in front of, between and behind the crops
    for c in crops:
        offs.append(total)
        total += (c.size + 15) // 16 * 16 + 32
    rects, keep = (_lib.StageRect * len(crops))(), []
    for i, (c, o) in enumerate(zip(crops, offs)):
        (address, pitch, rows, row), kept = _staging.crop_rect(c)
        assert (rows, row) == (c.shape[0], c.shape[1] * 3) and (kept is c) == _staging.packed_rgb(c)
        assert pitch == (row if rows == 1 else kept.strides[0]) and address == kept.ctypes.data
        keep.append(kept)
        rects[i] = _lib.StageRect(address, o, pitch, rows, row)
    assert rects[2].src_pitch == 140 * 3 and rects[2].src == wide.ctypes.data + 90 and rects[3].src_pitch == 70 * 3
    assert sum(c.size for c in crops) < _staging._SPLIT_BYTES   # as it is: one call

    def staged(expect_split):
        parts = []
        real = _lib.lib.af_stage_rows_u8
        monkeypatch.setattr(_lib.lib, "af_stage_rows_u8", lambda base, r, n: parts.append(n) or real(base, r, n))
        dst = np.full(total, 0xA5, dtype=np.uint8)
        _staging.stage_rects(dst.ctypes.data, rects, len(crops), total)
        monkeypatch.setattr(_lib.lib, "af_stage_rows_u8", real)
        assert sorted(parts) == ([2, 3] if expect_split else [5])
        untouched = np.ones(total, dtype=bool)
        for c, o in zip(crops, offs):
            assert np.array_equal(dst[o:o + c.size], np.ascontiguousarray(c).reshape(-1))
            untouched[o:o + c.size] = False
        assert (dst[untouched] == 0xA5).all() and untouched.sum() >= 48 + 32 * len(crops)

    staged(False)
    monkeypatch.setattr(_staging, "_SPLIT_BYTES", 1 << 10)
    staged(True)
    assert str(_staging.cuda_device("cpu")) == "cpu"            # only a CUDA device without an index is filled in


def _kinds(text):
    """'conv*2 ca' -> ['conv', 'conv', 'ca']"""
    out = []
    for word in text.split():
        kind, _, n = word.partition("*")
        out += [kind] * int(n or 1)
    return out


# launch kinds of the bf16 plans at 16 clips of 32 x 224 x 224, default switches (name*n = n launches in a row)
PLAN_KINDS = {
    "i3d_r50": "stem3_pool conv*2 ca conv ca conv*4 dual conv*11 dual conv*17 dual conv*6 head",
    "slowfast_r50": "stem3_pool stem pool conv*3 dual conv*6 abc*3 conv*3 dual conv*11 dual abc*3 conv*3 dual conv*17 dual conv*18 dual "
                    "conv*8 dual conv*6 avgpool*2 linear",
    "ftcn_tt": "tstem_pool3 conv*2 ca conv ca conv*34 tt_head",
}
PLAN_KINDS_I3D_CPA = "stem3_pool conv*2 ca conv ca conv cpa conv dual conv*11 dual conv*17 dual conv*6 head"


def _main_and_shortcut(launch):
    """(the conv, its projection shortcut or None) of a `conv` / `dual` launch"""
    return (launch.convs["c"], launch.convs["branch1"]) if launch.kind == "dual" else (launch.convs["conv"], None)


def _load_tests_module(name):
    """a test module of this directory, for its CASES and case_key functions"""
    import importlib.util
    spec = importlib.util.spec_from_file_location(name, os.path.join(ROOT, "tests", name + ".py"))
    module = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(module)
    return module


def _gen_conv_paths_golden():
    import importlib.util
    spec = importlib.util.spec_from_file_location("gen_conv_paths_golden", os.path.join(ROOT, "tools", "gen_conv_paths_golden.py"))
    gen = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(gen)
    return gen


def test_plans_need_no_device_and_keep_their_launch_kinds(monkeypatch):
    """planning is host logic (spec + the library's *_fusable predicates): a drifting switch default or fusion decision shows up
    here as a changed sequence of launch kinds"""
    import plan_cases
    from af_mi355x import engine
    plan_cases.set_switches(monkeypatch, {})
    for net, want in PLAN_KINDS.items():
        p = plan_cases.plan(net, "bf16", 16)
        assert [launch.kind for launch in p.launches] == _kinds(want), net
        assert p.rgb3 == (net == "i3d_r50") and p.rgb3_inputs == ({"IN_S"} if net == "slowfast_r50" else set())
        assert len(p.inputs) == (2 if net == "slowfast_r50" else 1) and p.head_dims is not None and p.head_width > 0
    assert engine.SWITCHES == {"AF_FUSE_BC": False, "AF_FUSE_CA": True, "AF_FUSE_CPA": False, "AF_FUSE_ABC": True,
                               "AF_FUSE_TSTEM_POOL": True, "AF_SLOWFAST_STEM3": True}
    monkeypatch.setenv("AF_FUSE_CPA", "1")           # read when the plan is built
    assert [launch.kind for launch in plan_cases.plan("i3d_r50", "bf16", 16).launches] == _kinds(PLAN_KINDS_I3D_CPA)


def test_plans_equal_the_recorded_ones():
    """every launch plan of the three networks (f32 / bf16 / f16, batch 1 .. 32, default switches and each switch flipped) is the
    recorded one: launch kinds, every integer of every conv and pool descriptor, buffers, row strides, buffer sizes, inputs, head
    and the questions asked of the library (fixture: tests/golden/plan_launches.json, digests written by
    tools/gen_conv_paths_golden.py --launches)"""
    gen = _gen_conv_paths_golden()
    want, got = load_json("plan_launches.json"), gen.collect_launches()
    assert sorted(got) == sorted(want) == sorted(gen.LAUNCH_CONFIGS) and len(want) == 6
    for config in sorted(want):
        assert len(want[config]) == 3 * 3 * 10, config
        changed = sorted(key for key in set(want[config]) | set(got[config]) if want[config].get(key) != got[config].get(key))
        assert not changed, "%s: %d plans differ from the recorded ones: %s" % (config, len(changed), changed)
    # the settings differ where their switch acts
    assert want["AF_FUSE_CPA=1"]["i3d_r50/bf16/16"] != want["default"]["i3d_r50/bf16/16"]
    assert want["unfused"]["ftcn_tt/bf16/16"] != want["default"]["ftcn_tt/bf16/16"]


def test_conv_paths_and_fusion_answers_equal_the_recorded_ones():
    """for every conv of the three networks (f32 / bf16 / f16, batch 1 / 8 / 16) af_conv_variant gives the recorded id, the id has the
    recorded name and af_conv_workspace_bytes the recorded size; the engine's bc / ca / cpa / abc fusion questions get the recorded
    answers in the recorded order (fixture: tests/golden/conv_paths.json, written by tools/gen_conv_paths_golden.py).  How the
    launches are cut is recorded as well (tests/golden/conv_work_units.json, same tool): per conv what af_conv_work_units returns
    - variant, units, workgroups, or its refusal in words -, per fusion answered yes what the pair's *_work_units function says."""
    gen = _gen_conv_paths_golden()
    got_work = {}
    want, got, want_work = load_json("conv_paths.json"), gen.collect(got_work), load_json("conv_work_units.json")
    assert sorted(got) == sorted(want) and len(want) == 3 * 3 * 3
    assert sorted(got_work) == sorted(want) and sorted(want_work) == sorted(want)
    for key in sorted(want):
        assert got[key]["convs"] == want[key]["convs"], key
        assert got[key]["fusable"] == want[key]["fusable"], key
        assert len(want[key]["convs"]) >= 40 and len(want[key]["fusable"]) >= 10, key
        assert got_work[key]["convs"] == want_work[key]["convs"], key
        assert got_work[key]["fused"] == want_work[key]["fused"], key
        assert len(want_work[key]["convs"]) == len(want[key]["convs"]), key
        assert len(want_work[key]["fused"]) == sum(yes for _, yes in want[key]["fusable"]), key
        # the recorded variant of a launch that is cut into units is the one af_conv_variant gave
        assert all(w[0] == c[1] for w, c in zip(want_work[key]["convs"], want[key]["convs"]) if w[0] >= 0), key
    assert sum(len(v["fused"]) for v in want_work.values()) >= 60
    for key in sorted(want_work):                     # the narrow-layer path's refusal: SlowFast's Fast pathway at 16 bits, nowhere else
        refused = [w for w in want_work[key]["convs"] if w[0] < 0]
        assert bool(refused) == (key.startswith("slowfast_r50/") and "/f32/" not in key), key
        assert all("not cut into units" in w[1] for w in refused), key


def test_conv_matrix_covers_what_ships(monkeypatch):
    """every (conv_igemm tile, dtype, epilogue form, K-step class) that the three networks launch at batch 1..32 is a case of
    tests/test_hip_conv_matrix.py (which runs it against fp64 on the GPU): a new layer shape or pick_variant threshold that ships
    an untested pair fails here.  The plans are built with the fusions off, as tools/gen_conv_paths_golden.py builds them; form =
    (two inputs, residual, tpool, out_ld != cout, split-K); K-steps S class as S up to 6 and as S mod 6 beyond."""
    import plan_cases
    from af_mi355x._lib import lib
    matrix = _load_tests_module("test_hip_conv_matrix")
    covered = {matrix.case_key(c, dt) for dt in matrix.DTYPES for c in matrix.CASES if not c.nonfinite}
    monkeypatch.delenv("AF_FORCE_VAR", raising=False)
    shipped = {}
    for net, dtype, batch, _, p in plan_cases.plans(monkeypatch, [plan_cases.UNFUSED]):
        bk = 32 if dtype == "f32" else 64
        for launch in p.launches:
            if launch.kind not in ("conv", "dual"):
                continue
            cv, cv2 = _main_and_shortcut(launch)
            dual, refs = cv2 is not None, (launch.refs() + [None])[:2]
            tile = lib.af_conv_variant(*refs)
            if tile not in matrix.TILES:
                continue                                # a specialised kernel: its own tests pin the variant
            s = cv.kernel[0] * cv.kernel[1] * cv.kernel[2] * -(-cv.cin // bk) + (-(-cv2.cin // bk) if dual else 0)
            split = not dual and lib.af_conv_workspace_bytes(refs[0]) > 0
            form = (dual, launch.res is not None, launch.tpool, launch.ld != cv.cout, split)
            shipped.setdefault((tile, dtype, form, s if s <= 6 else ("big", s % 6)), "%s batch %d: %d -> %d %s, S = %d" % (
                net, batch, cv.cin, cv.cout, tuple(cv.kernel), s))
    assert len(shipped) >= 200, len(shipped)
    missing = sorted("%s (%s)" % (k, v) for k, v in shipped.items() if k not in covered)
    assert not missing, "%d shipped tile x form pairs without a matrix case:\n%s" % (len(missing), "\n".join(missing))


def test_persist_matrix_covers_what_ships(monkeypatch):
    """every conv the three networks launch on a persistent specialised kernel (conv311, conv133g, conv311g: variants 8, 11, 13) at
    batch 1..32 - default fusions, and the four fusion switches off - is a case of tests/test_hip_conv_persist.py, which runs it
    against fp64 on the GPU at the same number of rounds of units per workgroup: key = (variant, dtype, cout, kernel, K slabs, T of
    the temporal kernels or (h, w) of the spatial ones, rounds class).  (units, workgroups) come from af_conv_work_units, which
    answers for 256 CUs where there is no device."""
    import ctypes as C
    import plan_cases
    from af_mi355x._lib import lib
    matrix = _load_tests_module("test_hip_conv_persist")
    covered = {matrix.case_key(c, dt) for c in matrix.CASES for dt in c.dtypes if c.form != "nonfinite"}
    monkeypatch.delenv("AF_FORCE_VAR", raising=False)
    shipped = {}
    for net, dtype, batch, setting, p in plan_cases.plans(monkeypatch, [{}, plan_cases.UNFUSED]):
        for launch in p.launches:
            if launch.kind != "conv":
                continue
            cv, (d,) = launch.convs["conv"], launch.descs
            v = lib.af_conv_variant(C.byref(d), None)
            if v not in (8, 11, 13):
                continue
            units, groups = C.c_int64(0), C.c_int(0)
            assert lib.af_conv_work_units(C.byref(d), None, C.byref(units), C.byref(groups)) == v
            assert 0 < groups.value <= 256 and groups.value == min(units.value, 256)
            key = (v, dtype, cv.cout, tuple(cv.kernel), matrix.kslabs(cv.cin, dtype), d.t if cv.kernel[1] == 1 else (d.h, d.w),
                   matrix.rounds_class(units.value, groups.value))
            shipped.setdefault(key, "%s batch %d%s: %d -> %d %s, %d units on %d workgroups" % (
                net, batch, setting, cv.cin, cv.cout, tuple(cv.kernel), units.value, groups.value))
    assert len(shipped) >= 60, len(shipped)
    missing = sorted("%s (%s)" % (k, v) for k, v in shipped.items() if k not in covered)
    assert not missing, "%d shipped persistent-kernel launches without a case:\n%s" % (len(missing), "\n".join(missing))


def test_fused_matrix_covers_what_ships(monkeypatch):
    """every fused conv launch of the three networks at batch 1..32 - kind `ca`, `abc` with the default switches, `cpa` under
    AF_FUSE_CPA=1, `bc` under AF_FUSE_BC=1 - is a case of tests/test_hip_conv_fused.py, which runs it against fp64 on the GPU in the
    same kernel form, at the same K-slab count and in the same class of tiles per workgroup (conv_ca, conv_cpa) or with the same
    patch rows and time segments (block_abc); the keys are that file's case_key().  How a launch is cut comes from
    af_conv_ca_work_units / af_conv_cpa_work_units / af_block_abc_work_units, which answer for 256 CUs where there is no device."""
    import collections
    import ctypes as C
    import hip_helpers as hh
    import plan_cases
    from af_mi355x._lib import lib
    matrix = _load_tests_module("test_hip_conv_fused")
    covered = {matrix.case_key(c, dt) for c in matrix.CASES for dt in c.dtypes}
    for name in ("AF_FORCE_VAR", "AF_ABC_INNER32"):
        monkeypatch.delenv(name, raising=False)
    ref = C.byref
    shipped, kinds = {}, collections.Counter()
    settings = [{}, {"AF_FUSE_CPA": "1"}, {"AF_FUSE_BC": "1"}]
    for net, dtype, batch, setting, p in plan_cases.plans(monkeypatch, settings, dtypes=("bf16", "f16")):
        for launch in p.launches:
            kind, convs = launch.kind, launch.convs
            if kind == "ca":
                cv, cv1, cv2 = convs["c"], convs["branch1"], convs["a_next"]
                dc = launch.descs[0]
                tiles, groups, form, pix = C.c_int64(0), C.c_int(0), C.c_int(-1), C.c_int(0)
                assert lib.af_conv_ca_work_units(*launch.refs(), ref(tiles), ref(groups), ref(form), ref(pix)) == 1
                assert groups.value == 256 and pix.value * dc.t == 256 and (form.value == 2) == (cv1 is not None)
                key = ("ca", hh.CA_FORMS[form.value], dtype, dc.t, cv.cout // 64, matrix.rounds_class(tiles.value, groups.value))
                what = "%d -> %d -> %d, %d tiles on %d workgroups" % (cv.cin, cv.cout, cv2.cout, tiles.value, groups.value)
            elif kind == "cpa":
                cv, cv2 = convs["c"], convs["a_next"]
                tiles, groups = C.c_int64(0), C.c_int(0)
                assert lib.af_conv_cpa_work_units(*launch.refs(), launch.x_sub, ref(tiles), ref(groups)) == 1
                assert groups.value == 256
                key = ("cpa", dtype, cv.cout // 64, launch.x_sub, matrix.rounds_class(tiles.value, groups.value))
                what = "%d -> %d -> %d, %d tiles on %d workgroups" % (cv.cin, cv.cout, cv2.cout, tiles.value, groups.value)
            elif kind == "abc":
                cv, cv3, cv4 = convs["a"], convs["c"], convs["branch1"]
                d = (launch.descs[0].t, launch.descs[0].h, launch.descs[0].w)
                rows, seg, units = C.c_int(0), C.c_int(0), C.c_int64(0)
                assert lib.af_block_abc_work_units(*launch.refs(), ref(rows), ref(seg), ref(units)) == 1
                assert units.value == batch * -(-d[1] // rows.value) * -(-d[2] // 14) * seg.value
                key = ("abc", cv.cout, cv.kernel[0], cv4 is not None, dtype, rows.value, seg.value)
                what = "%d -> %d, %s frames of %d x %d, %d units" % (cv.cin, cv3.cout, d[0], d[1], d[2], units.value)
            elif kind == "bc":
                cv, cv2 = convs["b"], convs["c"]
                db = launch.descs[0]
                assert lib.af_conv_bc_fusable(*launch.refs()) == 1
                key = ("bc", dtype, cv.cin, cv.cout, cv2.cout, (db.h, db.w))
                what = "%d -> %d -> %d" % (cv.cin, cv.cout, cv2.cout)
            else:
                continue
            kinds[kind] += 1
            shipped.setdefault(key, "%s batch %d%s: %s" % (net, batch, setting, what))
    # today 40 keys: 8 ca (plain-CWL and projection, T = 32, 4 slabs, classes "4-5" and ">5"), 4 cpa, 24 abc, 4 bc
    assert len(shipped) >= 40 and all(kinds[k] for k in ("ca", "cpa", "abc", "bc")), (len(shipped), kinds)
    missing = sorted("%s (%s)" % (k, v) for k, v in shipped.items() if k not in covered)
    assert not missing, "%d shipped fused launches without a case:\n%s" % (len(missing), "\n".join(missing))


def test_conv111_and_small_matrices_cover_what_ships(monkeypatch):
    """every `conv` and `dual` launch of the three networks at batch 1..32 - default fusions, and the four fusion switches off -
    that runs on the persistent 1x1x1 stream (conv111, variant 10) is a case of tests/test_hip_conv111.py, and every one on the
    narrow-layer path (conv_small, variant 9) a case of tests/test_hip_conv_small.py; both files run their cases against fp64 on
    the GPU.  conv111: key = (dtype, cin, cin2 or 0, cout, tpool, residual, out_ld != cout, my_tiles % NSLOT), one key per residue
    that occurs among the launch's workgroups - (tiles, workgroups) come from af_conv_work_units for (d, d2), which answers for
    256 CUs where there is no device.  conv_small: key = (dtype, cin, cout, kernel, stride, second segment, residual,
    out_ld != cout, M > 2 097 152: the grid-stride loop runs twice)."""
    import ctypes as C
    import plan_cases
    from af_mi355x._lib import lib
    m111, msmall = _load_tests_module("test_hip_conv111"), _load_tests_module("test_hip_conv_small")
    covered111 = set().union(*(m111.case_keys(c, dt) for c in m111.CASES for dt in m111.DT16 if c.form != "nonfinite"))
    covered_small = {msmall.case_key(c, dt) for c in msmall.CASES for dt in msmall.DT16 if c.form != "nonfinite" and c.variant == 9}
    monkeypatch.delenv("AF_FORCE_VAR", raising=False)
    shipped111, shipped_small = {}, {}
    for net, dtype, batch, setting, p in plan_cases.plans(monkeypatch, [{}, plan_cases.UNFUSED]):
        for launch in p.launches:
            if launch.kind not in ("conv", "dual"):
                continue
            cv, cv2 = _main_and_shortcut(launch)
            dual, refs, d = cv2 is not None, (launch.refs() + [None])[:2], launch.descs[0]
            v = lib.af_conv_variant(*refs)
            if v not in (9, 10):
                continue
            assert dtype != "f32"
            cin2, res, ld = cv2.cin if dual else 0, launch.res is not None, launch.ld != cv.cout
            where = "%s batch %d%s: %d%s -> %d %s" % (net, batch, setting, cv.cin, " + %d" % cin2 if dual else "", cv.cout, tuple(cv.kernel))
            if v == 9:
                m = d.n * d.to * d.ho * d.wo
                key = msmall.shipped_key(dtype, cv.cin, cv.cout, cv.kernel, cv.stride, dual, res, ld, m)
                shipped_small.setdefault(key, "%s stride %s, %d positions" % (where, tuple(cv.stride), m))
                continue
            tiles, groups = C.c_int64(0), C.c_int(0)
            assert lib.af_conv_work_units(*refs, C.byref(tiles), C.byref(groups)) == 10
            ncol = cv.cout // 256
            assert 0 < groups.value <= 256 and groups.value == 256 // ncol * ncol and tiles.value >= 4 * groups.value // ncol
            for residue in m111.residues_of(tiles.value, groups.value, cv.cin, cv.cout):
                key = m111.shipped_key(dtype, cv.cin, cin2, cv.cout, launch.tpool, res, ld, residue)
                shipped111.setdefault(key, "%s, %d tiles on %d workgroups" % (where, tiles.value, groups.value))
    # today 34 conv111 keys (17 per dtype: K = 128 with all four residues, and three of them with out_ld) and 24 conv_small keys (the
    # eight shapes, four of them also beyond the launch cap)
    assert len(shipped111) >= 34 and len(shipped_small) >= 24, (len(shipped111), len(shipped_small))
    assert any(k[-1] for k in shipped_small) and {k[-1] for k in shipped111 if k[1] == 128} == {0, 1, 2, 3}
    missing = sorted("%s (%s)" % (k, v) for k, v in shipped111.items() if k not in covered111)
    assert not missing, "%d shipped conv111 launches without a case in test_hip_conv111.py:\n%s" % (len(missing), "\n".join(missing))
    missing = sorted("%s (%s)" % (k, v) for k, v in shipped_small.items() if k not in covered_small)
    assert not missing, "%d shipped conv_small launches without a case in test_hip_conv_small.py:\n%s" % (len(missing), "\n".join(missing))


def test_stem_matrix_covers_what_ships(monkeypatch):
    """every stem launch of the three networks at batch 1..32 with the default switches - the first launch of every network - is a
    case of tests/test_hip_stem_matrix.py, which runs it against fp64 on the GPU in the same class.  The fused stems (stem3_pool,
    stem_pool): key = (kind, dtype, kT, 8-tile form, bands > 1, one-row last band, rounds class, unit map, out_ld != 64), with
    (units, bands, workgroups) from af_stem_work_units - the function the launchers take their bands and grid from -, which answers
    for 256 CUs where there is no device.  stem, tstem and tstem_pool3: key = (kind, dtype, kT, cout).  A change of the band rule,
    the CU count or the 7-tile threshold that ships an untested class fails here."""
    import ctypes as C
    import plan_cases
    from af_mi355x._lib import lib
    matrix = _load_tests_module("test_hip_stem_matrix")
    covered = matrix.covered_keys()
    shipped = {}
    for net, dtype, batch, setting, p in plan_cases.plans(monkeypatch):
        stems = [launch for launch in p.launches if launch.kind in ("stem3_pool", "stem_pool", "stem", "tstem", "tstem_pool3")]
        assert len(stems) == (2 if net == "slowfast_r50" else 1) and p.launches[0] in stems, (net, dtype, batch)
        for launch in stems:
            cv, (d,) = launch.convs["conv"], launch.descs
            if launch.kind in ("stem3_pool", "stem_pool"):
                units, bands, groups = C.c_int64(0), C.c_int(0), C.c_int(0)
                fused = 2 if launch.kind == "stem3_pool" else 1
                assert lib.af_stem_work_units(C.byref(d), fused, C.byref(units), C.byref(bands), C.byref(groups)) == 0
                hq = (d.ho - 1) // 2 + 1
                assert groups.value == min(units.value, 256) and units.value == d.n * d.to * bands.value and 1 <= bands.value <= max(1, hq // 4)
                key = matrix.launch_key(launch.kind, dtype, cv.kernel[0], d.w, hq, bands.value, units.value, groups.value, launch.ld)
                what = "%d units (%d bands) on %d workgroups, rows of %d" % (units.value, bands.value, groups.value, launch.ld)
            else:
                key = matrix.stem_case_key(launch.kind, dtype, cv.kernel[0], cv.cout)
                what = "%d positions" % (d.n * d.to * d.ho * d.wo)
            shipped.setdefault(key, "%s batch %d%s: %s" % (net, batch, setting, what))
    # today 20 keys: stem3_pool per 16-bit dtype I3D's kT = 5 without bands on the XCD map in rounds "1", "1-2", "2", ">2" and with
    # bands in "1", and SlowFast's kT = 1 with bands into rows of 80 (12); stem f32 kT 5 / 1 into 64 channels and kT 5 into 8 in all
    # three dtypes (5); tstem f32 (1), tstem_pool3 (2)
    assert len(shipped) >= 20, len(shipped)
    assert {k[6] for k in shipped if k[0] == "stem3_pool"} == {"1", "1-2", "2", ">2"} and any(k[0] == "stem3_pool" and k[8] for k in shipped)
    missing = sorted("%s (%s)" % (k, v) for k, v in shipped.items() if k not in covered)
    assert not missing, "%d shipped stem launches without a case in test_hip_stem_matrix.py:\n%s" % (len(missing), "\n".join(missing))
    # the query refuses what the launchers refuse
    d = plan_cases.plan("i3d_r50", "bf16", 1).launches[0].descs[0]
    units, bands, groups = C.c_int64(0), C.c_int(0), C.c_int(0)
    assert lib.af_stem_work_units(C.byref(d), 3, C.byref(units), C.byref(bands), C.byref(groups)) == -1
    assert lib.af_stem_work_units(C.byref(d), 2, None, C.byref(bands), C.byref(groups)) == -1
    assert lib.af_stem_work_units(C.byref(d), 2, C.byref(units), C.byref(bands), C.byref(groups)) == 0
    assert (units.value, bands.value, groups.value) == (256, 8, 256)


def test_engine_replay_covers_every_launch_form_that_ships(monkeypatch):
    """every launch kind of engine._ROLES, and every stem, pool and head kind, that a default or switched plan of the three networks
    produces at batch 1..32 - as the form (kind, projection shortcut, fused pool, x_sub, channel offset, residual) - is launched by a
    case of tests/test_hip_engine_replay.py, and engine_replay_ref has a reference and a tolerance for its kind.  A new launch kind
    without a replay reference fails here, on the CPU."""
    import plan_cases
    from af_mi355x import engine
    replay = _load_tests_module("test_hip_engine_replay")
    ref = _load_tests_module("engine_replay_ref")

    def form(launch):
        return (launch.kind, bool(launch.convs.get("branch1")), launch.tpool, launch.x_sub, launch.ch_off > 0, launch.res is not None)
    covered = set()
    for net, dtype, batch, env in replay.CASES:
        plan_cases.set_switches(monkeypatch, env)
        p = plan_cases.plan(net, dtype, batch)
        replay.expected_kinds((net, dtype, batch, env), p)             # what each case says it is there for, from its plan
        covered |= {form(launch) for launch in p.launches}
    assert {k[0] for k in covered} <= set(ref.REFERENCED_KINDS)
    assert set(engine._ROLES) <= {k[0] for k in covered}
    settings = [{}, plan_cases.UNFUSED] + [{name: "0" if on else "1"} for name, on in engine.SWITCHES.items()]
    shipped = {}
    for net, dtype, batch, setting, p in plan_cases.plans(monkeypatch, settings):
        for launch in p.launches:
            shipped.setdefault(form(launch), "%s %s batch %d%s" % (net, dtype, batch, setting))
            if launch.kind not in ref.HEAD_KINDS and not (launch.kind in ("ca", "cpa", "bc", "abc") and dtype == "f32"):
                assert ref.tolerance(launch, "dst", dtype) > 0
    # every kind the engine can emit ships in some plan, but stem_pool (the fused 16-bit stem without K-packed weights, which a
    # PackedWeights always has); the replay has a reference for that one too
    assert len(shipped) >= 20 and {k[0] for k in shipped} == (set(engine.Engine._EMIT) - {"stem_pool"}) | {"tt_head"}
    assert set(engine.Engine._EMIT) | {"tt_head"} <= set(ref.REFERENCED_KINDS)
    missing = sorted("%s (%s)" % (k, v) for k, v in shipped.items() if k not in covered)
    assert not missing, "%d shipped launch forms without a case in test_hip_engine_replay.py:\n%s" % (len(missing), "\n".join(missing))
