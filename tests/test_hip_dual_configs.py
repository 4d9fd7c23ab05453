"""GPU: the dualrun branch kernel (csrc/af_dual.hip, dual_branch_kernel) away from the shipped setup.  The drop-in classes
take the reference constructor's range - any depth, a head count dividing 256, dim_feedforward 4..768 and input widths
4..256 in steps of 4, 1..16 frames - while tests/test_hip_dualrun.py runs only d_model 256 / depth 4 / 4 heads / ff 768.

Here: the reference's own outputs at its defaults (ff 512) and other head counts / depths / widths
(tests/golden/f7b_dualrun_configs.*), a covering sweep against the fp64 oracle, and DualEncoderRGB at ff 512 / 16 frames.
An MLP width in (256, 512] at 9..16 frames is where the K-split of linear_rows once wrote its partial sums past `part`."""
import os
import sys

import numpy as np
import pytest
import torch

from conftest import ROOT, load_json, load_npz
sys.path.insert(0, os.path.join(ROOT, "oracle"))
import dualrun_oracle  # noqa: E402
from af_mi355x import dualrun, synth  # noqa: E402

pytestmark = pytest.mark.gpu


def _net(sp, sd):
    net = dualrun.DualEncoderAU_LMK(au_dim=sp.au_dim, lmk_dim=sp.lmk_dim, d_model=sp.d_model, depth=sp.depth, heads=sp.heads,
                                    mlp_ratio=sp.ff / sp.d_model, pool_tau=sp.pool_tau)
    assert net.spec == sp
    net.load_state_dict(sd)
    return net.cuda().eval()


def _err(got, want):
    return float(np.abs(np.asarray(got, np.float64) - np.asarray(want, np.float64)).max())


F7B = load_json("f7b_dualrun_configs.json")["cases"]


@pytest.mark.parametrize("case", F7B, ids=[c["tag"] for c in F7B])
def test_dual_encoder_matches_reference_at_other_configs(case):
    """the reference's fp32 outputs, same gates as test_dual_encoder_matches_reference.  Measured on one MI355X: worst
    |logit - ref| 3.0e-6, worst |z - ref| 9.7e-5 (ref_t16's clip of length 9, where the reference's own fp32 z is 2.2e-4
    from fp64; every other setup is within 7e-5)"""
    st = load_npz("f7b_dualrun_configs.npz")
    a = case["args"]
    sp = dualrun.DualSpec(a["au_dim"], a["lmk_dim"], a["d_model"], a["depth"], a["heads"], case["ff"], a["pool_tau"])
    sd = dualrun.dual_synthetic_state_dict(sp, seed=case["weights_seed"])
    assert synth.state_dict_sha256(sd) == case["weights_sha256"]
    net = _net(sp, sd)
    A, L, _ = dualrun.synthetic_dual_inputs(case["batch"], sp, frames=case["frames"], seed=case["inputs_seed"])
    lengths = None if case["lengths"] is None else torch.tensor(case["lengths"], dtype=torch.int32).cuda()
    with torch.inference_mode():
        out = net(A.cuda(), L.cuda(), lengths, return_z=True)
    tag = case["tag"]
    logits, z = out["bin_logits"].cpu().numpy(), out["z"].cpu().numpy()
    print("%s: max|logit - ref| %.2e  max|z - ref| %.2e" % (tag, _err(logits, st[tag + "_logits_f32"]), _err(z, st[tag + "_z_f32"])))
    np.testing.assert_allclose(logits, st[tag + "_logits_f32"], rtol=0, atol=2e-5)
    np.testing.assert_allclose(z, st[tag + "_z_f32"], rtol=2e-5, atol=1e-4)


def _lengths(kind, batch, frames, seed):
    if kind == "none":
        return None
    g = torch.Generator().manual_seed(seed)
    ln = torch.randint(1, frames + 1, (batch,), generator=g, dtype=torch.int32)
    if kind == "edge":                     # no valid frame (frame 0 kept), one, all, more than T
        ln[:4] = torch.tensor([0, 1, frames, frames + 5], dtype=torch.int32)[:batch]
    return ln


# (ff, heads, depth, (au, lmk), frames, lengths): every ff in (256, 512] at T <= 8 and at T >= 9 (G = 1 there).  With G = 2
# there the partial sums of the later rows landed past the LDS allocation for <= 8 heads (with 32 heads they stay inside the
# attention-probability region, unused at that point), and the lengths must reach those rows for the loss to show.
SWEEP = [
    (512, 4, 4, (36, 132), 16, "edge"),
    (512, 4, 1, (36, 132), 8, "ragged"),
    (512, 1, 1, (8, 20), 9, "none"),
    (512, 8, 1, (4, 256), 12, "edge"),
    (384, 8, 1, (4, 256), 12, "edge"),
    (384, 1, 4, (36, 132), 8, "edge"),
    (384, 4, 1, (8, 20), 16, "none"),
    (260, 4, 1, (36, 132), 9, "edge"),
    (128, 1, 0, (4, 256), 16, "edge"),
    (128, 8, 1, (36, 132), 1, "edge"),
    (128, 4, 4, (8, 20), 9, "ragged"),
    (256, 32, 4, (8, 20), 9, "ragged"),
    (256, 4, 0, (36, 132), 1, "none"),
    (768, 8, 1, (4, 256), 16, "edge"),
    (768, 1, 0, (8, 20), 12, "ragged"),
    (768, 32, 1, (36, 132), 8, "none"),
]


@pytest.mark.parametrize("ff,heads,depth,dims,frames,kind", SWEEP,
                         ids=["ff%d_h%d_d%d_in%dx%d_t%d_%s" % (f, h, d, a, l, t, k) for f, h, d, (a, l), t, k in SWEEP])
def test_dual_encoder_vs_fp64_oracle_sweep(ff, heads, depth, dims, frames, kind):
    """against dualrun_oracle.dual_forward in fp64 on a covering set of setups.  Measured on one MI355X over the sweep:
    worst |logit - fp64| 7.8e-6 and worst |z - fp64| 7.3e-5 (|z| up to ~15); asserted at the fp32 gates of
    test_dual_encoder_matches_reference: logits atol 2e-5, z rtol 2e-5 / atol 1e-4."""
    sp = dualrun.DualSpec(dims[0], dims[1], 256, depth, heads, ff, 1.0)
    seed = ff + 7 * heads + 31 * depth + dims[0] + frames
    sd = dualrun.dual_synthetic_state_dict(sp, seed=seed)
    net = _net(sp, sd)
    batch = 5
    A, L, _ = dualrun.synthetic_dual_inputs(batch, sp, frames=frames, seed=seed)
    lengths = _lengths(kind, batch, frames, seed)
    want, wz = dualrun_oracle.dual_forward(sd, A, L, lengths, heads=heads, tau=1.0, dtype=torch.float64)
    with torch.inference_mode():
        out = net(A.cuda(), L.cuda(), None if lengths is None else lengths.cuda(), return_z=True)
    logits, z = out["bin_logits"].cpu().numpy(), out["z"].cpu().numpy()
    print("max|logit - fp64| %.2e  max|z - fp64| %.2e" % (_err(logits, want.numpy()), _err(z, wz.numpy())))
    np.testing.assert_allclose(logits, want.numpy(), rtol=0, atol=2e-5)
    np.testing.assert_allclose(z, wz.numpy(), rtol=2e-5, atol=1e-4)


@pytest.mark.parametrize("tv", [16, 1])
def test_dual_rgb_ff512_t16_vs_fp64_oracle(tv):
    """DualEncoderRGB with ff_dim=2.0 (ff 512) at 16 frames and a suffix padding mask, V per frame or broadcast
    (tv = 1), against dualrun_oracle.dual_rgb_forward in fp64 (measured on one MI355X: 2.1e-7)"""
    vis, T, B = 2048, 16, 4
    sp = dualrun.DualSpec(36, 132, 256, 2, 4, 512, 0.7, 128)
    sd = dualrun.dual_rgb_synthetic_state_dict(sp, vis, seed=23)
    net = dualrun.DualEncoderRGB(36, 132, vis, d_model=256, depth=2, heads=4, ff_dim=2.0)
    assert net.spec.ff == 512
    net.load_state_dict(sd)
    net = net.cuda().eval()
    A, L, _ = dualrun.synthetic_dual_inputs(B, sp, frames=T, seed=29)
    V = 2 * torch.rand((B, tv, vis), generator=torch.Generator().manual_seed(31))
    pad = dualrun.DualEncoderRGB.lengths_to_mask(torch.tensor([16, 1, 9, 12]), T, "cpu")
    want, _ = dualrun_oracle.dual_rgb_forward(sd, A, L, V, pad, heads=4, tau=0.7, dtype=torch.float64)
    with torch.inference_mode():
        got = net(A.cuda(), L.cuda(), V.cuda(), pad.cuda()).cpu().numpy()
    print("tv %d: max|logit - fp64| %.2e" % (tv, _err(got, want.numpy())))
    np.testing.assert_allclose(got, want.numpy(), rtol=0, atol=2e-5)


def test_head_counts_that_fit_lds_only_at_8_frames():
    """64 heads fit af_dual_branch_encoders' LDS at 8 frames, not at 16: the module runs 8 and refuses 9 before any launch"""
    sp = dualrun.DualSpec(8, 20, 256, 1, 64, 256, 1.0)
    sd = dualrun.dual_synthetic_state_dict(sp, seed=3)
    net = _net(sp, sd)
    A, L, lengths = dualrun.synthetic_dual_inputs(2, sp, frames=9, seed=3)
    with pytest.raises(ValueError, match="1..8 frames"):
        net(A.cuda(), L.cuda())
    want, _ = dualrun_oracle.dual_forward(sd, A[:, :8], L[:, :8], None, heads=64, tau=1.0, dtype=torch.float64)
    with torch.inference_mode():
        got = net(A[:, :8].cuda(), L[:, :8].cuda())["bin_logits"].cpu().numpy()
    np.testing.assert_allclose(got, want.numpy(), rtol=0, atol=2e-5)
