"""GPU: the small C-ABI kernels that the model tests reach only at one fixed shape, or not at all, called directly through
af_mi355x._lib on device tensors and compared with plain fp64 restatements at the edges of each kernel's range:
  dualrun     af_mlp_head, af_dual_head, af_masked_mean_proj, af_gated_moe, af_transpose_f32   (csrc/af_dual.hip)
  FTCN-TT     af_layernorm, af_attention, af_gelu, af_tokens_assemble                           (csrc/af_ftcn.hip)
  heads       af_linear, af_linear_scores, af_avgpool, af_avgpool_fc_scores                      (csrc/af_pool.hip)
Each entry point must also refuse out-of-range arguments with AF_ERR_ARG before any launch.
The tolerances are fp32 rounding bounds for the operation's size; the worst errors measured on one MI355X are printed."""
import ctypes as C
import math
import os
import sys

import numpy as np
import pytest
import torch

from conftest import ROOT
sys.path.insert(0, os.path.join(ROOT, "oracle"))
import dualrun_oracle  # noqa: E402

pytestmark = pytest.mark.gpu

AF_ERR_ARG = -1                                         # include/af_hip.h


def _L():
    from af_mi355x import _lib
    return _lib


def _p(t):
    return None if t is None else C.c_void_p(t.data_ptr())


def _st():
    return C.c_void_p(torch.cuda.current_stream().cuda_stream)


def _ok(rc, what):
    L = _L()
    L.check(rc, what)
    torch.cuda.synchronize()


def _rejects(rc, *words):
    L = _L()
    assert rc == AF_ERR_ARG, rc
    msg = L.lib.af_last_error().decode()
    assert all(w in msg for w in words), msg


def _gen(seed):
    return torch.Generator().manual_seed(seed)


def _gelu64(x):
    return 0.5 * x * (1.0 + torch.erf(x / math.sqrt(2.0)))


def _report(name, got, want):
    err = float((got.double().cpu() - want.double().cpu()).abs().max()) if want.numel() else 0.0
    print("%s: max|err| %.2e" % (name, err))
    return err


# ---------------------------------------------------------------------------------------------------------- dualrun head
def _mlp_head_weights(n, hidden, g):
    gamma, beta = 1 + 0.1 * torch.randn(n, generator=g), 0.05 * torch.randn(n, generator=g)
    w1t = torch.randn(n, hidden, generator=g) / math.sqrt(n)
    b1, w2, b2 = 0.05 * torch.randn(hidden, generator=g), torch.randn(hidden, generator=g) / math.sqrt(hidden), torch.randn(1, generator=g)
    flat = torch.cat([gamma, beta, w1t.reshape(-1), b1, w2, b2])
    return flat, (gamma, beta, w1t, b1, w2, b2)


def _mlp_head64(z, parts):
    gamma, beta, w1t, b1, w2, b2 = [t.double() for t in parts]
    y = torch.nn.functional.layer_norm(z.double(), (z.shape[1],), gamma, beta, 1e-5)
    return _gelu64(y @ w1t + b1) @ w2 + b2


@pytest.mark.parametrize("n,hidden", [(1, 1), (7, 13), (512, 300), (768, 512), (4096, 257)])
@pytest.mark.parametrize("with_scores", [False, True])
def test_mlp_head_vs_fp64(n, hidden, with_scores):
    """LayerNorm(n) -> Linear(n, hidden) -> GELU -> Linear(hidden, 1) [-> sigmoid]: n from 1 (LayerNorm of one value = beta)
    to the 4096 limit, hidden neither a multiple of 8 (the kernel's unrolled k loop) nor of 256 (its thread loop)"""
    g = _gen(n + hidden)
    clips = 3
    flat, parts = _mlp_head_weights(n, hidden, g)
    z = 3 * torch.randn(clips, n, generator=g) + 0.5
    want = _mlp_head64(z, parts)
    logits = torch.full((clips,), float("nan"), device="cuda")
    scores = torch.full((clips,), float("nan"), device="cuda") if with_scores else None
    zd, wd = z.cuda(), flat.cuda()
    _ok(_L().lib.af_mlp_head(_p(zd), _p(wd), clips, n, hidden, _p(logits), _p(scores), _st()), "af_mlp_head")
    _report("mlp_head n %d hidden %d" % (n, hidden), logits, want)
    np.testing.assert_allclose(logits.cpu().numpy(), want.numpy(), rtol=0, atol=2e-5)
    if with_scores:
        np.testing.assert_allclose(scores.cpu().numpy(), torch.sigmoid(want).numpy(), rtol=0, atol=5e-6)


def test_dual_head_is_the_square_mlp_head():
    g = _gen(5)
    n, clips = 520, 4
    flat, parts = _mlp_head_weights(n, n, g)
    z = torch.randn(clips, n, generator=g)
    logits = torch.empty(clips, device="cuda")
    zd, wd = z.cuda(), flat.cuda()
    _ok(_L().lib.af_dual_head(_p(zd), _p(wd), clips, n, _p(logits), _st()), "af_dual_head")
    want = _mlp_head64(z, parts)
    _report("dual_head n %d" % n, logits, want)
    np.testing.assert_allclose(logits.cpu().numpy(), want.numpy(), rtol=0, atol=2e-5)


def test_mlp_head_rejects_bad_arguments():
    lib = _L().lib
    z, w, out = torch.zeros(2, 8, device="cuda"), torch.zeros(4096 * 8 + 64, device="cuda"), torch.zeros(2, device="cuda")
    for n, hidden in ((0, 4), (4097, 4), (8, 0)):
        _rejects(lib.af_mlp_head(_p(z), _p(w), 2, n, hidden, _p(out), None, _st()), "mlp_head")
    _rejects(lib.af_mlp_head(None, _p(w), 2, 8, 4, _p(out), None, _st()), "mlp_head")
    _rejects(lib.af_mlp_head(_p(z), _p(w), -1, 8, 4, _p(out), None, _st()), "mlp_head")
    _rejects(lib.af_dual_head(_p(z), _p(w), 2, 0, _p(out), _st()), "mlp_head")
    torch.cuda.synchronize()


# ------------------------------------------------------------------------------------------------ masked mean + projection
def _masked_mean_proj64(V, lengths, tmask, wt):
    """AltFreezingRGBEncoder.from_features + rgb_proj (dual_rgb.py:27-44): the clamp is per element before the sum"""
    V = V.double()
    if lengths is None:
        pooled = V.mean(dim=1)
    else:
        valid = (torch.arange(tmask).view(1, -1) < lengths.view(-1, 1).long()).double()
        w = valid / valid.clamp_min(1e-6).sum(dim=1, keepdim=True)
        pooled = (V * w.unsqueeze(-1)).sum(dim=1)                 # tv = 1 broadcasts over the mask, as torch does
    return pooled @ wt.double()


@pytest.mark.parametrize("vis", [1, 7, 2048, 16384])
@pytest.mark.parametrize("tmask,tv", [(6, 6), (6, 1), (1, 1)])
@pytest.mark.parametrize("masked", [True, False])
def test_masked_mean_proj_vs_fp64(vis, tmask, tv, masked):
    """vis up to the 64 KB LDS limit, V per frame or broadcast (tv = 1), lengths 0 (no valid frame: z = 0), 1, T and
    above T; z_ld > d and the columns between d and z_ld stay untouched"""
    g = _gen(vis + 10 * tmask + tv)
    clips, d, z_ld = 5, 40, 53
    V = 2 * torch.rand(clips, tv, vis, generator=g)
    wt = torch.randn(vis, d, generator=g) / math.sqrt(vis)
    lengths = torch.tensor([0, 1, tmask, tmask + 3, max(1, tmask // 2)], dtype=torch.int32) if masked else None
    want = _masked_mean_proj64(V, lengths, tmask, wt)
    z = torch.full((clips, z_ld), 7.0, device="cuda")
    Vd, wd = V.cuda(), wt.cuda()
    ld = None if lengths is None else lengths.cuda()
    _ok(_L().lib.af_masked_mean_proj(_p(Vd), clips, tv, vis, _p(ld), tmask, _p(wd), d, _p(z), z_ld, _st()), "af_masked_mean_proj")
    got = z[:, :d].cpu()
    _report("masked_mean_proj vis %d tmask %d tv %d" % (vis, tmask, tv), got, want)
    np.testing.assert_allclose(got.numpy(), want.numpy(), rtol=1e-5, atol=1e-5)
    assert bool((z[:, d:] == 7.0).all())


def test_masked_mean_proj_rejects_bad_arguments():
    lib = _L().lib
    V, w, z = torch.zeros(2 * 4 * 16385, device="cuda"), torch.zeros(16385 * 8, device="cuda"), torch.zeros(2, 16, device="cuda")
    ok = dict(clips=2, tv=4, vis=16, tmask=4, d=8, z_ld=16)
    for bad in (dict(vis=16385), dict(vis=0), dict(tv=3), dict(tv=0), dict(tmask=0, tv=1), dict(d=0), dict(z_ld=7), dict(clips=-1)):
        a = dict(ok, **bad)
        _rejects(lib.af_masked_mean_proj(_p(V), a["clips"], a["tv"], a["vis"], None, a["tmask"], _p(w), a["d"], _p(z), a["z_ld"], _st()),
                 "masked_mean_proj")
    _rejects(lib.af_masked_mean_proj(None, 2, 4, 16, None, 4, _p(w), 8, _p(z), 16, _st()), "masked_mean_proj")
    torch.cuda.synchronize()


# ------------------------------------------------------------------------------------------------------------ gated MoE
@pytest.mark.parametrize("n", [1, 255, 257])
@pytest.mark.parametrize("hidden", [1, 16])
@pytest.mark.parametrize("temps", [(0.3, 0.02), (1.7, 0.6)])
def test_gated_moe_vs_fp64(n, hidden, temps):
    """GatedMoE (engine_rgb.py:376-384) across the 256-thread block edge; temperatures below the 1.0 / 0.1 clamps and above
    them.  z = logit((p + 1e-6) / (1 - p + 1e-6)) loses fp32 resolution as p nears 0 or 1: the z bound is the fp32 rounding
    of p (3e-7 absolute) times dz/dp, plus 2e-5 relative; the gate's is that of its pre-activation sum"""
    g = _gen(n * 100 + hidden)
    sd = {"t_rgb": torch.tensor(temps[0]), "t_dual": torch.tensor(temps[1]), "gate.0.weight": torch.randn(hidden, 3, generator=g),
          "gate.0.bias": 0.3 * torch.randn(hidden, generator=g), "gate.2.weight": torch.randn(1, hidden, generator=g),
          "gate.2.bias": 0.3 * torch.randn(1, generator=g)}
    zr, zd = 3 * torch.randn(n, 1, generator=g), 3 * torch.randn(n, 1, generator=g)
    want_z, want_g = dualrun_oracle.gated_moe({k: v.double() for k, v in sd.items()}, zr.double(), zd.double())
    w = torch.cat([sd["t_rgb"].view(1), sd["t_dual"].view(1), sd["gate.0.weight"].reshape(-1), sd["gate.0.bias"],
                   sd["gate.2.weight"].reshape(-1), sd["gate.2.bias"]]).cuda()
    z, gate = torch.empty(n, device="cuda"), torch.empty(n, device="cuda")
    a, b = zr.cuda(), zd.cuda()
    _ok(_L().lib.af_gated_moe(_p(a), _p(b), _p(w), hidden, n, _p(z), _p(gate), _st()), "af_gated_moe")
    want_z, want_g = want_z.view(-1), want_g.view(-1)
    x = torch.cat([zr, zd, (zr - zd).abs()], dim=1).double()
    sabs = torch.relu(x @ sd["gate.0.weight"].double().t() + sd["gate.0.bias"].double()) @ sd["gate.2.weight"].double().abs().t()
    _report("gated_moe gate n %d hidden %d" % (n, hidden), gate, want_g)
    gtol = 1e-6 + 0.25 * 4e-7 * (sabs.view(-1) + float(sd["gate.2.bias"].abs()))         # sigmoid' <= 1/4 times the gate sum's rounding
    assert bool(((gate.cpu().double() - want_g).abs() <= gtol).all())
    pr = torch.sigmoid(zr.double() / max(temps[0], 1.0)).view(-1)
    pd = torch.sigmoid(zd.double() / max(temps[1], 0.1)).view(-1)
    p = want_g * pr + (1 - want_g) * pd
    slope = 1 / (p + 1e-6) + 1 / (1 - p + 1e-6)
    tol = 2e-5 * want_z.abs() + 1e-5 + 3e-7 * slope
    err = (z.cpu().double() - want_z).abs()
    print("gated_moe z: max|err| %.2e, max err / bound %.2f" % (float(err.max()), float((err / tol).max())))
    assert bool((err <= tol).all())


def test_gated_moe_rejects_bad_arguments():
    lib = _L().lib
    x, w = torch.zeros(4, device="cuda"), torch.zeros(64, device="cuda")
    _rejects(lib.af_gated_moe(_p(x), _p(x), _p(w), 0, 4, _p(x), _p(x), _st()), "gated_moe")
    _rejects(lib.af_gated_moe(_p(x), _p(x), _p(w), 8, -1, _p(x), _p(x), _st()), "gated_moe")
    _rejects(lib.af_gated_moe(_p(x), None, _p(w), 8, 4, _p(x), _p(x), _st()), "gated_moe")
    torch.cuda.synchronize()


# ------------------------------------------------------------------------------------------------------------ transpose
@pytest.mark.parametrize("rows,cols", [(1, 1), (1, 300), (3, 700), (769, 5), (256, 768)])
def test_transpose_is_exact(rows, cols):
    src = torch.randn(rows, cols, generator=_gen(rows * cols)).cuda()
    dst = torch.full((cols, rows), float("nan"), device="cuda")
    _ok(_L().lib.af_transpose_f32(_p(src), rows, cols, _p(dst), _st()), "af_transpose_f32")
    assert torch.equal(dst, src.t())


def test_transpose_rejects_bad_arguments():
    lib = _L().lib
    x = torch.zeros(16, device="cuda")
    for rows, cols in ((0, 4), (4, 0), (-1, 4)):
        _rejects(lib.af_transpose_f32(_p(x), rows, cols, _p(x), _st()), "transpose")
    _rejects(lib.af_transpose_f32(None, 4, 4, _p(x), _st()), "transpose")
    torch.cuda.synchronize()


# ------------------------------------------------------------------------------------------------------------ layernorm
@pytest.mark.parametrize("dim,x_ld,y_ld", [(1, 1, 1), (37, 40, 37), (100, 100, 131), (768, 800, 768), (1000, 1000, 1000)])
@pytest.mark.parametrize("offset", [0.0, 1000.0])
def test_layernorm_vs_fp64(dim, x_ld, y_ld, offset):
    """nn.LayerNorm(dim) on strided rows.  Rows with a large common offset (1000, spread 0.5) are what the two-pass
    variance is for: a one-pass E[x^2] - E[x]^2 in fp32 loses the variance there.  The bound is the fp32 rounding of
    the mean (offset * 2e-7 / std, relative to the normalised output) plus 2e-5"""
    g = _gen(dim * 7 + int(offset))
    rows = 9
    x = offset + 0.5 * torch.randn(rows, x_ld, generator=g)
    gamma, beta = 1 + 0.1 * torch.randn(dim, generator=g), 0.1 * torch.randn(dim, generator=g)
    want = torch.nn.functional.layer_norm(x[:, :dim].double(), (dim,), gamma.double(), beta.double(), 1e-5)
    y = torch.full((rows, y_ld), 7.0, device="cuda")
    xd, gd, bd = x.cuda(), gamma.cuda(), beta.cuda()
    _ok(_L().lib.af_layernorm(_p(xd), x_ld, _p(gd), _p(bd), rows, dim, C.c_float(1e-5), _p(y), y_ld, _st()), "af_layernorm")
    got = y[:, :dim].cpu()
    _report("layernorm dim %d offset %g" % (dim, offset), got, want)
    tol = 2e-5 + 2e-7 * offset / 0.5 * 1.2
    np.testing.assert_allclose(got.numpy(), want.numpy(), rtol=0, atol=tol)
    assert bool((y[:, dim:] == 7.0).all())


def test_layernorm_rejects_bad_arguments():
    lib = _L().lib
    x = torch.zeros(64, device="cuda")
    _rejects(lib.af_layernorm(_p(x), 8, _p(x), _p(x), 2, 0, C.c_float(1e-5), _p(x), 8, _st()), "layernorm")
    _rejects(lib.af_layernorm(_p(x), 8, _p(x), _p(x), -1, 8, C.c_float(1e-5), _p(x), 8, _st()), "layernorm")
    _rejects(lib.af_layernorm(_p(x), 8, None, _p(x), 2, 8, C.c_float(1e-5), _p(x), 8, _st()), "layernorm")
    torch.cuda.synchronize()


# ------------------------------------------------------------------------------------------------------------ attention
def _attention64(qkv, n_tok, heads, dh):
    b = qkv.shape[0] // n_tok
    q, k, v = qkv.double().view(b, n_tok, 3, heads, dh).permute(2, 0, 3, 1, 4)
    p = torch.softmax(q @ k.transpose(-1, -2) / math.sqrt(dh), dim=-1)
    return (p @ v).permute(0, 2, 1, 3).reshape(b * n_tok, heads * dh)


@pytest.mark.parametrize("clips,n_tok,heads,dh", [(2, 1, 16, 64), (2, 17, 16, 64), (1, 64, 4, 128), (3, 17, 1, 1),
                                                  (1, 64, 16, 128), (2, 33, 7, 3)])
@pytest.mark.parametrize("spread", [1.0, 12.0])
def test_attention_vs_fp64(clips, n_tok, heads, dh, spread):
    """softmax(q k^T / sqrt(dh)) v per (clip, head) up to the 64-token x 128 limit.  spread 12 puts the scaled scores
    hundreds apart: without the max subtraction exp overflows.  The bound is the fp32 rounding of the scores
    (4 * 1.2e-7 * sum|q_i k_i| / sqrt(dh), in the weights) times max|v|, plus 2e-6"""
    g = _gen(clips * 1000 + n_tok * 10 + heads + dh)
    qkv = torch.randn(clips * n_tok, 3, heads * dh, generator=g)
    qkv[:, :2] *= spread
    qkv = qkv.reshape(clips * n_tok, 3 * heads * dh)
    want = _attention64(qkv, n_tok, heads, dh)
    out = torch.full((clips * n_tok, heads * dh), float("nan"), device="cuda")
    qd = qkv.cuda()
    _ok(_L().lib.af_attention(_p(qd), clips, n_tok, heads, dh, _p(out), _st()), "af_attention")
    err = _report("attention %d tok x %d heads x %d spread %g" % (n_tok, heads, dh, spread), out, want)
    q, k, v = qkv.double().view(clips, n_tok, 3, heads, dh).permute(2, 0, 3, 1, 4)
    sabs = float((q.abs() @ k.abs().transpose(-1, -2)).max()) / math.sqrt(dh)
    tol = 2e-6 + 4 * 1.2e-7 * (sabs + 1) * float(v.abs().max())
    assert err <= tol, (err, tol)


def test_attention_rejects_bad_arguments():
    lib = _L().lib
    x = torch.zeros(64 * 3 * 129, device="cuda")
    for n_tok, heads, dh in ((65, 1, 8), (0, 1, 8), (4, 1, 129), (4, 1, 0), (4, 0, 8)):
        _rejects(lib.af_attention(_p(x), 1, n_tok, heads, dh, _p(x), _st()), "attention")
    _rejects(lib.af_attention(_p(x), -1, 4, 1, 8, _p(x), _st()), "attention")
    torch.cuda.synchronize()


# ----------------------------------------------------------------------------------------------------- gelu, tokens
@pytest.mark.parametrize("n", [1, 255, 1000, 65537])
def test_gelu_vs_fp64(n):
    """exact (erf) GELU in place for |x| up to 10; n not a multiple of the 256-thread block.  For x << 0, 1 + erf(x / sqrt 2)
    cancels in fp32 (as in torch's own fp32 GELU): one ulp of 1 there is 0.5 * |x| * 1.2e-7 <= 6e-7 absolute"""
    x = (torch.rand(n, generator=_gen(n)) * 20 - 10)
    x[:4] = torch.tensor([-10.0, 10.0, 0.0, -1e-3])[:n]
    want = _gelu64(x.double())
    xd = x.cuda()
    _ok(_L().lib.af_gelu(_p(xd), n, _st()), "af_gelu")
    _report("gelu n %d" % n, xd, want)
    np.testing.assert_allclose(xd.cpu().numpy(), want.numpy(), rtol=2e-6, atol=6e-7)


def test_gelu_rejects_bad_arguments():
    lib = _L().lib
    x = torch.zeros(4, device="cuda")
    _rejects(lib.af_gelu(_p(x), -1, _st()), "gelu")
    _rejects(lib.af_gelu(None, 4, _st()), "gelu")
    torch.cuda.synchronize()


@pytest.mark.parametrize("clips,n_tok,dim", [(1, 1, 1), (2, 16, 1024), (3, 5, 37)])
def test_tokens_assemble_is_exact(clips, n_tok, dim):
    """tokens[b][0] = cls + pos[0], tokens[b][1 + t] = pooled[b][t] + pos[1 + t]: one fp32 add each, so exact"""
    g = _gen(clips + n_tok + dim)
    pooled, cls, pos = torch.randn(clips, n_tok, dim, generator=g), torch.randn(dim, generator=g), torch.randn(n_tok + 1, dim, generator=g)
    want = torch.cat([cls.expand(clips, 1, dim), pooled], dim=1) + pos
    out = torch.full((clips, n_tok + 1, dim), float("nan"), device="cuda")
    pd, cd, sd = pooled.cuda(), cls.cuda(), pos.cuda()
    _ok(_L().lib.af_tokens_assemble(_p(pd), _p(cd), _p(sd), clips, n_tok, dim, _p(out), _st()), "af_tokens_assemble")
    assert torch.equal(out.cpu(), want)


def test_tokens_assemble_rejects_bad_arguments():
    lib = _L().lib
    x = torch.zeros(64, device="cuda")
    for clips, n_tok, dim in ((-1, 2, 2), (1, 0, 2), (1, 2, 0)):
        _rejects(lib.af_tokens_assemble(_p(x), _p(x), _p(x), clips, n_tok, dim, _p(x), _st()), "tokens_assemble")
    torch.cuda.synchronize()


# ----------------------------------------------------------------------------------------------- linear, avgpool + fc
@pytest.mark.parametrize("in_features", [1, 300, 2051])
@pytest.mark.parametrize("classes", [1, 2, 5])
@pytest.mark.parametrize("scale", [1.0, 60.0])
def test_linear_scores_vs_fp64(in_features, classes, scale):
    """nn.Linear with the callers' score epilogue (sigmoid for one class, softmax[:, 1] for two); in_features not a multiple
    of the 256-thread block; scale 60 saturates the logits (|l| up to ~200: expf overflows to inf, scores must be 0 / 1)"""
    g = _gen(in_features * 10 + classes + int(scale))
    rows = 6
    x = torch.randn(rows, in_features, generator=g)
    w = scale * torch.randn(classes, in_features, generator=g) / math.sqrt(in_features)
    b = torch.randn(classes, generator=g)
    want = x.double() @ w.double().t() + b.double()
    y = torch.full((rows, classes), float("nan"), device="cuda")
    xd, wd, bd = x.cuda(), w.cuda(), b.cuda()
    lib = _L().lib
    if classes <= 2:
        scores = torch.full((rows,), float("nan"), device="cuda")
        _ok(lib.af_linear_scores(_p(xd), _p(wd), _p(bd), rows, in_features, classes, _p(y), _p(scores), _st()), "af_linear_scores")
        ws = torch.sigmoid(want[:, 0]) if classes == 1 else torch.softmax(want, dim=1)[:, 1]
        np.testing.assert_allclose(scores.cpu().numpy(), ws.numpy(), rtol=0, atol=2e-6)
    else:
        _ok(lib.af_linear(_p(xd), _p(wd), _p(bd), rows, in_features, classes, _p(y), _st()), "af_linear")
    _report("linear in %d classes %d scale %g" % (in_features, classes, scale), y, want)
    bound = 2e-6 + 2e-7 * math.sqrt(in_features) * float((x.abs().double() @ w.abs().double().t()).max())
    np.testing.assert_allclose(y.cpu().numpy(), want.numpy(), rtol=0, atol=bound)


def test_linear_rejects_bad_arguments():
    lib = _L().lib
    x = torch.zeros(64, device="cuda")
    for rows, fin, fout in ((0, 4, 1), (2, 0, 1), (2, 4, 0)):
        _rejects(lib.af_linear(_p(x), _p(x), _p(x), rows, fin, fout, _p(x), _st()), "linear")
    _rejects(lib.af_linear_scores(_p(x), _p(x), _p(x), 2, 4, 3, _p(x), _p(x), _st()), "scores")
    _rejects(lib.af_linear(_p(x), None, _p(x), 2, 4, 1, _p(x), _st()), "linear")
    torch.cuda.synchronize()


def _pool_desc(shape, kernel, dtype, stride=1):
    L = _L()
    n, t, h, w, c = shape
    d = L.PoolDesc()
    d.n, d.t, d.h, d.w, d.c = n, t, h, w, c
    d.kt, d.kh, d.kw = kernel
    d.st = d.sh = d.sw = stride
    d.pt = d.ph = d.pw = 0
    d.to, d.ho, d.wo = [(s - k) // stride + 1 for s, k in zip((t, h, w), kernel)]
    d.dtype = L.DTYPE_CODES[dtype]
    return d


def _avgpool64(x, kernel):
    xc = x.double().permute(0, 4, 1, 2, 3)                                  # NDHWC -> NCDHW
    p = torch.nn.functional.avg_pool3d(xc, kernel, stride=1)
    return p.permute(0, 2, 3, 4, 1).reshape(-1, x.shape[-1])               # rows (n, to, ho, wo), channels last


POOL_CASES = [("f32", (2, 4, 7, 7, 36), (4, 7, 7)), ("f32", (1, 3, 5, 6, 100), (2, 3, 3)),
              ("f16", (2, 4, 7, 7, 72), (4, 7, 7)), ("bf16", (1, 8, 14, 14, 200), (8, 7, 7)), ("bf16", (3, 1, 1, 1, 8), (1, 1, 1))]


@pytest.mark.parametrize("dtype,shape,kernel", POOL_CASES, ids=["%s_c%d_k%dx%dx%d" % ((d, s[-1]) + k) for d, s, k in POOL_CASES])
def test_avgpool_vs_fp64(dtype, shape, kernel):
    """AvgPool3d(kernel, stride 1) on NDHWC activations in f32 / f16 / bf16, channel counts that are not a multiple of the
    64-channel workgroup, several output positions, pooled_ld > c (the columns beyond c stay untouched)"""
    tdt = {"f32": torch.float32, "f16": torch.float16, "bf16": torch.bfloat16}[dtype]
    x = (torch.randn(shape, generator=_gen(sum(shape))) + 0.5).to(tdt)
    want = _avgpool64(x, kernel)
    d = _pool_desc(shape, kernel, dtype)
    ld = shape[-1] + 12
    pooled = torch.full((want.shape[0], ld), 7.0, device="cuda")
    xd = x.cuda()
    _ok(_L().lib.af_avgpool(C.byref(d), _p(xd), _p(pooled), ld, _st()), "af_avgpool")
    _report("avgpool %s %s" % (dtype, shape), pooled[:, :shape[-1]], want)
    win = kernel[0] * kernel[1] * kernel[2]
    np.testing.assert_allclose(pooled[:, :shape[-1]].cpu().numpy(), want.numpy(), rtol=0, atol=2e-7 * math.sqrt(win) * 4 + 1e-7)
    assert bool((pooled[:, shape[-1]:] == 7.0).all())


@pytest.mark.parametrize("classes", [1, 2])
def test_avgpool_fc_scores_vs_fp64(classes):
    """the fused head: avgpool -> Linear(c, classes) -> score, c = 200 (not a multiple of 64), bf16 activations"""
    shape, kernel = (3, 4, 5, 5, 200), (4, 5, 5)
    g = _gen(classes)
    x = (torch.randn(shape, generator=g) + 0.3).to(torch.bfloat16)
    w, b = 20 * torch.randn(classes, shape[-1], generator=g) / math.sqrt(shape[-1]), torch.randn(classes, generator=g)
    pooled64 = _avgpool64(x, kernel)
    want = pooled64 @ w.double().t() + b.double()
    d = _pool_desc(shape, kernel, "bf16")
    pooled = torch.empty(pooled64.shape, device="cuda")
    logits = torch.empty(pooled64.shape[0], classes, device="cuda")
    scores = torch.empty(pooled64.shape[0], device="cuda")
    xd, wd, bd = x.cuda(), w.cuda(), b.cuda()
    _ok(_L().lib.af_avgpool_fc_scores(C.byref(d), _p(xd), _p(wd), _p(bd), classes, _p(pooled), _p(logits), _p(scores), _st()),
        "af_avgpool_fc_scores")
    _report("avgpool_fc logits, %d classes" % classes, logits, want)
    np.testing.assert_allclose(pooled.cpu().numpy(), pooled64.numpy(), rtol=0, atol=2e-6)
    np.testing.assert_allclose(logits.cpu().numpy(), want.numpy(), rtol=0, atol=2e-5)
    ws = torch.sigmoid(want[:, 0]) if classes == 1 else torch.softmax(want, dim=1)[:, 1]
    np.testing.assert_allclose(scores.cpu().numpy(), ws.numpy(), rtol=0, atol=2e-6)


def test_avgpool_rejects_bad_arguments():
    lib = _L().lib
    x = torch.zeros(4 * 7 * 7 * 64, device="cuda")
    out = torch.zeros(64 * 8, device="cuda")
    fc = torch.zeros(2 * 64, device="cuda")
    _rejects(lib.af_avgpool(C.byref(_pool_desc((1, 4, 7, 7, 12), (4, 7, 7), "bf16")), _p(x), _p(out), 12, _st()), "multiple of 8")
    _rejects(lib.af_avgpool(C.byref(_pool_desc((1, 4, 7, 7, 6), (4, 7, 7), "f32")), _p(x), _p(out), 8, _st()), "multiple of 4")
    _rejects(lib.af_avgpool(C.byref(_pool_desc((1, 4, 7, 7, 8), (2, 3, 3), "f32", stride=2)), _p(x), _p(out), 8, _st()), "stride=1")
    _rejects(lib.af_avgpool(C.byref(_pool_desc((1, 4, 7, 7, 16), (4, 7, 7), "f32")), _p(x), _p(out), 15, _st()), "pooled_ld")
    bad = _pool_desc((1, 4, 7, 7, 16), (4, 7, 7), "f32")
    bad.wo = 2
    _rejects(lib.af_avgpool(C.byref(bad), _p(x), _p(out), 16, _st()), "output dims")
    _rejects(lib.af_avgpool_fc_scores(C.byref(_pool_desc((1, 4, 7, 7, 16), (4, 7, 7), "f32")), _p(x), _p(fc), _p(fc), 0,
                                      _p(out), _p(out), None, _st()), "avgpool_fc")
    _rejects(lib.af_avgpool_fc_scores(C.byref(_pool_desc((1, 4, 7, 7, 16), (4, 7, 7), "f32")), _p(x), _p(fc), _p(fc), 3,
                                      _p(out), _p(out), _p(out), _st()), "scores")
    torch.cuda.synchronize()
