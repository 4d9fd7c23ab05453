"""The fp64 reference of test_hip_engine_replay.py: the value the dataflow graph (engine_graph.py) gives a tensor at a set of
positions ("windows"), all channels, from snapshots looked up by graph name.  Plain torch: a gather of taps and a matmul per conv,
no vendor convolution.

Rounding model (the kernel tests' own, tests/test_hip_conv_fused.py): operands are taken as stored; weights are rounded once to the
storage type; where a launch adds a c conv and its projection shortcut in one accumulator (dual, the projection forms of ca and abc)
the BN scale is folded into the weights in fp32 before that one rounding and the two shifts are summed; a tensor made and read inside
one launch is rounded where the kernel rounds it (``rounded``).  BatchNorm otherwise in fp64 from the state dict, by the conv's name.
"""
import math

import torch

from af_mi355x.arch import BN_EPS

TORCH_DT = {"f32": torch.float32, "bf16": torch.bfloat16, "f16": torch.float16}
# relative to max|want| over the launch's windows: the kernel tests' own (test_hip_layers / test_hip_conv_matrix / test_hip_conv_fused)
TOL = {"lone": {"f32": 2e-6, "f16": 1.5e-3, "bf16": 1.2e-2}, "dual": {"f32": 5e-6, "f16": 3e-3, "bf16": 2.4e-2},
       "ca": {"f16": 1.5e-3, "bf16": 1.2e-2}, "ca_a": {"f16": 2.25e-3, "bf16": 1.8e-2}, "bc": {"f16": 2e-3, "bf16": 1.6e-2},
       "abc": {"f16": 3e-3, "bf16": 2.4e-2}, "abc_proj": {"f16": 4e-3, "bf16": 3e-2}}
LONE_KINDS = ("conv", "pool", "stem", "stem_pool", "stem3_pool", "tstem", "tstem_pool3")
HEAD_KINDS = ("head", "avgpool", "linear", "tt_head")
# every launch kind the replay has a reference for (test_host_cpu.py holds the plans to it)
REFERENCED_KINDS = LONE_KINDS + ("dual", "ca", "cpa", "bc", "abc") + HEAD_KINDS


def tolerance(launch, operand, dtype):
    kind = launch.kind
    if kind in ("ca", "cpa"):
        key = "ca_a" if operand == "dst_a" else "ca"
    elif kind == "abc":
        key = "abc_proj" if launch.convs["branch1"] is not None else "abc"
    elif kind in ("bc", "dual"):
        key = kind
    else:
        assert kind in LONE_KINDS, kind
        key = "lone"
    return TOL[key][dtype]             # (KeyError: a fused launch in fp32 - none ships, none has a reference)


def rounding(launch):
    """(roles whose output the kernel rounds to the storage type inside the launch, whether c and branch1 are folded)"""
    kind, cv = launch.kind, launch.convs
    if kind == "dual":
        return (), True
    if kind == "ca":
        return ("block",), cv["branch1"] is not None
    if kind == "cpa":
        return ("block",), False
    if kind == "abc":
        return ("a", "b"), cv["branch1"] is not None
    if kind == "bc":
        return ("b",), False
    return (), False


def window_rows(N, T, H, W, seed):
    """Sorted flattened rows r = ((n T + t) H + h) W + w of the windows of an (N, T, H, W) output: 1x2x2 boxes at the eight corners of
    the first and the last clip; four rows astride r = k m for m in 128, 224, 256, 512 and k = 1, a middle one and the last; the first
    and last four rows; across each of the first and last clip boundaries one interior pixel; 16 seeded random 1x2x2 boxes."""
    rows, R = set(), N * T * H * W

    def box(n, t, h, w):
        for dh in (0, 1):
            for dw in (0, 1):
                rows.add(((n * T + t) * H + min(h + dh, H - 1)) * W + min(w + dw, W - 1))

    for n in {0, N - 1}:
        for t in {0, T - 1}:
            for h in {0, max(H - 2, 0)}:
                for w in {0, max(W - 2, 0)}:
                    box(n, t, h, w)
    for m in (128, 224, 256, 512):
        last = (R - 1) // m
        for k in {1, max(last // 2, 1), last}:
            if k >= 1 and k * m < R:
                rows.update(r for r in range(k * m - 2, k * m + 2) if 0 <= r < R)
    rows.update(range(min(4, R)))
    rows.update(range(max(R - 4, 0), R))
    if N > 1:
        for n in {0, N - 2}:
            rows.add(((n * T + T - 1) * H + H // 2) * W + W // 2)
            rows.add((((n + 1) * T) * H + H // 2) * W + W // 2)
    gen = torch.Generator().manual_seed(seed)
    for _ in range(16):
        n, t, h, w = (int(torch.randint(0, d, (1,), generator=gen)) for d in (N, T, H, W))
        box(n, t, h, w)
    return sorted(rows)


def rows_to_pos(rows, dims, device):
    T, H, W = dims
    r = torch.as_tensor(rows, dtype=torch.int64, device=device)
    return torch.stack([r // (T * H * W), (r // (H * W)) % T, (r // W) % H, r % W], 1)


def _expand(pos, kernel, stride, pad, dims):
    """input positions (P, taps, 4) of a window op at output positions ``pos`` over an input of ``dims``, and which are inside"""
    dev = pos.device
    kt, kh, kw = kernel
    off = torch.stack(torch.meshgrid(torch.arange(kt, device=dev), torch.arange(kh, device=dev), torch.arange(kw, device=dev),
                                     indexing="ij"), -1).reshape(-1, 3)                        # taps in (kt, kh, kw) order
    st, pd = torch.tensor(stride, device=dev), torch.tensor(pad, device=dev)
    thw = pos[:, None, 1:] * st - pd + off[None]
    lim = torch.tensor(dims, device=dev)
    valid = ((thw >= 0) & (thw < lim)).all(-1)
    return torch.cat([pos[:, None, :1].expand(-1, off.shape[0], -1), thw], -1), valid


class Reference:
    def __init__(self, graph, sd, dtype, device):
        self.g, self.sd, self.dtype, self.tdt, self.dev = graph, sd, dtype, TORCH_DT[dtype], device
        self.snap = {}             # graph name -> (tensor (N, T', H', W', C) as stored, sub)

    def put(self, name, tensor, sub=1):
        self.snap[name] = (tensor, sub)

    def _p(self, key):
        return self.sd[key].detach().to(self.dev)

    def bn(self, cv):
        w, b, m, v = (self._p(cv.bn_key + s).double() for s in (".weight", ".bias", ".running_mean", ".running_var"))
        scale = w / torch.sqrt(v + BN_EPS)
        return scale, b - m * scale

    def weight(self, cv, fold):
        w = self._p(cv.conv + ".weight").float()
        assert tuple(w.shape) == cv.weight_shape
        if fold:                   # the scale in fp32, into the fp32 weights, before the one rounding (PackedWeights.w_folded)
            scale = self._p(cv.bn_key + ".weight").float() / torch.sqrt(self._p(cv.bn_key + ".running_var").float() + BN_EPS)
            w = w * scale.view(-1, 1, 1, 1, 1)
        return w.to(self.tdt).double().reshape(cv.cout, cv.cin, -1)

    # -- values ------------------------------------------------------------------------------------------
    def gather(self, name, pos):
        node = self.g[name]
        if name not in self.snap:
            if node.op == "concat":
                return torch.cat([self.gather(r, pos) for r in node.reads], 1)
            raise KeyError("no snapshot of %s" % name)
        t, sub = self.snap[name]
        h, w = pos[:, 2], pos[:, 3]
        if sub == 2:
            assert bool(((h % 2 == 0) & (w % 2 == 0)).all()), "%s is held at its even (h, w) only" % name
            h, w = h // 2, w // 2
        return t[pos[:, 0], pos[:, 1], h, w].double()

    def lookup(self, name, tp, valid, fill, ctx):
        """values of ``name`` at positions tp (P, taps, 4), ``fill`` outside; each distinct position is evaluated once"""
        T, H, W = self.g[name].dims
        key = ((tp[..., 0] * T + tp[..., 1]) * H + tp[..., 2]) * W + tp[..., 3]
        key = torch.where(valid, key, torch.full_like(key, -1))
        uniq, inv = torch.unique(key.reshape(-1), return_inverse=True)
        inside = uniq >= 0
        vals = self.value(name, rows_to_pos(uniq[inside], (T, H, W), self.dev), ctx)
        table = torch.full((uniq.numel(), vals.shape[1]), fill, dtype=torch.float64, device=self.dev)
        table[inside] = vals
        return table[inv].view(tp.shape[0], tp.shape[1], -1)

    def value(self, name, pos, ctx):
        """fp64 (P, C) of graph tensor ``name`` at ``pos`` (P, 4) = (n, t, h, w).  ctx = (made, rounded, folded): the names computed
        inside the launch (everything else is a snapshot), those of them rounded to the storage type, the convs whose scale is folded."""
        made, rounded, folded = ctx
        if name not in made:
            return self.gather(name, pos)
        node = self.g[name]
        if node.op == "conv":
            cv = node.conv
            if cv.pool_after_bn is not None:
                p = cv.pool_after_bn
                pp, valid = _expand(pos, p.kernel, p.stride, p.pad, cv.out_dims(*self.g[node.reads[0]].dims))
                y = self._conv_bn(node, pp.reshape(-1, 4), ctx).view(pp.shape[0], pp.shape[1], -1)
                y = torch.where(valid[..., None], y, torch.full_like(y, -math.inf)).amax(1)
            else:
                y = self._conv_bn(node, pos, ctx)
            if cv.relu:
                y = torch.relu(y)
        elif node.op == "add":
            y = torch.relu(self.value(node.reads[0], pos, ctx) + self.value(node.reads[1], pos, ctx))
        elif node.op == "pool":
            tp, valid = _expand(pos, node.pool.kernel, node.pool.stride, node.pool.pad, self.g[node.reads[0]].dims)
            y = self.lookup(node.reads[0], tp, valid, -math.inf, ctx).amax(1)
        else:
            raise ValueError("no windowed reference for a %s node" % node.op)
        if name in rounded:
            y = y.to(self.tdt).double()
        return y

    def _conv_bn(self, node, pos, ctx):
        cv, fold = node.conv, node.name in ctx[2]
        tp, valid = _expand(pos, cv.kernel, cv.stride, cv.pad, self.g[node.reads[0]].dims)
        x = self.lookup(node.reads[0], tp, valid, 0.0, ctx)                  # (P, taps, cin)
        y = torch.einsum("ptc,oct->po", x, self.weight(cv, fold))
        scale, shift = self.bn(cv)
        return y + shift if fold else y * scale + shift

    # -- the heads, dense --------------------------------------------------------------------------------
    def avgpool(self, name):
        """fp64 (N, positions, C) of an avgpool / tokens node from the snapshot of what it reads"""
        node = self.g[name]
        x = self.snap[node.reads[0]][0].double().permute(0, 4, 1, 2, 3)
        k = node.pool.kernel
        y = x.unfold(2, k[0], 1).unfold(3, k[1], 1).unfold(4, k[2], 1).mean((-3, -2, -1))
        return y.permute(0, 2, 3, 4, 1).reshape(y.shape[0], -1, y.shape[1])

    def linear(self, pooled, prefix):
        return pooled.double() @ self._p(prefix + ".weight").double().t() + self._p(prefix + ".bias").double()


def compare(got, want, what):
    """(max|d| / max|want|, max|want|, share of non-zero want) - NaN masks equal, infinities equal, the finite rest measured
    (hip_helpers.compare's rule)"""
    got = got.double()
    nan_w = torch.isnan(want)
    assert torch.equal(torch.isnan(got), nan_w), "%s: %d NaN in the output, %d in the reference" % (what, int(torch.isnan(got).sum()), int(nan_w.sum()))
    inf_w = torch.isinf(want)
    assert torch.equal(torch.isinf(got), inf_w) and torch.equal(got[inf_w], want[inf_w]), "%s: infinities differ" % what
    fin = ~(nan_w | inf_w)
    ref = want[fin].abs().max().item()
    err = (got[fin] - want[fin]).abs().max().item()
    return err / (ref + 1e-9), ref, float((want[fin] != 0).double().mean())
