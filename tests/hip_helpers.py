"""Thin test-side wrappers that call libafhip.so through its C ABI (af_mi355x._lib) on torch-owned
device buffers.  Layout conversions (NCDHW <-> NDHWC) are done with torch: they are test scaffolding."""
import ctypes as C

import torch

TORCH_DT = {"f32": torch.float32, "bf16": torch.bfloat16, "f16": torch.float16}
# stated tolerances of the per-layer and whole-net parity tests, relative to max|reference output|
LAYER_TOL = {"f32": 2e-5, "f16": 4e-3, "bf16": 3e-2}


def lib():
    from af_mi355x import _lib
    return _lib


def _p(t):
    return None if t is None else C.c_void_p(t.data_ptr())


def _stream():
    return C.c_void_p(torch.cuda.current_stream().cuda_stream)


def to_ndhwc(x_ncdhw, dtype):
    return x_ncdhw.permute(0, 2, 3, 4, 1).contiguous().to(device="cuda", dtype=TORCH_DT[dtype])


def to_ncdhw(x_ndhwc):
    return x_ndhwc.permute(0, 4, 1, 2, 3).float().cpu()


def fold_bn(sd, prefix):
    L = lib()
    ts = [sd[prefix + s].float().cuda().contiguous() for s in (".weight", ".bias", ".running_mean", ".running_var")]
    c = ts[0].numel()
    cpad = L.lib.af_padded_channels(c)            # the conv kernels read scale/shift over the padded channel tile
    scale = torch.zeros(cpad, device="cuda")
    shift = torch.zeros(cpad, device="cuda")
    L.check(L.lib.af_fold_bn(_p(ts[0]), _p(ts[1]), _p(ts[2]), _p(ts[3]), 1e-5, c, _p(scale), _p(shift), _stream()), "fold_bn")
    return scale, shift


def _pack(w_oidhw, dtype, scale=None):
    """conv weights in the kernels' packed layout; ``scale``: the BN scale folded into the rows in fp32, before the one rounding
    (af_pack_conv_weight_scaled)"""
    L = lib()
    code = L.DTYPE_CODES[dtype]
    shape = tuple(w_oidhw.shape)
    wsrc = w_oidhw.float().cuda().contiguous()
    nbytes = L.lib.af_packed_conv_weight_bytes(*shape, code)
    packed = torch.empty(nbytes // (4 if dtype == "f32" else 2), dtype=TORCH_DT[dtype], device="cuda")
    if scale is None:
        L.check(L.lib.af_pack_conv_weight(_p(wsrc), *shape, code, _p(packed), _stream()), "pack_conv_weight")
    else:
        L.check(L.lib.af_pack_conv_weight_scaled(_p(wsrc), _p(scale), *shape, code, _p(packed), _stream()), "pack_conv_weight_scaled")
    torch.cuda.current_stream().synchronize()
    return packed


_pack_plain = _pack          # the name the experiment scripts under tools/ call


def _desc(shape_ndhwc, cout, kernel, dtype, stride=(1, 1, 1), pad=(0, 0, 0), relu=True, dout=None, tpool=0):
    """ConvDesc of a conv over an input of shape (N,T,H,W,C)"""
    L = lib()
    n, t, h, w, cin = shape_ndhwc
    return L.conv_desc(n, (t, h, w), cin, cout, kernel, stride, pad, relu, L.DTYPE_CODES[dtype], dout, tpool)


def conv_bn_act(x_ndhwc, w_oidhw, scale, shift, stride, pad, relu, dtype, residual=None, out=None, out_ld=0, tpool=False,
                workspace="auto"):
    """workspace: "auto" = a caller-owned scratch of af_conv_workspace_bytes(d) bytes (the split-K path of small layers),
    None = no workspace (the layer must then run unsplit)."""
    L = lib()
    n = x_ndhwc.shape[0]
    cout, cin2, kt, kh, kw = w_oidhw.shape
    assert x_ndhwc.shape[-1] == cin2
    d = _desc(x_ndhwc.shape, cout, (kt, kh, kw), dtype, stride, pad, relu, tpool=tpool)
    conv_bn_act.last_variant = L.lib.af_conv_variant(C.byref(d), None)     # which kernel the library picks for this layer
    packed = _pack(w_oidhw, dtype)
    if out is None:
        q = 2 if int(tpool) == 2 else 1
        out = torch.empty((n, d.to // 2 if int(tpool) == 1 else d.to, d.ho // q, d.wo // q, cout), dtype=TORCH_DT[dtype], device="cuda")
    ws_bytes = L.lib.af_conv_workspace_bytes(C.byref(d)) if workspace == "auto" else 0
    ws = torch.empty(max(ws_bytes // 4, 4), dtype=torch.float32, device="cuda") if ws_bytes else None
    conv_bn_act.last_workspace_bytes = ws_bytes
    L.check(L.lib.af_conv3d_bn_act(C.byref(d), _p(x_ndhwc), _p(packed), _p(scale), _p(shift), _p(residual), _p(out),
                                   out_ld, _p(ws), ws_bytes, _stream()), "conv3d_bn_act")
    torch.cuda.current_stream().synchronize()          # ws / packed stay referenced until the launch has run
    return out


def conv_work_units(shape_ndhwc, cout, kernel, dtype, pad=(0, 0, 0), relu=True, tpool=0, shape2_ndhwc=None, stride2=(1, 1, 1)):
    """(variant, work units, workgroups) of the af_conv3d_bn_act launch of this layer (stride 1) over an input of shape (N,T,H,W,C):
    the library's own answer (af_conv_work_units), no tensor needed.  ``tpool``: the fused pool of the descriptor;
    ``shape2_ndhwc`` / ``stride2``: the second input of an af_conv3d_dual_bn_act launch (a 1x1x1 at that stride onto the same output)"""
    L = lib()
    d = _desc(shape_ndhwc, cout, kernel, dtype, pad=pad, relu=relu, tpool=tpool)
    d2 = None if shape2_ndhwc is None else _desc(shape2_ndhwc, cout, (1, 1, 1), dtype, stride=stride2, dout=(d.to, d.ho, d.wo))
    p2 = None if d2 is None else C.byref(d2)
    units, groups = C.c_int64(0), C.c_int(0)
    v = L.lib.af_conv_work_units(C.byref(d), p2, C.byref(units), C.byref(groups))
    L.check(min(v, 0), "conv_work_units")
    assert v == L.lib.af_conv_variant(C.byref(d), p2)
    return v, units.value, groups.value


def conv_variant(shape_ndhwc, cout, kernel, dtype, stride=(1, 1, 1), pad=(0, 0, 0), shape2_ndhwc=None, stride2=(1, 1, 1)):
    """the kernel the library picks for this layer (af_conv_variant), no tensor needed; also for the paths that are not cut into
    units, which af_conv_work_units refuses"""
    L = lib()
    d = _desc(shape_ndhwc, cout, kernel, dtype, stride=stride, pad=pad)
    d2 = None if shape2_ndhwc is None else _desc(shape2_ndhwc, cout, (1, 1, 1), dtype, stride=stride2, dout=(d.to, d.ho, d.wo))
    return L.lib.af_conv_variant(C.byref(d), None if d2 is None else C.byref(d2))


def compare(got, want, tol, what):
    """NaN masks equal, infinities equal, the finite rest within tol * max|finite want|"""
    nan_w = torch.isnan(want)
    assert torch.equal(torch.isnan(got), nan_w), "%s: %d NaN in the output, %d in the reference" % (what, int(torch.isnan(got).sum()), int(nan_w.sum()))
    inf_w = torch.isinf(want)
    assert torch.equal(torch.isinf(got), inf_w) and torch.equal(got[inf_w], want[inf_w]), "%s: infinities differ" % what
    fin = ~(nan_w | inf_w)
    ref = want[fin].abs().max().item() + 1e-9
    err = (got[fin] - want[fin]).abs().max().item()
    print("%s: max|d| / max|want| = %.3e (tolerance %.3e)" % (what, err / ref, tol))
    assert err <= tol * ref, "%s: max|d|=%.3e vs max|ref|=%.3e, tolerance %.3e" % (what, err, ref, tol)


def bc_descs(shape_ndhwc, cmid, cout, dtype):
    """(db, dc) of a fused b (1x3x3) + c (1x1x1) pair over an input of shape (N,T,H,W,C)"""
    n, t, h, w, cin = shape_ndhwc
    return _desc(shape_ndhwc, cmid, (1, 3, 3), dtype, pad=(0, 1, 1)), _desc((n, t, h, w, cmid), cout, (1, 1, 1), dtype)


def conv_bc(x_ndhwc, wb_oidhw, bn_b, wc_oidhw, bn_c, residual, dtype, out=None, out_ld=0):
    """relu(bn_c(conv1x1x1(relu(bn_b(conv1x3x3(x))))) + residual) as one af_conv3d_bc_bn_act launch; None if the library
    does not fuse this pair (af_conv_bc_fusable).  ``out`` / ``out_ld``: rows of a wider caller-owned buffer."""
    L = lib()
    n, t, h, w, cin = x_ndhwc.shape
    cmid, cout = wb_oidhw.shape[0], wc_oidhw.shape[0]
    db, dc = bc_descs(x_ndhwc.shape, cmid, cout, dtype)
    if not L.lib.af_conv_bc_fusable(C.byref(db), C.byref(dc)):
        return None
    pb, pc = _pack(wb_oidhw, dtype), _pack(wc_oidhw, dtype)
    if out is None:
        out = torch.empty((n, t, h, w, cout), dtype=TORCH_DT[dtype], device="cuda")
    L.check(L.lib.af_conv3d_bc_bn_act(C.byref(db), _p(x_ndhwc), _p(pb), _p(bn_b[0]), _p(bn_b[1]), C.byref(dc), _p(pc), _p(bn_c[0]),
                                      _p(bn_c[1]), _p(residual), _p(out), out_ld, _stream()), "conv3d_bc_bn_act")
    torch.cuda.current_stream().synchronize()
    return out


def abc_descs(shape_ndhwc, inner, kta, cout, dtype):
    """(da, db, dc, d1) of a bottleneck block (a: kT x 1 x 1, b: 1x3x3, c: 1x1x1, d1: its 1x1x1 projection shortcut) over an input
    of shape (N,T,H,W,C)"""
    n, t, h, w, cin = shape_ndhwc
    return tuple(_desc((n, t, h, w, ci), co, k, dtype, pad=p, dout=(t, h, w)) for ci, co, k, p in (
        (cin, inner, (kta, 1, 1), (kta // 2, 0, 0)), (inner, inner, (1, 3, 3), (0, 1, 1)),
        (inner, cout, (1, 1, 1), (0, 0, 0)), (cin, cout, (1, 1, 1), (0, 0, 0))))


def abc_work_units(shape_ndhwc, inner, kta, cout, dtype, proj=False):
    """(patch rows, time segments, units = workgroups) of the af_block_abc_bn_act launch of this block - the library's own answer
    (af_block_abc_work_units), no tensor needed; None if the library does not fuse the block"""
    L = lib()
    da, db, dc, d1 = abc_descs(shape_ndhwc, inner, kta, cout, dtype)
    ph, ts, units = C.c_int(0), C.c_int(0), C.c_int64(0)
    rc = L.lib.af_block_abc_work_units(C.byref(da), C.byref(db), C.byref(dc), C.byref(d1) if proj else None, C.byref(ph), C.byref(ts),
                                       C.byref(units))
    L.check(min(rc, 0), "block_abc_work_units")
    assert rc == L.lib.af_block_abc_fusable(C.byref(da), C.byref(db), C.byref(dc), C.byref(d1) if proj else None)
    return (ph.value, ts.value, units.value) if rc else None


def block_abc(x_ndhwc, wa_oidhw, bn_a, wb_oidhw, bn_b, wc_oidhw, bn_c, dtype, out_ld=0, w1_oidhw=None, bn_1=None, out=None):
    """relu(shortcut(x) + bn_c(c(relu(bn_b(b(relu(bn_a(a(x)))))))))  as one af_block_abc_bn_act launch (a: kT x 1 x 1, b: 1x3x3,
    c: 1x1x1; shortcut = x, or bn_1(conv1x1x1_1(x)) with w1 / bn_1: the projection form with folded weights); None if the
    library does not fuse this block (af_block_abc_fusable).  ``out``: rows of a caller-owned buffer (with ``out_ld``)."""
    L = lib()
    n, t, h, w, cin = x_ndhwc.shape
    inner, kta, cout = wa_oidhw.shape[0], wa_oidhw.shape[2], wc_oidhw.shape[0]
    da, db, dc, d1 = abc_descs(x_ndhwc.shape, inner, kta, cout, dtype)
    proj = w1_oidhw is not None
    if not L.lib.af_block_abc_fusable(C.byref(da), C.byref(db), C.byref(dc), C.byref(d1) if proj else None):
        return None
    pa, pb = _pack(wa_oidhw, dtype), _pack(wb_oidhw, dtype)
    if proj:
        pc, p1 = _pack(wc_oidhw, dtype, bn_c[0]), _pack(w1_oidhw, dtype, bn_1[0])
        sc3, sh3 = torch.ones_like(bn_c[0]), (bn_c[1] + bn_1[1]).contiguous()
    else:
        pc, p1, sc3, sh3 = _pack(wc_oidhw, dtype), None, bn_c[0], bn_c[1]
    ld = out_ld or cout
    if out is None:
        out = torch.full((n, t, h, w, ld), 7.0, dtype=TORCH_DT[dtype], device="cuda")
    L.check(L.lib.af_block_abc_bn_act(C.byref(da), _p(x_ndhwc), _p(pa), _p(bn_a[0]), _p(bn_a[1]), C.byref(db), _p(pb), _p(bn_b[0]),
                                      _p(bn_b[1]), C.byref(dc), _p(pc), _p(sc3), _p(sh3), C.byref(d1) if proj else None, _p(p1),
                                      _p(out), out_ld, _stream()), "block_abc_bn_act")
    torch.cuda.current_stream().synchronize()
    return out


CA_FORMS = ("plain", "plain-CWL", "projection")          # AF_CA_PLAIN, AF_CA_PLAIN_CWL, AF_CA_PROJECTION


def ca_descs(dims, ctrunk, dtype, proj=False, cmid=64, cout_a=64, cin1=64):
    """(dc, d1 or None, da) of a fused c (1x1x1, cmid -> ctrunk) + a (3x1x1, ctrunk -> cout_a) pair over dims = (n, t, h, w);
    proj: with the 1x1x1 projection shortcut d1 (cin1 -> ctrunk)"""
    n, t, h, w = dims
    dc = _desc((n, t, h, w, cmid), ctrunk, (1, 1, 1), dtype)
    da = _desc((n, t, h, w, ctrunk), cout_a, (3, 1, 1), dtype, pad=(1, 0, 0))
    return dc, (_desc((n, t, h, w, cin1), ctrunk, (1, 1, 1), dtype) if proj else None), da


def ca_work_units(dims, ctrunk, dtype, proj=False):
    """(tiles, workgroups, form, pixels per tile) of the af_conv3d_ca_bn_act launch of this pair - the library's own answer
    (af_conv_ca_work_units), no tensor needed; None if the library does not fuse the pair.  form: one of CA_FORMS"""
    L = lib()
    dc, d1, da = ca_descs(dims, ctrunk, dtype, proj)
    p1 = None if d1 is None else C.byref(d1)
    tiles, groups, form, pix = C.c_int64(0), C.c_int(0), C.c_int(-1), C.c_int(0)
    rc = L.lib.af_conv_ca_work_units(C.byref(dc), p1, C.byref(da), C.byref(tiles), C.byref(groups), C.byref(form), C.byref(pix))
    L.check(min(rc, 0), "conv_ca_work_units")
    assert rc == L.lib.af_conv_ca_fusable(C.byref(dc), p1, C.byref(da))
    return (tiles.value, groups.value, CA_FORMS[form.value], pix.value) if rc else None


def cpa_descs(dims, ctrunk, dtype, cmid=64, cout_a=128):
    """(dc, da) of the fused stage boundary: c (1x1x1, cmid -> ctrunk, the frame-pair max behind it) over dims = (n, t, h, w) and a
    (3x1x1, ctrunk -> cout_a) over the pooled tensor"""
    n, t, h, w = dims
    return (_desc((n, t, h, w, cmid), ctrunk, (1, 1, 1), dtype, tpool=1),
            _desc((n, t // 2, h, w, ctrunk), cout_a, (3, 1, 1), dtype, pad=(1, 0, 0)))


def cpa_work_units(dims, ctrunk, dtype, x_sub):
    """(tiles, workgroups) of the af_conv3d_cpa_bn_act launch of this pair (af_conv_cpa_work_units); None if it is not fused"""
    L = lib()
    dc, da = cpa_descs(dims, ctrunk, dtype)
    tiles, groups = C.c_int64(0), C.c_int(0)
    rc = L.lib.af_conv_cpa_work_units(C.byref(dc), C.byref(da), x_sub, C.byref(tiles), C.byref(groups))
    L.check(min(rc, 0), "conv_cpa_work_units")
    assert rc == L.lib.af_conv_cpa_fusable(C.byref(dc), C.byref(da), x_sub)
    return (tiles.value, groups.value) if rc else None


def conv_ca(b_ndhwc, wc_oidhw, bn_c, res_ndhwc, wa_oidhw, bn_a, dtype, x0_ndhwc=None, w1_oidhw=None, bn_1=None, out_x=None, out_a=None):
    """x = relu(bn_c(conv1x1x1(b)) + res), a_out = relu(bn_a(conv3x1x1(x))) as one af_conv3d_ca_bn_act launch -> (x, a_out);
    with x0 / w1 / bn_1 (a projection block) x = relu(bn_c(c(b)) + bn_1(conv1x1x1_1(x0))) and res must be None.
    None if the library does not fuse this pair (af_conv_ca_fusable).  ``out_x`` / ``out_a``: caller-owned contiguous outputs."""
    L = lib()
    n, t, h, w, cmid = b_ndhwc.shape
    ctrunk, cout_a = wc_oidhw.shape[0], wa_oidhw.shape[0]
    dc, d1, da = ca_descs((n, t, h, w), ctrunk, dtype, x0_ndhwc is not None, cmid, cout_a, 0 if x0_ndhwc is None else x0_ndhwc.shape[-1])
    if not L.lib.af_conv_ca_fusable(C.byref(dc), None if d1 is None else C.byref(d1), C.byref(da)):
        return None
    pa = _pack(wa_oidhw, dtype)
    x = torch.empty((n, t, h, w, ctrunk), dtype=TORCH_DT[dtype], device="cuda") if out_x is None else out_x
    a_out = torch.empty((n, t, h, w, cout_a), dtype=TORCH_DT[dtype], device="cuda") if out_a is None else out_a
    if d1 is None:
        pc, p1, sc, sf = _pack(wc_oidhw, dtype), None, bn_c[0], bn_c[1]
    else:           # both weight sets carry their BN scale, scale = ones, shift = the summed shifts (as the engine does)
        pc, p1 = _pack(wc_oidhw, dtype, bn_c[0]), _pack(w1_oidhw, dtype, bn_1[0])
        sc, sf = torch.ones(L.lib.af_padded_channels(ctrunk), device="cuda"), (bn_c[1] + bn_1[1]).contiguous()
    L.check(L.lib.af_conv3d_ca_bn_act(C.byref(dc), _p(b_ndhwc), _p(pc), None if d1 is None else C.byref(d1), _p(x0_ndhwc), _p(p1), _p(sc),
                                      _p(sf), _p(res_ndhwc), _p(x), C.byref(da), _p(pa), _p(bn_a[0]), _p(bn_a[1]), _p(a_out), _stream()),
            "conv3d_ca_bn_act")
    torch.cuda.current_stream().synchronize()
    return x, a_out


def conv_cpa(b_ndhwc, wc_oidhw, bn_c, res_ndhwc, wa_oidhw, bn_a, dtype, x_sub, out_x=None, out_a=None):
    """x = relu(bn_c(conv1x1x1(b)) + res), xp = max over frame pairs, a_out = relu(bn_a(conv3x1x1(xp))) as one
    af_conv3d_cpa_bn_act launch -> (xp or its even (h, w) positions, a_out); None if the library does not fuse this pair.
    ``out_x`` / ``out_a``: caller-owned contiguous outputs."""
    L = lib()
    n, t, h, w, cmid = b_ndhwc.shape
    ctrunk, cout_a = wc_oidhw.shape[0], wa_oidhw.shape[0]
    dc, da = cpa_descs((n, t, h, w), ctrunk, dtype, cmid, cout_a)
    if not L.lib.af_conv_cpa_fusable(C.byref(dc), C.byref(da), x_sub):
        return None
    pc, pa = _pack(wc_oidhw, dtype), _pack(wa_oidhw, dtype)
    xs = (n, t // 2, h // 2, w // 2, ctrunk) if x_sub == 2 else (n, t // 2, h, w, ctrunk)
    x = torch.full(xs, 7.0, dtype=TORCH_DT[dtype], device="cuda") if out_x is None else out_x
    a_out = torch.full((n, t // 2, h, w, cout_a), 7.0, dtype=TORCH_DT[dtype], device="cuda") if out_a is None else out_a
    L.check(L.lib.af_conv3d_cpa_bn_act(C.byref(dc), _p(b_ndhwc), _p(pc), _p(bn_c[0]), _p(bn_c[1]), _p(res_ndhwc), _p(x), x_sub,
                                       C.byref(da), _p(pa), _p(bn_a[0]), _p(bn_a[1]), _p(a_out), _stream()), "conv3d_cpa_bn_act")
    torch.cuda.current_stream().synchronize()
    return x, a_out


def conv_dual(x_ndhwc, w_oidhw, bn, x2_ndhwc, w2_oidhw, bn2, stride2, dtype, out=None, out_ld=0, tpool=0):
    """relu(bn(conv1x1x1(x)) + bn2(conv1x1x1_strided(x2))) as one af_conv3d_dual_bn_act launch; ``out`` / ``out_ld``: rows of a
    wider caller-owned buffer, ``tpool`` = 1: the frame-pair max fused behind the ReLU."""
    L = lib()
    (scale, shift), (scale2, shift2) = bn, bn2
    n, t, h, w, cin = x_ndhwc.shape
    cout = w_oidhw.shape[0]
    d = _desc(x_ndhwc.shape, cout, (1, 1, 1), dtype, tpool=tpool)
    d2 = _desc(x2_ndhwc.shape, cout, (1, 1, 1), dtype, stride=stride2, dout=(t, h, w))
    if out is None:
        out = torch.empty((n, t // 2 if int(tpool) == 1 else t, h, w, cout), dtype=TORCH_DT[dtype], device="cuda")
    ones = torch.ones(L.lib.af_padded_channels(cout), device="cuda")
    # keep every device buffer referenced until the launch has been enqueued (the caching allocator would
    # otherwise hand the first packed weight's memory to the second)
    pw, pw2, shift_sum = _pack(w_oidhw, dtype, scale), _pack(w2_oidhw, dtype, scale2), (shift + shift2).contiguous()
    conv_dual.last_variant = L.lib.af_conv_variant(C.byref(d), C.byref(d2))
    L.check(L.lib.af_conv3d_dual_bn_act(C.byref(d), _p(x_ndhwc), _p(pw), C.byref(d2), _p(x2_ndhwc), _p(pw2), _p(ones),
                                        _p(shift_sum), _p(out), out_ld, _stream()), "conv3d_dual_bn_act")
    torch.cuda.current_stream().synchronize()
    return out


def pack_input_f32(x_ncdhw_dev, dtype):
    L = lib()
    code = L.DTYPE_CODES[dtype]
    n, c, t, h, w = x_ncdhw_dev.shape
    nbytes = L.lib.af_stem_input_bytes(n, t, h, w, code)
    buf = torch.zeros(nbytes // (4 if dtype == "f32" else 2), dtype=TORCH_DT[dtype], device="cuda")
    s = x_ncdhw_dev.stride()
    L.check(L.lib.af_pack_input_f32(_p(x_ncdhw_dev), n, t, h, w, s[0], s[1], s[2], s[3], s[4], code, _p(buf), _stream()),
            "pack_input_f32")
    return buf


def pack_input_u8(clips_dev, mean, std, dtype):
    L = lib()
    code = L.DTYPE_CODES[dtype]
    n, t, h, w, _ = clips_dev.shape
    nbytes = L.lib.af_stem_input_bytes(n, t, h, w, code)
    buf = torch.zeros(nbytes // (4 if dtype == "f32" else 2), dtype=TORCH_DT[dtype], device="cuda")
    m = (C.c_float * 3)(*mean)
    s = (C.c_float * 3)(*std)
    L.check(L.lib.af_pack_input_u8(_p(clips_dev), n, t, h, w, m, s, code, _p(buf), _stream()), "pack_input_u8")
    return buf


def _stem_desc(dims, w_oidhw, dtype):
    """the stems' conv: 3 channels in, stride (1,2,2), pad (kT // 2, 3, 3) over a 7x7 window"""
    n, t, h, w = dims
    cout, _, kt, kh, kw = w_oidhw.shape
    return _desc((n, t, h, w, 3), cout, (kt, kh, kw), dtype, stride=(1, 2, 2), pad=(kt // 2, 3, 3),
                 dout=(t, (h + 6 - 7) // 2 + 1, (w + 6 - 7) // 2 + 1))


def stem_conv(stem_in, dims, w_oidhw, scale, shift, dtype):
    L = lib()
    code = L.DTYPE_CODES[dtype]
    n, t, h, w = dims
    cout, _, kt, kh, kw = w_oidhw.shape
    d = _stem_desc((n, t, h, w), w_oidhw, dtype)
    wsrc = w_oidhw.float().cuda().contiguous()
    nbytes = L.lib.af_packed_stem_weight_bytes(cout, kt, kh, code)
    packed = torch.empty(nbytes // (4 if dtype == "f32" else 2), dtype=TORCH_DT[dtype], device="cuda")
    L.check(L.lib.af_pack_stem_weight(_p(wsrc), cout, kt, kh, kw, code, _p(packed), _stream()), "pack_stem_weight")
    out = torch.empty((n, d.to, d.ho, d.wo, cout), dtype=TORCH_DT[dtype], device="cuda")
    L.check(L.lib.af_stem_conv_bn_relu(C.byref(d), _p(stem_in), _p(packed), _p(scale), _p(shift), _p(out), _stream()),
            "stem_conv_bn_relu")
    return out


def stem_conv_pool(stem_in, dims, w_oidhw, scale, shift, dtype):
    """conv + BN + ReLU + max-pool [1,3,3]/[1,2,2]/[0,1,1] as one launch (16-bit dtypes)."""
    L = lib()
    code = L.DTYPE_CODES[dtype]
    n, t, h, w = dims
    cout, _, kt, kh, kw = w_oidhw.shape
    d = _stem_desc((n, t, h, w), w_oidhw, dtype)
    wsrc = w_oidhw.float().cuda().contiguous()
    nbytes = L.lib.af_packed_stem_weight_bytes(cout, kt, kh, code)
    packed = torch.empty(nbytes // 2, dtype=TORCH_DT[dtype], device="cuda")
    L.check(L.lib.af_pack_stem_weight(_p(wsrc), cout, kt, kh, kw, code, _p(packed), _stream()), "pack_stem_weight")
    out = torch.empty((n, d.to, (d.ho - 1) // 2 + 1, (d.wo - 1) // 2 + 1, cout), dtype=TORCH_DT[dtype], device="cuda")
    L.check(L.lib.af_stem_conv_bn_relu_maxpool(C.byref(d), _p(stem_in), _p(packed), _p(scale), _p(shift), _p(out), _stream()),
            "stem_conv_bn_relu_maxpool")
    torch.cuda.current_stream().synchronize()
    return out


def stem3_conv_pool(x_ncdhw_dev, w_oidhw, scale, shift, dtype, u8=None, mean=None, std=None):
    """the K-packed fused stem (rgb3 input layout): pack (fp32 strided source, or uint8 clips) + conv + BN + ReLU + max-pool"""
    L = lib()
    code = L.DTYPE_CODES[dtype]
    if u8 is None:
        n, _, t, h, w = x_ncdhw_dev.shape
    else:
        n, t, h, w, _ = u8.shape
    nbytes = L.lib.af_stem_input_bytes_rgb3(n, t, h, w, code)
    buf = torch.zeros(nbytes // 2, dtype=TORCH_DT[dtype], device="cuda")
    if u8 is None:
        s = x_ncdhw_dev.stride()
        L.check(L.lib.af_pack_input_f32_rgb3(_p(x_ncdhw_dev), n, t, h, w, s[0], s[1], s[2], s[3], s[4], code, _p(buf), _stream()),
                "pack_input_f32_rgb3")
    else:
        m, sd_ = (C.c_float * 3)(*mean), (C.c_float * 3)(*std)
        L.check(L.lib.af_pack_input_u8_rgb3(_p(u8), n, t, h, w, m, sd_, code, _p(buf), _stream()), "pack_input_u8_rgb3")
    cout, _, kt, kh, kw = w_oidhw.shape
    d = _stem_desc((n, t, h, w), w_oidhw, dtype)
    wsrc = w_oidhw.float().cuda().contiguous()
    packed = torch.empty(L.lib.af_packed_stem_weight_bytes_rgb3(kt, code) // 2, dtype=TORCH_DT[dtype], device="cuda")
    L.check(L.lib.af_pack_stem_weight_rgb3(_p(wsrc), cout, kt, code, _p(packed), _stream()), "pack_stem_weight_rgb3")
    out = torch.empty((n, d.to, (d.ho - 1) // 2 + 1, (d.wo - 1) // 2 + 1, cout), dtype=TORCH_DT[dtype], device="cuda")
    L.check(L.lib.af_stem_conv_bn_relu_maxpool_rgb3(C.byref(d), _p(buf), _p(packed), _p(scale), _p(shift), _p(out), _stream()),
            "stem_conv_bn_relu_maxpool_rgb3")
    torch.cuda.current_stream().synchronize()
    return out


def maxpool(x_ndhwc, kernel, stride, pad, dtype):
    L = lib()
    n, t, h, w, c = x_ndhwc.shape
    d = L.pool_desc(n, (t, h, w), c, kernel, stride, pad, L.DTYPE_CODES[dtype])
    out = torch.empty((n, d.to, d.ho, d.wo, c), dtype=TORCH_DT[dtype], device="cuda")
    L.check(L.lib.af_maxpool3d(C.byref(d), _p(x_ndhwc), _p(out), _stream()), "maxpool3d")
    return out


def avgpool_fc(x_ndhwc, pool, fc_w, fc_b, dtype):
    L = lib()
    n, t, h, w, c = x_ndhwc.shape
    d = L.pool_desc(n, (t, h, w), c, pool, (1, 1, 1), (0, 0, 0), L.DTYPE_CODES[dtype])
    k = fc_w.shape[0]
    pos = d.to * d.ho * d.wo
    pooled = torch.empty((n, pos, c), device="cuda")
    logits = torch.empty((n, pos * k), device="cuda")
    fw, fb = fc_w.float().cuda().contiguous(), fc_b.float().cuda().contiguous()
    L.check(L.lib.af_avgpool_fc(C.byref(d), _p(x_ndhwc), _p(fw), _p(fb), k, _p(pooled), _p(logits), _stream()), "avgpool_fc")
    return pooled, logits
