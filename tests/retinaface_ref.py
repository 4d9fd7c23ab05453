"""Independent restatements for the RetinaFace tests: the network as a functional torch forward over the reference's
state-dict keys (any dtype, any device: fp64 on the CPU for the golden comparison, fp32 through MIOpen for the bench),
and batch_detect's post_process (decode, score cut, sort, py_cpu_nms, keep_top_k) in numpy."""
import math

import numpy as np
import torch
import torch.nn.functional as F

from af_mi355x import retinaface as rf


def _conv_bn(sd, x, conv, bn, stride=1, groups=1, leaky=None):
    w = sd[conv].to(x)
    x = F.conv2d(x, w, None, stride, w.shape[-1] // 2, 1, groups)
    x = F.batch_norm(x, sd[bn + ".running_mean"].to(x), sd[bn + ".running_var"].to(x), sd[bn + ".weight"].to(x),
                     sd[bn + ".bias"].to(x), False, 0.0, rf.BN_EPS)
    return F.leaky_relu(x, leaky) if leaky is not None else x


def forward(sd, frames_u8: torch.Tensor, dtype=torch.float64):
    """(B, H, W, 3) uint8 -> (loc (B, A, 4), softmax(conf) (B, A, 2), landms (B, A, 10)) in `dtype`"""
    x = frames_u8.to(dtype) - torch.tensor(rf.MEAN, dtype=dtype, device=frames_u8.device)
    x = x.permute(0, 3, 1, 2)
    x = _conv_bn(sd, x, rf._stage_key(0) + ".0.weight", rf._stage_key(0) + ".1", 2, leaky=0.1)
    taps = []
    for i, (cin, cout, st) in enumerate(rf.DW_BLOCKS, 1):
        p = rf._stage_key(i)
        x = _conv_bn(sd, x, p + ".0.weight", p + ".1", st, cin, leaky=0.1)
        x = _conv_bn(sd, x, p + ".3.weight", p + ".4", leaky=0.1)
        if i in (5, 11, 13):
            taps.append(x)
    o1 = _conv_bn(sd, taps[0], "fpn.output1.0.weight", "fpn.output1.1", leaky=0.1)
    o2 = _conv_bn(sd, taps[1], "fpn.output2.0.weight", "fpn.output2.1", leaky=0.1)
    o3 = _conv_bn(sd, taps[2], "fpn.output3.0.weight", "fpn.output3.1", leaky=0.1)
    o2 = o2 + F.interpolate(o3, size=o2.shape[2:], mode="nearest")
    o2 = _conv_bn(sd, o2, "fpn.merge2.0.weight", "fpn.merge2.1", leaky=0.1)
    o1 = o1 + F.interpolate(o2, size=o1.shape[2:], mode="nearest")
    o1 = _conv_bn(sd, o1, "fpn.merge1.0.weight", "fpn.merge1.1", leaky=0.1)
    outs = {"BboxHead": [], "ClassHead": [], "LandmarkHead": []}
    for l, f in enumerate((o1, o2, o3)):
        s = "ssh%d." % (l + 1)
        c3 = _conv_bn(sd, f, s + "conv3X3.0.weight", s + "conv3X3.1")
        c51 = _conv_bn(sd, f, s + "conv5X5_1.0.weight", s + "conv5X5_1.1", leaky=0.1)
        c5 = _conv_bn(sd, c51, s + "conv5X5_2.0.weight", s + "conv5X5_2.1")
        c72 = _conv_bn(sd, c51, s + "conv7X7_2.0.weight", s + "conv7X7_2.1", leaky=0.1)
        c7 = _conv_bn(sd, c72, s + "conv7x7_3.0.weight", s + "conv7x7_3.1")
        feat = F.relu(torch.cat([c3, c5, c7], 1))
        for head, k in rf.HEADS:
            y = F.conv2d(feat, sd["%s.%d.conv1x1.weight" % (head, l)].to(feat), sd["%s.%d.conv1x1.bias" % (head, l)].to(feat))
            outs[head].append(y.permute(0, 2, 3, 1).reshape(y.shape[0], -1, k))
    loc = torch.cat(outs["BboxHead"], 1)
    conf = F.softmax(torch.cat(outs["ClassHead"], 1), dim=-1)
    landms = torch.cat(outs["LandmarkHead"], 1)
    return loc, conf, landms


def decode_np(loc, conf, landms, h, w):
    """decode / decode_landm * [W, H] in fp32, the reference's operation order; (boxes (A, 4), scores (A,), landms (A, 10))"""
    p = rf.priors(h, w)
    f = np.float32
    loc, landms = np.asarray(loc, f), np.asarray(landms, f)
    v0, v1 = f(rf.VARIANCE[0]), f(rf.VARIANCE[1])
    cxcy = p[:, :2] + loc[:, :2] * v0 * p[:, 2:]
    wh = p[:, 2:] * np.exp(loc[:, 2:] * v1)
    x1y1 = cxcy - wh / f(2)
    boxes = np.concatenate([x1y1, wh + x1y1], 1) * np.array([w, h, w, h], f)
    lm = np.concatenate([p[:, :2] + landms[:, 2 * n:2 * n + 2] * v0 * p[:, 2:] for n in range(5)], 1)
    lm = lm * np.array([w, h] * 5, f)
    return boxes.astype(f), np.asarray(conf, f)[:, 1], lm.astype(f)


def nms_np(dets, thresh=rf.NMS_THRESHOLD, limit=None):
    """py_cpu_nms in fp32 over dets already in score order; stops after `limit` kept boxes"""
    x1, y1, x2, y2 = dets[:, 0], dets[:, 1], dets[:, 2], dets[:, 3]
    one = np.float32(1)
    areas = (x2 - x1 + one) * (y2 - y1 + one)
    order = np.arange(dets.shape[0])
    keep = []
    while order.size > 0 and (limit is None or len(keep) < limit):
        i = order[0]
        keep.append(i)
        xx1 = np.maximum(x1[i], x1[order[1:]])
        yy1 = np.maximum(y1[i], y1[order[1:]])
        xx2 = np.minimum(x2[i], x2[order[1:]])
        yy2 = np.minimum(y2[i], y2[order[1:]])
        ww = np.maximum(np.float32(0), xx2 - xx1 + one)
        hh = np.maximum(np.float32(0), yy2 - yy1 + one)
        inter = ww * hh
        ovr = inter / (areas[i] + areas[order[1:]] - inter)
        order = order[1:][ovr <= np.float32(thresh)]
    return keep


def post_process_np(loc, conf, landms, h, w, keep_top_k=rf.KEEP_TOP_K, return_anchors=False):
    """post_process on one frame's (A, 4) loc, (A, 2) conf, (A, 10) landms: (N, 15) rows x1 y1 x2 y2 score l0x .. l4y;
    exact score ties ordered by descending anchor index"""
    boxes, scores, lm = decode_np(loc, conf, landms, h, w)
    inds = np.nonzero(scores > np.float32(rf.CONF_THRESHOLD))[0]
    order = inds[np.lexsort((-inds, -scores[inds]))][:rf.TOP_K]
    dets = np.concatenate([boxes[order], scores[order, None]], 1).astype(np.float32)
    keep = nms_np(dets, limit=keep_top_k)
    rows = np.concatenate([dets[keep], lm[order][keep]], 1)
    return (rows, order[keep]) if return_anchors else rows


def nms_ovr_margin(dets, thresh=rf.NMS_THRESHOLD):
    """min |ovr - thresh| over the comparisons py_cpu_nms makes on score-ordered dets (kept box vs every remaining one)"""
    x1, y1, x2, y2 = dets[:, 0], dets[:, 1], dets[:, 2], dets[:, 3]
    one = np.float32(1)
    areas = (x2 - x1 + one) * (y2 - y1 + one)
    order = np.arange(dets.shape[0])
    best = math.inf
    while order.size > 1:
        i, rest = order[0], order[1:]
        ww = np.maximum(np.float32(0), np.minimum(x2[i], x2[rest]) - np.maximum(x1[i], x1[rest]) + one)
        hh = np.maximum(np.float32(0), np.minimum(y2[i], y2[rest]) - np.maximum(y1[i], y1[rest]) + one)
        inter = ww * hh
        ovr = inter / (areas[i] + areas[rest] - inter)
        best = min(best, float(np.abs(ovr.astype(np.float64) - thresh).min()))
        order = rest[ovr <= np.float32(thresh)]
    return best


def post_inputs(h, w, seed, bias, spread):
    """seeded raw head outputs for post_process alone (numpy PCG64): (loc (A, 4), conf (A, 2), landms (A, 10)) f32.  The
    face logits are a random permutation of A evenly spaced values in bias +- spread, so no two scores tie (the reference
    leaves the order of exact ties undefined)."""
    a = rf.num_anchors(h, w)
    r = np.random.Generator(np.random.PCG64(seed))
    loc = r.normal(0, 1, (a, 4)).astype(np.float32)
    landms = r.normal(0, 1, (a, 10)).astype(np.float32)
    logit = (bias + spread * ((r.permutation(a) + 0.5) / a * 2 - 1)).astype(np.float32)
    p1 = (1.0 / (1.0 + np.exp(-logit.astype(np.float64)))).astype(np.float32)
    conf = np.stack([np.float32(1) - p1, p1], 1).astype(np.float32)
    return loc, conf, landms
