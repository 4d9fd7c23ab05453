"""Inputs of the RetinaFace post-process edge cases, shared by test_detector_edges_host (which pins on the CPU the
properties each case was chosen for) and test_hip_detector_edges (which runs them through the kernels).  The seeds were
searched on the CPU until retinaface_ref.nms_ovr_margin of every case is at least EXACT_MARGIN."""
import functools

import numpy as np

from af_mi355x import retinaface as rf

import retinaface_ref as R

TIE_LEVELS = 64
# name -> (h, w, seed, bias, spread, distinct face logits or 0 for post_inputs as it is)
CASES = {
    "chunked": (704, 960, 22, 0.0, 2.0, 0),             # 27 720 candidates: sort_keys' running-set path, last chunk partial
    "chunked_ties": (704, 960, 22, 0.0, 2.0, TIE_LEVELS),
    "none": (240, 320, 30, -12.0, 2.0, 0),              # no score above 0.02
    "post_sparse": (240, 320, 11, -6.0, 4.0, 0),        # tests/golden/retinaface.json's post case of that name
    "all": (240, 320, 40, 0.0, 2.0, 0),                 # every anchor a candidate, one-shot sort
    "straddle": (240, 320, 53, -3.9, 0.2, 0),           # scores on both sides of 0.02
}
MIXED_BATCH = ("none", "post_sparse", "all", "straddle")


def quantised_inputs(h, w, seed, bias, spread, levels):
    """post_inputs' draws (same generator, same order), the face logits rounded to the centres of `levels` equal bins of
    bias +- spread before conf is formed: A / levels anchors share each score bit for bit"""
    a = rf.num_anchors(h, w)
    r = np.random.Generator(np.random.PCG64(seed))
    loc = r.normal(0, 1, (a, 4)).astype(np.float32)
    landms = r.normal(0, 1, (a, 10)).astype(np.float32)
    logit = bias + spread * ((r.permutation(a) + 0.5) / a * 2 - 1)
    q = np.clip(np.floor((logit - (bias - spread)) / (2 * spread) * levels), 0, levels - 1)
    logit = (bias - spread + (q + 0.5) * (2 * spread / levels)).astype(np.float32)
    p1 = (1.0 / (1.0 + np.exp(-logit.astype(np.float64)))).astype(np.float32)
    conf = np.stack([np.float32(1) - p1, p1], 1).astype(np.float32)
    return loc, conf, landms


@functools.lru_cache(maxsize=None)
def inputs(name):
    """(loc (A, 4), conf (A, 2), landms (A, 10)) f32 of case `name`; computed once, not to be written to"""
    h, w, seed, bias, spread, levels = CASES[name]
    out = quantised_inputs(h, w, seed, bias, spread, levels) if levels else R.post_inputs(h, w, seed, bias, spread)
    for t in out:
        t.setflags(write=False)
    return out


def size(name):
    return CASES[name][:2]


@functools.lru_cache(maxsize=None)
def sorted_dets(name):
    """what post_process hands to py_cpu_nms: the candidates' (x1 y1 x2 y2 score) in (score desc, anchor desc) order, cut
    to top_k; and the number of candidates before the cut"""
    h, w = size(name)
    loc, conf, landms = inputs(name)
    boxes, scores, _ = R.decode_np(loc, conf, landms, h, w)
    inds = np.nonzero(scores > np.float32(rf.CONF_THRESHOLD))[0]
    order = inds[np.lexsort((-inds, -scores[inds]))][:rf.TOP_K]
    dets = np.concatenate([boxes[order], scores[order, None]], 1).astype(np.float32)
    dets.setflags(write=False)
    return dets, int(inds.size)


@functools.lru_cache(maxsize=None)
def expected(name, keep_top_k=rf.KEEP_TOP_K):
    """post_process_np's rows of case `name`; computed once per keep_top_k, not to be written to"""
    h, w = size(name)
    rows = R.post_process_np(*inputs(name), h, w, keep_top_k=keep_top_k)
    rows.setflags(write=False)
    return rows
