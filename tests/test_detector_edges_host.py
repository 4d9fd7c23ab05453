"""CPU: what makes test_hip_detector_edges' exact post-process comparison fair, checked on the restatement alone (no
kernel runs here), and the fp64 references at the smallest frames."""
import os

import numpy as np
import pytest
import torch

from conftest import GOLDEN
from af_mi355x import onnx_min, retinaface as rf, synth

import retinaface_edge_cases as E
import retinaface_ref as R
import yunet_ref
from test_hip_retinaface import EXACT_MARGIN

SORT_LDS_KEYS, SORT_HALF = 16384, 8192          # csrc/af_detect.h: kSortLdsKeys, kSortHalf


def test_candidate_counts_are_what_each_case_was_chosen_for():
    h, w = E.size("chunked")
    a = rf.num_anchors(h, w)
    assert a == 27720
    for name in ("chunked", "chunked_ties"):
        dets, n = E.sorted_dets(name)
        assert n == a > SORT_LDS_KEYS and dets.shape[0] == rf.TOP_K == 5000
        # three merges of SORT_HALF keys into the running set, the last chunk partial
        assert -(-(n - SORT_HALF) // SORT_HALF) == 3 and (n - SORT_HALF) % SORT_HALF != 0
        assert E.expected(name).shape == (rf.KEEP_TOP_K, 15)
    dets, n = E.sorted_dets("none")
    assert n == 0 and dets.shape == (0, 5) and E.expected("none").shape == (0, 15)
    assert float(E.inputs("none")[1][:, 1].max()) < 1e-4 < rf.CONF_THRESHOLD
    assert E.sorted_dets("all")[1] == rf.num_anchors(240, 320) == 3160
    assert E.sorted_dets("post_sparse")[1] == 747
    score = E.inputs("straddle")[1][:, 1]
    above = int((score > np.float32(rf.CONF_THRESHOLD)).sum())
    assert E.sorted_dets("straddle")[1] == above and above >= 100 and score.size - above >= 100, (above, score.size)
    counts = [E.sorted_dets(n)[1] for n in E.MIXED_BATCH]
    assert len(set(counts)) == 4 and min(counts) == 0, counts
    assert {E.size(n) for n in E.MIXED_BATCH} == {(240, 320)}


def test_post_sparse_is_the_golden_case():
    name, ref = "post_sparse", np.load(os.path.join(GOLDEN, "retinaface_dets.npz"))["post_sparse"]
    assert np.array_equal(E.expected(name)[:, 4], ref[:, 4])
    np.testing.assert_allclose(E.expected(name), ref, rtol=1e-6, atol=1e-4)


def test_ties_only_where_they_were_put():
    loc, conf, landms = E.inputs("chunked")
    tloc, tconf, tlandms = E.inputs("chunked_ties")
    assert np.array_equal(loc, tloc) and np.array_equal(landms, tlandms)
    assert np.unique(tconf[:, 1]).size == E.TIE_LEVELS and np.unique(conf[:, 1]).size == conf.shape[0]
    s = E.sorted_dets("chunked")[0][:, 4]
    assert int((s[1:] == s[:-1]).sum()) == 0
    t = E.sorted_dets("chunked_ties")[0][:, 4]
    ties = int((t[1:] == t[:-1]).sum())
    assert t.size == 5000 and ties >= 100, ties
    # the top_k cut falls inside a group of equal scores, so the tie order decides which anchors reach the NMS at all
    assert int((tconf[:, 1] == t[-1]).sum()) > int((t == t[-1]).sum()) > 0
    # and the restatement's order within a group is the documented one: anchor index descending
    rows, anchors = R.post_process_np(tloc, tconf, tlandms, *E.size("chunked_ties"), return_anchors=True)
    same = rows[1:, 4] == rows[:-1, 4]
    assert same.sum() >= 100 and (anchors[1:][same] < anchors[:-1][same]).all()


@pytest.mark.parametrize("name", sorted(E.CASES))
def test_no_overlap_sits_on_the_nms_threshold(name):
    """min |ovr - 0.4| over every comparison py_cpu_nms makes on the score-ordered top 5 000 (the whole list, so it covers
    keep_top_k = 750 and 5 000 alike).  Measured: all 4.05e-05, chunked 6.01e-05, chunked_ties 6.01e-05, none inf (no
    box), post_sparse 1.15e-05, straddle 2.11e-04."""
    margin = R.nms_ovr_margin(E.sorted_dets(name)[0])
    print("%s: nms margin %.3g" % (name, margin))
    assert margin >= EXACT_MARGIN, margin


@pytest.mark.parametrize("h,w", [(1, 1), (17, 33)])
def test_retinaface_fp64_forward_on_tiny_frames(h, w):
    sd = synth.retinaface_state_dict(1, "sparse")
    frames = synth.retinaface_frames(2, h, w, seed=3)
    assert frames.shape == (2, h, w, 3) and frames.dtype == np.uint8
    loc, conf, landms = R.forward(sd, torch.from_numpy(frames), torch.float64)
    a = rf.num_anchors(h, w)
    assert a == sum(2 * (-(-h // s)) * (-(-w // s)) for s in (8, 16, 32)) and rf.priors(h, w).shape == (a, 4)
    assert tuple(loc.shape) == (2, a, 4) and tuple(conf.shape) == (2, a, 2) and tuple(landms.shape) == (2, a, 10)
    assert bool(torch.isfinite(loc).all()) and bool(torch.isfinite(landms).all())
    np.testing.assert_allclose(conf.sum(-1).numpy(), 1.0, rtol=0, atol=1e-12)
    rows = R.post_process_np(loc[0].numpy(), conf[0].numpy(), landms[0].numpy(), h, w)
    assert rows.ndim == 2 and rows.shape[1] == 15 and rows.shape[0] <= a
    # with every anchor a candidate the restatement still works on a 1 x 1 map per level
    every = np.stack([np.full(a, 0.25, np.float32), np.full(a, 0.75, np.float32)], 1)
    rows, anchors = R.post_process_np(loc[0].numpy(), every, landms[0].numpy(), h, w, return_anchors=True)
    assert 1 <= rows.shape[0] <= a and anchors[0] == a - 1 and np.isfinite(rows).all()


def test_yunet_fp64_graph_on_one_padded_tile():
    g = onnx_min.load(os.path.join(GOLDEN, "yunet_2023mar.onnx"))
    frame = np.full((1, 1, 3), 200, np.uint8)
    x = yunet_ref.preprocess(frame)
    assert tuple(x.shape) == (1, 3, 32, 32) and float(x.sum()) == 600.0
    outs = yunet_ref.run_graph(g, x)
    n = {8: 16, 16: 4, 32: 1}
    for s, cnt in n.items():
        for kind, ch in (("cls", 1), ("obj", 1), ("bbox", 4), ("kps", 10)):
            v = outs["%s_%d" % (kind, s)]
            assert v.shape == (1, cnt, ch) and np.isfinite(v).all(), (kind, s, v.shape)
    assert sum(n.values()) == 21
    cand = yunet_ref.decode({k: v[0] for k, v in outs.items()}, 1, 1, 0.0)
    assert cand.shape == (21, 15)
