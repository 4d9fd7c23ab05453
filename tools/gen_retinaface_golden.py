"""Generates tests/golden/retinaface*.{json,npz} from the reference's own, unmodified RetinaFace code.

    python tools/gen_retinaface_golden.py --reference <checkout of the reference project>

Runs only where the reference exists.  test_tools/ct/detection/alignment.py is loaded by file path; the one torchvision
name it imports (models._utils.IntermediateLayerGetter) is given a minimal stand-in in sys.modules.  Nothing from the
reference is copied into the repository: only its outputs are written.  The reference runs on the CPU with oneDNN off,
MKL_CBWR=COMPATIBLE and one thread.

Written:
  retinaface.json            the state-dict layout, prior-table hashes and sampled rows, per case the frame seed, the
                             margins that make exact comparison meaningful, and the post_process cases' parameters
  retinaface_raw_<HxW>*.npz  raw loc / softmax(conf) / landms of the reference module in fp64 (stored as fp32): every
                             anchor at 240x320 and 359x641, a fixed sample plus every kept anchor at 1080x1920
  retinaface_dets.npz        batch_detect's detections (fp32) per case and post_process's rows per post-process case
"""
import argparse
import hashlib
import importlib.util
import json
import math
import os
import sys
import types
from collections import OrderedDict

os.environ.setdefault("MKL_CBWR", "COMPATIBLE")
os.environ.setdefault("OMP_NUM_THREADS", "1")
os.environ.setdefault("MKL_NUM_THREADS", "1")

import numpy as np
import torch
import torch.nn as nn

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import af_mi355x  # noqa: E402,F401
from af_mi355x import retinaface as rf, synth  # noqa: E402
import retinaface_ref as R  # noqa: E402

GOLDEN = os.path.join(ROOT, "tests", "golden")
WEIGHT_SEED = 1
SIZES = [(240, 320), (359, 641), (1080, 1920)]
RECIPES = ["sparse", "dense"]
MARGIN = 1e-4
SAMPLE_1080 = 4096
SEED_TRIES = 8
POST_CASES = [  # (name, h, w, seed, face-logit bias, spread): seeded raw tensors for post_process alone
    ("post_sparse", 240, 320, 11, -6.0, 4.0),
    ("post_many", 359, 641, 12, 0.0, 2.0),      # > top_k candidates
]


class IntermediateLayerGetter(nn.ModuleDict):
    """stand-in for torchvision.models._utils.IntermediateLayerGetter: the backbone's children up to the last returned
    one, run in order; returns {return name: output} of the returned children"""

    def __init__(self, model, return_layers):
        layers = OrderedDict()
        todo = dict(return_layers)
        for name, module in model.named_children():
            layers[name] = module
            todo.pop(name, None)
            if not todo:
                break
        super().__init__(layers)
        self.return_layers = dict(return_layers)

    def forward(self, x):
        out = OrderedDict()
        for name, module in self.items():
            x = module(x)
            if name in self.return_layers:
                out[self.return_layers[name]] = x
        return out


def load_reference(root):
    tv = types.ModuleType("torchvision")
    tv.models = types.ModuleType("torchvision.models")
    tv.models._utils = types.ModuleType("torchvision.models._utils")
    tv.models._utils.IntermediateLayerGetter = IntermediateLayerGetter
    sys.modules.update({"torchvision": tv, "torchvision.models": tv.models, "torchvision.models._utils": tv.models._utils})
    path = os.path.join(root, "altfreezing", "test_tools", "ct", "detection", "alignment.py")
    spec = importlib.util.spec_from_file_location("ref_alignment", path)
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def case_margins(loc, conf, landms, h, w, rows):
    """min |score - 0.02| over all anchors; min gap between consecutive output scores and, above top_k candidates, between
    the top_k-th and the next score; min |ovr - 0.4| over the comparisons NMS makes"""
    s = np.asarray(conf, np.float32)[:, 1].astype(np.float64)
    thr = float(np.abs(s - rf.CONF_THRESHOLD).min())
    out = rows[:, 4].astype(np.float64)
    gap = float(np.abs(np.diff(out)).min()) if out.size > 1 else math.inf
    cand = np.sort(s[s > rf.CONF_THRESHOLD])[::-1]
    if cand.size > rf.TOP_K:
        gap = min(gap, float(cand[rf.TOP_K - 1] - cand[rf.TOP_K]))
    ovr = R.nms_ovr_margin(sorted_candidates(loc, conf, landms, h, w))
    return {"score_vs_threshold": thr, "consecutive_scores": gap, "ovr_vs_threshold": ovr}


def sorted_candidates(loc, conf, landms, h, w):
    boxes, scores, _ = R.decode_np(loc, conf, landms, h, w)
    inds = np.nonzero(scores > np.float32(rf.CONF_THRESHOLD))[0]
    order = inds[np.lexsort((-inds, -scores[inds]))][:rf.TOP_K]
    return np.concatenate([boxes[order], scores[order, None]], 1)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reference", required=True, help="root of the reference project checkout")
    args = ap.parse_args()
    torch.set_num_threads(1)
    ref = load_reference(args.reference)
    out = {"source": "reference test_tools/ct/detection/alignment.py (RetinaFace cfg_mnet, PriorBox, post_process, "
                     "batch_detect), PyTorch CPU, oneDNN off, one thread", "weight_seed": WEIGHT_SEED}
    with torch.backends.mkldnn.flags(enabled=False):
        net32 = ref.RetinaFace(cfg=ref.cfg_mnet, phase="test").eval()
        layout = [(k, list(v.shape)) for k, v in net32.state_dict().items()]
        out["layout"] = layout
        out["num_floats"] = int(sum(v.numel() for k, v in net32.state_dict().items() if not k.endswith("num_batches_tracked")))
        priors = {}
        for h, w in SIZES:
            p = ref.PriorBox(ref.cfg_mnet, image_size=(h, w)).forward().numpy()
            idx = np.linspace(0, p.shape[0] - 1, 64).astype(int)
            priors["%dx%d" % (h, w)] = {"n": int(p.shape[0]), "sha256": hashlib.sha256(p.astype(np.float32).tobytes()).hexdigest(),
                                        "idx": idx.tolist(), "rows": p[idx].tolist()}
        out["priors"] = priors
        cases, dets, raws = [], {}, {}
        for recipe in RECIPES:
            sd = synth.retinaface_state_dict(WEIGHT_SEED, recipe)
            net32.load_state_dict(sd, strict=True)
            net64 = ref.RetinaFace(cfg=ref.cfg_mnet, phase="test").eval()
            net64.load_state_dict(sd, strict=True)
            net64 = net64.double()
            for h, w in SIZES:
                chosen, best = None, -1.0
                for fseed in range(100, 100 + SEED_TRIES):
                    frames = synth.retinaface_frames(1, h, w, seed=fseed)
                    x = torch.from_numpy(frames).double() - torch.tensor([104, 117, 123], dtype=torch.float64)
                    with torch.no_grad():
                        loc, conf, landms = (t[0].numpy() for t in net64(x.permute(0, 3, 1, 2)))
                    rows64 = R.post_process_np(loc, conf, landms, h, w)
                    m = case_margins(loc, conf, landms, h, w, rows64)
                    worst = min(m.values())
                    if worst > best:
                        chosen, best = (fseed, frames, loc, conf, landms, m), worst
                    if worst > MARGIN:
                        break
                fseed, frames, loc, conf, landms, m = chosen
                m["exact"] = bool(min(m.values()) > MARGIN)
                name = "%s_%dx%d" % (recipe, h, w)
                det = ref.batch_detect(net32, frames, "cpu")[0]
                rows = np.array([np.concatenate([b, [s], l.ravel()]) for b, l, s in det], np.float32).reshape(-1, 15)
                ncand = int((conf[:, 1] > rf.CONF_THRESHOLD).sum())
                full_kept = len(R.post_process_np(loc, conf, landms, h, w, keep_top_k=None))
                if recipe == "dense":
                    assert ncand > rf.TOP_K and full_kept > rf.KEEP_TOP_K or (h, w) != (1080, 1920), (name, ncand, full_kept)
                else:
                    assert 0 < ncand < 20000 and (conf[:, 1] > 0.5).any(), (name, ncand)
                dets[name] = rows
                if (h, w) == (1080, 1920):
                    _, kept_anchors = R.post_process_np(loc, conf, landms, h, w, return_anchors=True)
                    idx = np.union1d(np.linspace(0, loc.shape[0] - 1, SAMPLE_1080).astype(np.int64), kept_anchors)
                else:
                    idx = np.arange(loc.shape[0])
                raws[name] = (idx, loc[idx], conf[idx], landms[idx])
                cases.append({"name": name, "recipe": recipe, "h": h, "w": w, "frame_seed": fseed, "candidates": ncand,
                              "kept_uncut": full_kept, "detections": int(rows.shape[0]), "margins": m})
                print(name, cases[-1], flush=True)
        out["cases"] = cases
        post = []
        cfg = ref.cfg_mnet
        for name, h, w, seed, bias, spread in POST_CASES:
            loc, conf, landms = R.post_inputs(h, w, seed, bias, spread)
            prior = ref.PriorBox(cfg, image_size=(h, w)).forward()
            scale = torch.tensor([w, h, w, h], dtype=torch.float32)
            scale1 = torch.tensor([w, h] * 5, dtype=torch.float32)
            res = ref.post_process(torch.from_numpy(loc), torch.from_numpy(conf), torch.from_numpy(landms), prior, cfg, scale,
                                   scale1, 1, rf.CONF_THRESHOLD, rf.TOP_K, rf.NMS_THRESHOLD, rf.KEEP_TOP_K)
            rows = np.array([np.concatenate([b, [s], l.ravel()]) for b, l, s in res], np.float32).reshape(-1, 15)
            dets[name] = rows
            m = case_margins(loc, conf, landms, h, w, rows)
            ncand = int((conf[:, 1] > rf.CONF_THRESHOLD).sum())
            assert m["consecutive_scores"] > 0 and m["score_vs_threshold"] > 0, (name, m)     # identical inputs on both sides
            if name == "post_many":
                assert ncand > rf.TOP_K and rows.shape[0] == rf.KEEP_TOP_K, (ncand, rows.shape)
            post.append({"name": name, "h": h, "w": w, "seed": seed, "bias": bias, "spread": spread, "candidates": ncand,
                         "detections": int(rows.shape[0]), "margins": m})
            print(name, post[-1], flush=True)
        out["post_cases"] = post
    with open(os.path.join(GOLDEN, "retinaface.json"), "w") as f:
        json.dump(out, f, indent=1)
    np.savez(os.path.join(GOLDEN, "retinaface_dets.npz"), **dets)
    groups = {"240x320": ["sparse_240x320", "dense_240x320"], "359x641_sparse": ["sparse_359x641"],
              "359x641_dense": ["dense_359x641"], "1080x1920": ["sparse_1080x1920", "dense_1080x1920"]}
    for g, names in groups.items():
        arrs = {}
        for n in names:
            idx, loc, conf, landms = raws[n]
            arrs.update({n + "/idx": idx.astype(np.int32), n + "/loc": loc.astype(np.float32), n + "/conf": conf.astype(np.float32),
                         n + "/landms": landms.astype(np.float32)})
        np.savez(os.path.join(GOLDEN, "retinaface_raw_%s.npz" % g), **arrs)



if __name__ == "__main__":
    main()
