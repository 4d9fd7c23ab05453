"""Writes tests/golden/lmk_disc.npz + .json: what the REFERENCE's own cli/test.py path makes of the raw landmark tracks already
committed in tests/golden/dual_video.npz - ``_seq_to_features`` with and without ``rot_invariant``
(dualrun/data/make_lmk_features.py), ``collate_pad`` (data/vox_ds.py), ``LMKDisc`` in fp64 with the seeded recipe weights,
``median_by_key`` and ``noisy_or`` (cli/test.py).

    python tools/gen_lmk_disc_golden.py [--reference DIR]

The reference files are loaded by path, as tools/gen_dual_video_golden.py loads them (``cv2`` and ``mediapipe`` are stand-ins by
name; nothing on the paths run here touches them).  tests/lmkdisc_ref.py (the numpy statement the kernels equal) is measured against
the recorded rows here and the figure goes into the json: tests/test_lmkdisc_host.py asserts at 8 x it.

Asserted before anything is written: the statement's unrotated rows equal the reference's bit for bit; every collated batch's
longest clip has T rows (a clip's logit depends on the padded length: DESIGN 24); every video has fewer than 8 tracks, so numpy's
``.sum()`` in ``noisy_or`` is the plain sequential sum; the statement's ``median_by_key`` / ``noisy_or`` results equal the
reference's exactly."""
import argparse
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for _p in ("oracle", "tests", "tools"):
    sys.path.insert(0, os.path.join(ROOT, _p))
sys.path.insert(0, ROOT)
import dualvideo_ref as R              # noqa: E402
import lmkdisc_ref as S                # noqa: E402
from gen_dual_video_golden import load_reference, write_npz      # noqa: E402

T = 8
WEIGHTS_SEED = 11
# the logit cases: (name, T, model variant, mask?, [(video, track, first, len)])
CLIPS_B6 = [(0, 2, 0, 8), (0, 1, 2, 5), (1, 1, 30, 1), (0, 1, 8, 8), (1, 0, 8, 8), (2, 0, 4, 3)]       # (0, 1, 8, 8) loses frame 9: 7 rows
CASES = [("b6", 8, "ff512", True, CLIPS_B6),
         ("b1", 8, "ff512", True, [(1, 1, 3, 8)]),
         ("t16", 16, "ff512", True, [(0, 2, 5, 16), (2, 0, 10, 1), (1, 1, 0, 9), (1, 1, 18, 12)]),
         ("nomask", 8, "ff512", False, [(0, 0, 0, 8), (0, 2, 21, 8), (1, 1, 24, 8), (2, 0, 3, 8)]),
         ("depth1", 8, "depth1", True, CLIPS_B6)]
VARIANTS = {"ff512": dict(d_model=256, nhead=4, num_layers=4, dim_ff=512), "depth1": dict(d_model=256, nhead=8, num_layers=1, dim_ff=384)}


def load_test_py(reference):
    """cli/test.py by path; its ``from data.vox_ds import ...`` and ``from model.dual_encoder import ...`` resolve on the dualrun
    directory that load_reference put on sys.path"""
    import importlib.util
    spec = importlib.util.spec_from_file_location("ref_lmk_test", os.path.join(reference, "dualrun", "cli", "test.py"))
    mod = importlib.util.module_from_spec(spec)
    sys.modules["ref_lmk_test"] = mod
    spec.loader.exec_module(mod)
    return mod


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reference", default=None)
    ap.add_argument("--out", default=os.path.join(ROOT, "tests", "golden", "lmk_disc"))
    opt = ap.parse_args()
    if opt.reference is None:
        import ref_import
        opt.reference = ref_import.REFERENCE_ROOT
    LM = load_reference(opt.reference)[0]
    TP = load_test_py(opt.reference)
    from af_mi355x import dualrun

    with open(os.path.join(ROOT, "tests", "golden", "dual_video.json")) as fh:
        src_doc = json.load(fh)
    src = np.load(os.path.join(ROOT, "tests", "golden", "dual_video.npz"))
    raw = [[src["v%d_t%d_lmk" % (vi, ti)] for ti in range(len(v["tracks"]))] for vi, v in enumerate(src_doc["videos"])]
    assert all(len(v) < 8 for v in raw)

    def ref_rows(lmk, rot):
        return LM._seq_to_features([f for f in lmk], rot_invariant=rot)[0]

    def collate(rows_list, frames):
        X, pad = TP.collate_pad([np.asarray(r, np.float32) for r in rows_list])
        assert X.shape[1] == frames, "a batch's longest clip must have T rows (got %d for T = %d)" % (X.shape[1], frames)
        return X, pad

    arrays = {}
    # ---- features: every clip_windows clip of every track, collated to T rows, with and without the rotation -------------------------
    clips, rows = [], {False: [], True: []}
    for vi, v in enumerate(src_doc["videos"]):
        for ti, t in enumerate(v["tracks"]):
            for s in t["clips"]:
                clips.append((vi, ti, s, T))
                for rot in (False, True):
                    rows[rot].append(ref_rows(raw[vi][ti][s:s + T], rot))
    nvalid = np.asarray([r.shape[0] for r in rows[False]], np.int32)
    assert [r.shape[0] for r in rows[True]] == nvalid.tolist() and nvalid.max() == T and (nvalid < T).sum() >= 2 and nvalid.min() >= 1
    d_rot = 0.0
    for rot in (False, True):
        X, pad = collate(rows[rot], T)
        assert np.array_equal((~pad).sum(1).numpy(), nvalid)
        arrays["ref_L_rot%d" % rot] = X.numpy()
        mine = np.stack([S.clip_features(raw[vi][ti][s:s + n], T=T, rot_invariant=rot)[0] for vi, ti, s, n in clips])
        if rot:
            d_rot = float(np.abs(mine - X.numpy()).max())
        else:
            assert np.array_equal(mine, X.numpy()), "the unrotated statement is no longer the reference bit for bit"
    arrays["ref_nvalid"] = nvalid
    assert 0 < d_rot < 1e-4, d_rot

    # ---- logits: the reference LMKDisc in fp64 on collated ragged clips --------------------------------------------------------------
    doc_cases, layouts, fp32_gap = [], {}, 0.0
    for name, frames, variant, masked, case_clips in CASES:
        kw = VARIANTS[variant]
        sd = dualrun.lmk_disc_synthetic_state_dict(R.LMK_DIM, seed=WEIGHTS_SEED, **kw)
        ref = TP.LMKDisc(in_dim=R.LMK_DIM, **kw)
        layouts[variant] = [[k, list(v.shape)] for k, v in ref.state_dict().items()]
        missing, unexpected = ref.load_state_dict(sd, strict=False)
        assert not missing and not unexpected, (missing, unexpected)
        ref = ref.eval()
        X, pad = collate([ref_rows(raw[vi][ti][s:s + n], False) for vi, ti, s, n in case_clips], frames)
        lengths = (~pad).sum(1).tolist()
        assert masked or min(lengths) == frames
        with torch.no_grad():
            z32 = ref(X, key_padding_mask=pad if masked else None)
            z64 = ref.double()(X.double(), key_padding_mask=pad if masked else None)
        fp32_gap = max(fp32_gap, float((z32.double() - z64).abs().max()))
        arrays["logits_" + name] = z64.numpy()
        doc_cases.append({"name": name, "T": frames, "variant": variant, "masked": masked, "clips": [list(c) for c in case_clips],
                          "lengths": lengths})
    assert [c["lengths"] for c in doc_cases[:3]] == [[8, 5, 1, 7, 8, 3], [8], [16, 1, 9, 12]], [c["lengths"] for c in doc_cases[:3]]

    # ---- the reduction: test.py's median_by_key and noisy_or on the statement's clip scores of the committed seeded logits -----------
    logits = src["red_logits"]
    assert len(logits) == len(clips)
    groups, keys = [], []
    for vi, v in enumerate(src_doc["videos"]):
        groups.append([[c for c, (cv, ct, _, _) in enumerate(clips) if (cv, ct) == (vi, ti)] for ti in range(len(v["tracks"]))])
    for vi, ti, _, _ in clips:
        keys.append("/data/%s/track_%s" % (src_doc["videos"][vi]["name"], src_doc["videos"][vi]["tracks"][ti]["key"]))
    assert any(len(g) % 2 == 0 and len(g) >= 2 for v in groups for g in v)
    reduction = {}
    for invert in (False, True):
        scores = [float(s) for s in S.clip_score(logits, invert)]
        track2p = TP.median_by_key(scores, keys)
        per_video = []
        for vi, v in enumerate(groups):
            tk = [keys[g[0]] for g in v]
            per_video.append({"tracks": [[k, track2p[k]] for k in tk], "score_video_or": TP.noisy_or([track2p[k] for k in tk]), "n_tracks": len(tk)})
        _, mine = S.reduce_lmk(logits, nvalid, groups, invert)
        for g, w in zip(mine, per_video):
            assert [float(x) for x in g["track_score"]] == [p for _, p in w["tracks"]] and float(g["video_score"]) == w["score_video_or"]
        reduction["invert" if invert else "plain"] = per_video
    edge = [[0.0], [1.0], [0.0, 1.0], [0.5, 1.0, 0.0], []]
    doc = {"what": "the reference's cli/test.py path on the tracks of dual_video.npz (tools/gen_lmk_disc_golden.py)",
           "numpy": np.__version__, "torch": torch.__version__.split("+")[0], "T": T, "weights_seed": WEIGHTS_SEED, "variants": VARIANTS,
           "state_dict": layouts, "clips": [list(c) for c in clips], "cases": doc_cases,
           "measured": {"rot_statement_vs_reference": d_rot, "unrotated_statement_vs_reference": 0.0, "reference_fp32_vs_fp64_logit": fp32_gap},
           "reduction": reduction, "track_keys": keys, "noisy_or_edges": [[p, TP.noisy_or(p)] for p in edge]}
    write_npz(opt.out + ".npz", arrays)
    with open(opt.out + ".json", "w") as fh:
        json.dump(doc, fh, indent=1, sort_keys=True)
    print("wrote %s.npz (%d bytes) and .json; %d clips, nvalid %s; max |statement - reference| with rotation %.3g; reference fp32 vs fp64 "
          "logit %.3g" % (opt.out, os.path.getsize(opt.out + ".npz"), len(clips), nvalid.tolist(), d_rot, fp32_gap))


if __name__ == "__main__":
    main()
