"""Host (no GPU): the numpy statement tests/lmkdisc_ref.py against what the reference's cli/test.py path returned
(tests/golden/lmk_disc.*, made by tools/gen_lmk_disc_golden.py from the tracks of dual_video.npz), the special cases of the rotation
and of noisy-OR, and ``LMKDisc``'s state dict and ``load``."""
import numpy as np
import pytest
import torch

from conftest import load_json, load_npz
import dualvideo_ref as R
import lmkdisc_ref as S
from af_mi355x import dualrun

F32 = np.float32


@pytest.fixture(scope="module")
def golden():
    doc, st, src_doc, src = load_json("lmk_disc.json"), load_npz("lmk_disc.npz"), load_json("dual_video.json"), load_npz("dual_video.npz")
    raw = [[src["v%d_t%d_lmk" % (vi, ti)] for ti in range(len(v["tracks"]))] for vi, v in enumerate(src_doc["videos"])]
    groups = [[[c for c, (cv, ct, _, _) in enumerate(doc["clips"]) if (cv, ct) == (vi, ti)] for ti in range(len(v))] for vi, v in enumerate(raw)]
    return doc, st, raw, groups, src["red_logits"]


def test_unrotated_zero_padded_rows_equal_the_reference_bit_for_bit(golden):
    doc, st, raw, _, _ = golden
    got = [S.clip_features(raw[vi][ti][s:s + n], T=doc["T"]) for vi, ti, s, n in doc["clips"]]
    assert np.array_equal(np.stack([g[0] for g in got]), st["ref_L_rot0"])
    assert [g[1] for g in got] == st["ref_nvalid"].tolist()
    assert doc["measured"]["unrotated_statement_vs_reference"] == 0.0
    short = [i for i, n in enumerate(st["ref_nvalid"]) if n < doc["T"]]
    assert len(short) >= 2
    for i in short:                                           # collate_pad's rows: +0.0, sign bit clear
        pad = st["ref_L_rot0"][i, st["ref_nvalid"][i]:]
        assert not pad.any() and not np.signbit(pad).any() and not np.signbit(got[i][0][st["ref_nvalid"][i]:]).any()


def test_rotated_rows_sit_within_8x_the_measured_figure_of_the_reference(golden):
    doc, st, raw, _, _ = golden
    tol = 8 * doc["measured"]["rot_statement_vs_reference"]
    assert 0 < tol < 1e-4
    got = np.stack([S.clip_features(raw[vi][ti][s:s + n], T=doc["T"], rot_invariant=True)[0] for vi, ti, s, n in doc["clips"]])
    d = np.abs(got - st["ref_L_rot1"])
    print("max |statement - reference| with rotation %.3g (recorded %.3g)" % (d.max(), doc["measured"]["rot_statement_vs_reference"]))
    assert d.max() <= tol
    pts = got.reshape(len(got), doc["T"], 66, 2)
    for i, n in enumerate(st["ref_nvalid"]):                  # the mouth line is horizontal, left corner to the left, nose at the origin
        assert (np.abs(pts[i, :n, S.PT_MR, 1] - pts[i, :n, S.PT_ML, 1]) <= 1e-6).all()
        assert (pts[i, :n, S.PT_MR, 0] > pts[i, :n, S.PT_ML, 0]).all() and not pts[i, :n, S.PT_NOSE].any() and not pts[i, n:].any()


def test_rotation_special_cases():
    assert S.rotation(F32(0.75), F32(0)) == (F32(1), F32(0))                    # dy = 0: exactly 1 and 0
    c, s = S.rotation(F32(0.75), F32(-0.0))
    assert c == 1 and s == 0
    c, s = S.rotation(F32(0), F32(2.5))                                         # dx = 0: a quarter turn back
    assert c == 0 and s == -1
    c, s = S.rotation(F32(0), F32(-2.5))
    assert c == 0 and s == 1
    c, s = S.rotation(F32(-3), F32(0))                                          # dx < 0: half a turn
    assert c == -1 and s == 0
    c, s = S.rotation(F32(-3), F32(4))
    assert c == F32(-0.6) and s == F32(-0.8)
    for z in (F32(0), F32(-0.0)):                                               # dx = dy = 0: atan2(0, 0) = 0
        assert S.rotation(z, F32(0)) == (F32(1), F32(0)) and S.rotation(F32(0), z) == (F32(1), F32(0))
    rng = np.random.default_rng(0)                                              # and it is what the trigonometry says, to fp32
    for dx, dy in rng.normal(0, 1, (200, 2)).astype(F32):
        th = np.arctan2(np.float64(dy), np.float64(dx))
        c, s = S.rotation(dx, dy)
        assert abs(np.float64(c) - np.cos(-th)) <= 2.0 ** -24 and abs(np.float64(s) - np.sin(-th)) <= 2.0 ** -24
    row = np.zeros((66, 2), F32)                                                # a vertical mouth line: (x, y) -> (y, -x)
    row[S.PT_ML], row[S.PT_MR], row[5] = (0.25, -0.5), (0.25, 0.5), (0.375, 0.125)
    out = S.rotate_row(row.reshape(-1)).reshape(66, 2)
    assert out[5].tolist() == [0.125, -0.375] and out[S.PT_ML].tolist() == [-0.5, -0.25] and out[S.PT_MR].tolist() == [0.5, -0.25]


def test_zero_padding_and_a_clip_longer_than_T(golden):
    _, _, raw, _, _ = golden
    L, nv = S.clip_features(raw[0][2][:3], T=8)
    assert nv == 3 and L[:3].any() and not L[3:].any()
    L, nv = S.clip_features(raw[0][2][:9], T=8)
    assert nv == 0 and not L.any()
    L, nv = S.clip_features(raw[0][1][9:10], T=8)                              # the ml == mr frame alone
    assert nv == 0 and not L.any()


def test_reduction_equals_the_reference_exactly(golden):
    doc, st, _, groups, logits = golden
    for name, invert in (("plain", False), ("invert", True)):
        score, got = S.reduce_lmk(logits, st["ref_nvalid"], groups, invert)
        assert score.dtype == np.float64
        for g, w in zip(got, doc["reduction"][name]):
            assert [float(x) for x in g["track_score"]] == [p for _, p in w["tracks"]]
            assert float(g["video_score"]) == w["score_video_or"] and g["n_tracks"] == w["n_tracks"]
    plain, inv = S.clip_score(logits), S.clip_score(logits, True)
    assert np.array_equal(inv, 1.0 - R.sigmoid(logits).astype(np.float64)) and np.array_equal(plain, R.sigmoid(logits).astype(np.float64))
    even = [g for v in groups for g in v if len(g) % 2 == 0]
    assert even and S.median_by_key(plain[even[0]], ["k"] * len(even[0]))["k"] == R.mid_median(plain[even[0]])


def test_noisy_or_clips_scores_of_exactly_zero_and_one(golden):
    doc = golden[0]
    for p, want in doc["noisy_or_edges"]:
        assert S.noisy_or(p) == want
    assert S.noisy_or([]) == 0.0
    assert S.noisy_or([0.0]) == 1.0 - np.exp(np.log1p(-1e-6)) and 0 < S.noisy_or([0.0]) < 1.1e-6
    assert S.noisy_or([1.0]) == 1.0 - np.exp(np.log1p(-(1 - 1e-6))) and 1 - 1.1e-6 < S.noisy_or([1.0]) < 1
    logits = np.asarray([40, -40, 40, -40], F32)                                # scores that clip at both ends
    score, out = S.reduce_lmk(logits, np.full(4, 8), [[[0], [1]], [[2, 3]], [[0]]])
    assert score[0] == 1.0 and 0 < score[1] < 1e-17
    assert out[0]["video_score"] == S.noisy_or([1.0, score[1]]) and out[1]["track_score"][0] == (score[2] + score[3]) / 2
    _, out = S.reduce_lmk(logits, np.asarray([0, 8, 0, 0]), [[[0], [1]], [[2, 3]]])
    assert out[0]["n_tracks"] == 1 and out[0]["track_count"].tolist() == [0, 1]
    assert out[1] == {**out[1], "video_score": 0.0, "video_pred": 0, "n_tracks": 0}


def test_state_dict_keys_equal_the_reference(golden):
    doc = golden[0]
    for variant, kw in doc["variants"].items():
        m = dualrun.LMKDisc(132, **kw)
        assert [[k, list(v.shape)] for k, v in m.state_dict().items()] == doc["state_dict"][variant]
        sd = dualrun.lmk_disc_synthetic_state_dict(132, seed=doc["weights_seed"], **kw)
        assert [[k, list(v.shape)] for k, v in sd.items()] == doc["state_dict"][variant]
    assert len(doc["state_dict"]["ff512"]) == 67 and dualrun.LMKDisc(132).spec.pool_tau == 0.7 and dualrun.LMKDisc(132).spec.ff == 512
    a, b = dualrun.lmk_disc_synthetic_state_dict(132, seed=1), dualrun.lmk_disc_synthetic_state_dict(132, seed=1)
    c = dualrun.lmk_disc_synthetic_state_dict(132, seed=2)
    assert all(torch.equal(a[k], b[k]) for k in a) and not torch.equal(a["head.1.weight"], c["head.1.weight"])


def test_load_follows_test_py(tmp_path):
    sd = dualrun.lmk_disc_synthetic_state_dict(132, seed=4)
    for ck in ({"model": sd, "epoch": 3}, dict(sd)):
        m = dualrun.LMKDisc(132)
        assert m.load(ck) == ([], [])
        assert all(torch.equal(v, sd[k]) for k, v in m.state_dict().items())
    path = str(tmp_path / "best_lmk_only.pt")
    torch.save({"model": sd}, path)
    m = dualrun.LMKDisc(132)
    assert m.load(path) == ([], []) and torch.equal(m.state_dict()["lmk_enc.pool.v"], sd["lmk_enc.pool.v"])
    part = {k: v for k, v in sd.items() if k != "head.4.bias"}
    part["au_enc.proj.weight"] = torch.zeros(256, 36)
    before = dualrun.LMKDisc(132)
    kept = before.state_dict()["head.4.bias"].clone()
    assert before.load({"model": part}) == (["head.4.bias"], ["au_enc.proj.weight"])                 # strict=False: reported, not raised
    assert torch.equal(before.state_dict()["head.4.bias"], kept) and torch.equal(before.state_dict()["head.1.weight"], sd["head.1.weight"])


def test_contract_errors():
    with pytest.raises(ValueError):
        dualrun.LMKDisc(130)                                                    # check_branch_spec: a multiple of 4
    with pytest.raises(ValueError):
        dualrun.LMKDisc(132, dim_ff=1024)
    with pytest.raises(ValueError):
        dualrun.LMKDisc(132, d_model=128)
    m = dualrun.LMKDisc(132).eval()
    with pytest.raises(RuntimeError, match="HIP"):
        m(torch.zeros(1, 8, 132))
    spec = dualrun.DualSpec()
    assert [n for n, _ in spec.branches()] == ["au_enc", "lmk_enc"] and [n for n, _ in m.spec.branches()] == ["lmk_enc"]
