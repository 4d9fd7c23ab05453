"""Host: how sharp the comparator of tests/test_hip_stem_matrix.py is - the derived per-element bound (that module's docstring)
must accept torch's own fp32 CPU stem of the same rounded operands, rounded to the storage type (so the reference side alone stays
inside the bound: were it not so, the bound's derivation would be wrong), and must reject the same computation with ONE tap
w[o, c, dt, dh, dw] of the 147 kT set to zero: a centre tap, and the tap (c = 2, dh = 6, dw = 6) of the last dt plane - in the
K-packed layout the last real element of the last fragment.  Also: the matrix's case data is consistent without a device."""
import os
import sys

import pytest
import torch
import torch.nn.functional as F

from conftest import ROOT

sys.path.insert(0, os.path.join(ROOT, "tests"))
import hip_helpers as hh  # noqa: E402
import test_hip_stem_matrix as matrix  # noqa: E402

DIMS = (2, 4, 18, 20)


def _fp32_stem(x, w, scale, shift, dtype):
    """conv + affine + ReLU + max-pool in torch's fp32 on the CPU, rounded once to the storage type"""
    kt = w.shape[2]
    y = F.conv3d(x, w, None, (1, 2, 2), (kt // 2, 3, 3)) * scale.view(1, -1, 1, 1, 1) + shift.view(1, -1, 1, 1, 1)
    return F.max_pool3d(F.relu(y), *matrix.POOL).to(hh.TORCH_DT[dtype]).double()


def _loudest_channel(w, tap):
    """the output channel with the largest weight at `tap`, among those a dropped tap can show in (4 has scale 0, 9 is all zero)"""
    mag = w[(slice(None),) + tap].abs().clone()
    mag[4], mag[9] = -1.0, -1.0
    return int(mag.argmax())


@pytest.mark.parametrize("dtype", matrix.DT16)
@pytest.mark.parametrize("kt", [1, 3, 5])
def test_bound_accepts_fp32_and_rejects_one_dropped_tap(kt, dtype):
    x, w, scale, shift = matrix.operands(kt, dtype, DIMS, 4100 + kt)
    want, b = matrix.reference(x, w, scale, shift)
    assert (want[:, 9] == 0).all() and (want[:, 4] > 0).all() and (want[:, 1::2] > 0).any() and (scale[1::2] < 0).all()
    ratio = matrix.check(_fp32_stem(x, w, scale, shift, dtype), want, b, dtype, "torch fp32, kt = %d" % kt)
    assert ratio <= 1.0
    for tap in ((1, kt // 2, 3, 3), (2, kt - 1, 6, 6)):
        o = _loudest_channel(w, tap)
        mutant = w.clone()
        assert mutant[(o,) + tap] != 0
        mutant[(o,) + tap] = 0.0
        assert int((mutant != w).sum()) == 1
        with pytest.raises(AssertionError, match="beyond the bound"):
            matrix.check(_fp32_stem(x, mutant, scale, shift, dtype), want, b, dtype, "kt = %d without tap %s of channel %d" % (kt, tap, o))


def test_comparator_on_non_finite_values():
    """NaN: the output's NaN set must lie between ATen's and the 8-column window's; +inf: only where the reference passes the f16
    rounding edge"""
    x, w, scale, shift = matrix.operands(3, "f16", DIMS, 4200, special="inf")
    x[1, 2, 1, 9, 10] = float("nan")            # column 2 (mod 4): the eighth column reaches one pooled column further
    want, b = matrix.reference(x, w, scale, shift)
    sets = (torch.isnan(want), matrix.nan_wide_mask(x, 3))
    assert sets[0].any() and not (sets[0] & ~sets[1]).any() and (sets[1] & ~sets[0]).any()
    got = want.to(torch.float16).double()
    assert torch.isinf(got).any()
    matrix.check(got, want, b, "f16", "rounded reference", sets)
    wide = got.clone()
    wide[sets[1].expand_as(wide)] = float("nan")
    matrix.check(wide, want, b, "f16", "NaN over the whole 8-column window", sets)
    with pytest.raises(AssertionError, match="NaN in the output"):
        matrix.check(got, want, b, "f16", "NaN not allowed")
    beyond = got.clone()
    beyond[0, 0, 0, 0, 0] = float("nan")
    assert not sets[1][0, 0, 0, 0, 0]
    with pytest.raises(AssertionError, match="outside the 8-column window"):
        matrix.check(beyond, want, b, "f16", "a NaN elsewhere", sets)
    short = got.clone()
    short[sets[0]] = 0.0
    with pytest.raises(AssertionError, match="finite where ATen"):
        matrix.check(short, want, b, "f16", "NaN lost", sets)
    capped = got.clone()
    capped[torch.isinf(got)] = 65504.0
    with pytest.raises(AssertionError, match="finite where the reference is beyond"):
        matrix.check(capped, want, b, "f16", "+inf lost", sets)
    spurious = got.clone()
    spurious[0, 0, 0, 0, 0] = float("inf")
    with pytest.raises(AssertionError, match="infinities where the reference has none"):
        matrix.check(spurious, want, b, "f16", "+inf too many", sets)


def test_matrix_case_data():
    """the classes the issue names are all there, per fused kernel; rounds_class and the unit maps' first units"""
    assert matrix.rounds_class(256, 256) == "1" and matrix.rounds_class(261, 256) == "1-2" and matrix.rounds_class(512, 256) == "2"
    assert matrix.rounds_class(513, 256) == ">2" and matrix.rounds_class(805, 256) == ">2" and matrix.rounds_class(5, 5) == "1"
    assert matrix.clips_for(261, 256) == (9, 29) and matrix.clips_for(805, 256) == (23, 35) and matrix.clips_for(512, 256) == (16, 32)
    # XCD-contiguous map on 261 units and 256 workgroups: 33 units per XCD, the 32 workgroups of an XCD start at its first 32 and one
    # runs a second unit; the last XCD has 30 units (231 .. 260), all of them first ones
    assert [matrix.is_first(u, 261, 256, "xcd") for u in (0, 31, 32, 33, 64, 65, 230, 231, 260)] == [True, True, False, True, True, False, False, True, True]
    assert matrix.is_first(255, 512, 256, "plain") and not matrix.is_first(256, 512, 256, "plain")
    for kind in ("stem3_pool", "stem_pool"):
        mine = [c for c in matrix.CASES if c.kind == kind]
        assert {c.rounds for c in mine} == {"1", "1-2", "2", ">2"} and {c.kt for c in mine} == {1, 3, 5}
        assert {c.special for c in mine} == {None, "nan", "inf"}
        assert any(c.bands == 4 for c in mine) and any(c.onerow for c in mine)
        assert any(matrix.tiles8(c.hw[1]) and c.bands > 1 for c in mine) and any(matrix.tiles8(c.hw[1]) and c.bands == 1 for c in mine)
        assert {(1, 1), (2, 3), (4, 5), (33, 37), (8, 32), (8, 33), (8, 224)} <= {c.hw for c in mine}
    s3 = [c for c in matrix.CASES if c.kind == "stem3_pool"]
    assert {c.out for c in s3} == {0, 64, 80} and {c.inp for c in s3} == {"f32", "u8"} and {c.umap for c in s3} == {"xcd", "plain"}
    assert {matrix.tiles8(c.hw[1]) for c in s3 if c.kt == 1} == {matrix.tiles8(c.hw[1]) for c in s3 if c.kt == 5} == {True, False}
    assert {c.cout for c in matrix.STEM_CASES} == {64, 16, 8, 4}
