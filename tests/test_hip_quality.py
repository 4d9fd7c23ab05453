"""GPU: af_face_quality_u8 (csrc/af_quality.hip) through live.FaceQuality against tests/quality_ref.py.

A 96 x 136 frame store with two slots of seeded random bytes, the second slot used, ONE launch over rectangles of every form of
the half-size step (2x2 blocks, whole ratios, the area table), sizes that are no multiple of the kernel's 8 x 32 tile, one taller
than three tiles and wider than one, one at the frame's origin, one ending at its far corner, two overlapping:
  exact        n_px, S1, S2 and the debug grey bytes equal quality_ref's, in both channel orders
  variance     lap agrees with numpy.var of the restated Laplacian to 1e-9 relative (the sums are exact; numpy's own fp64
               summation differs at about 1e-14)
  64 bits      a 640 x 480 checkerboard of two-pixel blocks has S2 = 320 * 240 * 1020^2 > 2^32, exact
  repeatable   two launches of the same input, and one with the rectangles reversed, give identical sums
  cleared      a second launch on the same stream after the slot's bytes changed gives the new sums
"""
import numpy as np
import pytest
import torch

import quality_ref as Q
from af_mi355x import _lib, evaluator, live

pytestmark = pytest.mark.gpu
H, W = 96, 136
# (x0, y0, w, h)
SHAPES = [(10, 10, 2, 2), (20, 7, 1, 5), (30, 9, 5, 1), (40, 11, 3, 3), (50, 13, 4, 4), (60, 15, 5, 4), (70, 17, 7, 9), (5, 30, 64, 64),
          (33, 20, 101, 75), (3, 2, 131, 93), (0, 0, 37, 23), (W - 41, H - 29, 41, 29), (60, 40, 30, 30), (75, 50, 33, 31), (90, 3, 1, 6)]
RECTS = [(1, x, y, x + w, y + h) for x, y, w, h in SHAPES]


def _store(frames):
    store = evaluator.FrameStore(torch.device("cuda", torch.cuda.current_device()))
    store.open(frames[0].shape, len(frames))
    store.put(list(frames), 0)
    return store


@pytest.fixture(scope="module")
def frames():
    rng = np.random.default_rng(12)
    return [rng.integers(0, 256, (H, W, 3), dtype=np.uint8) for _ in range(2)]


@pytest.fixture(scope="module")
def expected(frames):
    return {order: [Q.quality_sums(frames[s][y0:y1, x0:x1], order) for s, x0, y0, x1, y1 in RECTS] for order in ("rgb", "bgr")}


@pytest.mark.parametrize("order", ["rgb", "bgr"])
def test_sums_and_grey_bytes_equal_the_restatement(frames, expected, order):
    assert len(RECTS) >= 12 and any(max(1, h // 2) > 3 * 8 and max(1, w // 2) > 32 for _, _, w, h in SHAPES)
    quality = live.FaceQuality(_store(frames), order)
    sums, greys = quality.sums(RECTS, grey=True)
    for rect, got, grey, want in zip(RECTS, sums, greys, expected[order]):
        assert got == want[:3], (rect, got, want[:3])
        assert grey.shape == want[3].shape and np.array_equal(grey, want[3]), (rect, int((grey != want[3]).sum()))
    laps = quality(RECTS)
    for rect, (min_side, lap), want in zip(RECTS, laps, expected[order]):
        ref = float(np.var(Q.laplacian(want[3]).astype(np.float64)))
        assert min_side == float(min(rect[3] - rect[1], rect[4] - rect[2]))
        assert abs(lap - ref) <= 1e-9 * max(ref, 1.0), (rect, lap, ref)
    assert expected["rgb"][7][:3] != expected["bgr"][7][:3]      # the channel order matters to the grey weights


def test_reversed_order_repeat_and_cleared_accumulators(frames, expected):
    store = _store(frames)
    quality = live.FaceQuality(store, "rgb")
    first = quality.sums(RECTS)
    assert first == [e[:3] for e in expected["rgb"]]
    assert quality.sums(RECTS) == first
    assert quality.sums(RECTS[::-1]) == first[::-1]
    other = np.random.default_rng(13).integers(0, 256, (H, W, 3), dtype=np.uint8)
    store.put([other], 1)                                         # same stream: the copy, the clear and the launch are ordered
    second = quality.sums(RECTS)
    assert second == [Q.quality_sums(other[y0:y1, x0:x1])[:3] for _, x0, y0, x1, y1 in RECTS] and second != first
    assert quality.sums([(0,) + r[1:] for r in RECTS]) == [Q.quality_sums(frames[0][y0:y1, x0:x1])[:3] for _, x0, y0, x1, y1 in RECTS]


def test_sixty_four_bit_sums_on_a_checkerboard():
    yy, xx = np.mgrid[0:480, 0:640]
    board = np.repeat(np.where(((yy // 2) + (xx // 2)) % 2 == 0, 255, 0).astype(np.uint8)[..., None], 3, axis=2)
    quality = live.FaceQuality(_store([np.ascontiguousarray(board)]), "bgr")
    (n_px, s1, s2), = quality.sums([(0, 0, 0, 640, 480)])
    assert (n_px, s1, s2) == (320 * 240, 0, 320 * 240 * 1020 * 1020) and s2 > 2 ** 32
    assert quality([(0, 0, 0, 640, 480)]) == [(480.0, 1020.0 * 1020.0)]


def test_bad_rectangles_are_refused(frames):
    quality = live.FaceQuality(_store(frames), "rgb")
    for bad in [(2, 0, 0, 4, 4), (0, W - 3, 0, W + 1, 4), (0, 0, H - 1, 4, H + 1), (0, 5, 5, 5, 9), (-1, 0, 0, 4, 4)]:
        with pytest.raises(_lib.AfError):
            quality.sums([bad])
    assert quality.sums([]) == []
    many = [(1, i, 0, i + 4, 6) for i in range(70)]              # more than one launch's worth
    assert quality.sums(many) == [Q.quality_sums(frames[1][0:6, i:i + 4])[:3] for i in range(70)]
