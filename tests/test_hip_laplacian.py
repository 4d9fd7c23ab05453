"""The full-size mode of the quality kernel (``af_face_laplacian_stores_u8``, csrc/af_quality.hip) against tests/runner_ref.py: the
exact integer sums and the grey bytes of rectangles of two frame stores, one B, G, R and one R, G, B, in ONE launch; the refusals
of the half-size form; and the half-size launch on the same rectangles, which the new mode leaves as it was."""
import numpy as np
import pytest
import torch

from af_mi355x import _lib, evaluator, live
import quality_ref
import runner_ref

pytestmark = pytest.mark.gpu

SHAPES = ((80, 112), (64, 96))                # the two stores' frames
ORDERS = ("bgr", "rgb")
N_FRAMES = (3, 2)
# (store, slot, x0, y0, w, h): 1x1, 1x5, 5x1 (a dimension of 1 -> its own neighbour), the 8 x 32 tile (h x w) exactly and one past it
# both ways, more than one tile both ways, a tall narrow one; origins, far corners and edges of both frames among them
RECTS = [(0, 0, 0, 0, 1, 1), (1, 1, 95, 63, 1, 1), (0, 1, 20, 7, 5, 1), (1, 0, 0, 30, 1, 5), (0, 2, 40, 0, 32, 8), (1, 1, 96 - 33, 64 - 9, 33, 9),
         (0, 0, 112 - 64, 80 - 17, 64, 17), (1, 0, 3, 5, 7, 31), (0, 1, 0, 80 - 31, 7, 31), (1, 1, 10, 10, 8, 32), (0, 2, 5, 9, 9, 33)]


def _dev():
    return torch.device("cuda", torch.cuda.current_device())


@pytest.fixture(scope="module")
def stores():
    rng = np.random.default_rng(77)
    out = []
    for (h, w), n, order in zip(SHAPES, N_FRAMES, ORDERS):
        host = [rng.integers(0, 256, (h, w, 3), dtype=np.uint8) for _ in range(n)]
        host[0][:16, :16] = 200                                                   # a flat patch: Laplacian 0 inside it
        store = evaluator.FrameStore(_dev(), order)
        store.open((h, w, 3), n)
        store.put(host, 0)
        out.append((store, host))
    torch.cuda.synchronize()
    return out


def _rects(stores):
    return [(stores[s][0], ORDERS[s], slot, x, y, x + w, y + h) for s, slot, x, y, w, h in RECTS]


def _crops(stores):
    return [(stores[s][1][slot][y:y + h, x:x + w], ORDERS[s]) for s, slot, x, y, w, h in RECTS]


def test_full_size_sums_and_grey_equal_the_numpy_statement(stores):
    q = live.StoresQuality(_dev())
    got, grey = q.full_sums(_rects(stores), grey=True)
    assert q.launches == 1                                                        # two stores, both byte orders, one launch
    want = [runner_ref.full_sums(crop, order) for crop, order in _crops(stores)]
    assert got == [w[:3] for w in want]
    assert all(g.shape == w[3].shape and np.array_equal(g, w[3]) for g, w in zip(grey, want))
    assert got[0] == (1, 0, 0) and len(set(got)) >= 9                             # a 1 x 1 crop has no Laplacian; the rest differ
    back = q.full_sums(_rects(stores)[::-1])
    assert back == got[::-1]                                                      # integer sums: no order in them
    assert q.full_size(_rects(stores)) == [runner_ref.min_side_and_full_lap(crop, order) for crop, order in _crops(stores)]


def test_the_byte_order_is_read(stores):
    (store, host), (x, y, w, h) = stores[0], (7, 3, 9, 33)
    q = live.StoresQuality(_dev())
    as_bgr, as_rgb = q.full_sums([(store, "bgr", 1, x, y, x + w, y + h), (store, "rgb", 1, x, y, x + w, y + h)])
    crop = host[1][y:y + h, x:x + w]
    assert as_bgr == runner_ref.full_sums(crop, "bgr")[:3] and as_rgb == runner_ref.full_sums(crop, "rgb")[:3] and as_bgr != as_rgb


def test_face_quality_asks_for_the_full_size_sums_of_its_store(stores):
    store, host = stores[1]
    q = live.FaceQuality(store, "rgb")
    rects = [(slot, x, y, x + w, y + h) for s, slot, x, y, w, h in RECTS if s == 1]
    got, grey = q.full_sums(rects, grey=True)
    want = [runner_ref.full_sums(host[slot][y0:y1, x0:x1], "rgb") for slot, x0, y0, x1, y1 in rects]
    assert q.launches == 1 and got == [w[:3] for w in want] and all(np.array_equal(g, w[3]) for g, w in zip(grey, want))
    assert q.full_size(rects) == [runner_ref.min_side_and_full_lap(host[slot][y0:y1, x0:x1], "rgb") for slot, x0, y0, x1, y1 in rects]
    assert q.launches == 2
    many = [(1, i, 0, i + 4, 6) for i in range(70)]                               # more than one launch's worth, one read-back
    assert q.full_sums(many) == [runner_ref.full_sums(host[1][0:6, i:i + 4], "rgb")[:3] for i in range(70)] and q.launches == 4


def test_both_modes_behind_one_read_back(stores):
    q = live.StoresQuality(_dev())
    rects = _rects(stores)
    got = q.half_and_full(rects)
    assert q.launches == 2                                                        # one launch of each mode, one read-back
    want = [(Q[0],) + (Q[1], F[1]) for Q, F in zip([quality_ref.min_side_and_lap(c, o) for c, o in _crops(stores)],
                                                    [runner_ref.min_side_and_full_lap(c, o) for c, o in _crops(stores)])]
    assert got == want
    many = [(stores[1][0], "rgb", 1, i, 0, i + 4, 6) for i in range(70)]          # two launches of each mode, the records side by side
    half, full = q.sums(many, both=True)
    assert q.launches == 6 and half == q.sums(many) and full == q.full_sums(many) and half != full
    assert q.half_and_full([]) == []


def test_the_refusals_of_the_half_size_form(stores):
    q = live.StoresQuality(_dev())
    (a, _), (b, _) = stores
    for bad in ([(b, "rgb", 0, 96 - 3, 0, 96 + 1, 4)],                            # leaves store 1's frame (inside store 0's)
                [(b, "rgb", 2, 0, 0, 4, 4)],                                      # slot 2: store 0 has it, store 1 has not
                [(a, "bgr", 0, 0, 80 - 2, 4, 80 + 1)],                            # past the last row
                [(a, "bgr", 0, -1, 0, 4, 4)],                                     # a negative corner
                [(a, "bgr", 0, 4, 4, 4, 8)]):                                     # no width
        with pytest.raises(_lib.AfError):
            q.sums(bad)
        with pytest.raises(_lib.AfError):
            q.full_sums(bad)
    assert q.full_sums([]) == []


def test_the_half_size_launch_on_the_same_rectangles_is_unchanged(stores):
    q = live.StoresQuality(_dev())
    got, grey = q.sums(_rects(stores), grey=True)
    want = [quality_ref.quality_sums(crop, order) for crop, order in _crops(stores)]
    assert got == [w[:3] for w in want] and all(np.array_equal(g, w[3]) for g, w in zip(grey, want))
    q.full_sums(_rects(stores))                                                   # the other mode in between changes nothing
    assert q.sums(_rects(stores)) == got
