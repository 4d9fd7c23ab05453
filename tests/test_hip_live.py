"""GPU: live.LiveCall - every tracked face of a call scored out of one ring of captured frames - and the BGR form of the
window-batch warp it launches.  Frames are 96 x 131 (row pitch 393 bytes, odd); the network is a shrunken synthetic I3D in f16
(8 frames, 64 x 64), FTCN-TT for the one test that is about the other networks.

  bgr kernel    af_warp_affine_window_rects_bgr_u8 on a store S EQUALS af_warp_affine_window_rects_u8 on S with every pixel's
                channels reversed, every byte: 16 windows of 32 rectangles that touch all four frame edges and end with the store;
                the same with everything outside the rectangles set to 255 and to 0; the planner both launches share refuses a
                store without the 3 trailing bytes and a frame index outside the ring
  scores        three tracks close on one step (3 windows padded to 4): LiveCall's scores are torch.equal to forward_clips_u8 at
                B = 4 on the windows StreamingCropAligner.align_last makes from host-cut crops of the channel-reversed frames, and
                the warped bytes equal align_last's
  ring wrap     ring_frames at the constructor's minimum, 2.5 times as many steps: the same equality before and after the wrap
  replay        the graph replay at batch 1 and 2 equals the eager forward on the same bytes; FTCN-TT gives infer_scores' values
  new surface   the module and the library symbol this feature adds
"""
import ctypes as C

import numpy as np
import pytest
import torch

import af_mi355x
from af_mi355x import _lib, aligner, evaluator, synth
from af_mi355x.classifier import FtcnTT8x8, I3D8x8

pytestmark = pytest.mark.gpu
H, W = 96, 131
CLIP, SIZE = 8, 64
_nets = {}


def _net(kind="i3d"):
    if kind not in _nets:
        net = (I3D8x8 if kind == "i3d" else FtcnTT8x8)(clip_size=CLIP, crop_size=SIZE, precision="f16")
        net.load_state_dict(synth.synthetic_state_dict(net.spec, seed=5))
        _nets[kind] = net.cuda().eval()
    return _nets[kind]


# ---- 1. the BGR instantiation of the warp -------------------------------------------------------------------------------------------

N_FRAMES, N_WIN, ITEMS, WARP_SIZE = 4, 16, 32, 224
RECTS = [(0, 0, 70, 60), (W - 50, 10, W, 80), (20, H - 45, 110, H), (W - 64, H - 52, W, H)]      # (x0, y0, x1, y1) of frame f: left +
#                                                                         top edge, right edge, bottom edge, the store's last pixel


def _plan(store_bytes, frame_of=lambda w, t: (w + t) % N_FRAMES, seed=11):
    """(rc, host table) of 16 windows x 32 items: item (w, t) is the rectangle of frame `frame_of(w, t)`, pasted at an offset of
    its own on window w's canvas, under a rotation and scale of window w's own"""
    rng = np.random.default_rng(seed)
    desc = np.zeros(N_WIN, dtype=evaluator._WINDOW_DTYPE)
    rects = np.zeros((N_WIN, ITEMS), dtype=evaluator._RECT_DTYPE)
    for w in range(N_WIN):
        ch, cw = int(rng.integers(100, 140)), int(rng.integers(110, 150))
        ang, sc = rng.uniform(-0.4, 0.4), WARP_SIZE / 120.0 * rng.uniform(0.8, 1.3)
        a, b = sc * np.cos(ang), sc * np.sin(ang)
        desc[w] = ([a, -b, rng.uniform(-20, 30), b, a, rng.uniform(-20, 30)], ch, cw)
        for t in range(ITEMS):
            f = frame_of(w, t)
            x0, y0, x1, y1 = RECTS[f % N_FRAMES]
            iw, ih = x1 - x0, y1 - y0
            rects[w, t] = (f, x0, y0, ih, iw, int(rng.integers(0, cw - iw + 1)), int(rng.integers(0, ch - ih + 1)), 0)
    table = np.zeros(_lib.lib.af_window_rects_table_bytes(N_WIN, ITEMS) // 8, dtype=np.int64)
    st = _lib.FrameStore(store_bytes, H * W * 3, W * 3, N_FRAMES, H, W, 0)
    rc = _lib.lib.af_window_rects_plan_u8(desc.ctypes.data, rects.ctypes.data, N_WIN, ITEMS, WARP_SIZE, C.byref(st), table.ctypes.data,
                                          table.nbytes, None, None)
    return rc, table


def _launch(fn, store, table):
    out = torch.zeros((N_WIN, ITEMS, WARP_SIZE, WARP_SIZE, 3), dtype=torch.uint8, device="cuda")
    stream = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    _lib.check(getattr(_lib.lib, fn)(C.c_void_p(store.data_ptr()), C.c_void_p(table.data_ptr()), N_WIN, ITEMS, WARP_SIZE,
                                     C.c_void_p(out.data_ptr()), stream), fn)
    torch.cuda.synchronize()
    return out


def _reversed(store):
    """the store with every pixel's channels reversed; the bytes behind the last frame stay"""
    n = N_FRAMES * H * W * 3
    return torch.cat([store[:n].view(-1, 3).flip(1).contiguous().view(-1), store[n:]])


def test_bgr_launch_equals_rgb_launch_on_the_reversed_store():
    n = N_FRAMES * H * W * 3
    g = torch.Generator().manual_seed(4)
    store = torch.randint(0, 256, (n + 16,), dtype=torch.uint8, generator=g).cuda()
    assert RECTS[0][:2] == (0, 0) and RECTS[1][2] == W and RECTS[2][3] == H and RECTS[3][2:] == (W, H)
    rc, table = _plan(store.numel())
    assert rc == 0, _lib.lib.af_last_error()
    table = torch.from_numpy(table).cuda()
    want = _launch("af_warp_affine_window_rects_u8", _reversed(store), table)
    got = _launch("af_warp_affine_window_rects_bgr_u8", store, table)
    assert bool(want.any()) and torch.equal(got, want), "differs in %d bytes" % int((got != want).sum())
    plain = _launch("af_warp_affine_window_rects_u8", store, table)
    assert not torch.equal(plain, want) and torch.equal(plain.flip(-1), want)          # the arithmetic is per channel: only the order moves
    for fill in (255, 0):                                         # nothing outside a frame's rectangle may reach the result
        walled = torch.full_like(store, fill)
        frames, wf = store[:n].view(N_FRAMES, H, W, 3), walled[:n].view(N_FRAMES, H, W, 3)
        for f, (x0, y0, x1, y1) in enumerate(RECTS):
            wf[f, y0:y1, x0:x1] = frames[f, y0:y1, x0:x1]
        assert torch.equal(_launch("af_warp_affine_window_rects_bgr_u8", walled, table), want), fill
        assert torch.equal(_launch("af_warp_affine_window_rects_u8", _reversed(walled), table), want), fill


def test_the_shared_planner_refuses_a_store_without_slack_and_a_frame_outside_the_ring():
    n = N_FRAMES * H * W * 3
    assert _plan(n + 3)[0] == 0
    for short in (n, n + 2):                                      # the rectangle that ends the store needs 3 readable bytes behind it:
        assert _plan(short)[0] == -1 and b"3 readable bytes" in _lib.lib.af_last_error()   # no table, so neither launch can run
    rc, _ = _plan(n + 16, frame_of=lambda w, t: N_FRAMES if (w, t) == (5, 7) else (w + t) % N_FRAMES)
    assert rc == -1 and b"leaves the 4 frames" in _lib.lib.af_last_error()


# ---- 2. - 4. LiveCall against the parent's composition -------------------------------------------------------------------------------

def _script(n_steps, starts, seed):
    """per step the faces [(tid, tlbr, lm5)] of tracks that start at `starts[tid]` and drift; boxes partly leave the frame"""
    rng = np.random.default_rng(seed)
    std = (aligner.STD_POINTS_317 - aligner.STD_POINTS_317.mean(0)) / 317.0
    out = []
    for s in range(n_steps):
        faces = []
        for tid, first in starts.items():
            if s < first:
                continue
            cx, cy = 28.0 + 37.0 * (tid % 3) + 0.6 * s + rng.normal(0, 0.4), 40.0 + 9.0 * (tid % 2) + rng.normal(0, 0.4)
            half = 14.0 + 2.0 * (tid % 3) + rng.normal(0, 0.3)
            tlbr = np.array([cx - half, cy - half, cx + half, cy + half], dtype=np.float32)
            lm5 = (std * 2.2 * half + [cx, cy] + rng.normal(0, 0.5, (5, 2))).astype(np.float32)
            faces.append((tid, tlbr, lm5))
        out.append(faces)
    return out


class _Parent:
    """one StreamingCropAligner per face over host-cut crops of the frame reversed on the host (af_realtime.py:434-451), and the
    eager forward at the batch size LiveCall pads to"""

    def __init__(self, net, crop_scale):
        self.net, self.crop_scale, self.aligners = net, crop_scale, {}

    def push(self, frame_bgr, faces):
        frgb = frame_bgr[..., ::-1]
        for tid, tlbr, lm5 in faces:
            x1, y1, x2, y2 = map(int, evaluator.get_crop_box((H, W), tlbr, scale=self.crop_scale))
            assert x2 > x1 and y2 > y1
            top_left = np.array([[x1, y1]], dtype=np.float32)
            record = ((tlbr.reshape(2, 2).astype(np.float32) - top_left).reshape(-1), lm5.astype(np.float32) - top_left,
                      np.zeros((68, 2), np.float32), np.array([x1, y1, x2, y2], dtype=np.int32))
            if tid not in self.aligners:
                self.aligners[tid] = aligner.StreamingCropAligner(size=SIZE, capacity=32, max_crop_pixels=H * W)
            self.aligners[tid].push(record, frgb[y1:y2, x1:x2])

    def score(self, tids):
        clips = torch.stack([self.aligners[tid].align_last(CLIP)[1] for tid in tids])
        run = 1
        while run < len(tids):
            run *= 2
        batch = torch.cat([clips] + [clips[-1:]] * (run - len(tids)))
        with torch.inference_mode():
            scores = self.net.forward_clips_u8(batch, return_scores=True)["scores"][:len(tids)].float().cpu()
        return clips, scores, run


def _play(call, parent, script, seed):
    """steps the call and the parent's composition through the script; every closing step must agree bit for bit.
    Returns [(step, tids, run)] of the closing steps."""
    rng = np.random.default_rng(seed)
    closes = []
    for s, faces in enumerate(script):
        frame = rng.integers(0, 256, (H, W, 3), dtype=np.uint8)
        results = call.step(frame, faces)
        parent.push(frame, faces)
        assert torch.equal(call.frame_view(s).cpu(), torch.from_numpy(frame))
        if not results:
            continue
        tids = [tid for tid, _ in results]
        clips, want, run = parent.score(tids)
        got = torch.tensor([sc for _, sc in results], dtype=torch.float32)
        warped = call._scorers[run].clip
        assert warped.shape[0] == run and torch.equal(warped[:len(tids)], clips), (s, tids)
        assert torch.equal(warped[len(tids):], clips[-1:].expand(run - len(tids), -1, -1, -1, -1))
        assert torch.equal(got, want), (s, tids, got, want)
        assert all(0.0 < v < 1.0 for v in got.tolist())
        closes.append((s, tids, run))
    return closes


def test_three_tracks_closing_together_equal_the_parents_composition():
    net = _net()
    call = af_mi355x.LiveCall(net, clip_size=CLIP, size=SIZE, stride=4, ring_frames=32, drop_after=8)
    closes = _play(call, _Parent(net, call.crop_scale), _script(13, {1: 0, 2: 0, 3: 0}, seed=2), seed=3)
    assert closes == [(7, [1, 2, 3], 4), (11, [1, 2, 3], 4)]
    assert call.uploaded_bytes == 13 * H * W * 3                  # one upload per frame, not per face
    with pytest.raises(ValueError):
        call.frame_view(13)


def test_scores_before_and_after_the_ring_wraps():
    net = _net()
    drop = 4
    ring = CLIP + drop                                            # the constructor's minimum
    with pytest.raises(ValueError):
        af_mi355x.LiveCall(net, clip_size=CLIP, size=SIZE, ring_frames=ring - 1, drop_after=drop)
    call = af_mi355x.LiveCall(net, clip_size=CLIP, size=SIZE, stride=3, ring_frames=ring, drop_after=drop)
    steps = int(2.5 * ring)
    closes = _play(call, _Parent(net, call.crop_scale), _script(steps, {1: 0, 2: 3}, seed=5), seed=6)
    assert any(s < ring for s, _, _ in closes) and any(ring <= s < 2 * ring for s, _, _ in closes) and any(s >= 2 * ring for s, _, _ in closes)
    assert closes[0] == (7, [1], 1) and {run for _, _, run in closes[1:]} == {2} and len(closes) == 8     # steps 7, 10, 13 .. 28
    with pytest.raises(ValueError):
        call.frame_view(steps - 1 - ring)                         # overwritten
    assert call.frame_view(steps - ring).shape == (H, W, 3)


@pytest.mark.parametrize("kind,tracks", [("i3d", 1), ("i3d", 2), ("ftcn", 2)])
def test_graph_replay_equals_the_eager_forward(kind, tracks):
    net = _net(kind)
    call = af_mi355x.LiveCall(net, clip_size=CLIP, size=SIZE, stride=2, ring_frames=24, drop_after=8, channel_order="rgb")
    script = _script(12, {tid: 0 for tid in range(1, tracks + 1)}, seed=7)
    rng = np.random.default_rng(8)
    n_closes = 0
    for s, faces in enumerate(script):
        results = call.step(rng.integers(0, 256, (H, W, 3), dtype=np.uint8), faces)
        if results:
            assert len(results) == tracks and set(call._scorers) == {tracks}
            clips = call._scorers[tracks].clip.clone()
            with torch.inference_mode():
                eager = net.forward_clips_u8(clips, return_scores=True)["scores"].float().cpu()
            assert torch.equal(torch.tensor([sc for _, sc in results], dtype=torch.float32), eager), (s, results, eager)
            assert np.array_equal(net.infer_scores(clips), eager.numpy())
            n_closes += 1
    assert n_closes == 3                                          # steps 7, 9, 11


def test_the_feature_exists():
    from af_mi355x import live
    assert af_mi355x.LiveCall is live.LiveCall
    assert hasattr(_lib.lib, "af_warp_affine_window_rects_bgr_u8") and "af_warp_affine_window_rects_bgr_u8" in _lib.ABI
