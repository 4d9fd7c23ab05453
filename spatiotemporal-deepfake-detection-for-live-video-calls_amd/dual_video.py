"""dualrun at video level: raw per-frame landmark and AU arrays of each face track in, the dual encoder's video verdict out.

What the reference does around ``DualEncoderAU_LMK.forward`` in numpy / torch host code runs here as two launches around the existing
branch and head launches (csrc/af_dual_video.hip; the arithmetic and its order are stated in tests/dualvideo_ref.py):

  clip windows      preprocessing/preprocessing_parallel.py:96-102, 382-418   ``clip_windows`` / ``fill_last_known`` (host)
  landmark features dualrun/data/make_lmk_features.py:39-52, 152-187          af_dual_clip_features
  AU features       dualrun/data/make_au_features.py:41-53                    af_dual_clip_features
  fixT, z-score     dualrun/rgb/fusion.py:79-114, 331-336                     af_dual_clip_features
  track / video     fusion.py:118-130 (``infer_dual``, ``evaluate_dual``, engine_rgb.py:94-112, 193-205)   af_dual_video_reduce
  best.py's video aggregation   dualrun/cli/best.py:518-591                   af_dual_video_reduce, best family
  rot_invariant     dualrun/data/make_lmk_features.py:145-150, 173-176        af_dual_clip_features_ex
  cli/test.py       collate_pad, LMKDisc, median_by_key, noisy_or             ``LmkVideoScorer``: af_dual_clip_features_ex, af_lmk_video_reduce

Raw arrays go up once (one pinned fill, one copy), one launch makes every clip's normalised features, the dual forward scores them
in chunks, one launch reduces clip logits to track and video results, one read-back returns them.  No CPU fallback."""
import ctypes as C
import math
import types
from typing import List, Optional, Sequence

import numpy as np
import torch

from . import _staging
from .dualrun import DualEncoderAU_LMK, DualEncoderRGB, LMKDisc

CLIP_LENGTH, CLIP_STEP = 8, 4          # preprocessing_parallel.py:96-102 (the image, AU and landmark buffers share them)
# AF_DUALV_MIN_POINTS = REQ_MIN_LANDMARKS as make_lmk_features.py:52 computes it: the key set reaches index 466 (the comment there
# says 309, the mouth corner's index + 1; a frame of 309 points is refused upstream as too_few_points), and AF_DUALV_MAX_T
MIN_POINTS, MAX_CLIP_FRAMES = 467, 16
# Clips per dual forward.  The branch kernel is one workgroup per (clip, modality) and the head one per clip, so a result does not
# depend on the chunk a clip falls in; the chunk only bounds the forward's temporaries (z and logits: 2 KB a clip, 4 MB a chunk)
# and its grid (2 x 2048 workgroups, 16 rounds of the 256 CUs).
CHUNK_CLIPS = 2048


def clip_windows(n: int, first_known: int = 0, length: int = CLIP_LENGTH, step: int = CLIP_STEP) -> List[int]:
    """First frames of the clips ``handle_clip_buffers`` writes for a track of `n` frames: a window every `step` frames from the
    track's first frame on, written once `length` frames are there, and only if none of its frames precedes `first_known`, the
    first frame at which both modalities are known (before it a buffer holds None and the clip is skipped, :383-386; after it
    holes carry the last known value)."""
    if length < 1 or step < 1:
        raise ValueError("length and step must be >= 1")
    return [s for s in range(0, n - length + 1, step) if s >= first_known]


def fill_last_known(rows, present):
    """``last_known_data`` (:369-377): every row whose `present` is False becomes a copy of the last present row before it.
    Returns ``(filled, first)`` with `first` the first present row (``len(rows)`` if there is none); rows before it are left as
    they are and belong to no clip (``clip_windows(n, first_known=first)``)."""
    rows = np.array(rows, copy=True)
    present = np.asarray(present, dtype=bool)
    if present.shape != (rows.shape[0],):
        raise ValueError("present must hold one flag per row")
    idx = np.where(present, np.arange(rows.shape[0]), -1)
    last = np.maximum.accumulate(idx) if rows.shape[0] else idx
    first = int(np.argmax(present)) if present.any() else int(rows.shape[0])
    keep = last >= 0
    rows[keep] = rows[last[keep]]
    return rows, first


def person_key_order(keys) -> list:
    """``track_reduce``'s order of a video's distinct track keys (fusion.py:122): digit strings first, by value, then the others as
    strings."""
    return sorted(set(str(k) for k in keys), key=lambda t: (0, int(t)) if t.isdigit() else (1, t))


def sigmoid_to_logit(p: float, eps: float = 1e-6) -> float:
    """engine_rgb.py:42-44, in Python floats like there"""
    p = max(eps, min(1 - eps, float(p)))
    return float(math.log(p / (1 - p)))


class DualTrack:
    """One face track: `landmarks` (n, P, 2) with P >= 467 FaceMesh points (the 468- and 478-point meshes) and `aus` (n, K) with the columns in the reference's
    sorted-key order, both fp32, both host numpy arrays or both device tensors; `key` the person id (``get_person_id_from_path``);
    `clips` the clips to score as first frames (each `CLIP_LENGTH` long) or ``(first, length)`` pairs, default ``clip_windows(n)``.
    ``aus=None`` is a track of landmarks alone (``au_k`` 0): what ``LmkVideoScorer`` takes and ``DualVideoScorer`` refuses."""

    def __init__(self, landmarks, aus, key, clips=None):
        self.on_device = isinstance(landmarks, torch.Tensor)
        if aus is not None and self.on_device != isinstance(aus, torch.Tensor):
            raise ValueError("landmarks and aus must both be numpy arrays or both be tensors")
        if self.on_device:
            if not landmarks.is_cuda or landmarks.dtype != torch.float32 or (aus is not None and not (aus.is_cuda and aus.dtype == torch.float32)):
                raise ValueError("tensor tracks must be fp32 HIP device tensors (host data goes in as numpy arrays)")
            if landmarks.dim() == 3 and landmarks.shape[0] > 0 and (landmarks.stride(2) != 1 or landmarks.stride(1) != 2):
                landmarks = landmarks.contiguous()
            if aus is not None and aus.dim() == 2 and aus.shape[0] > 0 and aus.stride(1) != 1:
                aus = aus.contiguous()
        else:
            landmarks = np.asarray(landmarks, dtype=np.float32)
            aus = None if aus is None else np.asarray(aus, dtype=np.float32)
        if landmarks.ndim != 3 or landmarks.shape[2] != 2 or (aus is not None and (aus.ndim != 2 or aus.shape[0] != landmarks.shape[0])):
            raise ValueError("expected landmarks (n, P, 2) and aus (n, K) with the same n (got %s and %s)"
                             % (tuple(landmarks.shape), None if aus is None else tuple(aus.shape)))
        self.landmarks, self.aus, self.key = landmarks, aus, str(key)
        self.n, self.points, self.au_k = int(landmarks.shape[0]), int(landmarks.shape[1]), 0 if aus is None else int(aus.shape[1])
        if self.points < MIN_POINTS:
            raise ValueError("landmarks need the 467 FaceMesh points the key set reaches (indices up to 466); got P = %d" % self.points)
        clips = clip_windows(self.n) if clips is None else clips
        self.clips = [(int(c), CLIP_LENGTH) if np.ndim(c) == 0 else (int(c[0]), int(c[1])) for c in clips]
        for first, length in self.clips:
            if length < 1 or length > MAX_CLIP_FRAMES:
                raise ValueError("a clip holds 1..16 frames (got %d)" % length)
            if first < 0 or first + length > self.n:
                raise ValueError("clip (%d, %d) leaves the track's %d frames" % (first, length, self.n))


def _align(v, a=16):
    return (v + a - 1) // a * a


class _RawTrackScorer:
    """What the raw-track scorers share: a call's plan (track and clip tables, the CSR of the reduction, their places in one staging
    buffer), the one pinned fill and copy, the feature launch, and the layout of the one buffer that is read back.  A subclass names
    its model (``_net``), checks a track (``_check_track``) and orders a video's tracks for the reduction (``_reduce_order``)."""

    def _check_track(self, tr):
        raise NotImplementedError

    def _reduce_order(self, entries):
        """[(key, [clip numbers])] of a video's tracks in input order -> the same of its reduced tracks, in the reduction's order"""
        raise NotImplementedError

    @staticmethod
    def _out_layout(names):
        """{name: byte offset} of the [(name, dtype, n)] arrays in one buffer, and its size"""
        offs, off = {}, 0
        for name, dt, n in names:
            offs[name] = off
            off = _align(off + np.dtype(dt).itemsize * max(n, 1))
        return offs, off

    def _launch_features(self, p, slot, opts, A, L, nvalid, rot_invariant=False, pad_zero=False):
        """af_dual_clip_features on the plan's tables; with an option of cli/test.py's path (or A None), its _ex form"""
        from . import _lib
        base = slot.dev.data_ptr()
        st = C.c_void_p(torch.cuda.current_stream(p.device).cuda_stream)
        tables = (C.c_void_p(base + p.off_tracks), len(p.tracks), C.c_void_p(base + p.off_clips), p.n_clips, C.byref(opts))
        outs = (C.c_void_p(L.data_ptr()), C.c_void_p(nvalid.data_ptr()), st)
        if A is not None and not rot_invariant and not pad_zero:
            _lib.check(_lib.lib.af_dual_clip_features(*tables, C.c_void_p(A.data_ptr()), *outs), "af_dual_clip_features")
        else:
            _lib.check(_lib.lib.af_dual_clip_features_ex(*tables, int(rot_invariant), _lib.DUALV_PAD_ZERO if pad_zero else _lib.DUALV_PAD_FIXT,
                                                         None if A is None else C.c_void_p(A.data_ptr()), *outs), "af_dual_clip_features_ex")

    # ---- host side: checks and tables, before any launch ----------------------------------------------------------------------
    def _plan(self, videos):
        """a call's tables: the tracks, the clips, the CSR of the reduction, and where each sits in the staging buffer"""
        from . import _lib
        p = types.SimpleNamespace()
        p.tracks, p.clip_rows, p.videos = [], [], []       # DualTrack; (track, first, len); per video [(key, [clip numbers])]
        p.clip_keys = []
        for vi, tracks in enumerate(videos):
            entries = []
            for tr in tracks:
                if not isinstance(tr, DualTrack):
                    raise ValueError("videos is a list of lists of DualTrack")
                self._check_track(tr)
                ti = len(p.tracks)
                p.tracks.append(tr)
                entries.append((tr.key, list(range(len(p.clip_rows), len(p.clip_rows) + len(tr.clips)))))
                for first, length in tr.clips:
                    p.clip_rows.append((ti, first, length))
                    p.clip_keys.append(tr.key)
            p.videos.append(self._reduce_order(entries))
        p.n_clips, p.n_videos = len(p.clip_rows), len(p.videos)
        p.n_reduced = sum(len(v) for v in p.videos)
        on_dev = [tr for tr in p.tracks if tr.on_device]
        p.device = _staging.cuda_device(on_dev[0].landmarks.device if on_dev else next(self._net.parameters()).device)
        if p.device.type != "cuda":
            raise RuntimeError("the MI355X dual video path only runs on a HIP device (no CPU fallback): move the model to the GPU")
        for tr in on_dev:
            if tr.landmarks.device != p.device or (tr.aus is not None and tr.aus.device != p.device):
                raise ValueError("every device-resident track must sit on %s" % p.device)
        # the staging buffer: track table | clip table | video_tracks | track_clips | clip_index | raw rows of the host tracks
        off = 0
        p.off_tracks, off = off, _align(off + C.sizeof(_lib.DualvTrack) * max(len(p.tracks), 1))
        p.off_clips, off = off, _align(off + 16 * max(p.n_clips, 1))
        p.off_vt, off = off, _align(off + 4 * (p.n_videos + 1))
        p.off_tc, off = off, _align(off + 4 * (p.n_reduced + 1))
        p.off_ci, off = off, _align(off + 4 * max(p.n_clips, 1))
        p.raw = []
        for tr in p.tracks:
            if tr.on_device:
                p.raw.append(None)
                continue
            lo = off
            off = _align(off + 4 * tr.n * tr.points * 2)
            ao = off
            off = _align(off + 4 * tr.n * tr.au_k)
            p.raw.append((lo, ao))
        p.nbytes = off
        return p

    def _upload(self, p):
        """one fill of a pinned slot, one copy; returns the slot (its device twin holds the tables and the raw rows)"""
        from . import _lib
        slot = self._ring.acquire(p.nbytes, p.device)
        host = slot.host.numpy()
        base = slot.dev.data_ptr()
        tt = (_lib.DualvTrack * max(len(p.tracks), 1)).from_buffer(host, p.off_tracks)
        for i, tr in enumerate(p.tracks):
            if tr.on_device:
                tt[i] = _lib.DualvTrack(tr.landmarks.data_ptr(), None if tr.aus is None else tr.aus.data_ptr(),
                                        tr.landmarks.stride(0) if tr.n > 1 else 2 * tr.points,
                                        tr.aus.stride(0) if tr.aus is not None and tr.n > 1 else tr.au_k, tr.n)
            else:
                lo, ao = p.raw[i]
                host[lo:lo + 4 * tr.n * tr.points * 2].view(np.float32).reshape(tr.n, tr.points, 2)[...] = tr.landmarks
                if tr.aus is not None:
                    host[ao:ao + 4 * tr.n * tr.au_k].view(np.float32).reshape(tr.n, tr.au_k)[...] = tr.aus
                tt[i] = _lib.DualvTrack(base + lo, None if tr.aus is None else base + ao, 2 * tr.points, tr.au_k, tr.n)
        del tt
        ct = host[p.off_clips:p.off_clips + 16 * p.n_clips].view(np.int32).reshape(p.n_clips, 4)
        if p.n_clips:
            ct[:, :3] = np.asarray(p.clip_rows, dtype=np.int32)
            ct[:, 3] = 0
        vt = host[p.off_vt:p.off_vt + 4 * (p.n_videos + 1)].view(np.int32)
        tc = host[p.off_tc:p.off_tc + 4 * (p.n_reduced + 1)].view(np.int32)
        ci = host[p.off_ci:p.off_ci + 4 * p.n_clips].view(np.int32)
        t = e = 0
        vt[0] = tc[0] = 0
        for vi, tracks in enumerate(p.videos):
            for _, clips in tracks:
                ci[e:e + len(clips)] = clips
                e += len(clips)
                t += 1
                tc[t] = e
            vt[vi + 1] = t
        slot.dev[:p.nbytes].copy_(slot.host[:p.nbytes], non_blocking=True)
        return slot


class DualVideoScorer(_RawTrackScorer):
    """``videos`` (a list of lists of ``DualTrack``) -> per video the dual encoder's verdict.  Fusion family (default):
    ``track_reduce`` in ("median", "mean"), ``video_agg`` in ("max", "median", "mean"), as ``infer_dual`` / ``evaluate_dual`` /
    ``dual_video_logit`` compose them (median = ``torch.median``, the lower middle value).  With ``agg_mode`` in ("track_mean",
    "track_median", "track_majority") the reduction is ``best.py``'s ``aggregate_video_predictions`` on sigmoid(logit) with
    ``prob_thresh``.  ``zscore_mode`` "global" needs ``stats`` (au_mean, au_std, lmk_mean, lmk_std): the reference returns the
    features unchanged when its stats file is missing; here that silent difference is a ValueError - ask for "none" to get it.
    A clip whose landmark frames were all dropped is left out; a track left without clips is left out; a video left without any
    gives NaN (fusion) or score 0.0 / pred 0 (best), the reference's ``track_scores = []``.  ``rot_invariant=True`` is
    make_lmk_features.py's ``--rot-invariant``: every surviving frame turned so that its mouth line is horizontal, before fixT and
    the z-score (the arithmetic: tests/lmkdisc_ref.py)."""

    def __init__(self, dual, T: int = 8, zscore_mode: str = "clip", zscore_apply: str = "both", stats: Optional[dict] = None,
                 track_reduce: str = "median", video_agg: str = "max", agg_mode: Optional[str] = None, prob_thresh: float = 0.5,
                 use_delta: bool = True, use_delta2: bool = True, chunk_clips: int = CHUNK_CLIPS, rot_invariant: bool = False):
        from . import _lib
        if isinstance(dual, DualEncoderRGB):
            raise ValueError("DualEncoderRGB needs V, the AltFreezing feature of each clip window, which raw landmark / AU tracks do "
                             "not carry: the video-level path scores DualEncoderAU_LMK only")
        if not isinstance(dual, DualEncoderAU_LMK):
            raise ValueError("dual must be an af_mi355x DualEncoderAU_LMK (got %s)" % type(dual).__name__)
        zscore_mode, zscore_apply = str(zscore_mode).lower(), str(zscore_apply).lower()
        if zscore_mode not in _lib.DUALV_ZSCORE or zscore_apply not in _lib.DUALV_APPLY:
            raise ValueError("zscore_mode is none / clip / global and zscore_apply both / au / lmk (got %r, %r)" % (zscore_mode, zscore_apply))
        if not 1 <= int(T) <= min(_lib.DUALV_MAX_T, dual.max_frames):
            raise ValueError("T must be 1..%d for this model (got %d)" % (min(_lib.DUALV_MAX_T, dual.max_frames), T))
        if dual.spec.lmk_dim != _lib.DUALV_LMK_DIM:
            raise ValueError("the landmark features are 132 wide; the model takes %d" % dual.spec.lmk_dim)
        if zscore_mode == "global":
            if stats is None:
                raise ValueError("zscore_mode 'global' without stats: the reference then leaves the features unchanged "
                                 "(normalize_features, stats None); say zscore_mode='none' for that")
            for k, d in (("au_mean", dual.spec.au_dim), ("au_std", dual.spec.au_dim), ("lmk_mean", 132), ("lmk_std", 132)):
                if np.asarray(stats[k]).shape != (d,):
                    raise ValueError("stats[%r] must hold %d values" % (k, d))
        if agg_mode is not None and agg_mode not in _lib.DUALV_BEST:
            raise ValueError("agg_mode is one of %s (got %r)" % (sorted(_lib.DUALV_BEST), agg_mode))
        if track_reduce not in _lib.DUALV_TRACK or video_agg not in _lib.DUALV_VIDEO:
            raise ValueError("track_reduce is median / mean and video_agg max / median / mean (got %r, %r)" % (track_reduce, video_agg))
        if int(chunk_clips) < 1:
            raise ValueError("chunk_clips must be >= 1")
        self.dual, self.T = dual, int(T)
        self._net, self.rot_invariant = dual, bool(rot_invariant)
        self.zscore_mode, self.zscore_apply, self.stats = zscore_mode, zscore_apply, stats
        self.track_reduce, self.video_agg, self.agg_mode, self.prob_thresh = track_reduce, video_agg, agg_mode, float(prob_thresh)
        self.use_delta, self.use_delta2, self.chunk_clips = bool(use_delta), bool(use_delta2), int(chunk_clips)
        self.au_mult = 1 + int(self.use_delta) + int(self.use_delta2)
        self._ring = _staging.PinnedRing(slots=3, min_bytes=1 << 20, headroom=True)
        self._stats_dev = None

    def _check_track(self, tr):
        sp = self.dual.spec
        if tr.aus is None:
            raise ValueError("DualVideoScorer needs the action units of every track (aus=None is LmkVideoScorer's landmark-only track)")
        if tr.au_k * self.au_mult != sp.au_dim:
            raise ValueError("K * (1 + delta + delta2) = %d * %d differs from the model's au_dim %d" % (tr.au_k, self.au_mult, sp.au_dim))

    def _reduce_order(self, entries):
        buckets = {}
        for key, clips in entries:
            buckets.setdefault(key, []).extend(clips)
        return [(k, buckets[k]) for k in person_key_order(buckets)]

    def _stats(self, dev):
        if self.zscore_mode != "global":
            return [None] * 4
        if self._stats_dev is None or self._stats_dev[0].device != dev:
            self._stats_dev = [torch.from_numpy(np.ascontiguousarray(self.stats[k], dtype=np.float32)).to(dev)
                               for k in ("au_mean", "au_std", "lmk_mean", "lmk_std")]
        return [C.c_void_p(t.data_ptr()) for t in self._stats_dev]

    def _features(self, p, slot):
        from . import _lib
        sp = self.dual.spec
        dev = p.device
        A = torch.empty((p.n_clips, self.T, sp.au_dim), dtype=torch.float32, device=dev)
        L = torch.empty((p.n_clips, self.T, _lib.DUALV_LMK_DIM), dtype=torch.float32, device=dev)
        nvalid = torch.empty((p.n_clips,), dtype=torch.int32, device=dev)
        if p.n_clips:
            k = sp.au_dim // self.au_mult
            opts = _lib.DualvOpts(self.T, k, _lib.DUALV_ZSCORE[self.zscore_mode], _lib.DUALV_APPLY[self.zscore_apply], int(self.use_delta),
                                  int(self.use_delta2), *self._stats(dev))
            self._launch_features(p, slot, opts, A, L, nvalid, rot_invariant=self.rot_invariant)
        return A, L, nvalid

    def features(self, videos):
        """(A (clips, T, au_dim), L (clips, T, 132), nvalid (clips,) int32) on the device, clips in input order (video by video,
        track by track)"""
        p = self._plan(videos)
        with torch.cuda.device(p.device):
            slot = self._upload(p)
            out = self._features(p, slot)
            slot.record()
        return out

    def _run(self, videos):
        """every launch of a call; returns (plan, host arrays by name, video_logit on the device)"""
        from . import _lib
        p = self._plan(videos)
        dev = p.device
        best = self.agg_mode is not None
        nc, nt, nv = p.n_clips, p.n_reduced, p.n_videos
        # one device buffer for everything that is read back: fp64 first, then the 4-byte arrays
        names = [("track_score", np.float64, nt), ("video_score", np.float64, nv), ("nvalid", np.int32, nc), ("logits", np.float32, nc),
                 ("clip_prob", np.float32, nc), ("track_count", np.int32, nt), ("track_logit", np.float32, nt), ("track_prob", np.float32, nt),
                 ("track_pred", np.int32, nt), ("video_logit", np.float32, nv), ("video_prob", np.float32, nv), ("video_pred", np.int32, nv)]
        offs, off = self._out_layout(names)
        with torch.cuda.device(dev), torch.inference_mode():
            out = torch.zeros(off, dtype=torch.uint8, device=dev)
            ptr = {name: C.c_void_p(out.data_ptr() + offs[name]) for name, _, _ in names}
            slot = self._upload(p)
            A, L, nvalid = self._features(p, slot)
            view = lambda name, tdt, n: out[offs[name]:offs[name] + 4 * n].view(tdt)
            view("nvalid", torch.int32, nc).copy_(nvalid)
            logits = view("logits", torch.float32, nc)
            for lo in range(0, nc, self.chunk_clips):
                hi = min(nc, lo + self.chunk_clips)
                logits[lo:hi].copy_(self.dual(A[lo:hi], L[lo:hi])["bin_logits"])
            if nv:
                base = slot.dev.data_ptr()
                st = C.c_void_p(torch.cuda.current_stream(dev).cuda_stream)
                family = _lib.DUALV_FAMILY_BEST if best else _lib.DUALV_FAMILY_FUSION
                tmode = _lib.DUALV_BEST[self.agg_mode] if best else _lib.DUALV_TRACK[self.track_reduce]
                _lib.check(_lib.lib.af_dual_video_reduce(
                    ptr["logits"], ptr["nvalid"], nc, C.c_void_p(base + p.off_vt), nv, C.c_void_p(base + p.off_tc), nt, C.c_void_p(base + p.off_ci),
                    family, tmode, _lib.DUALV_VIDEO[self.video_agg], C.c_double(self.prob_thresh), ptr["track_logit"], ptr["track_prob"],
                    ptr["video_logit"], ptr["video_prob"], ptr["clip_prob"], ptr["track_score"], ptr["track_pred"], ptr["video_score"],
                    ptr["video_pred"], ptr["track_count"], st), "af_dual_video_reduce")
            slot.record()
            host = out.cpu().numpy()                        # the call's one synchronisation and one read-back
        got = {name: host[offs[name]:offs[name] + np.dtype(dt).itemsize * n].view(dt) for name, dt, n in names}
        video_logit = out[offs["video_logit"]:offs["video_logit"] + 4 * nv].view(torch.float32)
        return p, got, video_logit

    def clip_logits(self, videos):
        """(clip logits fp32, nvalid int32) as host arrays, clips in input order; a clip with nvalid 0 took no part in a verdict"""
        _, got, _ = self._run(videos)
        return got["logits"].copy(), got["nvalid"].copy()

    def score(self, videos) -> List[dict]:
        """Per video: ``infer_dual``'s dict (``prob_video_dual``, ``tracks`` = the person key of every scored clip,
        ``prob_dual_per_track`` in ``person_key_order``, ``n_clips``, ``agg``) plus ``logit_video`` and ``track_keys``; with
        ``agg_mode``, ``best.py``'s record: ``tracks`` {key: probs, preds, track_pred, track_score}, ``video_pred``, ``video_score``."""
        p, got, _ = self._run(videos)
        out, t = [], 0
        for vi, tracks in enumerate(p.videos):
            used = [[c for c in clips if got["nvalid"][c] > 0] for _, clips in tracks]
            if self.agg_mode is None:
                kept = [i for i, u in enumerate(used) if u]
                order = sorted(c for u in used for c in u)
                out.append({"prob_video_dual": float(got["video_prob"][vi]), "logit_video": float(got["video_logit"][vi]),
                            "tracks": [p.clip_keys[c] for c in order], "track_keys": [tracks[i][0] for i in kept],
                            "prob_dual_per_track": [float(got["track_prob"][t + i]) for i in kept],
                            "logit_dual_per_track": [float(got["track_logit"][t + i]) for i in kept],
                            "n_clips": len(order), "agg": {"track": self.track_reduce, "video": self.video_agg}})
            else:
                rec = {}
                first_seen = sorted((u[0], i) for i, u in enumerate(used) if u)           # the reference's dict fills in input order
                for _, i in first_seen:
                    probs = [float(got["clip_prob"][c]) for c in used[i]]
                    rec[tracks[i][0]] = {"probs": probs, "preds": [1 if q >= self.prob_thresh else 0 for q in probs],
                                         "track_pred": int(got["track_pred"][t + i]), "track_score": float(got["track_score"][t + i])}
                out.append({"tracks": rec, "video_pred": int(got["video_pred"][vi]), "video_score": float(got["video_score"][vi]),
                            "agg_mode": self.agg_mode})
            t += len(tracks)
        return out

    def fuse(self, videos, p_rgb: Sequence[float], moe):
        """``engine_rgb.evaluate_epoch``'s composition per video: z_rgb = sigmoid_to_logit(p_rgb), z_dual = the video logit,
        ``moe(z_rgb, z_dual)``.  Returns the fused logits and gates, (videos, 1) device tensors.  Fusion family only."""
        if self.agg_mode is not None:
            raise ValueError("fuse needs the video logit: construct the scorer without agg_mode")
        if len(p_rgb) != len(videos):
            raise ValueError("one p_rgb per video (got %d for %d videos)" % (len(p_rgb), len(videos)))
        z_rgb_host = torch.tensor([[sigmoid_to_logit(float(q))] for q in p_rgb], dtype=torch.float32).reshape(-1, 1)
        p, _, video_logit = self._run(videos)
        with torch.cuda.device(p.device), torch.inference_mode():
            return moe(z_rgb_host.to(p.device), video_logit.reshape(-1, 1).clone())


class LmkVideoScorer(_RawTrackScorer):
    """cli/test.py on raw landmark tracks: ``videos`` (a list of lists of ``DualTrack`` with ``aus=None``, host arrays or device
    tensors; the keys of a video's tracks are distinct - test.py keys a track by its path) -> per video test.py's three CSV levels.

      lmk_features.npy   make_lmk_features.py:152-187 (``rot_invariant`` = its ``--rot-invariant``)   af_dual_clip_features_ex
      collate_pad        data/vox_ds.py:19-26: the surviving rows, then zero rows, and the mask            af_dual_clip_features_ex
      LMKDisc            cli/test.py:34-57, 199-206                                                        ``dualrun.LMKDisc``
      sigmoid, --invert, median_by_key, noisy_or   cli/test.py:86-94, 205-256                              af_lmk_video_reduce

    ``T`` is fixed per scorer and every clip is padded to it.  This is the one deliberate difference from test.py, where a clip is
    padded to the longest clip of its DataLoader batch, so that its logit depends on its batch mates: the pad rows are masked in the
    attention and the pooling, but ``proj``'s bias, the moving average and the dilated depthwise convolutions carry them into the
    valid rows (the reference gives logits 0.12 apart for the same clips scored alone and padded to 8).  A clip longer than ``T`` is
    refused.  A clip with no surviving frame takes no part (``process_tree``'s ``min_frames = 1`` never writes it), a track left with
    none is left out, a video left with none scores ``noisy_or([]) = 0.0`` with ``n_tracks`` 0.  No CPU fallback."""

    def __init__(self, disc, T: int = CLIP_LENGTH, rot_invariant: bool = False, invert: bool = False, thresh: float = 0.5,
                 chunk_clips: int = CHUNK_CLIPS):
        from . import _lib
        if not isinstance(disc, LMKDisc):
            raise ValueError("disc must be an af_mi355x LMKDisc (got %s)" % type(disc).__name__)
        if not 1 <= int(T) <= min(_lib.DUALV_MAX_T, disc.max_frames):
            raise ValueError("T must be 1..%d for this model (got %d)" % (min(_lib.DUALV_MAX_T, disc.max_frames), T))
        if disc.spec.lmk_dim != _lib.DUALV_LMK_DIM:
            raise ValueError("the landmark features are 132 wide; the model takes %d" % disc.spec.lmk_dim)
        if int(chunk_clips) < 1:
            raise ValueError("chunk_clips must be >= 1")
        self.disc, self._net, self.T = disc, disc, int(T)
        self.rot_invariant, self.invert, self.thresh, self.chunk_clips = bool(rot_invariant), bool(invert), float(thresh), int(chunk_clips)
        self._ring = _staging.PinnedRing(slots=3, min_bytes=1 << 20, headroom=True)

    def _check_track(self, tr):
        if tr.aus is not None:
            raise ValueError("LmkVideoScorer takes tracks of landmarks alone: DualTrack(landmarks, None, key)")
        for first, length in tr.clips:
            if length > self.T:
                raise ValueError("clip (%d, %d) is longer than T = %d: collate_pad never shortens a clip" % (first, length, self.T))

    def _reduce_order(self, entries):
        keys = [k for k, _ in entries]
        if len(set(keys)) != len(keys):
            raise ValueError("the tracks of a video need distinct keys (cli/test.py keys a track by its path); got %s" % keys)
        return entries

    def _features(self, p, slot):
        from . import _lib
        L = torch.empty((p.n_clips, self.T, _lib.DUALV_LMK_DIM), dtype=torch.float32, device=p.device)
        nvalid = torch.empty((p.n_clips,), dtype=torch.int32, device=p.device)
        if p.n_clips:
            opts = _lib.DualvOpts(self.T, 0, _lib.DUALV_ZSCORE["none"], _lib.DUALV_APPLY["both"], 0, 0, None, None, None, None)
            self._launch_features(p, slot, opts, None, L, nvalid, rot_invariant=self.rot_invariant, pad_zero=True)
        return L, nvalid

    def features(self, videos):
        """(L (clips, T, 132), nvalid (clips,) int32) on the device, clips in input order: ``collate_pad``'s batch with every clip
        padded to T rows; its mask is ``arange(T) >= nvalid``"""
        p = self._plan(videos)
        with torch.cuda.device(p.device):
            slot = self._upload(p)
            out = self._features(p, slot)
            slot.record()
        return out

    def _run(self, videos):
        from . import _lib
        p = self._plan(videos)
        dev = p.device
        nc, nt, nv = p.n_clips, p.n_reduced, p.n_videos
        names = [("clip_score", np.float64, nc), ("track_score", np.float64, nt), ("video_score", np.float64, nv), ("nvalid", np.int32, nc),
                 ("logits", np.float32, nc), ("track_pred", np.int32, nt), ("track_count", np.int32, nt), ("video_pred", np.int32, nv),
                 ("video_count", np.int32, nv)]
        offs, off = self._out_layout(names)
        with torch.cuda.device(dev), torch.inference_mode():
            out = torch.zeros(off, dtype=torch.uint8, device=dev)
            ptr = {name: C.c_void_p(out.data_ptr() + offs[name]) for name, _, _ in names}
            slot = self._upload(p)
            L, nvalid = self._features(p, slot)
            out[offs["nvalid"]:offs["nvalid"] + 4 * nc].view(torch.int32).copy_(nvalid)
            logits = out[offs["logits"]:offs["logits"] + 4 * nc].view(torch.float32)
            lengths = nvalid.clamp(min=1)                   # a clip with nothing left is zeros and is left out below: any count will do
            for lo in range(0, nc, self.chunk_clips):
                hi = min(nc, lo + self.chunk_clips)
                logits[lo:hi].copy_(self.disc.forward_lengths(L[lo:hi], lengths[lo:hi]))
            if nv:
                base = slot.dev.data_ptr()
                st = C.c_void_p(torch.cuda.current_stream(dev).cuda_stream)
                _lib.check(_lib.lib.af_lmk_video_reduce(
                    ptr["logits"], ptr["nvalid"], nc, C.c_void_p(base + p.off_vt), nv, C.c_void_p(base + p.off_tc), nt, C.c_void_p(base + p.off_ci),
                    int(self.invert), C.c_double(self.thresh), ptr["clip_score"], ptr["track_score"], ptr["track_pred"], ptr["track_count"],
                    ptr["video_score"], ptr["video_pred"], ptr["video_count"], st), "af_lmk_video_reduce")
            slot.record()
            host = out.cpu().numpy()                        # the call's one synchronisation and one read-back
        return p, {name: host[offs[name]:offs[name] + np.dtype(dt).itemsize * n].view(dt) for name, dt, n in names}

    def clip_scores(self, videos):
        """(clip scores fp64 - sigmoid(logit), or 1 - it with ``invert`` -, clip logits fp32, nvalid int32) as host arrays, clips in
        input order; a clip with nvalid 0 took no part in a verdict"""
        _, got = self._run(videos)
        return got["clip_score"].copy(), got["logits"].copy(), got["nvalid"].copy()

    def score(self, videos) -> List[dict]:
        """Per video test.py's three levels: ``clips`` [(track key, score)] (per_clip.csv), ``tracks`` {key: {"score_track_median",
        "pred"}} (per_track.csv), ``score_video_or``, ``pred``, ``n_tracks`` (per_video.csv); preds are ``score >= thresh``"""
        p, got = self._run(videos)
        out, t = [], 0
        for vi, tracks in enumerate(p.videos):
            rec = {"clips": [(key, float(got["clip_score"][c])) for key, clips in tracks for c in clips if got["nvalid"][c] > 0],
                   "tracks": {key: {"score_track_median": float(got["track_score"][t + i]), "pred": int(got["track_pred"][t + i])}
                              for i, (key, _) in enumerate(tracks) if got["track_count"][t + i] > 0},
                   "score_video_or": float(got["video_score"][vi]), "pred": int(got["video_pred"][vi]), "n_tracks": int(got["video_count"][vi])}
            out.append(rec)
            t += len(tracks)
        return out
