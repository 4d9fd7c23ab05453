"""MI355X-native AltFreezing (I3D-ResNet-50) clip classifier: the one hot path of
Mariachiar/Spatiotemporal-Deepfake-Detection-for-Live-Video-Calls, rebuilt as hand-written
HIP (gfx950) behind the reference's classifier-plugin surface.  See DESIGN.md."""
from . import arch, synth  # noqa: F401


def __getattr__(name):
    # the evaluator's classes by their short names; loaded on first use, so importing the package stays light
    if name in ("VideoScorer", "TrackScorer"):
        from . import evaluator
        return getattr(evaluator, name)
    if name in ("LiveCall", "RealtimeCall", "CallServer", "FaceQuality"):
        from . import live
        return getattr(live, name)
    if name == "VideoRunner":
        from . import runner
        return runner.VideoRunner
    if name in ("YuvFrame", "CapturedFrame", "FrameResizer"):
        from . import frames
        return getattr(frames, name)
    if name == "TilePicker":
        from . import tile_picker
        return tile_picker.TilePicker
    if name in ("EvalSuite", "RankMetrics"):
        from . import eval_suite
        return getattr(eval_suite, name)
    if name in ("DualVideoScorer", "LmkVideoScorer", "DualTrack"):
        from . import dual_video
        return getattr(dual_video, name)
    if name == "LMKDisc":
        from . import dualrun
        return dualrun.LMKDisc
    if name == "ByteTracker":
        from . import tracker
        return tracker.ByteTracker
    if name == "DeviceByteTracker":
        from . import device_tracker
        return device_tracker.DeviceByteTracker
    raise AttributeError("module %r has no attribute %r" % (__name__, name))
