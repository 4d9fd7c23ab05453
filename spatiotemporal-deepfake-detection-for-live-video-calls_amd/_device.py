"""Device state shared by the face detectors (detector.YuNet, retinaface.FaceDetector): the packed weights uploaded once per
device, one scratch workspace per (device, stream), and the plain-or-timed call of a libafhip entry point.  libafhip is
imported inside the methods, so the detectors' host code works without it."""
import ctypes as C


class DeviceModel:
    """Base of a detector whose kernels read one packed fp32 weight blob and one workspace.  A subclass names the libafhip
    functions that size them (`_weight_floats_fn`, `_workspace_bytes_fn`); each entry point it calls is a pair
    (function name, name of its launch count in _lib) for `_call`."""

    _weight_floats_fn = ""
    _workspace_bytes_fn = ""

    def __init__(self, weights_host):
        self.weights_host = weights_host
        self._dev_weights = {}
        self._workspaces = {}

    def _weights(self, dev):
        """the packed weights on `dev`, shared read-only by every stream: the one upload per device is waited for on the
        host (set-up, once), so that a call on any other stream can read them"""
        import torch
        from . import _lib
        w = self._dev_weights.get(dev)
        if w is None:
            want = getattr(_lib.lib, self._weight_floats_fn)()
            if self.weights_host.size != want:
                raise RuntimeError("packed weights %d floats, libafhip expects %d" % (self.weights_host.size, want))
            w = torch.from_numpy(self.weights_host).to(dev)
            torch.cuda.current_stream(dev).synchronize()
            self._dev_weights[dev] = w
        return w

    def _workspace(self, dev, stream, desc):
        """scratch of one (device, stream) for descriptor `desc`.  Calls on one stream reuse it in stream order; calls on
        different streams never share it.  It is allocated while `stream` is current, so when a larger frame replaces it,
        the caching allocator orders that free after the stream's kernels."""
        import torch
        from . import _lib
        need = getattr(_lib.lib, self._workspace_bytes_fn)(C.byref(desc))
        if need <= 0:
            raise ValueError(_lib.lib.af_last_error().decode())
        key = (dev, stream.cuda_stream)
        ws = self._workspaces.get(key)
        if ws is None or ws.numel() < need:
            with torch.cuda.stream(stream):
                ws = self._workspaces[key] = torch.empty(need, dtype=torch.uint8, device=dev)
        return ws

    @staticmethod
    def _call(entry, args, timings):
        """libafhip `entry` = (function, launch-count name) on `args`; with `timings` (a list) its _timed form, which
        synchronises and leaves the per-launch device times in ms in `timings`"""
        from . import _lib
        fn, launches = entry
        if timings is None:
            _lib.check(getattr(_lib.lib, fn)(*args), fn[3:])
        else:
            ms = (C.c_float * getattr(_lib, launches))()
            _lib.check(getattr(_lib.lib, fn + "_timed")(*args, ms), fn[3:] + "_timed")
            timings[:] = list(ms)
