"""Reference-side shim for the offline evaluator's face detector.  In test_tools/common.py replace
``from .ct.detection import FaceDetector`` with ``from af_mi355x.retinaface import FaceDetector`` (or import it from
this file); the constructor (gpu_id, model_path, network), ``detect`` and ``__call__`` keep the reference's signatures
and return types; ``scale_detect`` resizes on the device with cv2.resize's arithmetic.

Requires this repository on ``sys.path`` (or ``AF_MI355X_ROOT`` pointing at it) with ``libafhip.so`` built.
"""
import os
import sys

_root = os.environ.get("AF_MI355X_ROOT")
if _root and _root not in sys.path:
    sys.path.insert(0, _root)

import af_mi355x  # noqa: E402,F401
from af_mi355x.retinaface import FaceDetector  # noqa: E402,F401

__all__ = ["FaceDetector"]
