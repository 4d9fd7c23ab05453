"""Reference-side shim for the face detector.  In test/af_realtime.py / TEST2.py replace
``from preprocessing.yunet.yunet import YuNet`` with ``from integration.yunet_mi355x import YuNet`` (or copy this file
next to the caller and import it from there); the constructor, ``name``, ``setBackendAndTarget``, ``setInputSize`` and
``infer`` keep the reference wrapper's signatures, and ``modelPath`` stays the reference's
preprocessing/yunet/face_detection_yunet_2023mar.onnx.

Requires this repository on ``sys.path`` (or ``AF_MI355X_ROOT`` pointing at it) with ``libafhip.so`` built.
"""
import os
import sys

_root = os.environ.get("AF_MI355X_ROOT")
if _root and _root not in sys.path:
    sys.path.insert(0, _root)

import af_mi355x  # noqa: E402,F401
from af_mi355x.detector import YuNet  # noqa: E402,F401

__all__ = ["YuNet"]
