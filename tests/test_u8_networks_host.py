"""No GPU: what the uint8 surface of FTCN-TT / SlowFast decides on the host - the argument checks of af_pack_input_u8_pathways
(every refusal returns before a launch), the op-list ABI it rides on, the shared network methods, and DualEncoderRGB's refusal of
a backbone whose pooled feature is not 2048 wide."""
import ctypes as C
import inspect

import pytest

from af_mi355x import _lib, dualrun
from af_mi355x.classifier import Classifier, FtcnTT8x8, FtcnTTClassifier, I3D8x8, SlowFast8x8, _HipNetwork


def _call(clips=4096, n=1, t=8, h=6, w=10, alpha=4, dtype=_lib.AF_BF16, slow=4096, slow_layout=_lib.AF_PACK_C4, fast=8192,
          fast_layout=_lib.AF_PACK_C4, mean=True):
    """pointers are never dereferenced on the host: made-up addresses do for calls that must be refused"""
    m, s = (C.c_float * 3)(1, 2, 3), (C.c_float * 3)(1, 1, 1)
    return _lib.lib.af_pack_input_u8_pathways(clips, n, t, h, w, m if mean else None, s, alpha, dtype, slow, slow_layout, fast,
                                              fast_layout, None)


def test_pathways_pack_argument_checks():
    err = lambda: _lib.lib.af_last_error()
    assert _call(alpha=3) == -1 and b"multiple of alpha" in err()
    assert _call(t=9, alpha=8) == -1
    assert _call(dtype=_lib.AF_F32, slow_layout=_lib.AF_PACK_RGB3) == -1 and b"16-bit" in err()
    assert _call(dtype=_lib.AF_F32, fast_layout=_lib.AF_PACK_RGB3) == -1 and b"16-bit" in err()
    assert _call(slow=4096 + 8) == -1 and b"16-byte aligned" in err()
    assert _call(fast=8192 + 4) == -1 and b"16-byte aligned" in err()
    for name in ("clips", "slow", "fast"):
        assert _call(**{name: None}) == -1 and b"null" in err(), name
    assert _call(mean=False) == -1 and b"null" in err()
    for bad in (dict(n=0), dict(t=0, alpha=1), dict(h=-1), dict(w=0), dict(alpha=0), dict(alpha=-4), dict(dtype=7)):
        assert _call(**bad) == -1, bad
    assert _call(slow_layout=2) == -1 and b"layout" in err()
    assert _call(fast_layout=-1) == -1


def test_op_list_abi_is_appended_not_moved():
    """new enumerators behind the old ones, the layout flags in the former padding word: no offset of af_op moves"""
    assert (_lib.AF_OP_CONV_CPA, _lib.AF_OP_PACK_PATHWAYS_U8, _lib.AF_OP_NOP) == (22, 23, 24)
    assert _lib.AF_ABI_VERSION == 6 == _lib.lib.af_version()
    assert _lib.Op.pack_rgb3.offset == _lib.Op.x_sub.offset + 4 and _lib.Op.pack_rgb3.size == 4
    assert C.sizeof(_lib.Op) == _lib.Op.pack_rgb3.offset + 4
    assert _lib.lib.af_run_ops((_lib.Op * 1)(_lib.Op(kind=_lib.AF_OP_NOP)), 1, None) == 0          # a NOP launches nothing
    assert _lib.lib.af_run_ops((_lib.Op * 1)(_lib.Op(kind=_lib.AF_OP_PACK_PATHWAYS_U8)), 1, None) == -1


def test_every_network_has_the_uint8_surface():
    for cls in (I3D8x8, FtcnTT8x8, SlowFast8x8):
        for name in ("forward_clips_u8", "infer_scores", "_scores_of", "_run"):
            assert getattr(cls, name) is not None
        assert "return_scores" in inspect.signature(cls.forward).parameters, cls
        for name in ("forward_clips_u8", "infer_scores", "_scores_of"):                           # one implementation
            assert getattr(cls, name) is getattr(_HipNetwork, name), (cls, name)
    assert set(inspect.signature(_HipNetwork.forward_clips_u8).parameters) >= {"mean", "std", "return_scores", "return_pooled"}


def test_dual_encoder_rgb_refuses_a_backbone_of_another_width():
    kw = dict(d_model=256, depth=1, heads=4, ff_dim=3.0, rgb_from_features=False)
    with pytest.raises(ValueError, match="2048-wide"):
        dualrun.DualEncoderRGB(36, 132, 2048, rgb_backbone=FtcnTTClassifier(), **kw)
    with pytest.raises(ValueError, match="2048-wide"):
        dualrun.DualEncoderRGB(36, 132, 2048, rgb_backbone=FtcnTT8x8(), **kw)
    with pytest.raises(ValueError, match="2304-wide"):
        dualrun.DualEncoderRGB(36, 132, 2304, rgb_backbone=SlowFast8x8(), **kw)
    with pytest.raises(ValueError, match="vis_dim = 1024"):
        dualrun.DualEncoderRGB(36, 132, 1024, rgb_backbone=Classifier(), **kw)
    clf = Classifier()
    assert dualrun.DualEncoderRGB(36, 132, 2048, rgb_backbone=clf, **kw).rgb_backbone[0] is clf
    assert dualrun.DualEncoderRGB(36, 132, 2048, rgb_backbone=clf.network, **kw).rgb_backbone[0] is clf.network
    assert dualrun.DualEncoderRGB(36, 132, 1024, **kw).rgb_backbone[0] is None                     # no backbone: any feature width
