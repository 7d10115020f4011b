"""ctypes binding of libtransception_hip.so -- the only way the Python host reaches the GPU arithmetic.

The binding is derived from include/transception_hip.h at import (_header.py): signatures, structs and constants are written
once, in the header.  What stands here is the list of names the host imports.  The connected-component post-processing entries,
which replace no reference call site, have a header and a version of their own (include/transception_post.h -> POST), and so has the
weight averaging (include/transception_ema.h -> EMA), the test-time augmentation (include/transception_tta.h -> TTA) and the resampling of
class scores (include/transception_resample.h -> RESAMPLE), the focal / Tversky loss (include/transception_loss.h -> LOSS) and the directed
surface-distance statistics (include/transception_surface.h -> SURFACE) and the uncertainty maps and calibration statistics
(include/transception_uncertainty.h -> UNCERT) and the top-k cross-entropy (include/transception_topk.h -> TOPK).

There is deliberately NO fallback: if the shared library is missing or a call returns a non-zero
status the host raises.  (The CPU oracle under oracle/ is test infrastructure and is never imported here.)
"""
from __future__ import annotations

import ctypes as C
import os

from . import _header

HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.environ.get("TC_LIB_PATH") or os.path.join(HERE, "libtransception_hip.so")   # override: A/B kernel experiments only

ABI = _header.load()
SIGNATURES = {name: f.argtypes for name, f in ABI.functions.items()}     # every pointer is a c_void_p: byref(), arrays, addresses, None
K, S = ABI.constants, ABI.structs
SIDE = {s.attr: _header.load(s.path) for s in _header.SIDE_HEADERS}       # the headers of their own: one line each in _header.SIDE_HEADERS
POST, EMA, TTA, RESAMPLE, BRIDGE, LOSS = SIDE["POST"], SIDE["EMA"], SIDE["TTA"], SIDE["RESAMPLE"], SIDE["BRIDGE"], SIDE["LOSS"]
SURFACE, UNCERT, TOPK = SIDE["SURFACE"], SIDE["UNCERT"], SIDE["TOPK"]

ABI_VERSION = K["TC_ABI_VERSION"]
TC_F32, TC_BF16, TC_F16 = K["TC_F32"], K["TC_BF16"], K["TC_F16"]
ACT_NONE, ACT_HSWISH, ACT_COORD, ACT_SIGMOID = K["TC_ACT_NONE"], K["TC_ACT_HSWISH"], K["TC_ACT_COORD"], K["TC_ACT_SIGMOID"]
ACT_GELU, ACT_SCALE, ACT_RELU = K["TC_ACT_GELU"], K["TC_ACT_SCALE"], K["TC_ACT_RELU"]
FFN_NONE, FFN_LN_A, FFN_LN_B, FFN_EP = K["TC_FFN_NONE"], K["TC_FFN_LN_A"], K["TC_FFN_LN_B"], K["TC_FFN_EP"]
EW_PATCHIFY, EW_DEINTERLEAVE, EW_COPY, EW_MULTI_MAX = K["TC_EW_PATCHIFY"], K["TC_EW_DEINTERLEAVE"], K["TC_EW_COPY"], K["TC_EW_MULTI_MAX"]
TC_AUG_WARP, TC_AUG_LINEAR, TC_AUG_BLUR, TC_AUG_PIECEWISE = K["TC_AUG_WARP"], K["TC_AUG_LINEAR"], K["TC_AUG_BLUR"], K["TC_AUG_PIECEWISE"]
TC_AUG_SKIP, TC_AUG_FROM_RAW = K["TC_AUG_SKIP"], K["TC_AUG_FROM_RAW"]
ATTN_DKV_SPLITS = K["TC_ATTN_DKV_SPLITS"]
TC_METRIC_NO_SOURCE, TC_METRIC_SELECT_WORK_BYTES = K["TC_METRIC_NO_SOURCE"], K["TC_METRIC_SELECT_WORK_BYTES"]
TC_IGNORE_NONE = K["TC_IGNORE_NONE"]
POST_ABI_VERSION, EMA_ABI_VERSION, TTA_ABI_VERSION, RESAMPLE_ABI_VERSION, BRIDGE_ABI_VERSION, SURFACE_ABI_VERSION, UNCERT_ABI_VERSION, TOPK_ABI_VERSION, LOSS_ABI_VERSION = (SIDE[s.attr].constants[s.version] for s in _header.SIDE_HEADERS)
TC_OVERLAP_DICE, TC_OVERLAP_TVERSKY = LOSS.constants["TC_OVERLAP_DICE"], LOSS.constants["TC_OVERLAP_TVERSKY"]
TC_CC_LARGEST, TC_CC_MIN_VOXELS = POST.constants["TC_CC_LARGEST"], POST.constants["TC_CC_MIN_VOXELS"]
TC_RESAMPLE_MAX_EXTENT = RESAMPLE.constants["TC_RESAMPLE_MAX_EXTENT"]
TC_SURFACE_WORK_BYTES = SURFACE.constants["TC_SURFACE_WORK_BYTES"]
TC_TTA_FLIP_H, TC_TTA_FLIP_W, TC_TTA_TRANSPOSE = TTA.constants["TC_TTA_FLIP_H"], TTA.constants["TC_TTA_FLIP_W"], TTA.constants["TC_TTA_TRANSPOSE"]
TC_UNCERT_LOGITS, TC_UNCERT_PROB_SUMS = UNCERT.constants["TC_UNCERT_LOGITS"], UNCERT.constants["TC_UNCERT_PROB_SUMS"]
TC_CALIB_FOREGROUND, TC_CALIB_MAX_BINS = UNCERT.constants["TC_CALIB_FOREGROUND"], UNCERT.constants["TC_CALIB_MAX_BINS"]

TcGemm, TcLnFold, TcDwFold, TcDwSeg, TcFfnSeg = S["TcGemm"], S["TcLnFold"], S["TcDwFold"], S["TcDwSeg"], S["TcFfnSeg"]
TcFfnFused, TcFfnBwd, TcEffAtt, TcEwSeg, TcSliceAug = S["TcFfnFused"], S["TcFfnBwd"], S["TcEffAtt"], S["TcEwSeg"], S["TcSliceAug"]
TcSrSrc, TcLnSeg = BRIDGE.structs["TcSrSrc"], BRIDGE.structs["TcLnSeg"]
SR_LN_MAX, LN_MULTI_MAX = BRIDGE.constants["TC_SR_LN_MAX"], BRIDGE.constants["TC_LN_MULTI_MAX"]


class TcError(RuntimeError):
    pass


class _Lib:
    calls = 0

    def __init__(self, path: str = LIB_PATH):
        if not os.path.exists(path):
            raise TcError(f"{path} is missing: build it with `python -m transception_amd.build` "
                          "(there is no CPU/PyTorch fallback for the TransCeption hot path)")
        self.path = path
        self.cdll = C.CDLL(path)
        headers = [(ABI, "TC_ABI_VERSION", "tc_abi_version", "ABI"),
                   *((SIDE[s.attr], s.version, s.entry, s.what + " ABI") for s in _header.SIDE_HEADERS)]
        for header, *_ in headers:
            for name, f in header.functions.items():
                fn = getattr(self.cdll, name)      # AttributeError if a declared symbol is not exported
                fn.argtypes = f.argtypes
                fn.restype = f.restype
                setattr(self, name, fn if f.query else self._checked(name, fn))
        for header, version, entry, what in headers:
            v, host = getattr(self.cdll, entry)(), header.constants[version]
            if v != host:
                raise TcError(f"{what} mismatch: library {v}, host {host}")

    @staticmethod
    def _checked(name, fn):
        def call(*a):
            _Lib.calls += 1                      # C-ABI entries since import (bench.py reports the per-step count)
            rc = fn(*a)
            if rc != 0:
                raise TcError(f"{name} failed with status {rc}")
        call.__name__ = name
        return call


_lib = None


def lib() -> _Lib:
    global _lib
    if _lib is None:
        _lib = _Lib()
    return _lib
