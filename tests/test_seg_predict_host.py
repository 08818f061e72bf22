"""CPU-side checks of the mask / validation-count path that works from the low-resolution logits (cavp_seg_predict_nhwc, ABI 15):
the library exports the entry point, the ABI versions agree, and every public entry fails loudly on CPU tensors."""
import ctypes
import types

import pytest
import torch


def _model(seg_model="DeepLabV3Plus"):
    from cavp_amd.cavp_model import CAVP
    args = types.SimpleNamespace(seg_model=seg_model, last_three_dilation_stride=[False, False, False], audio_backbone="vgg",
                                 num_classes=2, batch_size=2, local_rank="cpu")
    return CAVP(50, None, num_classes=2, args=args)


def test_library_exports_seg_predict_and_abi_15():
    from cavp_amd import _lib, build
    build.build(verbose=False)
    lib = ctypes.CDLL(_lib.LIB_PATH)
    assert hasattr(lib, "cavp_seg_predict_nhwc")
    assert "cavp_seg_predict_nhwc" in _lib.PROTOTYPES
    assert _lib.ABI_VERSION == 16 == _lib.load().cavp_abi_version()


def test_predict_needs_device_tensors():
    from cavp_amd._lib import CavpError
    m = _model().eval()
    image, audio = torch.zeros(1, 3, 32, 32), torch.zeros(1, 1, 96, 64)
    with pytest.raises(CavpError):
        m.predict(image, audio)
    with pytest.raises(CavpError):
        m.predict(image, audio, return_prob=True)
    with pytest.raises(CavpError):
        m.predict_lowres(image, audio)


def test_update_lowres_and_op_need_device_tensors():
    from cavp_amd import metrics as MT
    from cavp_amd import ops
    from cavp_amd._lib import CavpError
    lo, y = torch.zeros(1, 4, 4, 2), torch.zeros(1, 16, 16, dtype=torch.int64)
    for acc in (MT.MIoU(2, 255, 0), MT.ForegroundDetect(24)):
        with pytest.raises(CavpError):
            acc.update_lowres(lo, y)
    with pytest.raises(CavpError):
        ops.seg_predict(lo, (16, 16), mask=torch.zeros(1, 16, 16, dtype=torch.uint8))
    with pytest.raises(CavpError):
        ops.seg_predict(lo, (16, 16), labels=y, num_classes=2, M=torch.zeros(6, dtype=torch.int64))
