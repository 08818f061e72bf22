"""CPU-side checks of the native step's contrast term: the library exports the two entry points that work on the tape's fusion map,
the plan -> row addressing helper, and the public entries fail loudly without a device."""
import ctypes
import types

import numpy as np
import pytest
import torch


def _model():
    from cavp_amd.cavp_model import CAVP
    args = types.SimpleNamespace(seg_model="DeepLabV3Plus", last_three_dilation_stride=[False, False, False], audio_backbone="vgg",
                                 num_classes=2, batch_size=2, local_rank="cpu")
    return CAVP(50, None, num_classes=2, args=args)


def test_library_exports_the_nhwc_contrast_kernels():
    from cavp_amd import _lib, build
    build.build(verbose=False)
    lib = ctypes.CDLL(_lib.LIB_PATH)
    for name in ("cavp_contrast_gather_nhwc", "cavp_contrast_rows_bwd_add"):
        assert hasattr(lib, name) and name in _lib.PROTOTYPES
    _lib.load()


def test_kernels_reject_bad_arguments_on_the_host():
    """the argument checks run before any launch: no device needed"""
    from cavp_amd import _lib
    lib = _lib.load()
    buf = (ctypes.c_float * 64)()
    idx = (ctypes.c_int32 * 8)()
    p, i = ctypes.cast(buf, ctypes.c_void_p), ctypes.cast(idx, ctypes.c_void_p)

    def gather(dtype=_lib.BF16, C=16, ld=16, N=4, n_match=2, rows=4, x=p):
        return lib.cavp_contrast_gather_nhwc(dtype, x, 1, 4, ld, C, None, i, i, 0, N, n_match, rows, 1e-12, p, p, None)

    def add(dtype=_lib.BF16, C=16, ld=16, N=4, n_match=2):
        return lib.cavp_contrast_rows_bwd_add(dtype, p, 1, 4, ld, C, None, i, i, 0, N, n_match, p, p, p, 1.0, None)

    for call in (gather, add):
        assert call(C=36, ld=40) == _lib.ERR_BAD_ARG          # width not a multiple of 8
        assert call(C=16, ld=8) == _lib.ERR_BAD_ARG           # ld < C
        assert call(dtype=_lib.F32, C=8, ld=10) == _lib.ERR_BAD_ARG   # ld not a multiple of the 16-byte vector
        assert call(N=0) == _lib.ERR_BAD_ARG
        assert call(n_match=5) == _lib.ERR_BAD_ARG
        assert call(dtype=7) == _lib.ERR_BAD_ARG
    assert gather(rows=3) == _lib.ERR_BAD_ARG                  # fewer rows of A than anchors
    assert gather(x=None) == _lib.ERR_BAD_ARG


def test_chain_kernels_reject_bad_arguments_on_the_host():
    """the four entry points of the strided-f32 chain, in both count modes (header / host): checked before any launch"""
    from cavp_amd import _lib
    lib = _lib.load()
    buf = (ctypes.c_float * 64)()
    idx = (ctypes.c_int32 * 8)()
    p, i = ctypes.cast(buf, ctypes.c_void_p), ctypes.cast(idx, ctypes.c_void_p)

    def gather(header=None, cap=0, N=4, n_match=2, rows=4, C=16, xm=p, xs=p, ib=i, ip=i, A=p, norms=p):
        return lib.cavp_gather_l2norm(xm, 64, 1, 16, xs, 64, 1, 16, header, ib, ip, cap, N, n_match, rows, C, 1e-12, A, norms, None)

    def scatter(header=None, cap=0, N=4, n_match=2, C=16, dA=p, A=p, norms=p, ib=i, ip=i, dxm=p, dxs=p):
        return lib.cavp_l2norm_bwd_scatter(dA, A, norms, header, ib, ip, cap, N, n_match, C, dxm, 64, 1, 16, dxs, 64, 1, 16, None)

    def rows(header=None, cap=0, N=4, ld=4, S=p, labels=i, mlpp=p, loss=p):
        return lib.cavp_infonce_rows(S, labels, header, cap, N, ld, 1e-12, mlpp, loss, None, 1.0, None)

    for call, operands in ((gather, ("xm", "xs", "ib", "ip", "A", "norms")),
                           (scatter, ("dA", "A", "norms", "ib", "ip", "dxm", "dxs")), (rows, ("S", "labels", "mlpp", "loss"))):
        for name in operands:
            assert call(**{name: None}) == _lib.ERR_BAD_ARG, (call.__name__, name)
            assert call(header=i, cap=4, **{name: None}) == _lib.ERR_BAD_ARG, (call.__name__, name)
        for cap in (0, -1):
            assert call(header=i, cap=cap) == _lib.ERR_BAD_ARG       # header mode: N is ignored, the capacity is not
        for N in (0, -3):
            assert call(N=N) == _lib.ERR_BAD_ARG
    for call in (gather, scatter):
        assert call(n_match=-1) == _lib.ERR_BAD_ARG
        assert call(n_match=5) == _lib.ERR_BAD_ARG
        assert call(C=0) == _lib.ERR_BAD_ARG
    assert gather(rows=3) == _lib.ERR_BAD_ARG                     # fewer rows of A than the count, in either mode
    assert gather(header=i, cap=8, rows=7) == _lib.ERR_BAD_ARG
    assert rows(ld=3) == _lib.ERR_BAD_ARG
    assert rows(header=i, cap=8, ld=7) == _lib.ERR_BAD_ARG

    for bad in (dict(d=None), dict(g=None), dict(n=0), dict(n=-2)):
        a = dict(d=p, g=p, n=4)
        a.update(bad)
        for scale_dev in (None, p):
            assert lib.cavp_symm_add(a["d"], a["g"], a["n"], 1.0, scale_dev, None) == _lib.ERR_BAD_ARG
    # scale_dev == NULL is a legal call: it gets past the checks, to the launch.  Host memory must not reach a kernel, so this is
    # probed only where there is no device to launch on; with one, tests/test_gpu_train_step_contrast.py makes the call on device memory
    if not torch.cuda.is_available():
        assert lib.cavp_symm_add(p, p, 4, 1.0, None, None) != _lib.ERR_BAD_ARG


def test_anchor_rows_addresses_both_halves():
    from cavp_amd._lib import CavpError
    from cavp_amd.contrast import anchor_rows
    B, hw = 3, 10
    b, p = np.array([0, 2, 1, 2, 0], dtype=np.int32), np.array([0, 9, 4, 9, 7], dtype=np.int32)
    assert anchor_rows(b, p, 3, B, hw).tolist() == [0, 29, 14, (3 + 2) * 10 + 9, 3 * 10 + 7]
    assert anchor_rows(b, p, 5, B, hw).tolist() == [0, 29, 14, 29, 7]          # all in the match half
    assert anchor_rows(b, p, 0, B, hw).tolist() == [30, 59, 44, 59, 37]        # all in the shuffle half
    assert anchor_rows(b[:0], p[:0], 0, B, hw).shape == (0,)
    for bad in ((np.array([3]), np.array([0]), 1), (np.array([0]), np.array([10]), 1), (np.array([-1]), np.array([0]), 0),
                (np.array([0]), np.array([0]), 2)):
        with pytest.raises(CavpError):
            anchor_rows(bad[0], bad[1], bad[2], B, hw)


def test_native_contrast_step_needs_device_tensors():
    from cavp_amd._lib import CavpError
    from cavp_amd.contrast import ContrastLoss
    m = _model().train()
    crit = ContrastLoss(temperature=0.1, ignore_idx=255, max_views=32)
    image, audio = torch.zeros(2, 3, 32, 32), torch.zeros(4, 1, 96, 64)
    label = torch.zeros(2, 32, 32, dtype=torch.int64)
    with pytest.raises(CavpError):
        m.train_step(image, audio, label, contrast=crit, label_shuffle=label)
    with pytest.raises(CavpError):
        m.capture_train_step(image, audio, label, contrast=crit, label_shuffle=label)   # (and the host sampler cannot be captured)


def test_fusion_map_size_follows_the_stem():
    m = _model()
    assert m._fusion_hw(torch.zeros(1, 3, 224, 224)) == (56, 56)
    assert m._fusion_hw(torch.zeros(1, 3, 64, 64)) == (16, 16)
    assert m._fusion_hw(torch.zeros(1, 3, 65, 97)) == (17, 25)
