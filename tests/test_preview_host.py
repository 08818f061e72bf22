"""CPU-side checks of the preview stage (cavp_amd/preview.py, csrc/preview.hip): the numpy restatement (tests/_preview_ref.py)
equals tests/golden/preview.npz - written by the reference's own get_pallete / colorize_mask / DeNormalize through
tools/make_golden_preview.py - byte for byte, for the palettes, the three panels and the resized panels; the library exports the
two entry points and the header, the exports and the ctypes table agree; the public entry fails loudly before any launch."""
import ctypes
import os
import re
import zlib

import numpy as np
import pytest
import torch

from tests import _preview_ref as R

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ENTRY_POINTS = ("cavp_preview_panels", "cavp_preview_resize")
MEAN, STD = (0.485, 0.456, 0.406), (0.229, 0.224, 0.225)
KS = (2, 24, 71, 256)
SHAPES = {"s": (5, 7), "v": (32, 48)}


@pytest.fixture(scope="module")
def gold():
    with np.load(os.path.join(REPO, "tests", "golden", "preview.npz")) as z:
        return {k: z[k] for k in z.files}


# ---- the restatement against the reference's pictures ---------------------------------------------------------------------------
@pytest.mark.parametrize("K", KS)
def test_palette_equals_the_reference(gold, K):
    from cavp_amd.preview import PreviewStage, palette
    want = gold[f"palette_K{K}"].tolist()
    assert R.palette(K) == want and palette(K) == want and PreviewStage(K, MEAN, STD).palette == want
    assert want[765:] == [255, 255, 255] and len(want) == 768
    if K < 255:
        assert not any(want[3 * K:765])
    if K == 2:
        assert want[:6] == [0, 0, 0, 255, 255, 255]


@pytest.mark.parametrize("tag", SHAPES)
def test_x_and_y_panels_equal_the_reference(gold, tag):
    x, bad = R.x_panel(gold[f"image_{tag}"], MEAN, STD)
    assert bad == 0 and x.dtype == np.uint8 and np.array_equal(x, gold[f"x_{tag}"])
    y = R.y_panel(gold[f"labels_{tag}"])
    assert np.array_equal(y, gold[f"y_{tag}"]) and np.array_equal(R.y_panel(gold[f"labels_{tag}"].astype(np.uint8)), y)
    assert np.array_equal(R.y_panel(gold[f"labels_{tag}"][:, None]), y)                     # [B, 1, H, W]
    lab = gold[f"labels_{tag}"]
    assert y[lab == -1].tolist() == [255, 255] and y[lab == 259].tolist() == [3, 3] and (y[1] == 255).all()


def test_fixture_image_shows_truncation_and_contraction(gold):
    """The 32 x 48 image holds every level six times per channel; the reference's bytes are NOT the identity on it (some levels come
    back one lower), and a fused multiply-add in the de-normalisation would give other bytes in every channel."""
    img, x = gold["image_v"], gold["x_v"].astype(np.int64)
    s, m = (np.asarray(v, np.float32).astype(np.float64).reshape(1, 3, 1, 1) for v in (STD, MEAN))
    fused = ((img.astype(np.float64) * s + m).astype(np.float32) * np.float32(255)).astype(np.int64).transpose(0, 2, 3, 1) & 255
    rounded = np.rint(((img * s.astype(np.float32) + m.astype(np.float32)) * np.float32(255)).transpose(0, 2, 3, 1)).astype(np.int64)
    for c in range(3):
        assert np.array_equal(np.sort(rounded[0, ..., c].ravel()), np.repeat(np.arange(256), 6))
        assert (x[..., c] == rounded[..., c] - 1).any() and (fused[..., c] != x[..., c]).any()


def test_byte_cast_wraps_like_torch():
    """A pin of the restatement alone (it runs no product code): torch's CPU byte cast truncates toward zero and wraps mod 256, and
    _preview_ref.x_panel follows it; the device is held to the same rule by test_gpu_preview.py."""
    vals = np.array([-1.5, -0.3, 255.9, 256.7, 300, 511.2, -255.5], dtype=np.float32)
    want = [255, 0, 255, 0, 44, 255, 1]
    assert torch.from_numpy(vals).byte().tolist() == want
    img = np.zeros((1, 3, 1, vals.size), dtype=np.float32)
    img[0, :] = vals
    x, bad = R.x_panel(img, MEAN, STD)
    chain = torch.stack([t.mul(s).add(m) for t, m, s in zip(torch.from_numpy(img[0]), MEAN, STD)]).mul(255)
    assert (chain.min() < -250) and (chain.max() > 400)                  # well outside [0, 255]
    assert bad == 0 and np.array_equal(x[0], chain.byte().permute(1, 2, 0).numpy())
    img[0, 1, 0, :3] = [np.nan, np.inf, 1e12]
    x, bad = R.x_panel(img, (0, 0, 0), (1, 1, 1))
    assert bad == 3 and x[0, 0, :3, 1].tolist() == [0, 0, 0]


@pytest.mark.parametrize("K", KS)
@pytest.mark.parametrize("tag", SHAPES)
def test_y_tilde_equals_the_reference(gold, tag, K):
    lg = R.fixture_logits(K, SHAPES[tag])
    assert zlib.crc32(lg.tobytes()) == int(gold[f"crc_{tag}_K{K}"]), "the seeded logits are not the ones the fixture was made from"
    assert np.isnan(lg).sum() == 1
    lab = gold[f"labels_{tag}"]
    pred = R.argmax_first(lg)
    assert pred[0, 1, 2] == K // 2                                      # the NaN wins
    assert np.array_equal(pred, torch.argmax(torch.from_numpy(lg), 1).numpy().astype(np.uint8))
    yt = R.y_tilde_panel(pred, lab)
    assert np.array_equal(yt, gold[f"yt_{tag}_K{K}_i64"])
    assert np.array_equal(R.y_tilde_panel(pred, lab.astype(np.uint8)), gold[f"yt_{tag}_K{K}_u8"])
    assert (yt[1] == 255).all() and (yt[lab == -1] == pred[lab == -1]).all()        # a -1 label does not propagate
    assert (gold[f"yt_{tag}_K{K}_u8"][lab == -1] == 255).all()                       # as uint8 it IS 255
    assert np.array_equal(R.preview(None, None, logits=lg, mean=MEAN, std=STD)["y_tilde"], pred)


@pytest.mark.parametrize("rname,size", [("r256", (256, 256)), ("r9x13", (9, 13))])
@pytest.mark.parametrize("tag", SHAPES)
def test_resized_panels_equal_pil(gold, tag, rname, size):
    got = R.preview(gold[f"image_{tag}"], gold[f"labels_{tag}"], logits=R.fixture_logits(71, SHAPES[tag]), mean=MEAN, std=STD, size=size)
    assert got["x"].shape == (3,) + size + (3,) and got["y"].shape == (3,) + size
    assert np.array_equal(got["x"], gold[f"x_{tag}_{rname}"]) and np.array_equal(got["y"], gold[f"y_{tag}_{rname}"])
    assert np.array_equal(got["y_tilde"], gold[f"yt_{tag}_K71_i64_{rname}"])


def test_nearest_table_equals_the_augment_restatement_and_pil():
    """The stage's host table builder against tests/_augment_ref.nearest_index (the rule FrameAugment's device table is held to) for
    every (in, out) pair up to 40 x 64 and the sizes a trainer uses, and against PIL itself on a ramp where PIL is installed."""
    from cavp_amd.preview import nearest_table
    from tests._augment_ref import nearest_index
    pairs = [(i, o) for i in range(1, 41) for o in range(1, 65)] + [(224, 256), (256, 224), (512, 256), (7, 256), (1000, 3), (3, 1000)]
    for i, o in pairs:
        t = nearest_table(i, o)
        assert t.dtype == np.int32 and t.min() >= 0 and t.max() < i and np.array_equal(t, nearest_index(i, o)), (i, o)
    try:
        from PIL import Image
    except ImportError:
        return
    for i, o in pairs[::37] + pairs[-6:]:
        if i <= 256:
            ramp = Image.fromarray(np.arange(i, dtype=np.uint8)[None, :])
            assert np.array_equal(np.asarray(ramp.resize((o, 1), Image.NEAREST))[0], nearest_table(i, o)), (i, o)


# ---- the library ----------------------------------------------------------------------------------------------------------------
def test_library_exports_the_preview_entry_points():
    from cavp_amd import _lib, build
    assert "preview.hip" in build.SOURCES
    build.build(verbose=False)
    lib = ctypes.CDLL(_lib.LIB_PATH)
    for name in ENTRY_POINTS:
        assert hasattr(lib, name), name
        assert name in _lib.PROTOTYPES, name
    assert _lib.ABI_VERSION == 16 == _lib.load().cavp_abi_version()


def test_header_and_ctypes_table_agree():
    from cavp_amd import _lib
    text = open(os.path.join(REPO, "include", "cavp_hip.h")).read()
    as_ctype = {"int32_t": ctypes.c_int32, "int64_t": ctypes.c_int64}
    for name in ENTRY_POINTS:
        m = re.search(r"\bint\s+" + name + r"\s*\(([^)]*)\)\s*;", text)
        assert m, f"{name} is not declared in include/cavp_hip.h"
        want = []
        for arg in m.group(1).split(","):
            arg = " ".join(arg.split())
            want.append(ctypes.c_void_p if "*" in arg else as_ctype[arg.replace("const ", "").split(" ")[0]])
        res, args = _lib.PROTOTYPES[name]
        assert res is ctypes.c_int32 and args == want, name


# ---- the public entry -----------------------------------------------------------------------------------------------------------
def test_constructor_refusals_and_no_device_touched():
    from cavp_amd._lib import CavpError
    from cavp_amd.preview import PreviewStage
    pv = PreviewStage(71, MEAN, STD, size=(256, 256))
    assert pv._state is None and pv.size == (256, 256) and pv.mean_std_host.dtype == np.float32
    assert pv.mean_std_host.tolist() == [float(np.float32(v)) for v in MEAN + STD]
    for bad in (dict(num_classes=0), dict(num_classes=257), dict(max_batch=0), dict(max_batch=1025), dict(mean=(0.5, 0.5)),
                dict(std=(1, 1, float("nan"))), dict(size=(0, 4)), dict(size=(4,))):
        kw = dict(num_classes=71, mean=MEAN, std=STD)
        kw.update(bad)
        with pytest.raises(CavpError):
            PreviewStage(**kw)
    with pytest.raises(CavpError):
        pv.check()


def test_call_refusals_come_before_any_launch():
    from cavp_amd._lib import CavpError
    from cavp_amd.preview import PreviewStage
    pv = PreviewStage(71, MEAN, STD, max_batch=4)
    B, H, W = 2, 5, 7
    img, lab = torch.zeros(B, 3, H, W), torch.zeros(B, H, W, dtype=torch.int64)
    lg, mk = torch.zeros(B, 71, H, W), torch.zeros(B, H, W, dtype=torch.uint8)
    with pytest.raises(CavpError, match="exactly one"):
        pv(img, lab)
    with pytest.raises(CavpError, match="exactly one"):
        pv(img, lab, logits=lg, mask=mk)
    with pytest.raises(CavpError, match=r"float32 \[B, C, H, W\]"):
        pv(img, lab, logits=lg.double())
    with pytest.raises(CavpError, match=r"float32 \[B, C, H, W\]"):
        pv(img, lab, logits=lg[0])
    with pytest.raises(CavpError, match="256 classes"):
        pv(img, lab, logits=torch.zeros(B, 257, H, W))
    with pytest.raises(CavpError, match=r"uint8 \[B, H, W\]"):
        pv(img, lab, mask=mk.long())
    with pytest.raises(CavpError, match=r"uint8 \[B, H, W\]"):
        pv(img, lab, mask=mk[:, None])
    with pytest.raises(CavpError, match="max_batch"):
        pv(None, None, mask=torch.zeros(5, H, W, dtype=torch.uint8))
    with pytest.raises(CavpError, match="empty"):
        pv(None, None, mask=torch.zeros(B, 0, W, dtype=torch.uint8))
    with pytest.raises(CavpError, match="image must be float32"):
        pv(img.double(), lab, logits=lg)
    with pytest.raises(CavpError, match="image must be float32"):
        pv(torch.zeros(B, 3, H, W + 1), lab, logits=lg)
    with pytest.raises(CavpError, match="labels must be int64 or uint8"):
        pv(img, lab.int(), logits=lg)
    with pytest.raises(CavpError, match="labels must be int64 or uint8"):
        pv(img, torch.zeros(B, 2, H, W, dtype=torch.int64), logits=lg)
    with pytest.raises(CavpError, match="logits must be contiguous"):
        pv(img, lab, logits=torch.zeros(B, H, W, 71).permute(0, 3, 1, 2))
    with pytest.raises(CavpError, match="image must be contiguous"):
        pv(torch.zeros(B, H, W, 3).permute(0, 3, 1, 2), lab, logits=lg)
    with pytest.raises(CavpError, match="labels must be contiguous"):
        pv(img, torch.zeros(B, W, H, dtype=torch.int64).transpose(1, 2), logits=lg)
    with pytest.raises(CavpError, match="mask must be contiguous"):
        pv(img, lab, mask=torch.zeros(B, W, H, dtype=torch.uint8).transpose(1, 2))
    with pytest.raises(CavpError, match="CPU tensor"):
        pv(img, lab, logits=lg)
    assert pv._state is None                                             # nothing was allocated, nothing was launched
