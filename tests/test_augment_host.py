"""CPU-side checks of the frame augmentation (cavp_amd/augment.py, csrc/augment.hip): the library exports the three entry points
and the header, the exports and the ctypes table agree; the numpy restatement (tests/_augment_ref.ref_np, the specification the
kernels implement) equals PIL stage by stage - the two colour conversions and L over all 2^24 colours, the blend over all byte
pairs, the bicubic passes and the nearest index maps for every (size, scale) pair the GPU tests use and for 640 x 480 /
427 x 640 frames; ref_pil reproduces tests/golden/augment.npz; the public entry fails loudly."""
import ctypes
import os
import re

import numpy as np
import pytest
import torch

from tests import _augment_ref as R

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ENTRY_POINTS = ("cavp_aug_plan", "cavp_aug_contrast_mean", "cavp_aug_render")
FACTORS = (0.5, 0.8, 1.0, 1.3, 1.5)
Image = pytest.importorskip("PIL.Image")


def golden():
    return np.load(os.path.join(REPO, "tests", "golden", "augment.npz"))


def test_library_exports_the_augment_entry_points():
    from cavp_amd import _lib, build
    build.build(verbose=False)
    lib = ctypes.CDLL(_lib.LIB_PATH)
    for name in ENTRY_POINTS:
        assert hasattr(lib, name), name
        assert name in _lib.PROTOTYPES, name
    assert _lib.ABI_VERSION == _lib.load().cavp_abi_version()


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


# ------------------------------------------------------------------------------------------------------- stage by stage vs PIL
@pytest.fixture(scope="module")
def all_colours():
    v = np.arange(1 << 24, dtype=np.uint32)
    return np.stack([(v >> 16) & 255, (v >> 8) & 255, v & 255], -1).astype(np.uint8).reshape(4096, 4096, 3)


def test_rgb_to_hsv_all_colours(all_colours):
    pil = np.asarray(Image.fromarray(all_colours, "RGB").convert("HSV"))
    assert np.array_equal(pil, R.rgb_to_hsv(all_colours))


def test_hsv_to_rgb_all_triples(all_colours):
    pil = np.asarray(Image.fromarray(all_colours, "HSV").convert("RGB"))
    assert np.array_equal(pil, R.hsv_to_rgb(all_colours))


def test_luma_all_colours(all_colours):
    assert np.array_equal(np.asarray(Image.fromarray(all_colours, "RGB").convert("L")), R.luma(all_colours))


@pytest.mark.parametrize("factor", FACTORS)
def test_blend_all_byte_pairs(factor):
    a, b = np.meshgrid(np.arange(256, dtype=np.uint8), np.arange(256, dtype=np.uint8), indexing="ij")
    pil = np.asarray(Image.blend(Image.fromarray(a, "L"), Image.fromarray(b, "L"), factor))
    assert np.array_equal(pil, R.blend(a, b, factor))


def _size_pairs():
    """(in, out) of every resize pass: the fixture's sizes and (640, 480), (427, 640), at all seven scales."""
    pairs = set()
    for h, w in [tuple(s) for s in golden()["sizes"]] + [(640, 480), (427, 640)]:
        for s in R.COCO_SCALES:
            oh, ow = R.scaled_size(int(h), int(w), s)
            pairs.update({(int(h), oh), (int(w), ow)})
    return sorted(pairs)


def test_nearest_index_maps():
    """A mode-"I" index ramp through Image.resize(NEAREST) shows PIL's source index of every output index."""
    for n, m in _size_pairs():
        ramp = Image.fromarray(np.arange(n, dtype=np.int32)[None, :].repeat(2, 0), "I")
        pil = np.asarray(ramp.resize((m, 2), Image.NEAREST))[0]
        assert np.array_equal(pil, R.nearest_index(n, m)), (n, m)


def test_nearest_is_not_the_floor_rule():
    assert R.nearest_index(16, 12).tolist() == [0, 2, 3, 4, 5, 7, 8, 10, 11, 12, 14, 15]
    assert R.nearest_index(8, 14).tolist() == [0, 0, 1, 1, 2, 3, 3, 4, 4, 5, 5, 6, 7, 7]


def test_bicubic_coefficient_tables():
    """PIL does not show its tables; a one-pass resize of random and of extreme bytes (every tap's sign and the clipping at both
    ends) does, as far as 8 bits can: exact equality for every (in, out) pair, in both directions."""
    rng = np.random.default_rng(7)
    taps = 0
    for n, m in _size_pairs():
        strip = np.concatenate([rng.integers(0, 256, (3, n, 3), dtype=np.uint8), rng.choice(np.array([0, 255], np.uint8), (3, n, 3))])
        pil = np.asarray(Image.fromarray(strip, "RGB").resize((m, 6), Image.BICUBIC))
        assert np.array_equal(pil, R.resize_bicubic(strip, (6, m))), (n, m)
        col = np.ascontiguousarray(strip.transpose(1, 0, 2))
        pil = np.asarray(Image.fromarray(col, "RGB").resize((6, m), Image.BICUBIC))
        assert np.array_equal(pil, R.resize_bicubic(col, (m, 6))), (n, m)
        xmin, num, kk = R.bicubic_coeffs(n, m)
        assert (kk.sum(1) - (1 << 22)).__abs__().max() <= 8 and (xmin + num <= n).all()
        taps = max(taps, int(num.max()))
    assert taps <= 12        # kAugTaps of csrc/augment.hip


def _cases(g):
    for prefix, jitter in (("geo", False), ("pad", False), ("jit", True)):
        crop = tuple(int(v) for v in g[prefix + "_crop"])
        for k in range(len(g[prefix + "_sample"])):
            i = int(g[prefix + "_sample"][k])
            h, w = (int(v) for v in g["sizes"][i])
            yield prefix, k, g["frames"][i, :h, :w], g["masks"][i, :h, :w], crop, g[prefix + "_params"][k], jitter


def test_restatement_equals_pil_stage_by_stage():
    g = golden()
    n = 0
    for prefix, k, frame, mask, crop, row, jitter in _cases(g):
        a = R.replay_row(R.ref_pil, frame, mask, crop, row, jitter=jitter)
        b = R.replay_row(R.ref_np, frame, mask, crop, row, jitter=jitter)
        assert a[2].keys() == b[2].keys()
        for stage in a[2]:
            assert np.array_equal(a[2][stage], b[2][stage]), (prefix, k, stage)
        assert np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1])
        n += 1
    assert n == 54 + 4 + 24


def test_restatement_equals_fixture():
    """ref_np against the recorded ref_pil results: holds whatever PIL is installed."""
    g = golden()
    for prefix, k, frame, mask, crop, row, jitter in _cases(g):
        img, lbl, st = R.replay_row(R.ref_np, frame, mask, crop, row, jitter=jitter)
        assert np.array_equal(img, g[prefix + "_image"][k]) and np.array_equal(lbl, g[prefix + "_mask"][k]), (prefix, k)
        if jitter:
            assert st["contrast_mean"] == int(g["jit_mean"][k])


def test_pil_reproduces_fixture():
    import PIL
    g = golden()
    if PIL.__version__ != str(g["pil_version"]):
        pytest.skip(f"the fixture was recorded with PIL {g['pil_version']}, installed is {PIL.__version__}")
    for prefix, k, frame, mask, crop, row, jitter in _cases(g):
        img, lbl, _ = R.replay_row(R.ref_pil, frame, mask, crop, row, jitter=jitter)
        assert np.array_equal(img, g[prefix + "_image"][k]) and np.array_equal(lbl, g[prefix + "_mask"][k]), (prefix, k)


def test_fixture_bad_cases_raise_in_the_reference():
    g = golden()
    crop = tuple(int(v) for v in g["geo_crop"])
    assert len(g["bad_sample"]) >= 1
    for i, row in zip(g["bad_sample"], g["bad_params"]):
        h, w = (int(v) for v in g["sizes"][i])
        for ref in (R.ref_pil, R.ref_np):
            with pytest.raises(ValueError):
                R.replay_row(ref, g["frames"][i, :h, :w], g["masks"][i, :h, :w], crop, row)


def test_hue_shift_is_torchvisions_uint8():
    assert [R.hue_shift_u8(v) for v in (0.0, 0.25, -0.1, -0.25, 0.001)] == [0, 63, 231, 193, 0]


# ------------------------------------------------------------------------------------------------------------- loud failures
def test_frame_augment_fails_loudly():
    from cavp_amd._lib import CavpError
    from cavp_amd.augment import N_PARAMS, FrameAugment, make_params
    kw = dict(crop=(16, 24), stage=(48, 64), max_batch=4)
    with pytest.raises(CavpError, match="1/64"):
        FrameAugment(scales=(0.5, 0.7), **kw)
    with pytest.raises(CavpError, match="outside"):
        FrameAugment(scales=(0.25,), **kw)
    with pytest.raises(CavpError, match="fit the stage"):
        FrameAugment(crop=(49, 24), stage=(48, 64))
    with pytest.raises(CavpError, match="fit the stage"):
        FrameAugment(crop=(16, 65), stage=(48, 64))
    with pytest.raises(CavpError, match="stage"):
        FrameAugment(crop=(16, 24))
    with pytest.raises(CavpError, match="jitter"):
        FrameAugment(jitter=(.4, .4, .4, .1), **kw)
    with pytest.raises(CavpError, match="pad_fill"):
        FrameAugment(pad_fill=(0, 0, 256), **kw)
    with pytest.raises(CavpError, match="max_batch"):
        FrameAugment(crop=(16, 24), stage=(48, 64), max_batch=1025)
    aug = FrameAugment(**kw)
    assert aug.pad_fill == (123, 116, 103)
    frames, masks = torch.zeros(2, 48, 64, 3, dtype=torch.uint8), torch.zeros(2, 48, 64, dtype=torch.uint8)
    sizes = torch.tensor([[48, 64], [20, 30]], dtype=torch.int32)
    with pytest.raises(CavpError, match="CPU tensor"):
        aug(frames, masks, sizes)
    with pytest.raises(CavpError, match="CPU tensor"):
        aug.eval_(frames, masks, sizes)
    with pytest.raises(CavpError, match="frames"):
        aug(frames.float(), masks, sizes)
    with pytest.raises(CavpError, match="frames"):
        aug(frames.permute(0, 3, 1, 2).contiguous(), masks, sizes)
    with pytest.raises(CavpError, match="masks"):
        aug(frames, masks.long(), sizes)
    with pytest.raises(CavpError, match="masks"):
        aug(frames, masks[:, :40], sizes)
    with pytest.raises(CavpError, match="sizes"):
        aug(frames, masks, sizes.long())
    with pytest.raises(CavpError, match="params"):
        aug(frames, masks, sizes, params=torch.zeros(2, N_PARAMS))
    with pytest.raises(CavpError, match="max_batch"):
        aug(torch.zeros(5, 48, 64, 3, dtype=torch.uint8), torch.zeros(5, 48, 64, dtype=torch.uint8), torch.ones(5, 2, dtype=torch.int32))
    with pytest.raises(CavpError):
        aug.check()
    row = make_params(1, 3, 5, 7, order=(3, 1, 0, 2), brightness=1.5, contrast=0.5, saturation=1.25, hue_shift=231)
    assert row.dtype == torch.int32 and row.tolist() == R.params_row(1, 3, 5, 7, (3, 1, 0, 2), 1.5, 0.5, 1.25, 231).tolist()
