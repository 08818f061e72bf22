"""CPU-side checks of the resize variant of the frame augmentation (FrameAugment(resize=True), csrc/augment.hip): the library
exports the three entry points and the header, the exports and the ctypes table agree; ref_pil_resize (PIL calls) equals
ref_np_resize (integer numpy) stage by stage for every size triple the fixture uses; the fixture is what PIL gives and stays
inside the device variant's conditions; the composed nearest table equals the two-step result; the constructor refuses what the
kernels do not cover."""
import ctypes
import os
import re

import numpy as np
import pytest

from tests import _augment_ref as R
from tests import _augment_resize_ref as RR

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ENTRY_POINTS = ("cavp_aug_plan_resize", "cavp_aug_resize_store", "cavp_aug_resize_render")
GROUPS = {"geo": "main", "jit": "main", "eval": "main", "coco": "coco", "ident": "ident", "chain": "chain"}


def golden():
    return dict(np.load(os.path.join(REPO, "tests", "golden", "augment_resize.npz")))


def cases(g, group):
    """(k, frame corner, mask corner, output size, row, scales) of every case of a group."""
    s = GROUPS[group]
    size_out, scales = tuple(int(v) for v in g[s + "_out"]), tuple(float(v) for v in g[s + "_scales"])
    for k, (i, row) in enumerate(zip(g[group + "_sample"], g[group + "_params"])):
        h, w = (int(v) for v in g[s + "_sizes"][i])
        yield k, g[s + "_frames"][i, :h, :w], g[s + "_masks"][i, :h, :w], size_out, row, scales


def test_library_exports_the_resize_entry_points():
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


@pytest.mark.parametrize("group", sorted(GROUPS))
def test_pil_equals_numpy_stage_by_stage_and_the_fixture(group):
    g = golden()
    jitter, identity = group == "jit", group == "eval"
    n = 0
    for k, frame, mask, size_out, row, scales in cases(g, group):
        assert RR.ratios_ok(*mask.shape, size_out, None if identity else scales[int(row[1])])
        a = RR.replay_row(RR.ref_pil_resize, frame, mask, size_out, row, scales=scales, jitter=jitter, identity=identity)
        b = RR.replay_row(RR.ref_np_resize, frame, mask, size_out, row, scales=scales, jitter=jitter, identity=identity)
        assert set(a[2]) == set(b[2])
        for name in a[2]:
            assert np.array_equal(a[2][name], b[2][name]), (group, k, name)
        assert np.array_equal(a[0], g[group + "_image"][k]) and np.array_equal(a[1], g[group + "_mask"][k]), (group, k)
        if jitter:
            assert a[2].get("contrast_mean", -1) == g["jit_mean"][k]
        n += 1
    assert n == len(g[group + "_params"]) > 0


def test_fixture_reaches_the_branches():
    g = golden()
    assert tuple(g["main_stage"]) == (192, 64) and tuple(g["main_out"]) == (24, 72) and g["main_sizes"].tolist() == [[192, 64], [150, 61], [37, 29]]
    rows = g["geo_params"]
    assert len(rows) == 18 and set(rows[:, 0]) == {0, 1} and set(rows[:, 1]) == {0, 1, 2}
    xmin, num, _ = R.bicubic_coeffs(192, 24)
    assert 12 < num.max() == 32 <= 34                                 # ratio 8: above the crop variant's 12 taps, inside the 34
    assert len({tuple(r[2:6]) for r in g["jit_params"]}) == 24
    assert sorted(g["coco_params"][:, 1].tolist()) == [3, 3, 6, 6] and 2 * int(g["coco_stage"][0]) == 8 * int(g["coco_out"][0])
    assert np.array_equal(g["ident_image"][0], g["ident_frames"][0])  # the identity is an exact copy
    assert os.path.getsize(os.path.join(REPO, "tests", "golden", "augment_resize.npz")) < 400 * 1024


@pytest.mark.parametrize("sizes", [(150, 112, 24), (61, 45, 72), (37, 18, 24), (29, 14, 72), (192, 96, 24), (64, 64, 72), (16, 12, 9),
                                   (48, 48, 48), (96, 192, 24), (75, 93, 24), (64, 128, 72), (200, 150, 40), (29, 14, 40)])
@pytest.mark.parametrize("mirror", [False, True])
def test_composed_nearest_equals_the_two_steps(sizes, mirror):
    n_in, n_scaled, n_out = sizes
    src = np.arange(n_in)[::-1] if mirror else np.arange(n_in)
    two = src[R.nearest_index(n_in, n_scaled)][R.nearest_index(n_scaled, n_out)]
    assert np.array_equal(RR.composed_nearest(n_in, n_scaled, n_out, mirror), two)
    from PIL import Image
    pil = np.asarray(Image.fromarray(np.arange(n_in, dtype=np.uint8)[None, :].repeat(2, 0), "L").resize((n_scaled, 2), Image.NEAREST)
                     .resize((n_out, 2), Image.NEAREST))[0]
    assert np.array_equal(R.nearest_index(n_in, n_scaled)[R.nearest_index(n_scaled, n_out)], pil)


def test_constructor_refusals():
    from cavp_amd._lib import CavpError
    from cavp_amd.augment import FrameAugment
    ok = FrameAugment(crop=(24, 72), scales=R.AVS_SCALES, jitter=None, stage=(192, 64), resize=True)      # 192 = 8 * 24: the limit
    assert ok.resize and FrameAugment(crop=(24, 24), stage=(48, 64)).resize is False
    with pytest.raises(CavpError, match="at most 8"):
        FrameAugment(crop=(24, 72), scales=R.AVS_SCALES, jitter=None, stage=(193, 64), resize=True)
    with pytest.raises(CavpError, match="at most 8"):
        FrameAugment(crop=(24, 72), scales=R.COCO_SCALES, stage=(97, 64), resize=True)                     # 2 * 97 > 8 * 24
    with pytest.raises(CavpError, match="pad_fill"):
        FrameAugment(crop=(24, 72), scales=R.AVS_SCALES, stage=(192, 64), resize=True, pad_fill=(1, 2, 3))
    with pytest.raises(CavpError, match="fit the stage"):
        FrameAugment(crop=(24, 72), scales=R.AVS_SCALES, stage=(192, 64))                                  # the crop variant still refuses
    FrameAugment(crop=(24, 24), stage=(48, 64), pad_fill=(1, 2, 3))                                        # and still takes a fill
