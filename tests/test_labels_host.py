"""CPU-side checks of the label stage (cavp_amd/labels.py, csrc/labels.hip): the library exports the three entry points and the
header, the exports and the ctypes table agree; the numpy restatement (tests/_labels_ref.py) equals the reference data sets'
expressions evaluated with torch (unique / one_hot, the in-place remap loop over a class_dict / index_table pair, the binary
collapse, the AVSBench sum); the per-pixel closed form of the remap equals the literal loop over an exhaustive family of small
cases; the public entry fails loudly."""
import ctypes
import itertools
import os
import re

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from tests import _labels_ref as R

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ENTRY_POINTS = ("cavp_labels_presence", "cavp_labels_scan", "cavp_labels_expand")


def test_library_exports_the_label_entry_points():
    from cavp_amd import _lib, build
    assert "labels.hip" in build.SOURCES
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


# ---- the reference's expressions, evaluated with torch ---------------------------------------------------------------------------
def _torch_vpo(label, class_dict, index_table, K):
    """One image as the VPO data set treats it: the in-place loop over unique(label) without 0 and 255, then the class vector."""
    label = label.clone()
    values = torch.unique(label.clone())
    values = values[values != 0]
    values = values[values != 255].tolist()
    for v in values:
        label[label == v] = index_table.index(class_dict[str(v)])
    return label, F.one_hot(torch.unique(label[label != 255]), num_classes=K).sum(0)


def _tables(rng, K, raw_values):
    """A class_dict over raw mask values and an index_table of K names, as the data set holds them, and the int table of both."""
    index_table = ["background"] + [f"c{j}" for j in range(1, K)]
    class_dict, remap = {}, np.full(256, -1, dtype=np.int32)
    for v in raw_values:
        t = int(rng.integers(1, K))
        class_dict[str(v)] = index_table[t]
        remap[v] = t
    return class_dict, index_table, remap


@pytest.mark.parametrize("seed", range(6))
def test_restatement_equals_the_vpo_expressions(seed):
    """Raw values 1 .. 11 remapped into [1, K) at random, K = 7: targets meet raw values that are present and larger (the loop moves
    those pixels twice), smaller, or equal."""
    rng = np.random.default_rng(seed)
    K, raw = 7, list(range(1, 12))
    class_dict, index_table, remap = _tables(rng, K, raw)
    lab = rng.choice(np.array([0, 255] + raw), size=(4, 6, 9), p=[.3, .1] + [.6 / len(raw)] * len(raw)).astype(np.int64)
    lab[3] = 255
    got = R.label_stage(lab, K, "multi_hot", remap=remap)
    twice = 0
    for b in range(lab.shape[0]):
        want_label, want_vec = _torch_vpo(torch.from_numpy(lab[b]), class_dict, index_table, K)
        assert np.array_equal(got["label"][b], want_label.numpy()), b
        assert np.array_equal(got["img_label"][b], want_vec.numpy()), b
        twice += int((got["label"][b] != np.where((lab[b] == 0) | (lab[b] == 255), lab[b], remap[np.clip(lab[b], 0, 255)])).sum())
    assert got["bad"] == 0 and not got["img_label"][3].any()
    if seed == 0:
        assert twice > 0          # the family does show the chained move


@pytest.mark.parametrize("binary", [False, True])
def test_restatement_equals_the_avss_expressions(binary):
    rng = np.random.default_rng(5)
    K = 71
    lab = rng.choice(np.array([0, 3, 17, 70, 255]), size=(5, 7, 5)).astype(np.int64)
    lab[1], lab[2] = 0, 255
    got = R.label_stage(lab, K, "multi_hot", binary=binary)
    t = torch.from_numpy(lab.copy())
    want_vec = torch.stack([F.one_hot(torch.unique(t[i][t[i] != 255]), num_classes=K).sum(0) for i in range(len(t))])
    if binary:
        t[(t != 255) & (t != 0)] = 1
    assert np.array_equal(got["img_label"], want_vec.numpy()) and np.array_equal(got["label"], t.numpy()) and got["bad"] == 0
    assert got["img_label"][1].tolist() == [1] + [0] * (K - 1) and not got["img_label"][2].any()


def test_restatement_equals_the_avsbench_expression():
    masks = np.zeros((4, 1, 6, 6), dtype=np.int64)
    masks[1, 0, 5, 5] = 1
    masks[2, 0, 0, 0] = 255
    masks[3] = 1
    for b in range(4):
        t = torch.from_numpy(masks[b])
        want = F.one_hot((t.view(1, -1).sum(-1) != 0).long(), num_classes=2)[0]
        got = R.label_stage(masks[b], 2, "any_foreground")
        assert np.array_equal(got["img_label"][0], want.numpy()), b
    assert R.label_stage(masks[2], 2, "any_foreground")["img_label"].tolist() == [[0, 1]]


def test_values_where_the_reference_raises_are_counted():
    lab = np.array([[[0, 3, 200, 255], [3, 3, 70, 71]]], dtype=np.int64)
    with pytest.raises(RuntimeError):
        F.one_hot(torch.unique(torch.from_numpy(lab[0])[torch.from_numpy(lab[0]) != 255]), num_classes=71)
    got = R.label_stage(lab, 71)
    assert got["bad"] == 2 and got["img_label"][0].nonzero()[0].tolist() == [0, 3, 70]
    remap = np.full(256, -1, dtype=np.int32)
    remap[3] = 5
    got = R.label_stage(lab, 71, remap=remap)          # 200, 70, 71 have no entry: kept, bad; 200 and 71 are no class either
    assert got["bad"] == 3 and got["label"].tolist() == [[[0, 5, 200, 255], [5, 5, 70, 71]]]
    assert got["img_label"][0].nonzero()[0].tolist() == [0, 5, 70]


def test_empty_and_ignore_only_images():
    empty = np.zeros((2, 0, 5), dtype=np.int64)
    assert R.label_stage(empty, 4)["img_label"].tolist() == [[0] * 4] * 2
    assert R.label_stage(empty, 2, "any_foreground")["img_label"].tolist() == [[1, 0]] * 2
    t = torch.from_numpy(empty[0])
    assert F.one_hot(torch.unique(t[t != 255]), num_classes=4).sum(0).tolist() == [0] * 4
    ign = np.full((1, 3, 3), 255, dtype=np.int64)
    assert R.label_stage(ign, 4)["img_label"].tolist() == [[0] * 4]
    assert R.label_stage(ign, 4, remap=np.arange(256), binary=True)["label"].tolist() == ign.tolist()
    assert R.label_stage(ign, 2, "any_foreground")["img_label"].tolist() == [[0, 1]]


# ---- the closed form of the remap against the literal loop -----------------------------------------------------------------------
def _same(lab, remap):
    a, bad_a = R.remap_loop(lab, remap)
    b, bad_b = R.remap_closed_form(lab, remap)
    assert np.array_equal(a, b) and np.array_equal(bad_a, bad_b), (lab.tolist(), [int(v) for v in remap[:8]])
    return a, bad_a


def test_closed_form_named_cases():
    ident = np.arange(256, dtype=np.int32)
    lab = np.array([[0, 3, 3, 5, 255, 7, 9, 2]], dtype=np.int64)
    chained = ident.copy()
    chained[3], chained[5] = 5, 6                     # 3 -> 5 with 5 present: those pixels go on to 6
    out, bad = _same(lab, chained)
    assert out.tolist() == [[0, 6, 6, 6, 255, 7, 9, 2]] and not bad.any()
    absent = ident.copy()
    absent[3], absent[4] = 4, 6                       # 3 -> 4 with 4 absent: no step 4
    assert _same(lab, absent)[0].tolist() == [[0, 4, 4, 5, 255, 7, 9, 2]]
    down = ident.copy()
    down[7], down[2] = 2, 1                           # 7 -> 2 downwards: step 2 is over, the pixels stay 2
    assert _same(lab, down)[0].tolist() == [[0, 3, 3, 5, 255, 2, 9, 1]]
    hole = ident.copy()
    hole[3], hole[5], hole[9] = 5, -1, -1             # -1 at the end of a chain and on a raw value
    out, bad = _same(lab, hole)
    assert out.tolist() == [[0, 5, 5, 5, 255, 7, 9, 2]] and bad.tolist() == [[False, True, True, True, False, False, True, False]]
    to_ignore = ident.copy()
    to_ignore[2], to_ignore[3] = 255, 0               # onto 255 and 0: never moved again
    assert _same(lab, to_ignore)[0].tolist() == [[0, 0, 0, 5, 255, 7, 9, 255]]
    assert _same(lab, ident)[0].tolist() == lab.tolist()


def test_closed_form_equals_the_loop_exhaustively():
    """Raw values 1 .. 4 in every combination of presence (beside 0 and 255), remap[1 .. 3] over {-1, 0, 1, 2, 3, 4, 255} each and
    remap[4] over {-1, 2, 4, 255}: 343 * 4 tables x 16 images."""
    images = []
    for keep in itertools.product([False, True], repeat=4):
        vals = [0, 255] + [v for v, k in zip((1, 2, 3, 4), keep) if k]
        images.append(np.array([vals + vals[::-1]], dtype=np.int64))
    n = 0
    for t1, t2, t3 in itertools.product([-1, 0, 1, 2, 3, 4, 255], repeat=3):
        for t4 in (-1, 2, 4, 255):
            remap = np.arange(256, dtype=np.int32)
            remap[1:5] = (t1, t2, t3, t4)
            for lab in images:
                _same(lab, remap)
                n += 1
    assert n == 343 * 4 * 16


# ---- the public entry ------------------------------------------------------------------------------------------------------------
def test_label_stage_fails_loudly():
    from cavp_amd._lib import CavpError
    from cavp_amd.labels import LabelStage
    st = LabelStage(num_classes=6, max_batch=4)
    lab = torch.zeros(2, 5, 7, dtype=torch.int64)
    with pytest.raises(CavpError, match="CPU tensor"):
        st(lab)
    with pytest.raises(CavpError, match="int64 or uint8"):
        st(lab.int())
    with pytest.raises(CavpError, match="max_batch"):
        st(torch.zeros(5, 5, 7, dtype=torch.int64))
    with pytest.raises(CavpError, match="empty"):
        st(torch.zeros(2, 0, 7, dtype=torch.int64))
    with pytest.raises(CavpError):
        st.check()
    with pytest.raises(CavpError):
        LabelStage(num_classes=257)
    with pytest.raises(CavpError):
        LabelStage(num_classes=3, mode="any_foreground")
    with pytest.raises(CavpError):
        LabelStage(num_classes=3, mode="one_hot")
    with pytest.raises(CavpError, match="256"):
        LabelStage(num_classes=3, remap=np.zeros(255, dtype=np.int32))
    with pytest.raises(CavpError, match=r"\[-1, 255\]"):
        LabelStage(num_classes=3, remap=np.full(256, 256, dtype=np.int32))
    assert LabelStage(num_classes=3, remap=torch.arange(256, dtype=torch.int32)).remap_host.dtype == np.int32
