"""numpy restatement of the label stage's specification (cavp_amd/labels.py, csrc/labels.hip): what the reference's
data sets compute from the mask after the transform.  The remap is the reference's loop itself (sequential, in place, over the
value list taken before the loop); `remap_closed_form` is the per-pixel form the device uses, held to the loop by
tests/test_labels_host.py.  "bad" counts the pixels where the reference would raise (no remap entry; a value that is no class)."""
import numpy as np


def remap_loop(label, remap, ignore_index=255):
    """-> (remapped copy, bad pixels).  remap: int [256], -1 = the reference raises here: those pixels keep their value."""
    out = np.array(label, dtype=np.int64, copy=True)
    bad = np.zeros(out.shape, dtype=bool)
    values = [int(v) for v in np.unique(out) if v != 0 and v != ignore_index]      # the list is taken BEFORE the loop
    for i in values:
        hit = out == i
        if not 0 <= i <= 255 or not 0 <= int(remap[i]) <= 255:
            bad |= hit
            continue
        out[hit] = int(remap[i])
    return out, bad


def remap_closed_form(label, remap, ignore_index=255):
    """The same per pixel, from the presence mask of the raw image: x = v; t = remap[x]; while t > x, t was present and is neither
    0 nor ignore_index: x = t, t = remap[x]; the result is t."""
    lab = np.asarray(label, dtype=np.int64)
    present = set(int(v) for v in np.unique(lab))
    out = lab.copy()
    bad = np.zeros(lab.shape, dtype=bool)
    for idx in np.ndindex(lab.shape):
        v = int(lab[idx])
        if v == 0 or v == ignore_index:
            continue
        if not 0 <= v <= 255:
            bad[idx] = True
            continue
        x = v
        while True:
            t = int(remap[x])
            if not 0 <= t <= 255:
                bad[idx], out[idx] = True, x
                break
            out[idx] = t
            if t > x and t in present and t != 0 and t != ignore_index:
                x = t
            else:
                break
    return out, bad


def class_vector(label, K, mode="multi_hot", ignore_index=255):
    """-> (int64 [K], bad pixels) of ONE image (any shape, may be empty)."""
    lab = np.asarray(label, dtype=np.int64)
    vec = np.zeros(K, dtype=np.int64)
    if mode == "any_foreground":
        assert K == 2
        vec[1 if (lab != 0).any() else 0] = 1
        return vec, np.zeros(lab.shape, dtype=bool)
    keep = lab != ignore_index
    bad = keep & ((lab < 0) | (lab >= K))
    vec[np.unique(lab[keep & ~bad])] = 1
    return vec, bad


def collapse(label, ignore_index=255):
    out = np.array(label, dtype=np.int64, copy=True)
    out[(out != ignore_index) & (out != 0)] = 1
    return out


def label_stage(label, K, mode="multi_hot", remap=None, binary=False, ignore_index=255):
    """label [B, H, W] (any integer dtype) -> {"img_label" [B, K] i64, "label" [B, H, W] i64, "bad" int}: remap, class vector,
    collapse, in the reference's order; a pixel that is bad by several rules counts once."""
    lab = np.asarray(label).astype(np.int64)
    img = np.zeros((lab.shape[0], K), dtype=np.int64)
    out = lab.copy()
    n_bad = 0
    for b in range(lab.shape[0]):
        cur, bad = lab[b], np.zeros(lab[b].shape, dtype=bool)
        if remap is not None:
            cur, bad = remap_loop(cur, remap, ignore_index)
        img[b], bad2 = class_vector(cur, K, mode, ignore_index)
        if binary:
            cur = collapse(cur, ignore_index)
        out[b] = cur
        n_bad += int((bad | bad2).sum())
    return {"img_label": img, "label": out, "bad": n_bad}
