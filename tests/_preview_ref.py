"""Numpy restatement of the preview stage's specification (cavp_amd/preview.py, csrc/preview.hip, include/cavp_hip.h "preview
stage"): the three pictures per frame of the reference's Tensorboard.upload_wandb_image (utils/tensor_board.py:90-139), as bytes.
tests/test_preview_host.py holds it to tests/golden/preview.npz, which the reference's own functions wrote.

x        v = t * f32(std); v = v + f32(mean); u = v * 255: three float32 operations, each rounded (DeNormalize's t.mul_(s).add_(m),
         ToPILImage's pic.mul(255).byte()); the byte is u truncated toward zero, mod 256.  A non-finite u or |u| >= 2^31: 0, bad.
y        the label mod 256 (mask.astype(numpy.uint8)).
y_tilde  argmax over C (first maximal index, a NaN counts as the maximum), or the mask byte; 255 where the RAW label == ignore.
palette  colorize_mask(get_pallete(K)): the colour-map bits of j < K (K == 2: black, white), zeros beyond, the last entry white.
resize   Image.resize(NEAREST) = a gather through tests/_augment_ref.nearest_index, rows then columns."""
import numpy as np

from tests._augment_ref import nearest_index


def palette(K):
    pal = np.zeros((256, 3), dtype=np.int64)
    if K == 2:
        pal[1] = 255
    else:
        for j in range(K):
            lab, i = j, 0
            while lab:
                for c in range(3):
                    pal[j, c] |= ((lab >> c) & 1) << (7 - i)
                i, lab = i + 1, lab >> 3
    pal[255] = 255
    return pal.ravel().tolist()


def x_panel(image, mean, std):
    """image f32 [B, 3, H, W] -> (uint8 [B, H, W, 3], number of bad values)."""
    t = np.asarray(image, dtype=np.float32)
    s = np.asarray(std, dtype=np.float32).reshape(1, 3, 1, 1)
    m = np.asarray(mean, dtype=np.float32).reshape(1, 3, 1, 1)
    with np.errstate(all="ignore"):
        v = (t * s).astype(np.float32)
        v = (v + m).astype(np.float32)
        u = (v * np.float32(255)).astype(np.float32)
        bad = ~(np.abs(u) < np.float32(2147483648.0))
        byte = (np.trunc(np.where(bad, np.float32(0), u)).astype(np.int64) & 255).astype(np.uint8)
    return np.ascontiguousarray(byte.transpose(0, 2, 3, 1)), int(bad.sum())


def y_panel(labels):
    lab = np.asarray(labels)
    return (lab.reshape((lab.shape[0],) + lab.shape[-2:]).astype(np.int64) & 255).astype(np.uint8)


def argmax_first(logits):
    """np.argmax takes the first maximum and treats a NaN as the maximum, as torch.argmax does."""
    return np.argmax(np.asarray(logits, dtype=np.float32), axis=1).astype(np.uint8)


def y_tilde_panel(pred, labels, ignore=255):
    """pred: uint8 [B, H, W] class indices (argmax_first of the logits, or the mask)."""
    p = np.array(pred, dtype=np.uint8)
    if labels is not None:
        lab = np.asarray(labels)
        p[lab.reshape(p.shape).astype(np.int64) == ignore] = 255
    return p


def resize(panel, size):
    """panel [B, H, W(, 3)] -> [B, size[0], size[1](, 3)]."""
    return np.ascontiguousarray(panel[:, nearest_index(panel.shape[1], size[0])][:, :, nearest_index(panel.shape[2], size[1])])


def fixture_logits(K, hw, B=3):
    """The logits of a fixture case, float32 [B, K, H, W]: int8 values in [-4, 4] over 8 (many exact ties), a clear maximum at a
    random class on ~60 % of the pixels, one NaN.  Regenerated from a seed instead of stored (K = 256 alone would outgrow the
    fixture): RandomState's streams are frozen by numpy's compatibility policy, and the fixture keeps a CRC of every array."""
    rs = np.random.RandomState(1000 * K + hw[0])
    q = rs.randint(-4, 5, size=(B, K) + tuple(hw)).astype(np.int8)
    top = rs.randint(0, K, size=(B,) + tuple(hw))
    b, y, x = np.nonzero(rs.rand(B, *hw) < 0.6)
    q[b, top[b, y, x], y, x] = 5
    lg = q.astype(np.float32) / np.float32(8)
    lg[0, K // 2, 1, 2] = np.nan
    return lg


def preview(image, labels, *, logits=None, mask=None, mean, std, ignore=255, size=None):
    """{"x", "y", "y_tilde", "bad"}; x / y are None when image / labels are."""
    pred = argmax_first(logits) if logits is not None else np.asarray(mask, dtype=np.uint8)
    x, bad = x_panel(image, mean, std) if image is not None else (None, 0)
    out = {"x": x, "y": y_panel(labels) if labels is not None else None, "y_tilde": y_tilde_panel(pred, labels, ignore), "bad": bad}
    if size is not None:
        for k in ("x", "y", "y_tilde"):
            if out[k] is not None:
                out[k] = resize(out[k], size)
    return out
