"""numpy restatement of the device sampler's specification (include/cavp_hip.h, ABI 14) - TEST INFRASTRUCTURE.

Written from the specification, not from the kernels:
  * pixel i = b*hw + p of the reduced [B, hw] label map has three 64-bit keys, key(stream, i) = (r0 << 32) | r1 with
    r = Philox4x32-10(counter = (i, stream, offset_lo, offset_hi), key = (seed_lo, seed_hi)); stream 0 = per-class pick,
    1 = background, 2 = shuffle candidates;
  * "pick q of group G" = the q members of G with the smallest (key, i), in ascending (key, i);
  * rows: every foreground class c (c > 0, c != ignore) in ascending order with at least max_views pixels (the lowest
    max_classes of them) picks max_views (stream 0, label c); then sample_num = min(max_views, n_fg, n_bg) background pixels
    (stream 1, label 0); then sample_num of ALL match-foreground pixels (stream 2, label gt_shuffle there).
    n_match = n - sample_num; no class qualifies -> n = 0.
"""
import numpy as np

_M0, _M1 = np.uint64(0xD2511F53), np.uint64(0xCD9E8D57)
_W0, _W1 = 0x9E3779B9, 0xBB67AE85
_LO = np.uint64(0xFFFFFFFF)
_S32 = np.uint64(32)


def philox4x32_10(c0, c1, c2, c3, k0, k1):
    """Philox4x32-10 (Salmon et al., SC'11) on arrays of 32-bit words held in uint64.  Returns the four output words."""
    c0, c1, c2, c3 = (np.asarray(c, dtype=np.uint64) & _LO for c in (c0, c1, c2, c3))
    k0, k1 = int(k0) & 0xFFFFFFFF, int(k1) & 0xFFFFFFFF
    for _ in range(10):
        p0, p1 = _M0 * c0, _M1 * c2                      # 32 x 32 -> 64 bits: no overflow in uint64
        c0, c1, c2, c3 = (p1 >> _S32) ^ c1 ^ np.uint64(k0), p1 & _LO, (p0 >> _S32) ^ c3 ^ np.uint64(k1), p0 & _LO
        k0, k1 = (k0 + _W0) & 0xFFFFFFFF, (k1 + _W1) & 0xFFFFFFFF
    return c0, c1, c2, c3


def keys(stream: int, idx: np.ndarray, seed: int, offset: int) -> np.ndarray:
    seed, offset = int(seed) & 0xFFFFFFFFFFFFFFFF, int(offset) & 0xFFFFFFFFFFFFFFFF
    z = np.zeros(idx.shape, dtype=np.uint64)
    r0, r1, _, _ = philox4x32_10(idx.astype(np.uint64), z + np.uint64(stream), z + np.uint64(offset & 0xFFFFFFFF),
                                 z + np.uint64(offset >> 32), seed & 0xFFFFFFFF, seed >> 32)
    return (r0 << _S32) | r1


def pick(stream: int, members: np.ndarray, q: int, seed: int, offset: int) -> np.ndarray:
    """The q members (flat pixel indices) with the smallest (key, i), ascending."""
    k = keys(stream, members, seed, offset)
    order = np.lexsort((members, k))            # primary key k, ties by i
    return members[order[:q]]


def plan(gt_match: np.ndarray, gt_shuffle: np.ndarray, ignore_idx: int, max_views: int, max_classes: int, seed: int,
         offset: int) -> dict:
    """[B, hw] reduced label maps -> header {n, n_match, k_eligible, sample_num}, idx_b, idx_p, labels (n rows each) and the
    number of qualifying classes beyond max_classes."""
    B, HW = gt_match.shape
    gm, gs = gt_match.reshape(-1).astype(np.int64), gt_shuffle.reshape(-1).astype(np.int64)
    fg = np.flatnonzero((gm > 0) & (gm != ignore_idx))
    classes = [int(c) for c in np.unique(gm[fg]) if int((gm == c).sum()) >= max_views]
    dropped = max(0, len(classes) - max_classes)
    classes = classes[:max_classes]
    empty = np.zeros(0, dtype=np.int32)
    if not classes:
        return {"header": np.array([0, 0, 0, 0], dtype=np.int32), "idx_b": empty, "idx_p": empty, "labels": empty,
                "dropped": dropped}
    idx, lab = [], []
    for c in classes:
        idx.append(pick(0, np.flatnonzero(gm == c), max_views, seed, offset))
        lab.append(np.full(max_views, c, dtype=np.int64))
    bg = np.flatnonzero(gm == 0)
    sample_num = int(min(max_views, fg.shape[0], bg.shape[0]))
    idx.append(pick(1, bg, sample_num, seed, offset))
    lab.append(np.zeros(sample_num, dtype=np.int64))
    sh = pick(2, fg, sample_num, seed, offset)
    idx.append(sh)
    lab.append(gs[sh])
    idx, lab = np.concatenate(idx), np.concatenate(lab)
    n = idx.shape[0]
    b, p = np.divmod(idx, HW)
    return {"header": np.array([n, n - sample_num, len(classes), sample_num], dtype=np.int32), "idx_b": b.astype(np.int32),
            "idx_p": p.astype(np.int32), "labels": lab.astype(np.int32), "dropped": dropped}
