"""numpy restatement of the device DropPath draw's specification (include/cavp_hip.h, cavp_drop_path_draw) - TEST
INFRASTRUCTURE.

Written from the specification, not from the kernel:
  * r = Philox4x32-10 (Salmon et al., SC'11) at counter = (sample b, branch row k, offset_lo, offset_hi) under the key
    (seed_lo, seed_hi), seed and offset taken as 64-bit two's complement;
  * u = (r[0] >> 8) * 2^-24 as a float32 (exact: 24 bits), in [0, 1);
  * out[k, b] = inv_keep[k] if float32(keep[k] + u) >= 1 else 0 - timm 0.4.9's floor(keep + rand) / keep for 0 < keep <= 1.
"""
import numpy as np

M0, M1, W0, W1 = 0xD2511F53, 0xCD9E8D57, 0x9E3779B9, 0xBB67AE85
MASK32 = 0xFFFFFFFF


def philox_word0(c0: int, c1: int, c2: int, c3: int, k0: int, k1: int) -> int:
    """The first output word of Philox4x32-10, in plain Python integers."""
    for _ in range(10):
        p0, p1 = M0 * c0, M1 * c2
        c0, c1, c2, c3 = ((p1 >> 32) ^ c1 ^ k0) & MASK32, p1 & MASK32, ((p0 >> 32) ^ c3 ^ k1) & MASK32, p0 & MASK32
        k0, k1 = (k0 + W0) & MASK32, (k1 + W1) & MASK32
    return c0


def philox_word0_many(c0, c1, c2: int, c3: int, k0: int, k1: int) -> np.ndarray:
    """philox_word0 over arrays c0, c1 (broadcast together) in uint64 numpy arithmetic; tests/test_droppath_host.py holds it equal
    to the scalar version."""
    c0, c1 = np.broadcast_arrays(np.asarray(c0, dtype=np.uint64), np.asarray(c1, dtype=np.uint64))
    c0, c1 = c0.copy(), c1.copy()
    c2, c3 = np.full_like(c0, c2), np.full_like(c0, c3)
    m32, s32 = np.uint64(MASK32), np.uint64(32)
    for _ in range(10):
        p0, p1 = np.uint64(M0) * c0, np.uint64(M1) * c2      # 32 x 32 bit products: no overflow of uint64
        c0, c1, c2, c3 = ((p1 >> s32) ^ c1 ^ np.uint64(k0)) & m32, p1 & m32, ((p0 >> s32) ^ c3 ^ np.uint64(k1)) & m32, p0 & m32
        k0, k1 = (k0 + W0) & MASK32, (k1 + W1) & MASK32
    return c0


def u01(word) -> np.ndarray:
    """The top 24 bits of a 32-bit word as a float32 in [0, 1)."""
    return (np.asarray(word, dtype=np.uint64) >> np.uint64(8)).astype(np.float32) * np.float32(1.0 / 16777216.0)


def ref_scales(seed: int, offset: int, keep, inv_keep, B: int) -> np.ndarray:
    """float32 [n, B]: the factors of the n branches for the samples 0 .. B - 1 at this seed and offset."""
    keep, inv_keep = np.asarray(keep, dtype=np.float32).reshape(-1), np.asarray(inv_keep, dtype=np.float32).reshape(-1)
    n = keep.shape[0]
    seed, offset = int(seed) & 0xFFFFFFFFFFFFFFFF, int(offset) & 0xFFFFFFFFFFFFFFFF
    b, k = np.arange(B, dtype=np.uint64)[None, :], np.arange(n, dtype=np.uint64)[:, None]
    w = philox_word0_many(b, k, offset & MASK32, offset >> 32, seed & MASK32, seed >> 32)
    s = (keep[:, None] + u01(w)).astype(np.float32)        # the f32 sum, rounded once
    return np.where(s >= np.float32(1.0), inv_keep[:, None], np.float32(0.0)).astype(np.float32)


def keep_tables(probs):
    """(keep, inv_keep) as the host path computes them (pvt_train.draw_drop_path_scales): float32(1 - p), float32 ones / keep."""
    import torch
    keep = torch.tensor([1.0 - p for p in probs if p > 0], dtype=torch.float32)
    return keep.numpy().copy(), (torch.ones_like(keep) / keep).numpy().copy()
