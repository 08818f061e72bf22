"""numpy restatement of the device store's specification (include/cavp_hip.h, "device store") - TEST INFRASTRUCTURE.

Written from the specification, not from the kernels: plain Python integers, a list of items, slices.
  * rank and epoch: M = ceil(N / world) items per rank, spe = M // B steps per epoch (drop_last); step t has epoch e = t // spe, row
    i the rank-local position j = (t % spe) * B + i and the global position q = j * world + rank, q - N when q >= N
    (DistributedSampler's wrap-around padding); the item is pi_e(q);
  * pi_e: a balanced Feistel network on 2k bits, bits = max(2, bit_length(N - 1)), k = ceil(bits / 2), x = (L << k) | R, 8 rounds
    (L, R) <- (R, L ^ (f & (2^k - 1))), f = the first output word of Philox4x32-10 at counter (R, r, e_lo, e_hi) under the key
    (seed_lo, seed_hi); the whole cipher is applied again until x < N;
  * index= replaces the draw, an entry outside [0, N) is counted and replaced by 0; every feed advances t;
  * the gather writes the item's h x w window (top-left of its staging slot), each present channel up to its length, and the
    tables; for the source rows >= n_src only length = 0 and n_ch = 0.  Nothing else is written.
"""
import numpy as np

M0, M1, W0, W1 = 0xD2511F53, 0xCD9E8D57, 0x9E3779B9, 0xBB67AE85
MASK32 = 0xFFFFFFFF
ROUNDS = 8


def philox_word0(c0: int, c1: int, c2: int, c3: int, k0: int, k1: int) -> int:
    """The first output word of Philox4x32-10 (Salmon et al., SC'11)."""
    for _ in range(10):
        p0, p1 = M0 * c0, M1 * c2
        c0, c1, c2, c3 = ((p1 >> 32) ^ c1 ^ k0) & MASK32, p1 & MASK32, ((p0 >> 32) ^ c3 ^ k1) & MASK32, p0 & MASK32
        k0, k1 = (k0 + W0) & MASK32, (k1 + W1) & MASK32
    return c0


def half_bits(N: int) -> int:
    bits = max(2, (N - 1).bit_length())
    return (bits + 1) // 2


def permute(x: int, N: int, seed: int, epoch: int) -> int:
    """pi_e(x) for 0 <= x < N."""
    k = half_bits(N)
    mask = (1 << k) - 1
    seed &= 0xFFFFFFFFFFFFFFFF
    k0, k1, e0, e1 = seed & MASK32, seed >> 32, epoch & MASK32, (epoch >> 32) & MASK32
    while True:
        L, R = x >> k, x & mask
        for r in range(ROUNDS):
            L, R = R, L ^ (philox_word0(R, r, e0, e1, k0, k1) & mask)
        x = (L << k) | R
        if x < N:
            return x


def permute_many(x, N: int, seed: int, epoch) -> np.ndarray:
    """permute() over arrays of positions and epochs (broadcast together), in uint64 numpy arithmetic: for the statistics over
    thousands of epochs.  tests/test_store_host.py holds it equal to permute()."""
    x, epoch = np.broadcast_arrays(np.asarray(x, dtype=np.uint64), np.asarray(epoch, dtype=np.uint64))
    x, epoch = x.copy().reshape(-1), epoch.reshape(-1)
    k = np.uint64(half_bits(N))
    mask, m32, s32 = np.uint64((1 << int(k)) - 1), np.uint64(MASK32), np.uint64(32)
    seed &= 0xFFFFFFFFFFFFFFFF
    todo = np.ones(x.shape, dtype=bool)
    while todo.any():
        cur = x[todo]
        L, R = cur >> k, cur & mask
        e0, e1 = epoch[todo] & m32, epoch[todo] >> s32
        for r in range(ROUNDS):
            c0, c1, c2, c3 = R.copy(), np.full_like(R, r), e0.copy(), e1.copy()
            k0, k1 = seed & MASK32, seed >> 32
            for _ in range(10):
                p0, p1 = np.uint64(M0) * c0, np.uint64(M1) * c2
                c0, c1, c2, c3 = ((p1 >> s32) ^ c1 ^ np.uint64(k0)) & m32, p1 & m32, ((p0 >> s32) ^ c3 ^ np.uint64(k1)) & m32, p0 & m32
                k0, k1 = (k0 + W0) & MASK32, (k1 + W1) & MASK32
            L, R = R, L ^ (c0 & mask)
        x[todo] = (L << k) | R
        todo &= x >= np.uint64(N)
    return x.astype(np.int64)


def steps_per_epoch(N: int, B: int, world: int = 1) -> int:
    return -(-N // world) // B


def batch_indices(N: int, B: int, seed: int, t: int, rank: int = 0, world: int = 1) -> np.ndarray:
    """The B items of step t."""
    spe = steps_per_epoch(N, B, world)
    assert spe >= 1
    e = t // spe
    out = np.empty(B, dtype=np.int32)
    for i in range(B):
        q = ((t % spe) * B + i) * world + rank
        if q >= N:
            q -= N
        out[i] = permute(q, N, seed, e)
    return out


def epoch_indices(N: int, B: int, seed: int, epoch: int, rank: int = 0, world: int = 1) -> np.ndarray:
    """Everything one rank sees in one epoch, in order."""
    spe = steps_per_epoch(N, B, world)
    return np.concatenate([batch_indices(N, B, seed, epoch * spe + s, rank, world) for s in range(spe)])


class StoreRef:
    """items: [(frame u8 [h, w, 3], mask u8 [h, w], [(pcm [n_ch, len], rate_idx), ...])].  feed() writes INTO the buffers it is given
    (a dict with the FeedResult's fields as numpy arrays), so what was there before stays wherever the rules write nothing."""

    def __init__(self, items, B: int, seed: int = 0, rank: int = 0, world: int = 1):
        self.items, self.B, self.seed, self.rank, self.world = items, B, seed, rank, world
        self.t = 0
        self.bad = 0

    def feed(self, buf: dict, index=None) -> dict:
        N = len(self.items)
        if index is None:
            idx = batch_indices(N, self.B, self.seed, self.t, self.rank, self.world)
        else:
            idx = np.array(index, dtype=np.int32)
            wrong = (idx < 0) | (idx >= N)
            self.bad += int(wrong.sum())
            idx[wrong] = 0
        self.t += 1
        for b, it in enumerate(idx):
            frame, mask, srcs = self.items[int(it)]
            h, w = mask.shape
            buf["index"][b] = it
            buf["sizes"][b] = (h, w)
            buf["frames"][b, :h, :w] = frame
            buf["masks"][b, :h, :w] = mask
            S = buf["length"].shape[1]
            for s in range(S):
                if s < len(srcs):
                    pcm, rate = srcs[s]
                    buf["pcm"][b, s, :pcm.shape[0], :pcm.shape[1]] = pcm
                    buf["length"][b, s], buf["rate_idx"][b, s], buf["n_ch"][b, s] = pcm.shape[1], rate, pcm.shape[0]
                else:
                    buf["length"][b, s] = buf["n_ch"][b, s] = 0
        return buf
