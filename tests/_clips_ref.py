"""numpy restatement of the clip store's specification (include/cavp_hip.h, "clip store") - TEST INFRASTRUCTURE.

Written from the specification, not from the kernels: plain Python integers, a list of clips, slices.  The Philox word, the keyed
permutation and the clip rule of a training step are those of the device store and come from tests/_store_ref.py.
  * training, row i of step t: the clip is the device store's item (index= replaces it; an entry outside [0, N) is counted and
    becomes 0); the frame is frame=[i] (not a set bit of avail: counted, becomes the lowest set bit), else the r-th set bit of avail,
    r = (w * popcount(avail)) >> 32, w = word 0 of Philox4x32-10 at counter (i, 0xC11F, t_lo, t_hi) under the key (seed_lo, seed_hi);
    every feed advances the train counter and no other;
  * validation, row i of step t: P = ceil(ceil(N / world) / B), s = t mod P, q = (s * B + i) * world + rank; q < N: clip q with
    count = mask_num, index = q; q >= N: clip 0 with count = 0, index = -1; slot k < n_frames holds frame k (its mask only if it has
    one), the size of a slot >= n_frames is that of frame 0 and nothing is written there; every feed advances the eval counter and
    no other;
  * the gather writes windows (top-left of the slot), each present channel up to its length, and the tables; for the source rows >=
    n_src only length = 0 and n_ch = 0.  Nothing else is written.
"""
import numpy as np

from tests._store_ref import batch_indices, permute, philox_word0  # noqa: F401  (permute: re-exported for the tests)

MASK32 = 0xFFFFFFFF
DRAW_TAG = 0xC11F


def set_bits(avail: int) -> list:
    return [k for k in range(32) if (avail >> k) & 1]


def draw_frame(avail: int, seed: int, t: int, i: int) -> int:
    """The frame of row i at step t for a clip whose draw mask is `avail`."""
    bits = set_bits(avail)
    seed &= 0xFFFFFFFFFFFFFFFF
    w = philox_word0(i, DRAW_TAG, t & MASK32, (t >> 32) & MASK32, seed & MASK32, seed >> 32)
    return bits[(w * len(bits)) >> 32]


def steps_per_pass(N: int, B: int, world: int = 1) -> int:
    return -(-(-(-N // world)) // B)


def eval_rows(N: int, B: int, t: int, rank: int = 0, world: int = 1) -> list:
    """[(clip, padding)] of the B rows of eval step t."""
    s = t % steps_per_pass(N, B, world)
    rows = []
    for i in range(B):
        q = (s * B + i) * world + rank
        rows.append((q, False) if q < N else (0, True))
    return rows


class ClipsRef:
    """clips: [(frames [u8 [h, w, 3]], masks [u8 [h, w] or None, one per frame], [(pcm [n_ch, len], rate_idx), ...], avail, mask_num,
    tag)].  feed() / feed_clips() write INTO the buffers they are given (a dict with the result's fields as numpy arrays), so what
    was there before stays wherever the rules write nothing."""

    def __init__(self, clips, B: int, Tmax: int, seed: int = 0, rank: int = 0, world: int = 1):
        self.clips, self.B, self.Tmax, self.seed, self.rank, self.world = clips, B, Tmax, seed, rank, world
        self.t = 0
        self.t_eval = 0
        self.bad = 0

    def _sources(self, buf, b, srcs):
        for s in range(buf["length"].shape[1]):
            if s < len(srcs):
                pcm, rate = srcs[s]
                buf["pcm"][b, s, :pcm.shape[0], :pcm.shape[1]] = pcm
                buf["length"][b, s], buf["rate_idx"][b, s], buf["n_ch"][b, s] = pcm.shape[1], rate, pcm.shape[0]
            else:
                buf["length"][b, s] = buf["n_ch"][b, s] = 0

    def feed(self, buf: dict, index=None, frame=None) -> dict:
        N = len(self.clips)
        if index is None:
            idx = batch_indices(N, self.B, self.seed, self.t, self.rank, self.world)
        else:
            idx = np.array(index, dtype=np.int32)
            wrong = (idx < 0) | (idx >= N)
            self.bad += int(wrong.sum())
            idx[wrong] = 0
        for b, it in enumerate(idx):
            frames, masks, srcs, avail, _, tag = self.clips[int(it)]
            if frame is None:
                k = draw_frame(avail, self.seed, self.t, b)
            else:
                k = int(frame[b])
                if not (0 <= k < 32 and (avail >> k) & 1):
                    self.bad += 1
                    k = set_bits(avail)[0]
            h, w = masks[k].shape
            buf["index"][b], buf["select"][b], buf["tag"][b] = it, k, tag
            buf["sizes"][b] = (h, w)
            buf["frames"][b, :h, :w] = frames[k]
            buf["masks"][b, :h, :w] = masks[k]
            self._sources(buf, b, srcs)
        self.t += 1
        return buf

    def feed_clips(self, buf: dict) -> dict:
        T = self.Tmax
        for b, (clip, pad) in enumerate(eval_rows(len(self.clips), self.B, self.t_eval, self.rank, self.world)):
            frames, masks, srcs, _, mask_num, tag = self.clips[clip]
            buf["index"][b], buf["count"][b] = (-1, 0) if pad else (clip, mask_num)
            buf["n_frames"][b], buf["tag"][b] = len(frames), tag
            for k in range(T):
                if k >= len(frames):
                    buf["sizes"][b * T + k] = frames[0].shape[:2]
                    continue
                h, w = frames[k].shape[:2]
                buf["sizes"][b * T + k] = (h, w)
                buf["frames"][b, k, :h, :w] = frames[k]
                if masks[k] is not None:
                    buf["masks"][b, k, :h, :w] = masks[k]
            self._sources(buf, b, srcs)
        self.t_eval += 1
        return buf
