"""numpy restatement of the pair builder's specification (include/cavp_hip.h, "pair builder") - TEST INFRASTRUCTURE.

Written from the specification, not from the kernels: the bank is a plain per-class FIFO here (slot 0 = oldest), no ring.
  * perm[j] = the row with the j-th smallest (key, i), key = Philox stream 0 at (seed, offset); offset counts the calls;
  * if_match[i] = all(img_label[i] == img_label[perm[i]]);
  * with overwrite: of the rows with if_match == 0 the q = int(n_false * ow_rate) with the smallest (rank, i) are picked
    (rank = Philox stream 1, or the caller's ow_rank); a picked row with exactly one non-zero non-background label c becomes a
    match, takes its own image labels and the clip in slot 0 of class c as it was BEFORE this step's pushes;
  * then, rows ascending, every row with exactly one non-zero non-background label pushes its clip at the end of that FIFO;
  * label_shuffle[i] = pix_label[i] where if_match[i], background (0) elsewhere.
"""
import numpy as np

from tests._contrast_sampler_ref import keys


def ow_table(max_batch: int, ow_rate: float) -> np.ndarray:
    return np.array([int(n * ow_rate) for n in range(max_batch + 1)], dtype=np.int32)


def draw_perm(B: int, seed: int, offset: int) -> np.ndarray:
    idx = np.arange(B)
    return idx[np.lexsort((idx, keys(0, idx, seed, offset)))].astype(np.int32)


def rank_from_draw(if_match0: np.ndarray, draw: np.ndarray) -> np.ndarray:
    """The reference's `false_list[randperm(n_false)[:q]]` as per-row ranks: rank[false_list[draw[j]]] = j."""
    false_list = np.flatnonzero(np.asarray(if_match0) == 0)
    rank = np.zeros(len(if_match0), dtype=np.int32)
    rank[false_list[np.asarray(draw[:len(false_list)], dtype=np.int64)]] = np.arange(len(false_list), dtype=np.int32)
    return rank


class PairsRef:
    def __init__(self, num_classes: int, bank_slots: int, wave_len: int, ow_rate: float, seed: int = 0):
        self.K, self.S, self.A, self.ow_rate = num_classes, bank_slots, wave_len, ow_rate
        self.bank = np.zeros((num_classes, bank_slots, wave_len), dtype=np.float32)
        self.seed, self.offset = seed, 0

    def __call__(self, waveform, pix_label, img_label, overwrite, perm=None, ow_rank=None) -> dict:
        wav = np.asarray(waveform, dtype=np.float32).reshape(-1, self.A)
        pix, img = np.asarray(pix_label, dtype=np.int64), np.asarray(img_label, dtype=np.int64)
        B = wav.shape[0]
        rows = np.arange(B)
        perm = draw_perm(B, self.seed, self.offset) if perm is None else np.asarray(perm, dtype=np.int32)
        rank = keys(1, rows, self.seed, self.offset) if ow_rank is None else np.asarray(ow_rank).astype(np.uint64)
        self.offset += 1
        if_match = (img == img[perm]).all(axis=1)
        img_sh = img[perm].copy()
        source = perm.astype(np.int32).copy()
        shuffled = wav[perm].copy()
        nonzero = img[:, 1:] != 0
        single = np.where(nonzero.sum(axis=1) == 1, nonzero.argmax(axis=1) + 1, -1)
        false_list = np.flatnonzero(~if_match)
        n_false, q = len(false_list), 0
        if overwrite:
            q = int(n_false * self.ow_rate)
            picked = false_list[np.lexsort((false_list, rank[false_list]))][:q]
            for i in picked:
                if single[i] < 0:
                    continue
                if_match[i] = True
                img_sh[i] = img[i]
                source[i] = ~single[i]
                shuffled[i] = self.bank[single[i], 0]
        for i in rows:
            if single[i] >= 0:
                c = single[i]
                self.bank[c] = np.concatenate((self.bank[c, 1:], wav[i:i + 1]))
        label_shuffle = np.where(if_match[:, None, None], pix, 0)
        return {"waveforms": np.concatenate((wav, shuffled)).reshape(2 * B, 1, self.A), "label_shuffle": label_shuffle,
                "if_match": if_match.astype(np.uint8), "img_label_shuffle": img_sh, "perm": perm, "source": source,
                "n_false": n_false, "q": q}
