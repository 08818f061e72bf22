#!/usr/bin/env python3
"""Generate tests/golden/pairs.npz by running the REFERENCE's pair-building code (read-only import, the recipe of
tools/make_golden.py: stub packages in tools/_shims, the reference tree on sys.path).

Authoring-container only; nothing here is imported by the product or the tests.  What runs is the reference's own
`models.cavp_model.SoundBank` and its own `CAVP_TRAINER.overwrite_miss_match` (called unbound on a SimpleNamespace that carries
ow_rate).  The trainer module imports packages that are not installed here and that the two functions never touch
(torchaudio, wandb, cv2, loguru, visualisation.tsne, ...): those that cannot be imported get an empty stand-in module in
sys.modules before the import.  The statements of the training loop between them (trainer_cavp_vpo_mono.py:148-181: permute,
compare, concatenate, rewrite the pixel labels) are no function that could be called; drive() below makes the same calls in the
same order on the same tensors.

8 consecutive steps at B = 8, K = 6, S = 4, A = 64, H = W = 8, ow_rate = 0.5, overwrite from step 1 on.  The file is written
only if the run shows (a) an all-zero slot 0 handed out before a class has S pushes, (b) a ring wrap (a class pushed more than
S times), (c) a step in which an overwritten row's class is also pushed while its slot 0 holds a real clip.

usage: python tools/make_pairs_golden.py [--out tests/golden] [--seed N]
"""
import argparse
import importlib
import os
import sys
import types

sys.dont_write_bytecode = True
HERE = os.path.dirname(os.path.abspath(__file__))
REPO = os.path.dirname(HERE)
sys.path[:0] = [os.path.join(HERE, "_shims"), "/root/reference", REPO]

import numpy as np  # noqa: E402
import torch  # noqa: E402

B, K, S, A, H, W, OW_RATE, STEPS = 8, 6, 4, 64, 8, 8, 0.5, 8


class _Anything:
    """Attribute of a stand-in module: callable, subscriptable, and every attribute of it is another one."""

    def __call__(self, *a, **k):
        return self

    def __getattr__(self, name):
        return self


def _stand_in(name):
    m = types.ModuleType(name)
    m.__path__ = []
    m.__getattr__ = lambda attr: _Anything()
    sys.modules[name] = m


def import_reference():
    for name in ("torchaudio", "torchaudio.transforms", "wandb", "cv2", "loguru", "visualisation", "visualisation.tsne", "tqdm",
                 "einops", "matplotlib", "matplotlib.pyplot", "PIL", "PIL.Image"):
        try:
            importlib.import_module(name)
        except Exception:
            _stand_in(name)
    import models.visual.backbones.resnet as _R
    _R.load_model = lambda model, f, is_restore=False: model
    from models.cavp_model import SoundBank
    for _ in range(32):        # submodules of the stand-ins (torchaudio.functional, ...) as the trainer's imports ask for them
        try:
            from trainer.trainer_cavp_vpo_mono import CAVP_TRAINER
            return SoundBank, CAVP_TRAINER
        except ModuleNotFoundError as e:
            top = (e.name or "").split(".")[0]
            if top not in sys.modules or not isinstance(getattr(sys.modules[top], "__getattr__", None), types.LambdaType):
                raise
            _stand_in(e.name)
    raise RuntimeError("the reference trainer module does not import")


def make_batch(g, step):
    """Rows mix single-source (classes 1..3, so that a FIFO of 4 wraps within the run), two-source and background-only."""
    img = torch.zeros((B, K), dtype=torch.long)
    for i in range(B):
        kind = float(torch.rand((), generator=g))
        img[i, 0] = int(torch.randint(0, 2, (), generator=g))
        if kind < 0.65:
            img[i, 1 + int(torch.randint(0, 3, (), generator=g))] = 1
        elif kind < 0.85:
            a = int(torch.randint(1, K, (), generator=g))
            b = 1 + (a + int(torch.randint(0, K - 2, (), generator=g))) % (K - 1)
            img[i, a] = img[i, b] = 1
        else:
            img[i, 0] = 1
    wav = torch.randint(1, 100, (B, 1, A), generator=g).float() + 100.0 * step      # never zero: an empty slot is recognisable
    pix = torch.randint(0, K, (B, H, W), generator=g)
    return wav, pix, img


def drive(seed):
    SoundBank, CAVP_TRAINER = import_reference()
    args = types.SimpleNamespace(num_classes=K, batch_size=S)
    bank = SoundBank(out_dim=A, args=args, device="cpu")
    self_ = types.SimpleNamespace(ow_rate=OW_RATE)
    g = torch.Generator().manual_seed(seed)
    rec = {k: [] for k in ("waveform", "pix_label", "img_label", "overwrite", "perm", "if_match_shuffle", "n_false", "ow_draw",
                           "if_match", "img_label_shuffle", "mod_idx_map", "shuffle_audio", "shuffle_pix_label", "bank")}
    pushes = np.zeros(K, dtype=np.int64)
    saw_zero_slot = saw_wrap = saw_hazard = False
    for step in range(STEPS):
        waveform, pix_label, img_label = make_batch(g, step)
        rec["waveform"].append(waveform.numpy().copy())
        rec["pix_label"].append(pix_label.numpy().copy())
        rec["img_label"].append(img_label.numpy().copy())
        overwrite = step >= 1
        torch.manual_seed(1000 * seed + step)
        shuffle_idx = torch.randperm(B)
        shuffle_img_label = img_label.clone()[shuffle_idx]
        shuffle_pix_label = pix_label.clone()[shuffle_idx]
        if_match = torch.all(torch.eq(img_label, shuffle_img_label), dim=1)
        shuffle_audio = waveform.clone()[shuffle_idx]
        if_match0 = if_match.numpy().copy()
        n_false = int((~if_match).sum())
        draw = np.full(B, -1, dtype=np.int64)
        mod = np.full(B, -1, dtype=np.int64)
        if overwrite:
            state = torch.get_rng_state()
            draw[:n_false] = torch.randperm(n_false).numpy()       # the draw overwrite_miss_match is about to make
            torch.set_rng_state(state)
            if_match, shuffle_img_label, mod_idx_map = CAVP_TRAINER.overwrite_miss_match(self_, if_match, shuffle_img_label, img_label)
            slot0 = bank.bank_vault[:, 0].clone()
            shuffle_audio = bank.overwrite_audio_feature(shuffle_audio, waveform, mod_idx_map)
            for i, c in mod_idx_map.items():
                mod[i] = c
                saw_zero_slot |= pushes[c] < S and not bool(slot0[c].any())
        single = [int(r[1:].nonzero()[0, 0]) + 1 if int(r[1:].sum()) == 1 else -1 for r in img_label]
        for c in set(int(c) for c in mod if c >= 0):
            saw_hazard |= c in single and pushes[c] >= S
        bank.update_bank(waveform, img_label)       # (zeroes img_label[:, 0] in place; the inputs were recorded above)
        for c in single:
            if c >= 0:
                pushes[c] += 1
        saw_wrap |= bool((pushes > S).any())
        shuffle_pix_label[~if_match] = 0
        shuffle_pix_label[if_match] = pix_label[if_match]
        rec["overwrite"].append(np.array(overwrite))
        rec["perm"].append(shuffle_idx.numpy().astype(np.int32))
        rec["if_match_shuffle"].append(if_match0)
        rec["n_false"].append(np.array(n_false, dtype=np.int32))
        rec["ow_draw"].append(draw.astype(np.int32))
        rec["if_match"].append(if_match.numpy().copy())
        rec["img_label_shuffle"].append(shuffle_img_label.numpy().copy())
        rec["mod_idx_map"].append(mod.astype(np.int32))
        rec["shuffle_audio"].append(shuffle_audio.numpy().copy())
        rec["shuffle_pix_label"].append(shuffle_pix_label.numpy().copy())
        rec["bank"].append(bank.bank_vault.numpy().copy())
    return {k: np.stack(v) for k, v in rec.items()}, (saw_zero_slot, saw_wrap, saw_hazard)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(REPO, "tests", "golden"))
    ap.add_argument("--seed", type=int, default=0)
    a = ap.parse_args()
    rec, (zero_slot, wrap, hazard) = drive(a.seed)
    print(f"seed {a.seed}: zero slot handed out {zero_slot}, ring wrap {wrap}, ordering hazard {hazard}; "
          f"overwritten rows per step {[int((m >= 0).sum()) for m in rec['mod_idx_map']]}")
    if not (zero_slot and wrap and hazard):
        sys.exit("the run does not show all three cases: fixture NOT written (try another --seed)")
    rec["config"] = np.array([B, K, S, A, H, W, STEPS], dtype=np.int32)
    rec["ow_rate"] = np.array(OW_RATE)
    path = os.path.join(a.out, "pairs.npz")
    np.savez_compressed(path, **rec)
    print(f"wrote {path}: {os.path.getsize(path)} bytes")


if __name__ == "__main__":
    main()
