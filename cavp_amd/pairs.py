"""Mismatched audio-visual pairs on the GPU: the block in front of the model call of the reference trainers
(trainer/trainer_cavp_vpo_mono.py:87-115,148-181 with SoundBank, models/cavp_model.py:21-52) as four launches of
csrc/pairs.hip.  The batch is permuted, every row learns whether its shuffled clip still matches the frame, from epoch 1 on a
share `ow_rate` of the mismatched single-source rows is turned back into matches with the oldest clip of the right class from
a per-class FIFO, the FIFO takes this batch's single-source clips, and the shuffled pixel labels are written - with no host
value that depends on a device value, so the call can be captured in a hipGraph together with MelFrontEnd and the train step.

    pb = PairBuilder(num_classes=K, bank_slots=S, wave_len=A, ow_rate=r, seed=0, device=dev, max_batch=Bmax)
    out = pb(waveform, pix_label, img_label, overwrite=epoch >= 1)
    audio = mel(out.waveforms)                                   # [2B, 1, T, 64]
    loss = model.train_step(image, audio, pix_label, contrast=crit, label_shuffle=out.label_shuffle)

Opt-in and additive: `cavp_model.SoundBank` (the reference's host bookkeeping) is unchanged.  The rules are restated in
include/cavp_hip.h ("pair builder") and DESIGN.md 4n.

Randomness: the permutation and the overwrite pick are Philox4x32-10 draws in the device sampler's convention:
the same distributions as the reference's two torch.randperm calls, another stream - no seed reproduces torch.randperm's
values.  `perm=` / `ow_rank=` replace the draws (that is how the reference's own draws are replayed by the golden test)."""
from __future__ import annotations

import ctypes as C
from typing import Optional

import numpy as np
import torch

from . import _lib
from .ops import _ptr, _stream

MAX_BATCH, MAX_CLASSES = 1024, 256


def ow_table(max_batch: int, ow_rate: float) -> np.ndarray:
    """int(n * ow_rate) for n = 0 .. max_batch with Python's own float semantics: the device only looks the count up."""
    return np.array([int(n * ow_rate) for n in range(max_batch + 1)], dtype=np.int32)


class PairResult:
    """Outputs of one PairBuilder call, every field a device tensor:
    waveforms [2B, 1, A] f32 = cat(waveform, shuffled clips); label_shuffle [B, H, W] i64; if_match [B] u8; img_label_shuffle
    [B, K] i64; perm [B] i32; source [B] i32 (>= 0: row of `waveform`, < 0: ~class, taken from the bank).  `tables` holds the
    plan kernel's header | source table | write table (int32, see include/cavp_hip.h)."""
    __slots__ = ("waveforms", "label_shuffle", "if_match", "img_label_shuffle", "perm", "source", "tables")

    def __init__(self, B, A, K, hw, dev):
        self.waveforms = torch.empty((2 * B, 1, A), dtype=torch.float32, device=dev)
        self.label_shuffle = torch.empty((B,) + tuple(hw), dtype=torch.int64, device=dev)
        self.if_match = torch.empty(B, dtype=torch.uint8, device=dev)
        self.img_label_shuffle = torch.empty((B, K), dtype=torch.int64, device=dev)
        self.perm = torch.empty(B, dtype=torch.int32, device=dev)
        self.source = torch.empty(B, dtype=torch.int32, device=dev)
        self.tables = torch.empty(8 + 3 * B, dtype=torch.int32, device=dev)


class PairBuilder:
    """See the module docstring.  Limits: B <= max_batch <= 1024, num_classes <= 256, mono clips ([B, 1, A]; the stereo
    trainer's variant is out of scope).  Inputs must be contiguous device tensors and are never modified - the reference's
    SoundBank.update_bank zeroes `img_label[:, 0]` in place as a side effect; that is NOT reproduced.

    `img_label` must be multi-hot in {0, 1}: the host cannot look without a copy, so the plan kernel counts the entries outside
    (it treats them as "non-zero" and never reads out of bounds because of them) and last_plan() raises when there were any."""

    def __init__(self, num_classes: int, bank_slots: int, wave_len: int, ow_rate: float, seed: int = 0, device=None,
                 max_batch: int = 64):
        if not 1 <= int(num_classes) <= MAX_CLASSES:
            raise _lib.CavpError(f"PairBuilder: 1 <= num_classes <= {MAX_CLASSES}")
        if not 1 <= int(max_batch) <= MAX_BATCH:
            raise _lib.CavpError(f"PairBuilder: 1 <= max_batch <= {MAX_BATCH}")
        if int(bank_slots) < 1 or int(wave_len) < 1:
            raise _lib.CavpError("PairBuilder: bank_slots and wave_len must be positive")
        if not 0.0 <= float(ow_rate) <= 1.0:
            raise _lib.CavpError("PairBuilder: 0 <= ow_rate <= 1")
        self.K, self.S, self.A, self.max_batch = int(num_classes), int(bank_slots), int(wave_len), int(max_batch)
        self.ow_rate = float(ow_rate)
        self.ow_table_host = ow_table(self.max_batch, self.ow_rate)
        self._device = device
        self._seed = int(seed)
        self._state = None       # device buffers, allocated by the first call (the constructor touches no device)
        self._last = None

    # ---- device state ------------------------------------------------------------------------------------------------------
    def _ensure(self):
        if self._state is None:
            dev = torch.device(self._device) if self._device is not None else torch.device("cuda", torch.cuda.current_device())
            if dev.type != "cuda":
                raise _lib.CavpError("PairBuilder lives on a HIP device (there is no CPU fallback)")
            self.device = dev
            self._bank = torch.zeros((self.K, self.S, self.A), dtype=torch.float32, device=dev)      # physical ring order
            self._head = torch.zeros(self.K, dtype=torch.int32, device=dev)
            self._table = torch.from_numpy(self.ow_table_host).to(dev)
            self._state = torch.zeros(4, dtype=torch.int64, device=dev)       # {seed, offset, bad_inputs, reserved}
            self.manual_seed(self._seed)
        return self._state

    def manual_seed(self, seed: int) -> None:
        """Reset the seed and the call counter (offset 0).  A host-to-device write: not legal during a capture; graphs captured
        earlier see the new values on their next replay."""
        s = int(seed) & 0xFFFFFFFFFFFFFFFF
        self._seed = s - (1 << 64) if s >= (1 << 63) else s
        if self._state is not None:
            self._state[:2].copy_(torch.tensor([self._seed, 0], dtype=torch.int64))

    def rollback_ranges(self, bank: bool = True):
        """[(name, tensor, byte_offset, nbytes)]: the bytes a call mutates that are state - the sound bank (`bank=False` leaves it
        out), the ring heads and {seed, offset} of the state block.  `bad_inputs` is a diagnostic and is not named: a rolled-back
        call must not hide that its input was bad.  For cavp_amd.rollback.StepRollback.add()."""
        state = self._ensure()
        out = [("bank", self._bank, 0, self._bank.numel() * 4)] if bank else []
        return out + [("head", self._head, 0, self._head.numel() * 4), ("state", state, 0, 16)]

    @property
    def bank_vault(self) -> torch.Tensor:
        """[K, S, A] in the reference's logical order (slot 0 = oldest), materialised from the ring: for tests and checkpoints."""
        self._ensure()
        slot = (self._head.long()[:, None] + torch.arange(self.S, device=self.device)[None, :]) % self.S
        return self._bank.gather(1, slot[:, :, None].expand(-1, -1, self.A))

    def load_bank(self, t: torch.Tensor) -> None:
        """Set the bank from a [K, S, A] tensor in logical order (a SoundBank.bank_vault, a checkpoint)."""
        self._ensure()
        if tuple(t.shape) != (self.K, self.S, self.A):
            raise _lib.CavpError(f"load_bank: expected {(self.K, self.S, self.A)}, got {tuple(t.shape)}")
        self._bank.copy_(t.to(torch.float32))
        self._head.zero_()

    def last_plan(self) -> dict:
        """Synchronises and returns the host-side plan of the most recent call (of the captured call, after a replay): perm,
        if_match, source, n_false, q, n_overwritten, n_written, offset, seed, src_table, wr_table, head.  For tests and
        debugging.  Raises CavpError if an img_label entry outside {0, 1} or a `perm=` entry outside [0, B) was seen since the
        last check."""
        if self._state is None or self._last is None:
            raise _lib.CavpError("last_plan: no PairBuilder call yet")
        state = self._state.cpu()
        bad = int(state[2])
        if bad:
            self._state[2:3].zero_()
            raise _lib.CavpError(f"PairBuilder: {bad} input value(s) out of range (img_label outside {{0, 1}} or perm outside [0, B))")
        r = self._last
        tab = r.tables.cpu().numpy()
        B = r.perm.shape[0]
        return {"perm": r.perm.cpu().numpy(), "if_match": r.if_match.cpu().numpy(), "source": r.source.cpu().numpy(),
                "n_false": int(tab[0]), "q": int(tab[1]), "n_overwritten": int(tab[2]), "n_written": int(tab[3]),
                "offset": (int(tab[4]) & 0xFFFFFFFF) | ((int(tab[5]) & 0xFFFFFFFF) << 32),
                "seed": (int(tab[6]) & 0xFFFFFFFF) | ((int(tab[7]) & 0xFFFFFFFF) << 32),
                "src_table": tab[8:8 + 2 * B].copy(), "wr_table": tab[8 + 2 * B:8 + 3 * B].copy(), "head": self._head.cpu().numpy()}

    # ---- the call -----------------------------------------------------------------------------------------------------------
    def _check_inputs(self, waveform, pix_label, img_label, perm, ow_rank):
        if waveform.dim() != 3 or waveform.dtype != torch.float32:
            raise _lib.CavpError("PairBuilder: waveform must be float32 [B, 1, A]")
        B, Cw, A = waveform.shape
        if Cw != 1:
            raise _lib.CavpError(f"PairBuilder: mono clips only ([B, 1, A]), got {Cw} channels; the stereo trainer's variant is out of scope")
        if A != self.A:
            raise _lib.CavpError(f"PairBuilder: built for wave_len {self.A}, got {A}")
        if not 1 <= B <= self.max_batch:
            raise _lib.CavpError(f"PairBuilder: batch {B} outside [1, max_batch = {self.max_batch}]")
        if pix_label.dtype != torch.int64 or pix_label.dim() != 3 or pix_label.shape[0] != B:
            raise _lib.CavpError("PairBuilder: pix_label must be int64 [B, H, W]")
        if img_label.dtype != torch.int64 or tuple(img_label.shape) != (B, self.K):
            raise _lib.CavpError(f"PairBuilder: img_label must be int64 [B, {self.K}]")
        for name, t in (("perm", perm), ("ow_rank", ow_rank)):
            if t is not None and (t.dtype != torch.int32 or tuple(t.shape) != (B,)):
                raise _lib.CavpError(f"PairBuilder: {name} must be int32 [B]")
        for name, t in (("waveform", waveform), ("pix_label", pix_label), ("img_label", img_label), ("perm", perm), ("ow_rank", ow_rank)):
            if t is None:
                continue
            if not t.is_cuda:
                raise _lib.CavpError(f"PairBuilder: {name} is a CPU tensor; the pair builder needs HIP device tensors (no CPU fallback)")
            if not t.is_contiguous():
                raise _lib.CavpError(f"PairBuilder: {name} must be contiguous")
        return B

    def __call__(self, waveform: torch.Tensor, pix_label: torch.Tensor, img_label: torch.Tensor, overwrite: bool, *,
                 perm: Optional[torch.Tensor] = None, ow_rank: Optional[torch.Tensor] = None,
                 out: Optional[PairResult] = None) -> PairResult:
        """overwrite: the trainers' `epoch >= 1`, a host bool (a captured graph keeps the value it was captured with).
        out: a previous result of the same shapes whose buffers are written again (static addresses for a captured graph)."""
        B = self._check_inputs(waveform, pix_label, img_label, perm, ow_rank)
        state = self._ensure()
        dev = self.device
        if waveform.device != dev:
            raise _lib.CavpError(f"PairBuilder lives on {dev}, inputs on {waveform.device}")
        hw = tuple(pix_label.shape[1:])
        if out is None:
            out = PairResult(B, self.A, self.K, hw, dev)
        elif out.waveforms.shape != (2 * B, 1, self.A) or out.label_shuffle.shape != pix_label.shape or out.waveforms.device != dev:
            raise _lib.CavpError("PairBuilder: out= was made for other shapes")
        lib = _lib.load()
        st = C.c_void_p(_stream())
        header, src_table, wr_table = out.tables[:8], out.tables[8:8 + 2 * B], out.tables[8 + 2 * B:]
        K, S, A = self.K, self.S, self.A
        _lib.check(lib.cavp_pairs_plan(_ptr(img_label), B, K, S, _ptr(perm), _ptr(ow_rank), 1 if overwrite else 0,
                                       _ptr(self._table), self._table.numel(), _ptr(state), _ptr(self._head), _ptr(header),
                                       _ptr(out.perm), _ptr(out.if_match), _ptr(out.img_label_shuffle), _ptr(out.source),
                                       _ptr(src_table), _ptr(wr_table), st), "cavp_pairs_plan")
        # ORDER: the gather must be on the stream before the bank update.  An overwritten row reads logical slot 0 of its class
        # (physical slot `head`), which is exactly the slot the first push to that class in this step replaces; the stream
        # order between the two launches is what keeps the old clip readable.  One fused kernel would have no such order
        # between its workgroups.
        _lib.check(lib.cavp_pairs_gather(_ptr(waveform), _ptr(self._bank), _ptr(src_table), B, K, S, A, _ptr(out.waveforms), st),
                   "cavp_pairs_gather")
        _lib.check(lib.cavp_pairs_bank_update(_ptr(waveform), _ptr(wr_table), B, K, S, A, _ptr(self._bank), st),
                   "cavp_pairs_bank_update")
        _lib.check(lib.cavp_pairs_labels(_ptr(pix_label), _ptr(out.if_match), B, hw[0] * hw[1], _ptr(out.label_shuffle), st),
                   "cavp_pairs_labels")
        self._last = out
        return out
