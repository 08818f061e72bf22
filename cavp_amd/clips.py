"""The device store for clip-shaped data sets (the reference's S4Dataset / MS3Dataset / AVSS VisualDataset: up to 10 frames and
masks, one waveform, two availability vectors per item): ClipStore holds the decoded clips, ClipFeeder draws clip AND frame on
the device and gathers only that frame (training), or walks the clips in order and gathers every frame (validation).  Two launches
of csrc/store.hip per feed, no host value that depends on a device value: both feeds are capturable.

    store = ClipStore(stage=(Hs, Ws), max_frames=T, max_sources=1, max_channels=Cm, max_len=Lmax, pcm_dtype=torch.int16, device=dev)
    for frames, masks, sources in decoded_clips:                # [uint8 [h, w, 3]] * n, [uint8 [h, w] or None], [(pcm, rate_idx)]
        store.append(frames, masks, sources, available=None, mask_num=None, tag=category)
    store.freeze()
    feeder = ClipFeeder(store, batch=B, seed=0, rank=rank, world=world)
    fed = feeder.feed(out=fed)                                  # ClipFeedResult: one frame per row
    aug(fed.frames, fed.masks, fed.sizes, out=augmented)
    wave(fed.pcm, fed.length, fed.rate_idx, fed.n_ch, select=fed.select, out=cut)        # WaveStage(segments=T)
    ev = feeder.feed_clips(out=ev)                              # ClipEvalResult: whole clips, in order
    a = aug.eval_(ev.frames.view(B * T, Hs, Ws, 3), ev.masks.view(B * T, Hs, Ws), ev.sizes)
    cv.update(model.predict(a.image, audio), a.label.view(B, T, H, W), ev.count)

Opt-in and additive.  The rules are restated in include/cavp_hip.h ("clip store"), tests/_clips_ref.py and DESIGN.md 4y.

Training: the clip of row i at step t is BatchFeeder's item rule unchanged (rank striding, DistributedSampler padding, drop_last, the
keyed permutation per epoch, `index=`).  The frame is the r-th set bit of the clip's `avail` mask, r = (w * popcount(avail)) >> 32
with w the first Philox4x32-10 word at counter (i, 0xC11F, t) under the feeder's seed: the reference's random.choice over
`(frame_available + mask_available) == 2` on another stream - the same distribution, no seed reproduces Python's values.
`frame=` replaces the draw.

Validation: P = ceil(ceil(N / world) / B) steps per pass; row i of step s is clip q = (s * B + i) * world + rank, a padding row
(count 0, index -1, fed with clip 0's bytes) when q >= N.  The train and the eval counter are separate words of the state block: a
validation pass in the middle of an epoch does not move the training stream."""
from __future__ import annotations

import ctypes as C
from typing import Optional, Sequence

import numpy as np
import torch

from . import _lib
from .ops import _ptr, _stream
from .store import MAX_BATCH, MAX_LEN, MAX_STAGE, _PCM, _as_numpy

MAX_FRAMES = 32
_FRAME_TABLES = ("frame_off", "mask_off", "size")
_CLIP_TABLES = ("first", "n_frames", "avail", "mask_num", "tag", "n_src", "pcm_off", "length", "rate_idx", "n_ch")


class ClipStore:
    """A frozen, device-resident set of ragged clips: the three byte arenas of DeviceStore (frames, masks, PCM; packed back to
    back, no padding), per-frame tables (frame_off, mask_off with -1 = no mask, size) and per-clip tables (first, n_frames, avail,
    mask_num, tag and the PCM tables).  Limits: max_frames <= 32, stage sides <= 16384, max_len <= 2^28, 2 * max_frames +
    max_sources * max_channels <= 65535, fewer than 2^31 frames.  The constructor and append() touch no device."""

    def __init__(self, stage, max_frames: int, max_sources: int, max_channels: int, max_len: int, pcm_dtype=torch.int16, device=None):
        E = _lib.CavpError
        if stage is None or len(tuple(stage)) != 2:
            raise E("ClipStore: stage=(Hs, Ws) is required")
        self.Hs, self.Ws = (int(v) for v in stage)
        if not (1 <= self.Hs <= MAX_STAGE and 1 <= self.Ws <= MAX_STAGE):
            raise E(f"ClipStore: stage sides must lie in [1, {MAX_STAGE}]")
        self.T = int(max_frames)
        if not 1 <= self.T <= MAX_FRAMES:
            raise E(f"ClipStore: 1 <= max_frames <= {MAX_FRAMES}")
        self.S, self.Cm, self.Lmax = int(max_sources), int(max_channels), int(max_len)
        if self.S < 1 or self.Cm < 1 or 2 * self.T + self.S * self.Cm > 65535:
            raise E("ClipStore: max_sources and max_channels must be positive, 2 * max_frames + max_sources * max_channels <= 65535")
        if not 1 <= self.Lmax <= MAX_LEN:
            raise E(f"ClipStore: 1 <= max_len <= {MAX_LEN}")
        if isinstance(pcm_dtype, str):
            pcm_dtype = getattr(torch, pcm_dtype, None)
        if pcm_dtype not in _PCM:
            raise E("ClipStore: pcm_dtype is torch.int16 or torch.float32")
        self.pcm_dtype = pcm_dtype
        self.elem = 2 if pcm_dtype == torch.int16 else 4
        self._device = device
        self._clips = []          # (frames, masks, [(pcm, rate_idx)], avail, mask_num, tag) until freeze()
        self._host = None
        self._dev = None
        self._n = 0
        self._n_frames = 0
        self._frozen = False

    def __len__(self) -> int:
        return self._n

    @property
    def frozen(self) -> bool:
        return self._frozen

    @property
    def total_frames(self) -> int:
        return self._n_frames

    # ---- filling -----------------------------------------------------------------------------------------------------------
    def append(self, frames: Sequence, masks: Sequence = (), sources: Sequence = (), available=None, mask_num=None, tag: int = 0) -> int:
        """One clip: frames = 1 .. max_frames arrays uint8 [h, w, 3] (each frame has its own size); masks = uint8 [h, w] per frame,
        shorter than frames or holding None where a frame has no mask; sources as DeviceStore.append.  available: the frames a
        training draw may take, a sequence of truth values (at most one per frame) or an int bit mask; default: every frame that has
        a mask.  mask_num: how many leading frames validation scores; default: the number of leading frames that have a mask.  The
        arrays are copied.  Returns the clip's index."""
        E = _lib.CavpError
        if self._frozen:
            raise E("ClipStore.append: the store is frozen")
        frames, masks = list(frames), list(masks)
        n = len(frames)
        if not 1 <= n <= self.T:
            raise E(f"ClipStore.append: {n} frames, 1 <= n_frames <= max_frames = {self.T}")
        if len(masks) > n:
            raise E(f"ClipStore.append: {len(masks)} masks for {n} frames")
        masks += [None] * (n - len(masks))
        kept_f, kept_m = [], []
        for k in range(n):
            frame = _as_numpy(frames[k], f"frame {k}")
            if frame.dtype != np.uint8 or frame.ndim != 3 or frame.shape[2] != 3:
                raise E(f"ClipStore.append: frame {k} must be uint8 [h, w, 3], got {frame.dtype} {tuple(frame.shape)}")
            h, w = frame.shape[:2]
            if not (1 <= h <= self.Hs and 1 <= w <= self.Ws):
                raise E(f"ClipStore.append: frame {k} of {h} x {w} does not fit the stage {self.Hs} x {self.Ws}")
            kept_f.append(np.array(frame, order="C"))
            if masks[k] is None:
                kept_m.append(None)
                continue
            mask = _as_numpy(masks[k], f"mask {k}")
            if mask.dtype != np.uint8 or tuple(mask.shape) != (h, w):
                raise E(f"ClipStore.append: mask {k} must be uint8 [{h}, {w}], got {mask.dtype} {tuple(mask.shape)}")
            kept_m.append(np.array(mask, order="C"))
        has_mask = sum(1 << k for k in range(n) if kept_m[k] is not None)
        leading = next((k for k in range(n) if kept_m[k] is None), n)
        if available is None:
            avail = has_mask
        elif isinstance(available, (int, np.integer)) and not isinstance(available, (bool, np.bool_)):
            avail = int(available)
            if avail < 0 or avail >> n:
                raise E(f"ClipStore.append: available = {avail:#x} names a frame outside the clip's {n}")
        else:
            bits = [bool(v) for v in np.asarray(available).reshape(-1)]
            if len(bits) > n:
                raise E(f"ClipStore.append: available has {len(bits)} entries for {n} frames")
            avail = sum(1 << k for k, v in enumerate(bits) if v)
        if avail == 0:
            raise E("ClipStore.append: available is empty (no frame has a mask, or none was named): a training draw has nothing to take")
        if avail & ~has_mask:
            raise E(f"ClipStore.append: available = {avail:#x} names a frame without a mask (frames with masks: {has_mask:#x})")
        if mask_num is None:
            mask_num = leading
        mask_num = int(mask_num)
        if not 0 <= mask_num <= leading:
            raise E(f"ClipStore.append: mask_num = {mask_num} exceeds the {leading} leading frames that have a mask")
        if not -(1 << 31) <= int(tag) < 1 << 31:
            raise E("ClipStore.append: tag must be an int32")
        sources = list(sources)
        if len(sources) > self.S:
            raise E(f"ClipStore.append: {len(sources)} sources, max_sources = {self.S}")
        kept = []
        want = _PCM[self.pcm_dtype]
        for src in sources:
            if not isinstance(src, (tuple, list)) or len(src) != 2:
                raise E("ClipStore.append: a source is (pcm [n_ch, len], rate_idx)")
            pcm, rate = _as_numpy(src[0], "pcm"), int(src[1])
            if pcm.dtype != want or pcm.ndim != 2:
                raise E(f"ClipStore.append: pcm must be {np.dtype(want).name} [n_ch, len], got {pcm.dtype} {tuple(pcm.shape)}")
            if not (1 <= pcm.shape[0] <= self.Cm and 1 <= pcm.shape[1] <= self.Lmax):
                raise E(f"ClipStore.append: pcm {tuple(pcm.shape)} outside [1 .. {self.Cm}, 1 .. {self.Lmax}]")
            if not 0 <= rate < 1 << 31:
                raise E("ClipStore.append: rate_idx must be a non-negative int32")
            kept.append((np.array(pcm, order="C"), rate))
        if self._n_frames + n >= 1 << 31:
            raise E("ClipStore.append: fewer than 2^31 frames")
        self._clips.append((kept_f, kept_m, kept, avail, mask_num, int(tag)))
        self._n += 1
        self._n_frames += n
        return self._n - 1

    def pack(self) -> dict:
        """The arenas and tables as numpy arrays (pure host arithmetic; what freeze() uploads)."""
        N, S, F = self._n, self.S, self._n_frames
        frame_off, mask_off, size = np.zeros(F, np.int64), np.full(F, -1, np.int64), np.zeros((F, 2), np.int32)
        first, n_frames, mask_num, tag, n_src = (np.zeros(N, np.int32) for _ in range(5))
        avail = np.zeros(N, np.uint32)
        pcm_off = np.zeros((N, S), np.int64)
        length, rate_idx, n_ch = (np.zeros((N, S), np.int32) for _ in range(3))
        fo = mo = po = f = 0
        fparts, mparts, pparts = [], [], []
        for i, (frames, masks, srcs, av, mn, tg) in enumerate(self._clips):
            first[i], n_frames[i], avail[i], mask_num[i], tag[i], n_src[i] = f, len(frames), av, mn, tg, len(srcs)
            for frame, mask in zip(frames, masks):
                frame_off[f], size[f] = fo, frame.shape[:2]
                fparts.append(frame.reshape(-1))
                fo += frame.size
                if mask is not None:
                    mask_off[f] = mo
                    mparts.append(mask.reshape(-1))
                    mo += mask.size
                f += 1
            for s, (pcm, rate) in enumerate(srcs):
                pcm_off[i, s], length[i, s], rate_idx[i, s], n_ch[i, s] = po, pcm.shape[1], rate, pcm.shape[0]
                pparts.append(pcm.reshape(-1).view(np.uint8))
                po += pcm.size * self.elem
        cat = lambda parts: np.concatenate(parts) if parts else np.zeros(0, np.uint8)
        return {"frames": cat(fparts), "masks": cat(mparts), "pcm": cat(pparts), "frame_off": frame_off, "mask_off": mask_off,
                "size": size, "first": first, "n_frames": n_frames, "avail": avail, "mask_num": mask_num, "tag": tag, "n_src": n_src,
                "pcm_off": pcm_off, "length": length, "rate_idx": rate_idx, "n_ch": n_ch}

    def freeze(self, upload: bool = True) -> "ClipStore":
        """Pack everything and upload it once; append() raises afterwards.  upload=False leaves the upload to the first feed (the
        packed host copy is dropped then)."""
        if self._frozen:
            raise _lib.CavpError("ClipStore.freeze: already frozen")
        if self._n == 0:
            raise _lib.CavpError("ClipStore.freeze: the store is empty")
        self._host = self.pack()
        self._clips = None
        self._frozen = True
        self._bytes = {k: int(v.nbytes) for k, v in self._host.items()}
        if upload:
            self._ensure()
        return self

    def _ensure(self) -> dict:
        if self._dev is None:
            if not self._frozen:
                raise _lib.CavpError("ClipStore: call freeze() first")
            dev = torch.device(self._device) if self._device is not None else torch.device("cuda", torch.cuda.current_device())
            if dev.type != "cuda":
                raise _lib.CavpError("ClipStore lives on a HIP device (there is no CPU fallback)")
            if dev.index is None:
                dev = torch.device("cuda", torch.cuda.current_device())
            self.device = dev
            # an arena nobody can read from still gets an address; uint32 travels as its int32 bit pattern
            def up(v):
                v = v if v.size else np.zeros(16, v.dtype)
                return torch.from_numpy(v.view(np.int32) if v.dtype == np.uint32 else v).to(dev)
            self._dev = {k: up(v) for k, v in self._host.items()}
            self._host = None
        return self._dev

    @property
    def nbytes(self) -> int:
        """Bytes resident after freeze(): the three arenas and the tables."""
        if not self._frozen:
            raise _lib.CavpError("ClipStore.nbytes: call freeze() first")
        return sum(self._bytes.values())

    def arena_bytes(self) -> dict:
        """{"frames", "masks", "pcm"}: the packed bytes per arena."""
        if not self._frozen:
            raise _lib.CavpError("ClipStore.arena_bytes: call freeze() first")
        return {k: self._bytes[k] for k in ("frames", "masks", "pcm")}

    def clip(self, i: int):
        """Host read-back of clip i: (frames, masks, [(pcm, rate_idx), ...], available, mask_num, tag) - numpy arrays, None where a
        frame has no mask, `available` as an int bit mask.  Synchronises after the upload; for tests."""
        if not 0 <= int(i) < self._n:
            raise _lib.CavpError(f"ClipStore.clip: {i} outside [0, {self._n})")
        i = int(i)
        if not self._frozen:
            frames, masks, srcs, av, mn, tg = self._clips[i]
            return ([f.copy() for f in frames], [None if m is None else m.copy() for m in masks], [(p.copy(), r) for p, r in srcs],
                    av, mn, tg)
        t = self._dev if self._dev is not None else self._host
        get = (lambda k, a=None, b=None: t[k][a:b].cpu().numpy()) if self._dev is not None else (lambda k, a=None, b=None: t[k][a:b].copy())
        one = lambda k: get(k, i, i + 1)[0]
        f0, n, ns = int(one("first")), int(one("n_frames")), int(one("n_src"))
        frames, masks = [], []
        for f in range(f0, f0 + n):
            (h, w), fo, mo = (int(v) for v in get("size", f, f + 1)[0]), int(get("frame_off", f, f + 1)[0]), int(get("mask_off", f, f + 1)[0])
            frames.append(get("frames", fo, fo + 3 * h * w).reshape(h, w, 3))
            masks.append(None if mo < 0 else get("masks", mo, mo + h * w).reshape(h, w))
        po, ln, rt, nc = (one(k) for k in ("pcm_off", "length", "rate_idx", "n_ch"))
        srcs = []
        for s in range(ns):
            raw = get("pcm", int(po[s]), int(po[s]) + int(nc[s]) * int(ln[s]) * self.elem)
            srcs.append((raw.view(_PCM[self.pcm_dtype]).reshape(int(nc[s]), int(ln[s])), int(rt[s])))
        return frames, masks, srcs, int(one("avail")) & 0xFFFFFFFF, int(one("mask_num")), int(one("tag"))


class ClipFeedResult:
    """Outputs of one ClipFeeder.feed call, every field a device tensor: frames u8 [B, Hs, Ws, 3], masks u8 [B, Hs, Ws], sizes i32
    [B, 2] (what FrameAugment takes); pcm [B, S, Cm, Lmax], length / rate_idx / n_ch i32 [B, S] and select i32 [B] (what
    WaveStage(segments=T) takes); index i32 [B] (the clips), tag i32 [B]; `plan` is the kernel's int64 [B, 4 + 3 S] table.  The
    buffers start as zeros; a feed writes only the windows."""
    __slots__ = ("frames", "masks", "sizes", "pcm", "length", "rate_idx", "n_ch", "index", "select", "tag", "plan")

    def __init__(self, B: int, store: ClipStore, dev):
        z = lambda shape, dt: torch.zeros(shape, dtype=dt, device=dev)
        self.frames = z((B, store.Hs, store.Ws, 3), torch.uint8)
        self.masks = z((B, store.Hs, store.Ws), torch.uint8)
        self.sizes = z((B, 2), torch.int32)
        self.pcm = z((B, store.S, store.Cm, store.Lmax), store.pcm_dtype)
        self.length, self.rate_idx, self.n_ch = (z((B, store.S), torch.int32) for _ in range(3))
        self.index, self.select, self.tag = (z((B,), torch.int32) for _ in range(3))
        self.plan = z((B, 4 + 3 * store.S), torch.int64)


class ClipEvalResult:
    """Outputs of one ClipFeeder.feed_clips call, every field a device tensor: frames u8 [B, T, Hs, Ws, 3], masks u8 [B, T, Hs, Ws],
    sizes i32 [B * T, 2] (FrameAugment.eval_ takes frames.view(B * T, Hs, Ws, 3), masks.view(B * T, Hs, Ws), sizes); pcm and its
    tables as ClipFeedResult; count i32 [B] (ClipValidation / VideoValidation: frames t < count[b] are scored; 0 on a padding row),
    index i32 [B] (the clip, -1 on a padding row), n_frames i32 [B], tag i32 [B]; `plan` int64 [B, 4 T + 3 S].  A frame slot >=
    n_frames and the mask of a frame without one keep what the buffers held (zeros at first)."""
    __slots__ = ("frames", "masks", "sizes", "pcm", "length", "rate_idx", "n_ch", "index", "count", "n_frames", "tag", "plan")

    def __init__(self, B: int, store: ClipStore, dev):
        z = lambda shape, dt: torch.zeros(shape, dtype=dt, device=dev)
        T = store.T
        self.frames = z((B, T, store.Hs, store.Ws, 3), torch.uint8)
        self.masks = z((B, T, store.Hs, store.Ws), torch.uint8)
        self.sizes = z((B * T, 2), torch.int32)
        self.pcm = z((B, store.S, store.Cm, store.Lmax), store.pcm_dtype)
        self.length, self.rate_idx, self.n_ch = (z((B, store.S), torch.int32) for _ in range(3))
        self.index, self.count, self.n_frames, self.tag = (z((B,), torch.int32) for _ in range(4))
        self.plan = z((B, 4 * T + 3 * store.S), torch.int64)


class ClipFeeder:
    """See the module docstring.  batch <= 1024 (feed_clips: batch * max_frames <= 1024, the downstream stages' batch limit), world
    <= len(store); feed() needs one full batch per rank and epoch.  Several feeders can share one store.  Device state: int64
    {seed, t_train, bad_inputs, t_eval}; the train plan is the only writer of t_train, the eval plan of t_eval."""

    def __init__(self, store: ClipStore, batch: int, seed: int = 0, rank: int = 0, world: int = 1):
        E = _lib.CavpError
        if not isinstance(store, ClipStore):
            raise E("ClipFeeder: a ClipStore is required")
        self.store, self.B, self.rank, self.world = store, int(batch), int(rank), int(world)
        self.N = len(store)
        if self.N < 1:
            raise E("ClipFeeder: the store is empty")
        if not 1 <= self.B <= MAX_BATCH:
            raise E(f"ClipFeeder: 1 <= batch <= {MAX_BATCH}")
        if self.world < 1 or not 0 <= self.rank < self.world or self.world > self.N:
            raise E("ClipFeeder: 0 <= rank < world <= len(store)")
        self.items_per_rank = -(-self.N // self.world)
        self.steps_per_epoch = self.items_per_rank // self.B          # training, drop_last (0: feed() raises)
        self.steps_per_pass = -(-self.items_per_rank // self.B)       # validation, nothing dropped
        self._seed = int(seed)
        self._state = None
        self.manual_seed(seed)

    # ---- device state ------------------------------------------------------------------------------------------------------
    def _ensure(self):
        if self._state is None:
            if not self.store.frozen:
                raise _lib.CavpError("ClipFeeder: the store is not frozen")
            if len(self.store) != self.N:
                raise _lib.CavpError("ClipFeeder: the store grew after the feeder was made")
            self.store._ensure()
            self.device = self.store.device
            if _lib.load().cavp_clips_plan_words(self.store.T, self.store.S) != 4 * self.store.T + 3 * self.store.S:
                raise _lib.CavpError("ClipFeeder: libcavp_hip.so was built with another plan row; rebuild")
            self._state = torch.zeros(4, dtype=torch.int64, device=self.device)       # {seed, t_train, bad_inputs, t_eval}
            self._state[:1].copy_(torch.tensor([self._seed], dtype=torch.int64))
        return self._state

    def manual_seed(self, seed: int) -> None:
        """Reset the seed and the train counter (t = 0); the eval counter stays.  A host-to-device write: not legal during a capture."""
        s = int(seed) & 0xFFFFFFFFFFFFFFFF
        self._seed = s - (1 << 64) if s >= (1 << 63) else s
        if self._state is not None:
            self._state[:2].copy_(torch.tensor([self._seed, 0], dtype=torch.int64))

    def set_step(self, t: int, eval_step: Optional[int] = None) -> None:
        """The next feed is step t; eval_step, when given, the step of the next feed_clips (host-to-device writes, as manual_seed)."""
        if int(t) < 0 or (eval_step is not None and int(eval_step) < 0):
            raise _lib.CavpError("ClipFeeder.set_step: t >= 0")
        self._ensure()[1:2].copy_(torch.tensor([int(t)], dtype=torch.int64))
        if eval_step is not None:
            self._state[3:4].copy_(torch.tensor([int(eval_step)], dtype=torch.int64))

    def step(self) -> int:
        """Synchronises: the step the next feed (or replay) will draw."""
        return int(self._ensure()[1].item())

    def eval_step(self) -> int:
        """Synchronises: the step the next feed_clips (or replay) will walk; eval_step() % steps_per_pass is its place in the pass."""
        return int(self._ensure()[3].item())

    def state_dict(self) -> dict:
        """Synchronises: {"seed", "t", "t_eval"}."""
        st = self._ensure().cpu()
        return {"seed": int(st[0]), "t": int(st[1]), "t_eval": int(st[3])}

    def load_state_dict(self, d: dict) -> None:
        self.manual_seed(int(d["seed"]))
        self.set_step(int(d["t"]), int(d.get("t_eval", 0)))

    def rollback_ranges(self):
        """[(name, tensor, byte_offset, nbytes)]: {seed, t_train} of the state block - a skipped training step then sees the same
        batch and the same frames again.  The eval counter and `bad_inputs` are not named."""
        return [("state", self._ensure(), 0, 16)]

    def check(self) -> None:
        """Synchronises and raises CavpError if, since the last check, an `index=` entry was outside [0, len(store)), a `frame=`
        entry was not a frame the clip's `available` names, or a table entry of the store left its limits."""
        if self._state is None:
            raise _lib.CavpError("check: no ClipFeeder call yet")
        bad = int(self._state[2].item())
        if bad:
            self._state[2:3].zero_()
            raise _lib.CavpError(f"ClipFeeder: {bad} input value(s) out of range (index outside [0, {self.N}) or frame not available)")

    def epoch_of(self, t: int) -> int:
        return int(t) // self.steps_per_epoch

    # ---- the calls ----------------------------------------------------------------------------------------------------------
    def _override(self, t, name):
        if t is None:
            return
        E = _lib.CavpError
        if not isinstance(t, torch.Tensor) or t.dtype != torch.int32 or tuple(t.shape) != (self.B,):
            raise E(f"ClipFeeder: {name} must be int32 [B]")
        if not t.is_cuda:
            raise E(f"ClipFeeder: {name} is a CPU tensor; the feeder needs HIP device tensors (no CPU fallback)")
        if t.device != self.device or not t.is_contiguous():
            raise E(f"ClipFeeder: {name} must be contiguous on {self.device}")

    def _check_out(self, out, cls, frames_shape):
        st = self.store
        if not isinstance(out, cls) or tuple(out.frames.shape) != frames_shape or out.frames.device != self.device or \
                tuple(out.pcm.shape) != (self.B, st.S, st.Cm, st.Lmax) or out.pcm.dtype != st.pcm_dtype:
            raise _lib.CavpError("ClipFeeder: out= was made for other shapes")
        for name in cls.__slots__:
            if not getattr(out, name).is_contiguous():
                raise _lib.CavpError(f"ClipFeeder: out.{name} must be contiguous")

    def _tables(self):
        st = self.store
        d = st._ensure()
        nb = st.arena_bytes()
        return d, [_ptr(d[k]) for k in _FRAME_TABLES + _CLIP_TABLES] + [nb["frames"], nb["masks"], nb["pcm"], st.total_frames, self.N,
                                                                      self.B, st.S, st.T, st.Hs, st.Ws, st.Cm, st.Lmax, st.elem,
                                                                      self.rank, self.world]

    def _gather(self, lib, d, out, T_out, stream):
        st = self.store
        _lib.check(lib.cavp_clips_gather(_ptr(d["frames"]), _ptr(d["masks"]), _ptr(d["pcm"]), _ptr(out.plan), self.B, T_out, st.S, st.Hs,
                                         st.Ws, st.Cm, st.Lmax, st.elem, _ptr(out.frames), _ptr(out.masks), _ptr(out.pcm), stream),
                   "cavp_clips_gather")

    def feed(self, out: Optional[ClipFeedResult] = None, index: Optional[torch.Tensor] = None,
             frame: Optional[torch.Tensor] = None) -> ClipFeedResult:
        """Training: one drawn frame per row.  Two launches on the current stream.  out: a previous result whose buffers are written
        again (static addresses for a captured graph).  index / frame: int32 [B] on the device, the clips / the frames to feed
        instead of the draws."""
        state = self._ensure()
        if self.steps_per_epoch == 0:
            raise _lib.CavpError(f"ClipFeeder.feed: {self.items_per_rank} clips per rank hold no full batch of {self.B} (drop_last)")
        self._override(index, "index")
        self._override(frame, "frame")
        st = self.store
        if out is None:
            out = ClipFeedResult(self.B, st, self.device)
        else:
            self._check_out(out, ClipFeedResult, (self.B, st.Hs, st.Ws, 3))
        lib = _lib.load()
        d, args = self._tables()
        stream = C.c_void_p(_stream())
        _lib.check(lib.cavp_clips_plan_train(*args, _ptr(index), _ptr(frame), _ptr(state), _ptr(out.index), _ptr(out.select),
                                             _ptr(out.tag), _ptr(out.sizes), _ptr(out.length), _ptr(out.rate_idx), _ptr(out.n_ch),
                                             _ptr(out.plan), stream), "cavp_clips_plan_train")
        self._gather(lib, d, out, 1, stream)
        return out

    def feed_clips(self, out: Optional[ClipEvalResult] = None) -> ClipEvalResult:
        """Validation: the next B clips in order, every frame slot.  Two launches on the current stream; steps_per_pass calls walk
        the store once."""
        state = self._ensure()
        st = self.store
        if self.B * st.T > MAX_BATCH:
            raise _lib.CavpError(f"ClipFeeder.feed_clips: batch * max_frames = {self.B * st.T} > {MAX_BATCH}")
        if out is None:
            out = ClipEvalResult(self.B, st, self.device)
        else:
            self._check_out(out, ClipEvalResult, (self.B, st.T, st.Hs, st.Ws, 3))
        lib = _lib.load()
        d, args = self._tables()
        stream = C.c_void_p(_stream())
        _lib.check(lib.cavp_clips_plan_eval(*args, _ptr(state), _ptr(out.index), _ptr(out.count), _ptr(out.n_frames), _ptr(out.tag),
                                            _ptr(out.sizes), _ptr(out.length), _ptr(out.rate_idx), _ptr(out.n_ch), _ptr(out.plan),
                                            stream), "cavp_clips_plan_eval")
        self._gather(lib, d, out, st.T, stream)
        return out
