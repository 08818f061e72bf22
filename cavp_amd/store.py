"""A data set that lives on the GPU: DeviceStore holds the decoded items, BatchFeeder draws each batch on the device and gathers
it into the staging buffers FrameAugment and WaveStage read - the `DataLoader` + `.cuda()` lines of the reference trainers
(RandomSampler / DistributedSampler with drop_last=True, main_vpo_mono.py:188-201) as two launches of csrc/store.hip with no host
value that depends on a device value: capturable at the head of the prologue of `capture_train_step`, so that a whole epoch, the
move to the next epoch's shuffle included, is graph replays.

    store = DeviceStore(stage=(Hs, Ws), max_sources=S, max_channels=Cm, max_len=Lmax, pcm_dtype=torch.int16, device=dev)
    for frame, mask, sources in decoded_items:                  # uint8 [h, w, 3], uint8 [h, w], [(pcm [n_ch, len], rate_idx), ...]
        store.append(frame, mask, sources)
    store.freeze()                                              # byte arenas + offset tables, one upload
    feeder = BatchFeeder(store, batch=B, seed=0, rank=rank, world=world)
    fed = feeder.feed(out=fed)                                  # FeedResult: the tensors the two stages take
    aug(fed.frames, fed.masks, fed.sizes, out=augmented)
    wave(fed.pcm, fed.length, fed.rate_idx, fed.n_ch, out=cut)

Opt-in and additive: nothing that exists changes.  Decoding stays on the host, once; the store holds raw bytes (`store.nbytes`).
The rules are restated in include/cavp_hip.h ("device store"), tests/_store_ref.py and DESIGN.md 4x.

Sampling: step t of a feeder has epoch e = t // spe, spe = ceil(N / world) // B; row i is rank-local position j = (t % spe) * B + i,
global position q = j * world + rank (q - N when q >= N: DistributedSampler's padding) and item pi_e(q), a keyed bijection of
[0, N) computed per element: a balanced Feistel network with Philox4x32-10 as the round function, cycle-walked into [0, N).  As
for the pair builder and the augmentation this is the reference sampler's distribution on another stream: no seed reproduces
torch.randperm's values.  `index=` replaces the draw.

What the gather writes: the item's h x w window of its staging slot, each present channel up to its length, and the tables.  Outside
them nothing is written - the consumers never read there."""
from __future__ import annotations

import ctypes as C
from typing import Optional, Sequence

import numpy as np
import torch

from . import _lib
from .ops import _ptr, _stream

MAX_BATCH, MAX_STAGE, MAX_LEN = 1024, 16384, 1 << 28
_PCM = {torch.int16: np.int16, torch.float32: np.float32}


def _as_numpy(a, what: str) -> np.ndarray:
    if isinstance(a, torch.Tensor):
        if a.is_cuda:
            raise _lib.CavpError(f"DeviceStore.append: {what} is a device tensor; append takes numpy arrays or CPU tensors")
        a = a.numpy()
    if not isinstance(a, np.ndarray):
        raise _lib.CavpError(f"DeviceStore.append: {what} must be a numpy array or a CPU tensor")
    return a


class DeviceStore:
    """A frozen, device-resident ragged data set.  Items are packed back to back with no padding into three byte arenas (frames,
    masks, PCM), so most rows start at addresses that are not 16-byte aligned; the gather kernel is written for that.  Limits: stage
    sides <= 16384, max_len <= 2^28, 2 + max_sources * max_channels <= 65535, fewer than 2^31 items.  The constructor and append()
    touch no device."""

    def __init__(self, stage, max_sources: int, max_channels: int, max_len: int, pcm_dtype=torch.int16, device=None):
        E = _lib.CavpError
        if stage is None or len(tuple(stage)) != 2:
            raise E("DeviceStore: stage=(Hs, Ws) is required")
        self.Hs, self.Ws = (int(v) for v in stage)
        if not (1 <= self.Hs <= MAX_STAGE and 1 <= self.Ws <= MAX_STAGE):
            raise E(f"DeviceStore: stage sides must lie in [1, {MAX_STAGE}]")
        self.S, self.Cm, self.Lmax = int(max_sources), int(max_channels), int(max_len)
        if self.S < 1 or self.Cm < 1 or 2 + self.S * self.Cm > 65535:
            raise E("DeviceStore: max_sources and max_channels must be positive, 2 + max_sources * max_channels <= 65535")
        if not 1 <= self.Lmax <= MAX_LEN:
            raise E(f"DeviceStore: 1 <= max_len <= {MAX_LEN}")
        if isinstance(pcm_dtype, str):
            pcm_dtype = getattr(torch, pcm_dtype, None)
        if pcm_dtype not in _PCM:
            raise E("DeviceStore: pcm_dtype is torch.int16 or torch.float32")
        self.pcm_dtype = pcm_dtype
        self.elem = 2 if pcm_dtype == torch.int16 else 4
        self._device = device
        self._items = []          # (frame, mask, [(pcm, rate_idx)]) until freeze()
        self._host = None         # the packed arenas and tables between freeze() and the upload
        self._dev = None          # the same on the device
        self._n = 0
        self._frozen = False

    def __len__(self) -> int:
        return self._n

    @property
    def frozen(self) -> bool:
        return self._frozen

    # ---- filling -----------------------------------------------------------------------------------------------------------
    def append(self, frame, mask, sources: Sequence = ()) -> int:
        """One item: frame uint8 [h, w, 3], mask uint8 [h, w], sources = [(pcm [n_ch, len], rate_idx), ...] with pcm of the store's
        dtype.  The arrays are copied.  Returns the item's index."""
        E = _lib.CavpError
        if self._frozen:
            raise E("DeviceStore.append: the store is frozen")
        frame, mask = _as_numpy(frame, "frame"), _as_numpy(mask, "mask")
        if frame.dtype != np.uint8 or frame.ndim != 3 or frame.shape[2] != 3:
            raise E(f"DeviceStore.append: frame must be uint8 [h, w, 3], got {frame.dtype} {tuple(frame.shape)}")
        h, w = frame.shape[:2]
        if not (1 <= h <= self.Hs and 1 <= w <= self.Ws):
            raise E(f"DeviceStore.append: frame {h} x {w} does not fit the stage {self.Hs} x {self.Ws}")
        if mask.dtype != np.uint8 or tuple(mask.shape) != (h, w):
            raise E(f"DeviceStore.append: mask must be uint8 [{h}, {w}], got {mask.dtype} {tuple(mask.shape)}")
        sources = list(sources)
        if len(sources) > self.S:
            raise E(f"DeviceStore.append: {len(sources)} sources, max_sources = {self.S}")
        kept = []
        want = _PCM[self.pcm_dtype]
        for src in sources:
            if not isinstance(src, (tuple, list)) or len(src) != 2:
                raise E("DeviceStore.append: a source is (pcm [n_ch, len], rate_idx)")
            pcm, rate = _as_numpy(src[0], "pcm"), int(src[1])
            if pcm.dtype != want or pcm.ndim != 2:
                raise E(f"DeviceStore.append: pcm must be {np.dtype(want).name} [n_ch, len], got {pcm.dtype} {tuple(pcm.shape)}")
            if not (1 <= pcm.shape[0] <= self.Cm and 1 <= pcm.shape[1] <= self.Lmax):
                raise E(f"DeviceStore.append: pcm {tuple(pcm.shape)} outside [1 .. {self.Cm}, 1 .. {self.Lmax}]")
            if not 0 <= rate < 1 << 31:
                raise E("DeviceStore.append: rate_idx must be a non-negative int32")
            kept.append((np.array(pcm, order="C"), rate))
        if self._n + 1 >= 1 << 31:
            raise E("DeviceStore.append: fewer than 2^31 items")
        self._items.append((np.array(frame, order="C"), np.array(mask, order="C"), kept))
        self._n += 1
        return self._n - 1

    def pack(self) -> dict:
        """The arenas and tables as numpy arrays (pure host arithmetic; what freeze() uploads)."""
        N, S = self._n, self.S
        frame_off, mask_off = np.zeros(N, np.int64), np.zeros(N, np.int64)
        size, n_src = np.zeros((N, 2), np.int32), np.zeros(N, np.int32)
        pcm_off = np.zeros((N, S), np.int64)
        length, rate_idx, n_ch = (np.zeros((N, S), np.int32) for _ in range(3))
        fo = mo = po = 0
        fparts, mparts, pparts = [], [], []
        for i, (frame, mask, srcs) in enumerate(self._items):
            frame_off[i], mask_off[i], size[i], n_src[i] = fo, mo, frame.shape[:2], len(srcs)
            fparts.append(frame.reshape(-1))
            mparts.append(mask.reshape(-1))
            fo += frame.size
            mo += mask.size
            for s, (pcm, rate) in enumerate(srcs):
                pcm_off[i, s], length[i, s], rate_idx[i, s], n_ch[i, s] = po, pcm.shape[1], rate, pcm.shape[0]
                pparts.append(pcm.reshape(-1).view(np.uint8))
                po += pcm.size * self.elem
        cat = lambda parts: np.concatenate(parts) if parts else np.zeros(0, np.uint8)
        return {"frames": cat(fparts), "masks": cat(mparts), "pcm": cat(pparts), "frame_off": frame_off, "mask_off": mask_off,
                "size": size, "n_src": n_src, "pcm_off": pcm_off, "length": length, "rate_idx": rate_idx, "n_ch": n_ch}

    def freeze(self, upload: bool = True) -> "DeviceStore":
        """Pack everything and upload it once; append() raises afterwards.  upload=False leaves the upload to the first feed (the
        packed host copy is dropped then)."""
        if self._frozen:
            raise _lib.CavpError("DeviceStore.freeze: already frozen")
        if self._n == 0:
            raise _lib.CavpError("DeviceStore.freeze: the store is empty")
        self._host = self.pack()
        self._items = None
        self._frozen = True
        self._bytes = {k: int(v.nbytes) for k, v in self._host.items()}
        if upload:
            self._ensure()
        return self

    def _ensure(self) -> dict:
        if self._dev is None:
            if not self._frozen:
                raise _lib.CavpError("DeviceStore: call freeze() first")
            dev = torch.device(self._device) if self._device is not None else torch.device("cuda", torch.cuda.current_device())
            if dev.type != "cuda":
                raise _lib.CavpError("DeviceStore lives on a HIP device (there is no CPU fallback)")
            if dev.index is None:
                dev = torch.device("cuda", torch.cuda.current_device())
            self.device = dev
            # an arena nobody can read from (no PCM at all) still gets an address
            self._dev = {k: torch.from_numpy(v if v.size else np.zeros(16, v.dtype)).to(dev) for k, v in self._host.items()}
            self._host = None
        return self._dev

    @property
    def nbytes(self) -> int:
        """Bytes resident after freeze(): the three arenas and the tables."""
        if not self._frozen:
            raise _lib.CavpError("DeviceStore.nbytes: call freeze() first")
        return sum(self._bytes.values())

    def arena_bytes(self) -> dict:
        """{"frames", "masks", "pcm"}: the packed bytes per arena."""
        if not self._frozen:
            raise _lib.CavpError("DeviceStore.arena_bytes: call freeze() first")
        return {k: self._bytes[k] for k in ("frames", "masks", "pcm")}

    def item(self, i: int):
        """Host read-back of item i: (frame, mask, [(pcm, rate_idx), ...]) as numpy arrays.  Synchronises; for tests."""
        if not 0 <= int(i) < self._n:
            raise _lib.CavpError(f"DeviceStore.item: {i} outside [0, {self._n})")
        i = int(i)
        if not self._frozen:
            frame, mask, srcs = self._items[i]
            return frame.copy(), mask.copy(), [(p.copy(), r) for p, r in srcs]
        t = self._dev if self._dev is not None else self._host
        get = (lambda k, a=None, b=None: t[k][a:b].cpu().numpy()) if self._dev is not None else (lambda k, a=None, b=None: t[k][a:b].copy())
        (h, w), ns = (int(v) for v in get("size", i, i + 1)[0]), int(get("n_src", i, i + 1)[0])
        fo, mo = int(get("frame_off", i, i + 1)[0]), int(get("mask_off", i, i + 1)[0])
        frame = get("frames", fo, fo + 3 * h * w).reshape(h, w, 3)
        mask = get("masks", mo, mo + h * w).reshape(h, w)
        po, ln, rt, nc = (get(k, i, i + 1)[0] for k in ("pcm_off", "length", "rate_idx", "n_ch"))
        srcs = []
        for s in range(ns):
            raw = get("pcm", int(po[s]), int(po[s]) + int(nc[s]) * int(ln[s]) * self.elem)
            srcs.append((raw.view(_PCM[self.pcm_dtype]).reshape(int(nc[s]), int(ln[s])), int(rt[s])))
        return frame, mask, srcs


class FeedResult:
    """Outputs of one BatchFeeder.feed call, every field a device tensor: frames u8 [B, Hs, Ws, 3], masks u8 [B, Hs, Ws], sizes i32
    [B, 2] (what FrameAugment takes); pcm [B, S, Cm, Lmax] of the store's dtype, length / rate_idx / n_ch i32 [B, S] (what WaveStage
    takes); index i32 [B], the items of the batch.  `plan` is the plan kernel's int64 [B, 4 + 3 S] table (include/cavp_hip.h).
    The buffers start as zeros; a feed writes only the windows (see the module docstring)."""
    __slots__ = ("frames", "masks", "sizes", "pcm", "length", "rate_idx", "n_ch", "index", "plan")

    def __init__(self, B: int, store: DeviceStore, dev):
        z = lambda shape, dt: torch.zeros(shape, dtype=dt, device=dev)
        self.frames = z((B, store.Hs, store.Ws, 3), torch.uint8)
        self.masks = z((B, store.Hs, store.Ws), torch.uint8)
        self.sizes = z((B, 2), torch.int32)
        self.pcm = z((B, store.S, store.Cm, store.Lmax), store.pcm_dtype)
        self.length, self.rate_idx, self.n_ch = (z((B, store.S), torch.int32) for _ in range(3))
        self.index = z((B,), torch.int32)
        self.plan = z((B, 4 + 3 * store.S), torch.int64)


class BatchFeeder:
    """See the module docstring.  batch <= 1024, world <= len(store), and an epoch must hold one full batch per rank.  Several
    feeders (ranks, a validation pass) can share one store.  Device state: int64 {seed, t, bad_inputs, reserved}; the plan kernel
    is the only writer of t, and it advances t on every feed, with `index=` too."""

    def __init__(self, store: DeviceStore, batch: int, seed: int = 0, rank: int = 0, world: int = 1):
        E = _lib.CavpError
        if not isinstance(store, DeviceStore):
            raise E("BatchFeeder: a DeviceStore is required")
        self.store, self.B, self.rank, self.world = store, int(batch), int(rank), int(world)
        self.N = len(store)
        if self.N < 1:
            raise E("BatchFeeder: the store is empty")
        if not 1 <= self.B <= MAX_BATCH:
            raise E(f"BatchFeeder: 1 <= batch <= {MAX_BATCH}")
        if self.world < 1 or not 0 <= self.rank < self.world or self.world > self.N:
            raise E("BatchFeeder: 0 <= rank < world <= len(store)")
        self.items_per_rank = -(-self.N // self.world)
        self.steps_per_epoch = self.items_per_rank // self.B
        if self.steps_per_epoch == 0:
            raise E(f"BatchFeeder: {self.items_per_rank} items per rank hold no full batch of {self.B} (drop_last)")
        self._seed = int(seed)
        self._state = None
        self.manual_seed(seed)

    # ---- device state ------------------------------------------------------------------------------------------------------
    def _ensure(self):
        if self._state is None:
            if not self.store.frozen:
                raise _lib.CavpError("BatchFeeder: the store is not frozen")
            if len(self.store) != self.N:
                raise _lib.CavpError("BatchFeeder: the store grew after the feeder was made")
            self.store._ensure()
            self.device = self.store.device
            if _lib.load().cavp_store_plan_words(self.store.S) != 4 + 3 * self.store.S:
                raise _lib.CavpError("BatchFeeder: libcavp_hip.so was built with another plan row; rebuild")
            self._state = torch.zeros(4, dtype=torch.int64, device=self.device)       # {seed, t, bad_inputs, reserved}
            self._state[:1].copy_(torch.tensor([self._seed], dtype=torch.int64))
        return self._state

    def manual_seed(self, seed: int) -> None:
        """Reset the seed and the step counter (t = 0).  A host-to-device write: not legal during a capture; graphs captured earlier
        see the new values on their next replay."""
        s = int(seed) & 0xFFFFFFFFFFFFFFFF
        self._seed = s - (1 << 64) if s >= (1 << 63) else s
        if self._state is not None:
            self._state[:2].copy_(torch.tensor([self._seed, 0], dtype=torch.int64))

    def set_step(self, t: int) -> None:
        """The next feed is step t (a host-to-device write, as manual_seed)."""
        if int(t) < 0:
            raise _lib.CavpError("BatchFeeder.set_step: t >= 0")
        self._ensure()[1:2].copy_(torch.tensor([int(t)], dtype=torch.int64))

    def step(self) -> int:
        """Synchronises: the step the next feed (or replay) will draw."""
        return int(self._ensure()[1].item())

    def state_dict(self) -> dict:
        """Synchronises: {"seed", "t"} - with the store's contents, everything that decides the batches to come."""
        st = self._ensure()[:2].cpu()
        return {"seed": int(st[0]), "t": int(st[1])}

    def load_state_dict(self, d: dict) -> None:
        self.manual_seed(int(d["seed"]))
        self.set_step(int(d["t"]))

    def rollback_ranges(self):
        """[(name, tensor, byte_offset, nbytes)]: {seed, t} of the state block, the only state a feed mutates - a skipped step then
        sees the same batch again (`bad_inputs` is a diagnostic and is not named).  For cavp_amd.rollback.StepRollback.add()."""
        return [("state", self._ensure(), 0, 16)]

    def check(self) -> None:
        """Synchronises and raises CavpError if, since the last check, an `index=` entry was outside [0, len(store)) (item 0 was fed
        in its place) or a table entry of the store left its limits."""
        if self._state is None:
            raise _lib.CavpError("check: no BatchFeeder call yet")
        bad = int(self._state[2].item())
        if bad:
            self._state[2:3].zero_()
            raise _lib.CavpError(f"BatchFeeder: {bad} input value(s) out of range (index outside [0, {self.N}))")

    def epoch_of(self, t: int) -> int:
        return int(t) // self.steps_per_epoch

    # ---- the call -----------------------------------------------------------------------------------------------------------
    def feed(self, out: Optional[FeedResult] = None, index: Optional[torch.Tensor] = None) -> FeedResult:
        """Two launches on the current stream.  out: a previous result whose buffers are written again (static addresses for a
        captured graph).  index: int32 [B] on the device, the items to feed instead of the draw."""
        E = _lib.CavpError
        state = self._ensure()
        st, dev, B = self.store, self.device, self.B
        if index is not None:
            if not isinstance(index, torch.Tensor) or index.dtype != torch.int32 or tuple(index.shape) != (B,):
                raise E("BatchFeeder: index must be int32 [B]")
            if not index.is_cuda:
                raise E("BatchFeeder: index is a CPU tensor; the feeder needs HIP device tensors (no CPU fallback)")
            if index.device != dev or not index.is_contiguous():
                raise E(f"BatchFeeder: index must be contiguous on {dev}")
        if out is None:
            out = FeedResult(B, st, dev)
        else:
            if not isinstance(out, FeedResult) or tuple(out.frames.shape) != (B, st.Hs, st.Ws, 3) or out.frames.device != dev or \
                    tuple(out.pcm.shape) != (B, st.S, st.Cm, st.Lmax) or out.pcm.dtype != st.pcm_dtype:
                raise E("BatchFeeder: out= was made for other shapes")
            for name in FeedResult.__slots__:
                if not getattr(out, name).is_contiguous():
                    raise E(f"BatchFeeder: out.{name} must be contiguous")
        lib = _lib.load()
        d = st._ensure()
        nb = st.arena_bytes()
        stream = C.c_void_p(_stream())
        _lib.check(lib.cavp_store_plan(_ptr(d["frame_off"]), _ptr(d["mask_off"]), _ptr(d["size"]), _ptr(d["n_src"]), _ptr(d["pcm_off"]),
                                       _ptr(d["length"]), _ptr(d["rate_idx"]), _ptr(d["n_ch"]), nb["frames"], nb["masks"], nb["pcm"],
                                       self.N, B, st.S, st.Hs, st.Ws, st.Cm, st.Lmax, st.elem, self.rank, self.world, _ptr(index),
                                       _ptr(state), _ptr(out.index), _ptr(out.sizes), _ptr(out.length), _ptr(out.rate_idx),
                                       _ptr(out.n_ch), _ptr(out.plan), stream), "cavp_store_plan")
        _lib.check(lib.cavp_store_gather(_ptr(d["frames"]), _ptr(d["masks"]), _ptr(d["pcm"]), _ptr(out.plan), B, st.S, st.Hs, st.Ws,
                                         st.Cm, st.Lmax, st.elem, _ptr(out.frames), _ptr(out.masks), _ptr(out.pcm), stream),
                   "cavp_store_gather")
        return out


_CLIP_NAMES = ("ClipStore", "ClipFeeder", "ClipFeedResult", "ClipEvalResult")


def __getattr__(name):
    """The clip store (cavp_amd/clips.py) is re-exported from here; resolved on first use, since clips.py builds on this module."""
    if name in _CLIP_NAMES:
        from . import clips
        return getattr(clips, name)
    raise AttributeError(f"module {__name__!r} has no attribute {name!r}")
