"""The step rollback on the device (csrc/rollback.hip, cavp_amd/rollback.py, CAVP.capture_train_step(rollback=)).

Kernel level: one table mixing ranges of 4 .. 192 bytes and ranges around a workgroup's span at every live / shadow offset from a
16-byte boundary, every byte outside the ranges a canary; save, guarded restore with the word clear and set, forced restore,
scrub ranges, the counters, an empty table, and the same through a captured graph.  Everything is compared bit for bit.

End to end: the whole iteration in one graph (CFG3 of tests/test_gpu_optim_sched.py) replayed on a clean batch, a batch with one
NaN pixel and a clean batch again, against a twin that never saw the poisoned one."""
import ctypes as C

import numpy as np
import pytest
import torch

from cavp_amd.synth import synth_inputs
from tests.test_gpu_optim_sched import CFG3, SEED
from tests.test_gpu_train_model import _build

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
SPAN = 16 * 1024          # bytes one workgroup serves per pass (rollback.SPAN_BLOCKS x rollback.BLOCK_BYTES)
NAN_WORDS = np.array([0x7FC00000, 0xFFFFFFFF, 0x7F800001, 0x7F800000, 0xFF800000, 0x00000001], dtype=np.uint32)


# ------------------------------------------------------------------------------------------------------------- kernel level
def _cases():
    """(nbytes, live offset, shadow offset, scrub): the small sizes at all 16 offset pairs, the sizes around a span at the four equal
    pairs and two unequal ones, and scrub ranges of three sizes"""
    out = []
    for n in (4, 8, 12, 16, 20, 48 * 4):
        out += [(n, lo, so, False) for lo in (0, 4, 8, 12) for so in (0, 4, 8, 12)]
    for n in (SPAN - 16, SPAN, SPAN + 4, 3 * SPAN + 8):
        out += [(n, o, o, False) for o in (0, 4, 8, 12)] + [(n, 4, 0, False), (n, 8, 12, False)]
    out += [(20, 4, 0, True), (48 * 4, 8, 0, True), (SPAN + 4, 12, 0, True), (2 * SPAN, 0, 0, True)]
    return out


class _Rig:
    """Two byte buffers (live, shadow) holding the ranges of _cases() with at least 16 canary bytes either side of each, the
    device table built by rollback.build_table's block rule (shadows placed by hand, so that both offsets vary) and the state
    block."""

    def __init__(self):
        from cavp_amd import _lib
        from cavp_amd.rollback import ROLLBACK_SCRUB, RollbackRange, RollbackState
        self.lib = _lib.load()
        cases = _cases()
        place, cur = [], [0, 0]                       # per case: (live start, shadow start) relative to the buffers
        for n, lo, so, scrub in cases:
            starts = []
            for k, off in ((0, lo), (1, so)):
                slot = (cur[k] + 15) // 16 * 16 + 32  # >= 16 canary bytes below the range
                starts.append(slot + off)
                cur[k] = slot + off + n + 16          # ... and above it
            place.append(tuple(starts))
        rng = np.random.default_rng(7)
        size = [(c + 63) // 64 * 64 for c in cur]
        self.live0 = np.full(size[0], 0xA5, dtype=np.uint8)
        self.shadow0 = np.full(size[1], 0x5A, dtype=np.uint8)
        self.in_live = np.zeros(size[0], dtype=bool)
        self.in_scrub = np.zeros(size[0], dtype=bool)
        self.in_shadow = np.zeros(size[1], dtype=bool)
        self.pattern = self.live0.copy()              # what the "forward" leaves in the live ranges: NaN bit patterns among noise
        for (n, lo, so, scrub), (ls, ss) in zip(cases, place):
            words = rng.integers(0, 1 << 32, n // 4, dtype=np.uint32)
            self.live0[ls:ls + n] = words.view(np.uint8)
            pat = rng.integers(0, 1 << 32, n // 4, dtype=np.uint32)
            pat[::3] = NAN_WORDS[np.arange(len(pat[::3])) % len(NAN_WORDS)]
            self.pattern[ls:ls + n] = pat.view(np.uint8)
            (self.in_scrub if scrub else self.in_live)[ls:ls + n] = True
            if not scrub:
                self.in_shadow[ss:ss + n] = True
        self.live = torch.from_numpy(self.live0.copy()).to(DEV)
        self.shadow = torch.from_numpy(self.shadow0.copy()).to(DEV)
        self.pattern_dev = torch.from_numpy(self.pattern).to(DEV)
        assert self.live.data_ptr() % 16 == 0 and self.shadow.data_ptr() % 16 == 0
        tab = (RollbackRange * len(cases))()
        blk = 0
        for i, ((n, lo, so, scrub), (ls, ss)) in enumerate(zip(cases, place)):
            live = self.live.data_ptr() + ls
            assert live % 16 == lo and (scrub or (self.shadow.data_ptr() + ss) % 16 == so)
            tab[i] = RollbackRange(live, None if scrub else self.shadow.data_ptr() + ss, n, blk, ROLLBACK_SCRUB if scrub else 0)
            blk += int(self.lib.cavp_rollback_blocks(live, n))
        self.n, self.total = len(cases), blk
        self.table = torch.frombuffer(bytearray(bytes(tab)), dtype=torch.uint8).to(DEV)
        self.state = torch.zeros(C.sizeof(RollbackState), dtype=torch.uint8, device=DEV)
        self.word = torch.zeros(4, dtype=torch.int32, device=DEV)
        self.place, self.cases = place, cases
        # the shadow image of the live ranges: shadow bytes in range order equal live bytes in range order
        self.live_idx = np.concatenate([np.arange(ls, ls + n) for (n, _, _, s), (ls, _) in zip(cases, place) if not s])
        self.shadow_idx = np.concatenate([np.arange(ss, ss + n) for (n, _, _, s), (_, ss) in zip(cases, place) if not s])

    def save(self):
        from cavp_amd import _lib
        from cavp_amd.ops import _ptr, _stream
        _lib.check(self.lib.cavp_rollback_save(_ptr(self.table), self.n, self.total, _ptr(self.state), C.c_void_p(_stream())), "save")

    def restore(self, word=None):
        from cavp_amd import _lib
        from cavp_amd.ops import _ptr, _stream
        _lib.check(self.lib.cavp_rollback_restore(_ptr(self.table), self.n, self.total, _ptr(word), _ptr(self.state),
                                                  C.c_void_p(_stream())), "restore")

    def counters(self):
        from cavp_amd.rollback import RollbackState
        s = RollbackState.from_buffer_copy(self.state.cpu().numpy().tobytes())
        return int(s.saves), int(s.restores)

    def expect(self, ranges, scrubs):
        """the live buffer with `ranges` in the restore ranges, `scrubs` in the scrub ranges (None: zeros) and canaries elsewhere"""
        want = self.live0.copy()
        want[self.in_live] = ranges[self.in_live]
        want[self.in_scrub] = 0 if scrubs is None else scrubs[self.in_scrub]
        return want


@pytest.fixture(scope="module")
def rig():
    return _Rig()


def test_table_shape(rig):
    """the table mixes what it should: small ranges sharing workgroups, ranges of many workgroups, both vector classes"""
    assert rig.n == 6 * 16 + 4 * 6 + 4
    assert rig.total < rig.n + sum(n for n, *_ in rig.cases) // 1024 + 1          # one block per small range, not one workgroup
    assert (rig.total + 15) // 16 < rig.n                                          # fewer workgroup spans than ranges


def test_save_restore_sequence(rig):
    """save; overwrite; restore with the word clear, set, forced and set to another non-zero value; counters exact after each; every
    byte outside the ranges untouched."""
    live, shadow = rig.live, rig.shadow
    live.copy_(torch.from_numpy(rig.live0))
    shadow.copy_(torch.from_numpy(rig.shadow0))
    rig.state.zero_()
    rig.save()
    got_shadow = shadow.cpu().numpy()
    assert np.array_equal(live.cpu().numpy(), rig.live0)                            # a save writes no live byte
    assert np.array_equal(got_shadow[~rig.in_shadow], rig.shadow0[~rig.in_shadow])  # ... and no shadow byte outside the ranges
    assert np.array_equal(got_shadow[rig.shadow_idx], rig.live0[rig.live_idx])
    saved = got_shadow.copy()

    live.copy_(rig.pattern_dev)                                                     # the iteration: NaN patterns into every range
    rig.word.zero_()
    rig.restore(rig.word)                                                           # word clear: nothing happens
    assert np.array_equal(live.cpu().numpy(), rig.expect(rig.pattern, rig.pattern))
    assert rig.counters() == (1, 0)

    rig.word[0] = 1
    rig.restore(rig.word)                                                           # word set
    assert np.array_equal(live.cpu().numpy(), rig.expect(rig.live0, None))
    assert rig.counters() == (1, 1)

    live.copy_(rig.pattern_dev)
    rig.restore(None)                                                               # forced
    assert np.array_equal(live.cpu().numpy(), rig.expect(rig.live0, None))
    assert rig.counters() == (1, 2)

    live.copy_(rig.pattern_dev)
    rig.word[0] = -(1 << 31)                                                        # any non-zero word is "set"
    rig.restore(rig.word[:1])
    assert np.array_equal(live.cpu().numpy(), rig.expect(rig.live0, None))
    assert rig.counters() == (1, 3)
    assert np.array_equal(shadow.cpu().numpy(), saved)                              # a restore writes no shadow byte


def test_empty_table_is_a_noop():
    from cavp_amd import _lib
    from cavp_amd.ops import _stream
    from cavp_amd.rollback import StepRollback
    lib = _lib.load()
    st = C.c_void_p(_stream())
    assert lib.cavp_rollback_save(None, 0, 0, None, st) == 0
    assert lib.cavp_rollback_restore(None, 0, 0, None, None, st) == 0
    assert lib.cavp_rollback_save(None, 3, 5, None, st) == _lib.ERR_BAD_ARG        # a table is required once there are ranges
    rb = StepRollback(DEV).freeze()
    rb.save()
    rb.restore()
    torch.cuda.synchronize()
    assert rb.stats() == {"saves": 0, "restores": 0} and rb.ranges() == [] and rb.registered_bytes() == {}


def test_captured_save_and_guarded_restore(rig):
    """graph = save -> the "iteration" (+1 on every range byte) -> restore(word), replayed three times with the word flipped in
    between: clear = the iteration stands, set = the replay did not happen (and the scrub ranges are zero)."""
    live = rig.live
    live.copy_(torch.from_numpy(rig.live0))
    rig.shadow.copy_(torch.from_numpy(rig.shadow0))
    rig.state.zero_()
    rig.word.zero_()
    inc = torch.from_numpy((rig.in_live | rig.in_scrub).astype(np.uint8)).to(DEV)
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        rig.save()
        live.add_(inc)
        rig.restore(rig.word)
    torch.cuda.synchronize()
    assert np.array_equal(live.cpu().numpy(), rig.live0) and rig.counters() == (0, 0)     # the capture ran nothing
    plus1, plus2 = rig.live0 + (rig.in_live | rig.in_scrub), rig.live0 + 2 * (rig.in_live | rig.in_scrub).astype(np.uint8)
    g.replay()                                                                      # word clear
    assert np.array_equal(live.cpu().numpy(), plus1)
    rig.word[0] = 1
    g.replay()                                                                      # word set: back to + 1, scrub ranges zero
    assert np.array_equal(live.cpu().numpy(), rig.expect(plus1, None))
    rig.word[0] = 0
    g.replay()
    want = rig.expect(plus2, np.ones_like(rig.live0))
    assert np.array_equal(live.cpu().numpy(), want)
    assert rig.counters() == (3, 1)


def test_step_rollback_object():
    """StepRollback on loose tensors: a slice of an f32 vector at an odd offset, half of an int64[4], an int32 vector, a 0-dim
    counter, a scrub buffer; restore_if_skipped reads an attached guard's skip word."""
    from cavp_amd.optim import StepGuard
    from cavp_amd.rollback import StepRollback
    g = torch.Generator(device=DEV).manual_seed(3)
    vec = torch.randn(5000, generator=g, device=DEV)
    state = torch.arange(4, dtype=torch.int64, device=DEV) + (1 << 40)
    head = torch.arange(7, dtype=torch.int32, device=DEV)
    count = torch.tensor(5, dtype=torch.int64, device=DEV)
    work = torch.full((300,), float("nan"), device=DEV)
    rb = StepRollback(DEV).add_tensor(vec, 4, 4 * 4500).add_tensor(state, 0, 16).add_tensor(head).add_tensor(count).add_scrub(work)
    assert rb.registered_bytes() == {"tensors": 18000 + 16 + 28 + 8, "scrub": 1200}
    rb.freeze()
    assert [v.numel() for v in rb.ranges()] == [18000, 16, 28, 8]
    guard = StepGuard()
    guard._attach(1, torch.device(DEV))
    before = [t.clone() for t in (vec, state, head, count)]
    rb.save()
    for t in (vec, state, head, count):
        t.add_(1)
    work.fill_(float("inf"))
    after = [t.clone() for t in (vec, state, head, count)]
    rb.restore_if_skipped(guard)                                                    # skip == 0: a no-op
    assert all(torch.equal(t, a) for t, a in zip((vec, state, head, count), after)) and torch.isinf(work).all()
    guard.last()["skip"].fill_(1)
    rb.restore_if_skipped(guard)
    assert torch.equal(vec[1:4501], before[0][1:4501]) and torch.equal(vec[:1], after[0][:1]) and torch.equal(vec[4501:], after[0][4501:])
    assert torch.equal(state[:2], before[1][:2]) and torch.equal(state[2:], after[1][2:])     # the diagnostic half stays
    assert torch.equal(head, before[2]) and torch.equal(count, before[3])
    assert torch.equal(work, torch.zeros_like(work))
    assert rb.stats() == {"saves": 1, "restores": 1}
    rb.reset_stats()
    assert rb.stats() == {"saves": 0, "restores": 0}


# --------------------------------------------------------------------------------------------------------------- end to end
def _iteration(rollback: bool, overwrite: bool = True):
    """The rig of test_whole_iteration_in_one_graph with a guarded optimiser: PairBuilder + MelFrontEnd prologue, CE + contrast on
    the device sampler, update, all in one graph; `rollback` adds a StepRollback over the model, the pair builder and the sampler.
    Returns a namespace; `snap` holds the buffers, bank, heads and counters from before the capture call."""
    import types
    from cavp_amd.audio_frontend import MelFrontEnd
    from cavp_amd.contrast import ContrastLoss
    from cavp_amd.optim import FusedSGDAdam, StepGuard
    from cavp_amd.pairs import PairBuilder, PairResult
    B, K, A = CFG3["B"], 3, 16000
    r = types.SimpleNamespace()
    image, audio0, label = synth_inputs(B, CFG3["hw"], audio_batch=2 * B, num_classes=K, seed=21)
    label[:, 8:40, 8:48] = 1
    label[:, 44:60, 4:60] = 2
    label[:, :4] = 255
    image_b = synth_inputs(B, CFG3["hw"], audio_batch=2 * B, num_classes=K, seed=22)[0]
    g = torch.Generator().manual_seed(3)
    r.batch_a = (image.to(DEV), (torch.randn(B, 1, A, generator=g) * 0.1).to(DEV))
    r.batch_b = (image_b.to(DEV), (torch.randn(B, 1, A, generator=g) * 0.1).to(DEV))
    poisoned = r.batch_b[0].clone()
    poisoned[1, 2, 17, 5] = float("nan")                         # ONE pixel of one frame
    r.batch_p = (poisoned, r.batch_b[1])
    r.clean = (r.batch_a[0], audio0[:B].contiguous().to(DEV))    # for the eval forward
    label = label.to(DEV)
    img_label = torch.tensor([[0, 1, 0], [0, 0, 1], [0, 1, 0], [1, 1, 1]], dtype=torch.int64, device=DEV)
    mel = MelFrontEnd(None, device=DEV)
    r.model, _ = _build(CFG3)
    r.model.train_step(r.batch_a[0], audio0.to(DEV), label)      # creates the arena the optimiser is built on
    r.opt = FusedSGDAdam(r.model, r.model._grad_arena, 1e-3, momentum=0.9, weight_decay=1e-4).use_device_schedule(1e-3, 0.9, 100)
    r.guard = StepGuard(history=16)
    r.opt.use_step_guard(r.guard)
    r.pairs = PairBuilder(num_classes=K, bank_slots=2, wave_len=A, ow_rate=0.5, seed=SEED, device=DEV, max_batch=B)
    r.crit = ContrastLoss(temperature=0.1, ignore_idx=255, max_views=32).use_device_sampler(4, seed=SEED)
    r.pairs._ensure()
    built = PairResult(B, A, K, CFG3["hw"], torch.device(DEV))
    r.image, r.wave = torch.zeros_like(r.batch_a[0]), torch.zeros_like(r.batch_a[1])
    audio, shuf = torch.zeros_like(audio0.to(DEV)), torch.zeros_like(label)
    r.image.copy_(r.batch_a[0])
    r.wave.copy_(r.batch_a[1])

    def prologue():
        r.pairs(r.wave, label, img_label, overwrite, out=built)
        audio.copy_(mel(built.waveforms))
        shuf.copy_(built.label_shuffle)

    # the static buffers and the stages must outlive this function: the graph holds their addresses, not references
    r.keep = (label, img_label, mel, built, audio, shuf, prologue)
    r.rb = None
    kw = {}
    if rollback:
        from cavp_amd.rollback import StepRollback
        r.rb = StepRollback(DEV).add_model(r.model).add(r.pairs).add(r.crit).freeze()
        kw["rollback"] = r.rb
    r.snap = _device_state(r)
    r.replay = r.model.capture_train_step(r.image, audio, label, contrast=r.crit, label_shuffle=shuf, optimizer=r.opt,
                                          prologue=prologue, **kw)
    torch.cuda.synchronize()
    return r


def _device_state(r):
    """everything an iteration's forward mutates: BatchNorm buffers, bank, ring heads, the two {seed, offset} pairs"""
    out = {"bn." + k: b.clone() for k, b in r.model.named_buffers()}
    out.update(bank=r.pairs._bank.clone(), head=r.pairs._head.clone(), pairs=r.pairs._state[:2].clone(), sampler=r.crit._dev[1][:2].clone())
    return out


def _trained_state(r):
    out = {"p." + k: p.detach().clone() for k, p in r.model.named_parameters()}
    out.update(m=r.opt.state_m.clone(), v=r.opt.state_v.clone(), t=r.opt._t_view.clone(), lr=r.opt.last_lr().clone())
    return out


def _run(r, batch):
    r.image.copy_(batch[0])
    r.wave.copy_(batch[1])
    loss = r.replay().clone()
    torch.cuda.synchronize()
    return loss


def _bits(t):
    """bytes of a tensor: NaN compares equal to the same NaN"""
    return t.detach().reshape(-1).contiguous().view(torch.uint8)


def _same(a, b):
    """keys whose tensors differ in any bit"""
    assert a.keys() == b.keys()
    return [k for k in a if not torch.equal(_bits(a[k]), _bits(b[k]))]


def test_poisoned_iteration_did_not_happen(deterministic):
    """Replays A, P (= B with one NaN pixel), B against a twin's A, B.  After P: skipped, one restore, every registered range and
    the trained state as after A, all BatchNorm buffers finite, the eval forward bit-equal to the one made after A.  After B:
    everything, the loss included, bit-equal to the twin's.  Before any replay: the capture left the device state where it was."""
    r, c = _iteration(True), _iteration(True)
    # warm-up undo: two real passes and the capture behind them left no trace, and the capture's own launches are not counted
    assert _same(_device_state(r), r.snap) == []
    assert int(r.snap["bn.backbone.backbone.bn1.num_batches_tracked"]) == 1 and r.opt.iteration() == 0
    assert r.rb.stats() == {"saves": 0, "restores": 0}
    groups = r.rb.registered_bytes()
    print(f"registered bytes: {groups}")
    assert groups["PairBuilder.bank"] == 3 * 2 * 16000 * 4 and groups["PairBuilder.state"] == 16 and groups["ContrastLoss.state"] == 16

    loss_a = _run(r, r.batch_a)
    assert torch.isfinite(loss_a).all() and r.opt.iteration() == 1
    after_a = ([v.clone() for v in r.rb.ranges()], _device_state(r), _trained_state(r))
    assert _same(after_a[1], r.snap) != []                        # the iteration did move the statistics, the bank, the counters
    r.model.eval()
    eval_a = [t.clone() for t in r.model.predict(*r.clean, return_prob=True)]
    r.model.train()
    assert torch.isfinite(eval_a[1]).all()

    loss_p = _run(r, r.batch_p)
    rec = r.guard.read()
    print(f"poisoned replay: loss {float(loss_p)}, skipped {rec['skipped'].tolist()}, non-finite gradient elements {rec['nonfinite'].tolist()}")
    assert rec["skipped"].tolist() == [False, True]
    assert r.rb.stats() == {"saves": 2, "restores": 1}
    assert all(torch.equal(v, w) for v, w in zip(r.rb.ranges(), after_a[0]))
    assert _same(_device_state(r), after_a[1]) == []
    assert all(torch.isfinite(b).all() for _, b in r.model.named_buffers())
    assert _same(_trained_state(r), after_a[2]) == [] and r.opt.iteration() == 1          # the guard's promise, re-checked
    r.model.eval()
    eval_p = r.model.predict(*r.clean, return_prob=True)
    r.model.train()
    assert torch.isfinite(eval_p[1]).all()
    assert torch.equal(eval_p[0], eval_a[0]) and torch.equal(eval_p[1], eval_a[1])

    loss_b = _run(r, r.batch_b)
    _run(c, c.batch_a)
    loss_c = _run(c, c.batch_b)
    print(f"losses: A {float(loss_a):.6f}, B after the poisoned replay {float(loss_b):.6f}, B on the twin {float(loss_c):.6f}")
    assert torch.isfinite(loss_b).all()
    assert torch.equal(_bits(loss_b), _bits(loss_c))
    assert _same(_device_state(r), _device_state(c)) == []
    assert _same(_trained_state(r), _trained_state(c)) == []
    sd_r, sd_c = r.model.state_dict(), c.model.state_dict()
    assert all(torch.equal(_bits(sd_r[k]), _bits(sd_c[k])) for k in sd_r)
    assert r.opt.iteration() == 2 and c.opt.iteration() == 2
    assert r.rb.stats() == {"saves": 3, "restores": 1} and c.rb.stats() == {"saves": 2, "restores": 0}


def test_gap_without_rollback(deterministic):
    """The gap the rollback closes, pinned: without `rollback=` the capture's warm-up passes stay in the statistics
    (num_batches_tracked == 3 after one eager step and the capture), and one poisoned replay, skipped by the guard, leaves a
    running_mean that is not finite."""
    r = _iteration(False)
    state = _device_state(r)
    assert int(state["bn.backbone.backbone.bn1.num_batches_tracked"]) == 3
    assert _same(state, r.snap) != []
    _run(r, r.batch_p)
    rec = r.guard.read()
    assert rec["skipped"].tolist() == [True]
    assert all(torch.isfinite(p).all() for p in r.model.parameters())             # the guard kept the weights ...
    assert not torch.isfinite(r.model.backbone.backbone.conv1[1].running_mean).all()             # ... and nobody kept the statistics
