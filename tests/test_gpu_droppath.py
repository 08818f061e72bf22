"""DropPath masks drawn on the device (csrc/pvt_train.hip cavp_drop_path_draw, cavp_amd/droppath.py): the kernel
against the numpy restatement of its rule (tests/_droppath_ref.py) bit for bit, a graph holding one draw, and the PVT model with
the sampler - eager step, captured step, rollback, the cases that draw nothing, the graphed autograd node.  Smallest PVT set-up of
tests/test_gpu_pvt_train.py: C = 5, B = 2, 64 x 64, f32."""
import ctypes
import types

import numpy as np
import pytest
import torch

from cavp_amd.synth import synth_inputs, synth_state_dict
from tests import _droppath_ref as R

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
C_, B_, HW = 5, 2, (64, 64)
CANARY = -7.5


def _i32(t):
    return (t.detach().cpu().numpy() if isinstance(t, torch.Tensor) else np.asarray(t)).astype(np.float32, copy=False).view(np.int32)


def _bits_equal(a, b):
    a, b = _i32(a), _i32(b)
    return a.shape == b.shape and bool(np.array_equal(a, b))


def _b5_probs():
    """The drop probabilities of PVTv2-B5's 104 branches as the backbone computes them (pvt.py: linspace over the 52 blocks)."""
    dpr = [x.item() for x in torch.linspace(0, 0.1, 52)]
    return [p for p in dpr for _ in range(2)]


def _probs(n):
    if n == 102:
        return [p for p in _b5_probs() if p > 0]
    return [float(p) for p in np.linspace(0.03, 0.6, n)]


def _raw_draw(state, keep_d, inv_d, n, B, out):
    from cavp_amd import _lib
    p = lambda t: ctypes.c_void_p(t.data_ptr())
    st = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
    _lib.check(_lib.load().cavp_drop_path_draw(p(state), p(keep_d), p(inv_d), n, B, p(out), st), "cavp_drop_path_draw")


@pytest.mark.parametrize("seed,offset", [(0, 0), ((1 << 32) + 12345, 3), (-987654321, 7), (5, (1 << 32) - 1)],
                         ids=["seed0", "seed_ge_2p32", "seed_negative", "offset_crosses_low_word"])
@pytest.mark.parametrize("n,B", [(1, 1), (102, 2), (102, 5), (7, 64)])
def test_kernel_matches_reference_bit_for_bit(n, B, seed, offset):
    keep, inv = R.keep_tables(_probs(n))
    assert keep.shape == (n,)
    keep_d, inv_d = torch.from_numpy(keep).to(DEV), torch.from_numpy(inv).to(DEV)
    state = torch.tensor([seed, offset], dtype=torch.int64, device=DEV)
    pad = 37
    big = torch.full((pad + n * B + pad,), CANARY, dtype=torch.float32, device=DEV)
    out = big[pad:pad + n * B].view(n, B)
    for call in range(2):
        _raw_draw(state, keep_d, inv_d, n, B, out)
        torch.cuda.synchronize()
        assert _bits_equal(out, R.ref_scales(seed, offset + call, keep, inv, B)), (n, B, seed, offset + call)
        assert state.tolist() == [seed, offset + call + 1]            # the offset advances by exactly 1 per call, the seed stays
        assert bool((big[:pad] == CANARY).all()) and bool((big[pad + n * B:] == CANARY).all())   # nothing outside [n, B] is written


def test_graph_holding_one_draw():
    from cavp_amd.droppath import DropPathSampler
    probs, B, seed = _probs(102), 3, 21
    keep, inv = R.keep_tables(probs)
    dp = DropPathSampler(seed=seed, device=DEV)
    out = torch.empty((len(probs), B), dtype=torch.float32, device=DEV)
    dp.draw(probs, B, out)                      # first use: allocates the state and uploads the tables (not legal in a capture)
    torch.cuda.synchronize()
    assert _bits_equal(out, R.ref_scales(seed, 0, keep, inv, B))
    o = dp.offset()
    assert o == 1
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        dp.draw(probs, B, out)
    assert dp.offset() == o                     # a capture runs nothing
    for i in range(3):
        g.replay()
        torch.cuda.synchronize()
        assert _bits_equal(out, R.ref_scales(seed, o + i, keep, inv, B)), i
    assert dp.offset() == o + 3
    dp.manual_seed(seed)                        # in place: the graph captured earlier sees it
    g.replay()
    torch.cuda.synchronize()
    assert _bits_equal(out, R.ref_scales(seed, 0, keep, inv, B)) and dp.offset() == 1


# ---------------------------------------------------------------------------------------------------------------- the model
class _Rig:
    pass


@pytest.fixture(scope="module")
def rig():
    from cavp_amd.cavp_model import CAVP
    args = types.SimpleNamespace(seg_model="PVT", last_three_dilation_stride=[False, False, False], audio_backbone="vgg",
                                 num_classes=C_, batch_size=B_, local_rank="cpu", allow_random_pvt=True)
    r = _Rig()
    r.m = CAVP(50, None, num_classes=C_, args=args)
    r.sd = synth_state_dict({k: tuple(v.shape) for k, v in r.m.state_dict().items()}, seed=1)
    r.m.load_state_dict(r.sd, strict=True)
    r.m.train().to(DEV).set_compute_dtype(torch.float32)
    r.image, r.audio, r.label = [t.to(DEV) for t in synth_inputs(B_, HW, audio_batch=2 * B_, num_classes=C_, seed=4)]
    bb = r.m.backbone
    r.probs = [blk.drop_prob for i in range(4) for blk in getattr(bb, f"block{i + 1}") for _ in range(2)]
    r.n = sum(1 for p in r.probs if p > 0)
    assert r.n == len(r.probs) - 2 == 2 * sum(bb.depths) - 2       # every branch but block 0's two
    r.keep, r.inv = R.keep_tables(r.probs)
    yield r
    r.m.use_device_drop_path(None)


def _reset_bn(r):
    r.m.load_state_dict({k: v for k, v in r.sd.items() if "running_" in k or "num_batches" in k}, strict=False)


def _ref(r, seed, offset):
    return R.ref_scales(seed, offset, r.keep, r.inv, B_)


def _forbid_host_refresh(monkeypatch):
    from cavp_amd import pvt_train

    def boom(*a, **k):
        raise AssertionError("refresh_drop_path was called although a device sampler is set")
    monkeypatch.setattr(pvt_train, "refresh_drop_path", boom)


def test_eager_step_equals_step_with_reference_masks(rig):
    from cavp_amd import _lib
    r, m, seed = rig, rig.m, 11
    _lib.set_deterministic(True, device=torch.device(DEV))
    try:
        dp = m.use_device_drop_path(seed=seed)
        assert m.use_device_drop_path(seed=seed) is not dp and m.backbone._dp_sampler is not dp   # a new sampler replaces the old
        dp = m.backbone._dp_sampler
        _reset_bn(r)
        m.train_step(r.image, r.audio, r.label, all_reduce=False)      # first use (state, tables); also moves the offset off 0
        o = dp.offset()
        assert o == 1
        _reset_bn(r)
        rng = torch.get_rng_state()
        l1 = m.train_step(r.image, r.audio, r.label, all_reduce=False).clone()
        g1 = m._grad_arena.flat.clone()
        assert dp.offset() == o + 1
        assert torch.equal(torch.get_rng_state(), rng)                 # the host generator is not consumed
        # the same step with the reference's masks for that offset as the override: launches nothing, same bits
        ref = torch.from_numpy(_ref(r, seed, o)).to(DEV)
        rows = iter(ref)
        m._pvt_drop_scales = [next(rows) if p > 0 else None for p in r.probs]
        _reset_bn(r)
        l2 = m.train_step(r.image, r.audio, r.label, all_reduce=False).clone()
        g2 = m._grad_arena.flat.clone()
        torch.cuda.synchronize()
        assert dp.offset() == o + 1                                    # the override wins and leaves the offset alone
        assert bool(torch.isfinite(l1).all()) and bool(torch.isfinite(g1).all())
        assert _bits_equal(l1, l2), (float(l1), float(l2))
        assert _bits_equal(g1, g2), float((g1 - g2).abs().max())
    finally:
        m._pvt_drop_scales = None
        m.use_device_drop_path(None)
        _lib.set_deterministic(False)


def test_captured_step_draws_its_own_masks(rig, monkeypatch):
    r, m, seed = rig, rig.m, 3
    dp = m.use_device_drop_path(seed=seed)
    try:
        _forbid_host_refresh(monkeypatch)
        _reset_bn(r)
        step = m.capture_train_step(r.image, r.audio, r.label)
        o = dp.offset()          # where the capture left it (the warm-up passes drew for real; documented in capture_train_step)
        print("device DropPath: offset after capture_train_step without rollback =", o)
        rng = torch.get_rng_state()
        losses, masks = [], []
        for i in range(3):
            _reset_bn(r)
            losses.append(float(step().item()))
            torch.cuda.synchronize()
            masks.append(_ref(r, seed, o + i))
            assert _bits_equal(m.backbone._dp_buf, masks[-1]), i
            assert dp.offset() == o + i + 1
        assert all(np.isfinite(l) for l in losses)
        for i, j in ((0, 1), (0, 2), (1, 2)):
            assert not np.array_equal(masks[i], masks[j])
            assert abs(losses[i] - losses[j]) > 1e-7, (losses, i, j)    # other masks, another loss
        for s in (seed, 1 << 40):                                     # manual_seed between replays restarts the sequence
            dp.manual_seed(s)
            for i in range(2):
                _reset_bn(r)
                step()
                torch.cuda.synchronize()
                assert _bits_equal(m.backbone._dp_buf, _ref(r, s, i)), (s, i)
            assert dp.offset() == 2
        assert torch.equal(torch.get_rng_state(), rng)                 # replays leave the host generator alone
    finally:
        m.use_device_drop_path(None)


def test_rollback_covers_the_sampler(rig):
    from cavp_amd.optim import FusedSGDAdam, StepGuard
    from cavp_amd.rollback import StepRollback
    r, m, seed = rig, rig.m, 17
    dp = m.use_device_drop_path(seed=seed)
    try:
        probs = [p for p in r.probs if p > 0]
        out = torch.empty((r.n, B_), dtype=torch.float32, device=DEV)
        dp.draw(probs, B_, out)
        rb = StepRollback(DEV).add(dp).freeze()
        o = dp.offset()
        rb.save()
        dp.draw(probs, B_, out)
        first = out.clone()
        assert dp.offset() == o + 1
        rb.restore()
        assert dp.offset() == o                                        # the offset is back ...
        dp.draw(probs, B_, out)
        torch.cuda.synchronize()
        assert _bits_equal(out, first) and _bits_equal(out, _ref(r, seed, o))   # ... and the next draw repeats the rows
        # the captured step with rollback= undoes its own warm-up passes: the offset is where it was
        _reset_bn(r)
        arena = m.grad_arena(torch.device(DEV))
        opt = FusedSGDAdam(m, arena, 1e-6, momentum=0.9, weight_decay=0.0).use_device_schedule(1e-6, 0.9, 100)
        opt.use_step_guard(StepGuard(history=4))
        rb2 = StepRollback(DEV).add_model(m).add(dp).freeze()
        before = dp.offset()
        step = m.capture_train_step(r.image, r.audio, r.label, optimizer=opt, rollback=rb2)
        assert dp.offset() == before
        step()
        torch.cuda.synchronize()
        assert _bits_equal(m.backbone._dp_buf, _ref(r, seed, before)) and dp.offset() == before + 1   # a step that was not skipped
    finally:
        m.use_device_drop_path(None)
        m.load_state_dict(r.sd, strict=True)      # the replay above updated the weights
        m.params_changed()


def test_eval_backbone_and_override_draw_nothing(rig, monkeypatch):
    from cavp_amd.droppath import DropPathSampler
    r, m = rig, rig.m
    dp = m.use_device_drop_path(seed=9)
    try:
        _reset_bn(r)
        m.train_step(r.image, r.audio, r.label, all_reduce=False)
        o = dp.offset()
        assert o == 1

        def boom(*a, **k):
            raise AssertionError("a draw was launched")
        monkeypatch.setattr(DropPathSampler, "draw", boom)
        m.backbone.eval()
        try:
            loss = m.train_step(r.image, r.audio, r.label, all_reduce=False)
            assert bool(torch.isfinite(loss).all()) and dp.offset() == o
        finally:
            m.backbone.train()
        ones = torch.ones(B_, dtype=torch.float32, device=DEV)
        m._pvt_drop_scales = [ones if p > 0 else None for p in r.probs]
        loss = m.train_step(r.image, r.audio, r.label, all_reduce=False)
        assert bool(torch.isfinite(loss).all()) and dp.offset() == o
    finally:
        m._pvt_drop_scales = None
        m.use_device_drop_path(None)


def test_graphed_autograd_with_the_sampler(rig, monkeypatch):
    from cavp_amd import train_ops as T
    r, m, seed = rig, rig.m, 29
    dp = m.use_device_drop_path(seed=seed)
    m.enable_graphed_autograd()
    try:
        _forbid_host_refresh(monkeypatch)
        _reset_bn(r)
        rng = torch.get_rng_state()
        for call in range(2):
            out, fus, pack = m(r.image, r.audio, None, False)
            assert len(m._graphed_autograd) == 1                       # captured, not the eager fall-back
            off = dp.offset()
            assert _bits_equal(m.backbone._dp_buf, _ref(r, seed, off - 1)), call   # the masks of the replay that just ran
            loss, dl = T.ce_loss(out.detach(), r.label, B_)
            out.backward(dl)
            torch.cuda.synchronize()
            assert dp.offset() == off                                  # the backward graph draws nothing
            g = dict(m.named_parameters())["backbone.block3.20.attn.kv.weight"].grad
            assert np.isfinite(float(loss.item())) and g is not None and bool(torch.isfinite(g).all()) and float(g.abs().max()) > 0
            m.zero_grad(set_to_none=True)
        assert torch.equal(torch.get_rng_state(), rng)
    finally:
        m.enable_graphed_autograd(False)
        m.use_device_drop_path(None)
