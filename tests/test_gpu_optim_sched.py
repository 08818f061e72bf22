"""The device-resident optimiser schedule (struct cavp_opt_state, cavp_optimizer_schedule + cavp_optimizer_step_dev,
FusedSGDAdam.use_device_schedule) and CAVP.capture_train_step(optimizer=..., prologue=...): the schedule scalars against the host
arithmetic, the update against torch.optim and against the host-argument launch, checkpoints, and the update recorded in the
training graph(s)."""
import ctypes as C
import math

import numpy as np
import pytest
import torch

from cavp_amd.synth import synth_inputs
from tests.test_gpu_train_model import _build
from tests.test_optim import build_model, load_synth_weights

pytestmark = pytest.mark.gpu
DEV = "cuda:0"

# (start_lr, lr_power, total_iters, warmup_steps, end_lr): the defaults of use_device_schedule, and a set whose warm-up, poly
# range, clamp and end all lie within a few steps
DEFAULTS = (1e-3, 0.9, 1000, 0, 1e-8)
SHORT = (1e-2, 0.9, 4, 2, 1e-4)
BETAS = (0.9, 0.999)


def host_lr(t, consts):
    """The rate of step t as a host trainer computes it: the configured rate for step 0, then get_lr(t - 1) (the reference sets
    the rate after the step); get_lr(i) for i >= total_iters, outside the reference's domain, is defined as end_lr."""
    from cavp_amd.optim import warmup_poly_lr
    start, power, total, warm, end = consts
    if t == 0:
        return start
    cur = t - 1
    if cur >= warm and cur >= total:
        return end
    return warmup_poly_lr(start, power, total, warm, end)(cur)


def host_bias_corrections(t):
    """cavp_optimizer_step's host arithmetic for step count t + 1: the f32 betas widened to double."""
    b1, b2 = (float(np.float32(b)) for b in BETAS)
    return 1.0 - b1 ** float(t + 1), math.sqrt(1.0 - b2 ** float(t + 1))


def within_one_ulp(got, want64):
    want = np.float32(want64)
    return abs(float(np.float32(got)) - float(want)) <= float(np.spacing(np.abs(want)))


# --------------------------------------------------------------------------------------------------------- schedule scalars
@pytest.mark.parametrize("consts", [DEFAULTS, SHORT], ids=["defaults", "short"])
def test_schedule_scalars(consts):
    """cavp_optimizer_schedule on a bare state block.  t covers 0, 1, inside the warm-up, the first poly iteration, cur_iter ==
    total_iters - 1, == total_iters, > total_iters and 10^6 (beta^t underflows, the corrections saturate at 1).  Both sides
    compute in double with a sub-ulp pow, so only the final rounding to f32 can differ: one f32 ulp, derived, not measured."""
    from cavp_amd import _lib
    from cavp_amd.optim import OptState
    from cavp_amd.ops import _ptr, _stream
    lib = _lib.load()
    start, power, total, warm, end = consts
    ts = sorted({0, 1, 2, warm, warm + 1, total - 1, total, total + 1, total + 2, total + 7, 10 ** 6})
    for t in ts:
        host = OptState(t=t, total_iters=total, warmup_steps=warm, start_lr=start, lr_power=power, end_lr=end, base_lr=3e-4,
                        beta1=BETAS[0], beta2=BETAS[1], lr_sgd=-1.0, lr_adam=-1.0, bc1=-1.0, bc2_sqrt=-1.0, first_step=7)
        state = torch.frombuffer(bytearray(bytes(host)), dtype=torch.uint8).to(DEV)
        _lib.check(lib.cavp_optimizer_schedule(_ptr(state), C.c_void_p(_stream())), "cavp_optimizer_schedule")
        got = OptState.from_buffer_copy(state.cpu().numpy().tobytes())
        bc1, bc2_sqrt = host_bias_corrections(t)
        lr = host_lr(t, consts)
        print(f"t={t}: lr {got.lr_sgd:.9e} (host {lr:.9e}) bc1 {got.bc1:.9e} ({bc1:.9e}) bc2_sqrt {got.bc2_sqrt:.9e} ({bc2_sqrt:.9e})")
        assert within_one_ulp(got.lr_sgd, lr), (t, got.lr_sgd, lr)
        assert within_one_ulp(got.bc1, bc1), (t, got.bc1, bc1)
        assert within_one_ulp(got.bc2_sqrt, bc2_sqrt), (t, got.bc2_sqrt, bc2_sqrt)
        assert got.lr_adam == np.float32(3e-4)
        assert got.first_step == (1 if t == 0 else 0) and got.t == t + 1
        # the constants are untouched
        assert (got.total_iters, got.warmup_steps, got.start_lr, got.lr_power, got.end_lr) == (total, warm, start, power, end)
        if t == 10 ** 6:
            assert got.bc1 == 1.0 and got.bc2_sqrt == 1.0
    if consts is SHORT:
        assert host_lr(1, consts) == 0.0 and host_lr(5, consts) == end and host_lr(6, consts) == end


# ----------------------------------------------------------------------------------------------------------------- op level
def _op_model():
    from cavp_amd.train import GradArena
    m = build_model(num_classes=3, lds=[False, False, False], batch=2)
    load_synth_weights(m, seed=1)
    m = m.to(DEV)
    return m, GradArena(list(m.parameters()), DEV)


def _worst(m, ref):
    """the metric of test_fused_optimizer_vs_torch_optim: max |difference| over a tensor, relative to its largest magnitude"""
    worst = 0.0
    for k, p in m.named_parameters():
        r = ref[k].detach().cpu()
        worst = max(worst, float((p.detach().cpu() - r).abs().max()) / (1e-6 + float(r.abs().max())))
    return worst


def test_device_schedule_vs_torch_optim():
    """7 steps of SHORT against torch.optim.SGD + Adam on the CPU driven by the host schedule with the t - 1 rule: the start rate,
    a zero-rate warm-up step, mid warm-up, two poly steps, the clamp, past the end.  Metric and bar (2e-6) of
    test_fused_optimizer_vs_torch_optim; one ulp in a scalar is 1.2e-7 of an update."""
    from cavp_amd.optim import FusedSGDAdam, set_group_lr
    m, arena = _op_model()
    ref = {k: p.detach().cpu().clone().requires_grad_(True) for k, p in m.named_parameters()}
    names = {id(p): k for k, p in m.named_parameters()}
    lr0, mom, wd = SHORT[0], 0.9, 1e-3
    groups = [dict({kk: vv for kk, vv in g.items() if kk != "params"}, params=[ref[names[id(p)]] for p in g["params"]],
                   lr=g["lr"] * lr0) for g in set_group_lr(m, 1.0)]
    opt_v = torch.optim.SGD(groups, lr=lr0, momentum=mom, weight_decay=wd)
    opt_a = torch.optim.Adam([ref["audio_backbone." + k] for k, _ in m.audio_backbone.named_parameters()], lr=lr0)
    fused = FusedSGDAdam(m, arena, lr0, momentum=mom, weight_decay=wd).use_device_schedule(*SHORT)
    never = {id(p) for p in m.params_without_grad()}
    gen = torch.Generator(device=DEV).manual_seed(5)
    rates = []
    for it in range(7):
        lr = host_lr(it, SHORT)
        arena.flat.copy_(torch.randn(arena.flat.numel(), generator=gen, device=DEV) * 0.1)
        for k, p in m.named_parameters():
            ref[k].grad = None if id(p) in never else arena.views[id(p)].detach().cpu().clone()
        for i, g in enumerate(opt_v.param_groups):
            g["lr"] = lr * (1.0 if i < 4 else 10.0)
        opt_v.step()
        opt_a.step()
        fused.step()
        rates.append(float(fused.last_lr().item()))
        assert within_one_ulp(rates[-1], lr), (it, rates[-1], lr)
        worst = _worst(m, ref)
        print(f"step {it}: lr {rates[-1]:.6e}, worst relative difference {worst:.3e}")
        assert worst <= 2e-6, (it, worst)
    assert rates[1] == 0.0 and rates[5] == rates[6] == float(np.float32(SHORT[4]))
    assert fused.iteration() == 7 and fused.steps == 7


def _sgd_adam_split(m, opt):
    """[(name, parameter, momentum slice, is_adam)] in the optimiser's order (state offsets as FusedSGDAdam lays them out)"""
    names = {id(p): k for k, p in m.named_parameters()}
    audio = {id(p) for p in m.audio_backbone.parameters()}
    out, off = [], 0
    for p in opt.params:
        out.append((names[id(p)], p, opt.state_m[off:off + p.numel()], id(p) in audio))
        off += (p.numel() + 3) // 4 * 4
    return out


def test_device_step_is_bit_identical_to_host_argument_step():
    """Two optimisers on identical parameters and gradients: step() against step(float(last_lr())).  The SGD groups get the same
    f32 rate and flag through one shared device function: parameters and momentum buffers are torch.equal, unconditionally.
    Adam's tensors are held to the 2e-6 bar only."""
    from cavp_amd.optim import FusedSGDAdam
    (m1, a1), (m2, a2) = _op_model(), _op_model()
    consts = (1e-2, 0.9, 100, 0, 1e-8)
    o1 = FusedSGDAdam(m1, a1, 1e-2, momentum=0.9, weight_decay=1e-3).use_device_schedule(*consts)
    o2 = FusedSGDAdam(m2, a2, 1e-2, momentum=0.9, weight_decay=1e-3)
    gen = torch.Generator(device=DEV).manual_seed(6)
    for it in range(3):
        g = torch.randn(a1.flat.numel(), generator=gen, device=DEV) * 0.1
        a1.flat.copy_(g)
        a2.flat.copy_(g)
        o1.step()
        o2.step(float(o1.last_lr().item()))
    torch.cuda.synchronize()
    n_sgd = n_adam = 0
    for (k, p1, b1, adam), (_, p2, b2, _) in zip(_sgd_adam_split(m1, o1), _sgd_adam_split(m2, o2)):
        if adam:
            n_adam += 1
            d = float((p1 - p2).detach().abs().max()) / (1e-6 + float(p2.detach().abs().max()))
            assert d <= 2e-6, (k, d)
        else:
            n_sgd += 1
            assert torch.equal(p1, p2), k
            assert torch.equal(b1, b2), k
    assert n_sgd > 100 and n_adam > 10
    assert o1.iteration() == 3 and o2.steps == 3


def test_checkpoint_restores_the_device_counter():
    """After 2 steps, state_dict() into a fresh optimiser on a copy of the model; one more step on the same gradients: equal
    parameters and state, iteration() == 3.  A dict without "t" (written before the device schedule) keeps loading."""
    from cavp_amd.optim import FusedSGDAdam
    (m1, a1), (m2, a2) = _op_model(), _op_model()
    o1 = FusedSGDAdam(m1, a1, 1e-2, momentum=0.9, weight_decay=1e-3).use_device_schedule(*SHORT)
    gen = torch.Generator(device=DEV).manual_seed(8)
    for it in range(2):
        a1.flat.copy_(torch.randn(a1.flat.numel(), generator=gen, device=DEV) * 0.1)
        o1.step()
    sd = o1.state_dict()
    assert sd["t"] == 2 and sd["steps"] == 2
    m2.load_state_dict(m1.state_dict())
    o2 = FusedSGDAdam(m2, a2, 1e-2, momentum=0.9, weight_decay=1e-3).use_device_schedule(*SHORT)
    o2.load_state_dict(sd)
    assert o2.iteration() == 2
    g = torch.randn(a1.flat.numel(), generator=gen, device=DEV) * 0.1
    a1.flat.copy_(g)
    a2.flat.copy_(g)
    o1.step()
    o2.step()
    torch.cuda.synchronize()
    for (k, p1), (_, p2) in zip(m1.named_parameters(), m2.named_parameters()):
        assert torch.equal(p1, p2), k
    assert torch.equal(o1.state_m, o2.state_m) and torch.equal(o1.state_v, o2.state_v)
    assert torch.equal(o1.last_lr(), o2.last_lr())
    assert o1.iteration() == 3 and o2.iteration() == 3
    old = {k: v for k, v in sd.items() if k != "t"}
    o2.load_state_dict(old)
    assert o2.iteration() == 2
    o3 = FusedSGDAdam(m2, a2, 1e-2)          # host-scheduled optimiser: takes the same dict
    o3.load_state_dict(sd)
    assert o3.steps == 2


# ------------------------------------------------------------------------------------------------------------ captured step
CFG2 = dict(C=2, B=4, hw=(64, 64), lds=[False, False, False])
CAP = (1e-3, 0.9, 10, 0, 1e-8)


def _with_optimizer(cfg, seed, consts=CAP, lr=1e-3):
    """model, inputs and a device-scheduled optimiser on the model's arena (which the first train_step creates)"""
    from cavp_amd.optim import FusedSGDAdam
    B = cfg["B"]
    image, audio, label = [t.to(DEV) for t in synth_inputs(B, cfg["hw"], audio_batch=2 * B, num_classes=cfg["C"], seed=seed)]
    m, _ = _build(cfg)
    m.train_step(image, audio, label)
    opt = FusedSGDAdam(m, m._grad_arena, lr, momentum=0.9, weight_decay=1e-4).use_device_schedule(*consts)
    return m, opt, (image, audio, label)


def _state(m):
    return {k: v.clone() for k, v in m.state_dict().items()}


def test_captured_step_with_optimizer(deterministic):
    """One model, two captures: rA with the update recorded, rB without.  The capture itself trains nothing; three replays of rA
    equal three times (rB, eager step()) bit for bit in fixed-order mode - both routes run the same kernels on the same scalars,
    so a difference means the recorded update read the arena before a stream was joined; the logged rates follow the host
    schedule; a fourth replay sees the updated weights."""
    m, opt, (image, audio, label) = _with_optimizer(CFG2, seed=11)
    before = [p.detach().clone() for p in m.parameters()]
    rA = m.capture_train_step(image, audio, label, optimizer=opt)
    assert len(m._train_graph) == 1
    torch.cuda.synchronize()
    assert all(torch.equal(p, b) for p, b in zip(m.parameters(), before))
    assert opt.iteration() == 0
    rB = m.capture_train_step(image, audio, label)
    assert all(torch.equal(p, b) for p, b in zip(m.parameters(), before)) and opt.iteration() == 0
    snap, snap_opt = _state(m), opt.state_dict()
    rates, losses_a = [], []
    for it in range(3):
        losses_a.append(float(rA().item()))
        rates.append(float(opt.last_lr().item()))
    assert opt.iteration() == 3
    assert all(p.grad is None or p.grad.data_ptr() == m._grad_arena.views[id(p)].data_ptr() for p in m.parameters())
    route_a, m_a, v_a = _state(m), opt.state_m.clone(), opt.state_v.clone()
    l4 = float(rA().item())
    m.load_state_dict(snap)
    opt.load_state_dict(snap_opt)
    opt.set_iteration(0)
    losses_b = []
    for it in range(3):
        losses_b.append(float(rB().item()))
        opt.step()
    torch.cuda.synchronize()
    assert opt.iteration() == 3
    route_b = _state(m)
    print(f"losses, recorded update {losses_a} + {l4}; replay + eager step {losses_b}; rates {rates}")
    for k in route_a:
        assert torch.equal(route_a[k], route_b[k]), k
    assert torch.equal(m_a, opt.state_m) and torch.equal(v_a, opt.state_v)
    assert losses_a == losses_b
    for it, r in enumerate(rates):
        assert within_one_ulp(r, host_lr(it, CAP)), (it, r)
    assert any(not torch.equal(route_a[k], snap[k]) for k, _ in m.named_parameters())
    assert abs(l4 - losses_a[2]) > 1e-6 * abs(l4) and abs(losses_a[1] - losses_a[0]) > 1e-6 * abs(l4)


def test_split_capture_with_optimizer():
    """split=True (two graphs, the update at the end of the second) against split=False from one snapshot, one replay each: the
    bars of test_split_graph_capture_matches_single_graph on the SGD groups' weight update p_after - p_before."""
    m1, o1, (image, audio, label) = _with_optimizer(CFG2, seed=12, consts=(1e-2, 0.9, 100, 0, 1e-8), lr=1e-2)
    m2, o2, _ = _with_optimizer(CFG2, seed=12, consts=(1e-2, 0.9, 100, 0, 1e-8), lr=1e-2)
    r1 = m1.capture_train_step(image, audio, label, split=False, optimizer=o1)
    r2 = m2.capture_train_step(image, audio, label, split=True, optimizer=o2)
    assert len(m2._train_graph) == 2 and len(m1._train_graph) == 1
    assert o1.iteration() == 0 and o2.iteration() == 0
    sd = _state(m1)
    m1.load_state_dict(sd)
    m2.load_state_dict(sd)

    def sgd_flat(m, o):
        return torch.cat([p.detach().double().flatten() for _, p, _, adam in _sgd_adam_split(m, o) if not adam])
    p0 = sgd_flat(m1, o1)
    assert torch.equal(p0, sgd_flat(m2, o2))
    l1, l2 = float(r1().item()), float(r2().item())
    torch.cuda.synchronize()
    assert abs(l1 - l2) <= 1e-4 * abs(l1), (l1, l2)
    a, b = sgd_flat(m1, o1) - p0, sgd_flat(m2, o2) - p0
    assert float(a.norm()) > 0.0
    cos = float((a @ b) / (a.norm() * b.norm()))
    print(f"split capture: weight-update cosine {cos:.6f}, norm ratio {float(a.norm() / b.norm()):.6f}")
    assert cos >= 0.9995 and abs(float(a.norm() / b.norm()) - 1.0) <= 5e-3, cos
    assert o1.iteration() == 1 and o2.iteration() == 1
    assert all(torch.isfinite(p).all() for p in m2.parameters())


# ---------------------------------------------------------------------------------------------------------- whole iteration
CFG3 = dict(C=3, B=4, hw=(64, 64), lds=[False, False, False])
SEED = 1234


def test_whole_iteration_in_one_graph():
    """PairBuilder + MelFrontEnd (prologue) + forward + CE + contrast (device sampler) + backward + update as ONE graph.  After
    reseeding the pair builder and the sampler the first replay's loss is within 5e-3 of the eager sequence on a twin (the bar of
    test_captured_step_replays_with_fresh_anchors); the pair builder's call offset advances by one per replay; four replays leave
    every parameter finite and every tensor the optimiser owns different from the start (the parameters of params_without_grad()
    never receive a gradient, are not the optimiser's, and stay)."""
    from cavp_amd.audio_frontend import MelFrontEnd
    from cavp_amd.contrast import ContrastLoss
    from cavp_amd.optim import FusedSGDAdam
    from cavp_amd.pairs import PairBuilder, PairResult
    B, K, A = CFG3["B"], 3, 16000
    image, audio0, label = synth_inputs(B, CFG3["hw"], audio_batch=2 * B, num_classes=K, seed=21)
    label[:, 8:40, 8:48] = 1
    label[:, 44:60, 4:60] = 2
    label[:, :4] = 255
    image, audio0, label = image.to(DEV), audio0.to(DEV), label.to(DEV)
    g = torch.Generator().manual_seed(3)
    wave = (torch.randn(B, 1, A, generator=g) * 0.1).to(DEV)
    img_label = torch.tensor([[0, 1, 0], [0, 0, 1], [0, 1, 0], [1, 1, 1]], dtype=torch.int64, device=DEV)
    mel = MelFrontEnd(None, device=DEV)

    def crit_of(seed):
        return ContrastLoss(temperature=0.1, ignore_idx=255, max_views=32).use_device_sampler(4, seed=seed)

    def builder_of(seed):
        return PairBuilder(num_classes=K, bank_slots=2, wave_len=A, ow_rate=0.5, seed=seed, device=DEV, max_batch=B)

    # eager twin
    m1, sd0 = _build(CFG3)
    pb1, crit1 = builder_of(SEED), crit_of(SEED)
    built1 = pb1(wave, label, img_label, False)
    l1 = m1.train_step(image, mel(built1.waveforms), label, contrast=crit1, label_shuffle=built1.label_shuffle)
    # captured
    m2, _ = _build(CFG3)
    m2.train_step(image, audio0, label)                      # creates the arena the optimiser is built on
    opt = FusedSGDAdam(m2, m2._grad_arena, 1e-3, momentum=0.9, weight_decay=1e-4).use_device_schedule(1e-3, 0.9, 100)
    pb2, crit2 = builder_of(0), crit_of(0)
    built = PairResult(B, A, K, CFG3["hw"], torch.device(DEV))
    audio, shuf = torch.zeros_like(audio0), torch.zeros_like(label)

    def prologue():
        pb2(wave, label, img_label, False, out=built)
        audio.copy_(mel(built.waveforms))
        shuf.copy_(built.label_shuffle)

    replay = m2.capture_train_step(image, audio, label, contrast=crit2, label_shuffle=shuf, optimizer=opt, prologue=prologue)
    assert len(m2._train_graph) == 1
    assert opt.iteration() == 0
    m2.load_state_dict(sd0)
    pb2.manual_seed(SEED)
    crit2.manual_seed(SEED)
    start = {k: p.detach().clone() for k, p in m2.named_parameters()}
    l2 = float(replay().item())
    offsets = [pb2.last_plan()["offset"]]
    print(f"whole iteration: eager {float(l1.item()):.6f}, first replay {l2:.6f} (contrast term {float(m2._last_losses[1].item()):.6f})")
    assert float(m2._last_losses[1].item()) > 0.0
    assert abs(float(l1.item()) - l2) <= 5e-3
    assert torch.equal(built.label_shuffle, built1.label_shuffle) and torch.equal(audio, mel(built1.waveforms))
    for _ in range(3):
        replay()
        offsets.append(pb2.last_plan()["offset"])
    torch.cuda.synchronize()
    assert offsets == [0, 1, 2, 3], offsets
    assert opt.iteration() == 4
    owned = {id(p) for p in opt.params}
    assert len(owned) > 200
    for k, p in m2.named_parameters():
        assert torch.isfinite(p).all(), k
        if id(p) in owned:
            assert not torch.equal(p, start[k]), f"{k} did not move in four steps"
        else:
            assert torch.equal(p, start[k]), f"{k} is not the optimiser's and moved"


# ------------------------------------------------------------------------------------------------------------------- errors
def test_errors_raise_before_any_launch():
    from cavp_amd._lib import CavpError
    from cavp_amd.optim import FusedSGDAdam
    m, opt, (image, audio, label) = _with_optimizer(CFG2, seed=13)
    other, other_opt, _ = _with_optimizer(CFG2, seed=13)
    plain = FusedSGDAdam(m, m._grad_arena, 1e-3)
    before = [p.detach().clone() for p in m.parameters()]
    stats = {k: b.clone() for k, b in m.named_buffers()}
    with pytest.raises(CavpError):
        m.capture_train_step(image, audio, label, optimizer=plain)          # no device schedule
    with pytest.raises(CavpError):
        opt.step(1e-3)                                                      # the schedule is on the device
    with pytest.raises(CavpError):
        plain.step()                                                        # no schedule at all
    with pytest.raises(CavpError):
        m.capture_train_step(image, audio, label, optimizer=other_opt)      # another model's arena
    with pytest.raises(CavpError):
        plain.last_lr()
    torch.cuda.synchronize()
    assert all(torch.equal(p, b) for p, b in zip(m.parameters(), before))
    assert all(torch.equal(b, stats[k]) for k, b in m.named_buffers())      # not even a warm-up pass ran
    assert opt.iteration() == 0 and other_opt.iteration() == 0 and plain.steps == 0
    assert getattr(m, "_train_graph", None) is None
