"""Plain-torch restatement of the ResNet-18 audio encoder IN TRAINING (tests/_audio18_ref.py restates its eval forward): the same graph
with F.batch_norm(training=True) - batch statistics, running statistics updated with momentum 0.1 and the unbiased variance,
num_batches_tracked + 1 - or with frozen statistics (every module in eval(), gradients still flowing), and F.adaptive_max_pool2d, whose
backward sends the gradient to the FIRST maximum in (h, w) scan order.  Runs in the dtype asked for (float64 for expected values)
under torch.autograd.  For the whole model it is composed with oracle.cavp_oracle's backbone / feature / fusion / head stages, as
tests/test_gpu_audio18.py composes them for eval.  CPU only; shared by tests/test_audio18_train_host.py and
tests/test_gpu_audio18_train.py."""
from __future__ import annotations

import functools

import torch
import torch.nn.functional as F

from tests._audio18_ref import EPS, PREFIX, args18, audio_input  # noqa: F401

MOM = 0.1
TAP = 2e-4                      # the project's tap bound: TAP * max(1, max|ref|) (tests/test_gpu_model.py)
# (shape, audio_input seed): inputs whose global max does not hang on which of two near-equal values wins (margin_report below)
ENCODER_INPUTS = (((4, 2, 37, 20), 37), ((2, 2, 75, 32), 5), ((2, 1, 75, 32), 4))


def bn_names(p=PREFIX):
    """the 20 BatchNorm modules of the encoder, in forward order"""
    out = [p + ".bn1"]
    for li in range(1, 5):
        for bi in range(2):
            q = f"{p}.layer{li}.{bi}"
            out.append(q + ".bn1")
            if bi == 0 and li > 1:
                out.append(q + ".downsample.1")
            out.append(q + ".bn2")
    return out


def split_state(sd, dtype, p=PREFIX):
    """(params with requires_grad, buffers) of the encoder's part of a state_dict, both in `dtype` (counters stay int64), keyed
    relative to the encoder."""
    params, bufs = {}, {}
    for k, v in sd.items():
        if not k.startswith(p + "."):
            continue
        r = k[len(p) + 1:]
        if "running_" in r or r.endswith("num_batches_tracked"):
            bufs[r] = v.clone().to(dtype) if v.is_floating_point() else v.clone()
        else:
            params[r] = v.detach().clone().to(dtype).requires_grad_(True)
    return params, bufs


def _bn(x, P, B, q, bn_train):
    """bn_train: F.batch_norm updates B's running statistics in place, like the module"""
    if bn_train:
        y = F.batch_norm(x, B[q + ".running_mean"], B[q + ".running_var"], P[q + ".weight"], P[q + ".bias"], True, MOM, EPS)
        B[q + ".num_batches_tracked"] += 1
        return y
    return F.batch_norm(x, B[q + ".running_mean"], B[q + ".running_var"], P[q + ".weight"], P[q + ".bias"], False, 0.0, EPS)


def audio18_train_forward(audio, P, B, bn_train=True, taps=None):
    """fea_a [N, out_plane] in P's dtype.  P / B from split_state (B is updated in place when bn_train).  taps (optional dict): z (the
    raw stem map), stem (after the pool), layer1..4, pool, arg (the winners' h * W + w)."""
    dt = P["conv1.weight"].dtype
    z = F.conv2d(audio.to(dt), P["conv1.weight"], None, 2, 3)
    x = F.max_pool2d(F.relu(_bn(z, P, B, "bn1", bn_train)), 3, 2, 1)
    if taps is not None:
        taps["z"], taps["stem"] = z, x
    for li in range(1, 5):
        for bi in range(2):
            q = f"layer{li}.{bi}"
            stride = 2 if (bi == 0 and li > 1) else 1
            o = F.relu(_bn(F.conv2d(x, P[q + ".conv1.weight"], None, stride, 1), P, B, q + ".bn1", bn_train))
            res = x
            if (q + ".downsample.0.weight") in P:
                res = _bn(F.conv2d(x, P[q + ".downsample.0.weight"], None, stride, 0), P, B, q + ".downsample.1", bn_train)
            o = _bn(F.conv2d(o, P[q + ".conv2.weight"], None, 1, 1), P, B, q + ".bn2", bn_train)
            x = F.relu(o + res)
        if taps is not None:
            taps[f"layer{li}"] = x
    pooled, arg = F.adaptive_max_pool2d(x, 1, return_indices=True)
    pooled = pooled.flatten(1)
    if taps is not None:
        taps["pool"], taps["arg"] = pooled, arg.flatten(1)
    return F.linear(pooled, P["fc.weight"], P["fc.bias"])


def margin_report(layer4):
    """(gap, bound): the smallest lead of a POSITIVE winner of the global max over its runner-up, and the tap bound TAP * max(1,
    max|layer4|).  A 1 x 1 map has no runner-up (gap inf).  Winners at 0 sit behind the block's ReLU, whose backward removes whatever
    gradient they receive: which of several zeros wins does not matter."""
    n, c = layer4.shape[:2]
    flat = layer4.detach().reshape(n, c, -1)
    bound = TAP * max(1.0, float(flat.abs().max()))
    if flat.shape[-1] < 2:
        return float("inf"), bound
    top = flat.topk(2, dim=-1).values
    pos = top[..., 0] > 0
    gap = float((top[..., 0] - top[..., 1])[pos].min()) if bool(pos.any()) else float("inf")
    return gap, bound


@functools.lru_cache(maxsize=None)
def model_state(in_plane, C=5, B=2, seg_model="DeepLabV3Plus"):
    """state_dict of a CAVP with the ResNet-18 audio encoder, synthetic weights keyed by name (seed 1); built on the CPU"""
    from cavp_amd.cavp_model import CAVP
    from cavp_amd.synth import synth_state_dict
    m = CAVP(50, None, num_classes=C, args=args18(C, B, seg_model=seg_model), in_plane=in_plane)
    return synth_state_dict({k: tuple(v.shape) for k, v in m.state_dict().items()}, seed=1)


@functools.lru_cache(maxsize=None)
def encoder_reference(shape, seed, bn_train=True, dtype=torch.float64):
    """The encoder on `forward_audio`'s graph - features of the N clips followed by the same features in reversed order - with a
    fixed random upstream gradient: dict(audio, fea [2N, 304], grads {key: tensor}, buffers {key: tensor} after the step, taps).
    Computed once per argument set and shared; never modified."""
    N, cin = shape[0], shape[1]
    sd = model_state(cin)
    audio = audio_input(*shape, seed=seed)
    P, B = split_state(sd, dtype)
    taps = {}
    fea = audio18_train_forward(audio, P, B, bn_train, taps)
    idx = torch.arange(N - 1, -1, -1)
    out = torch.cat((fea, fea[idx]), 0)
    g = torch.Generator(device="cpu").manual_seed(1000 + seed)
    dout = torch.randn(out.shape, generator=g)
    out.backward(dout.to(dtype))
    return dict(audio=audio, idx=idx, dout=dout, fea=out.detach(), grads={k: v.grad for k, v in P.items()}, buffers=B,
                taps={k: v.detach() for k, v in taps.items()})


def whole_model_reference(sd, image, audio, label, B, dtype=torch.float64, bn_train=True):
    """forward_train + CE of a CAVP with the ResNet-18 audio encoder: oracle.cavp_oracle's stages around audio18_train_forward.
    Returns (out_pred, loss, {state_dict key: gradient}, encoder buffers after the step)."""
    from oracle import cavp_oracle as O
    params = {k: v.detach().clone().to(dtype).requires_grad_(True) for k, v in sd.items()
              if v.is_floating_point() and "running_" not in k}
    sd2 = {k: (v.to(dtype) if v.is_floating_point() else v) for k, v in sd.items()}
    sd2.update(params)
    lds = [False, False, False]
    fea_v = O.forward_feature(O.backbone_forward(image.to(dtype), sd2, lds, bn_train), sd2, bn_train)
    fea_v = torch.cat((fea_v, fea_v.clone()), 0)
    P = {k[len(PREFIX) + 1:]: v for k, v in params.items() if k.startswith(PREFIX + ".")}
    _, Bf = split_state(sd, dtype)
    fea_a = audio18_train_forward(audio, P, Bf, bn_train)
    fus, _ = O.forward_fusion(fea_v, fea_a, sd2)
    out = O.forward_cls(fus, sd2, tuple(image.shape[-2:]), bn_train)
    loss = O.ce_loss_train(out, label, B)
    loss.backward()
    return out.detach(), float(loss.item()), {k: p.grad for k, p in params.items() if p.grad is not None}, Bf
