#!/usr/bin/env python3
"""Time the AVSBench-semantic metric on the GPU: `SemanticValidation.update` / `update_lowres` on a whole batch of clips against a
loop of the reference's shape on the same device tensors (softmax, argmax, then per frame three `.cpu()` copies and three
torch.histc calls and the float tail on the host), written here from torch calls.

Workload: 8 clips x 10 frames at 224 x 224, K = 71, logits of the bf16 eval forward with synthetic weights.  Every number is the
median of `--rounds` rounds (timing protocol of tools/bench_clip_validation.py: device events around `--iters` replays of a captured
hipGraph; host wall time for the loop, first round discarded):
  update_logits    one hipGraph: SemanticValidation.update on the full-resolution f32 logits (two launches)
  update_mask      one hipGraph: SemanticValidation.update on the uint8 mask of CAVP.predict (two launches)
  update_lowres    one hipGraph: SemanticValidation.update_lowres on the low-resolution logits (three launches)
  forward_predict  one hipGraph: CAVP.predict (B = 80) alone;   batched_mask   = predict + update in one graph
  forward_lowres   one hipGraph: CAVP.predict_lowres alone;     batched_lowres = predict_lowres + update_lowres in one graph
  loop_reference   the reference-shaped host loop on the full-resolution logits, host wall time
`bytes` is what each update variant reads, computed from the shapes (logits or mask or low-resolution logits, plus the int64
labels; update_lowres also writes and re-reads its mask), `gbps` = bytes / median time.  The per-class sums of the device path and
of the loop are compared.  One JSON line is appended to --out (profiles/semantic_validation_bench.jsonl).

usage: python tools/bench_semantic_validation.py [--iters 20] [--rounds 5] [--out profiles/semantic_validation_bench.jsonl]
"""
import argparse
import json
import os
import sys
import types

import torch

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

from bench_video_validation import capture, replay_us, wall_us  # noqa: E402
from cavp_amd import metrics as MT  # noqa: E402
from cavp_amd import ops  # noqa: E402

DEV = "cuda:0"
K, B, T, HW = 71, 8, 10, (224, 224)


def make_labels(pred):
    """Labels that agree with the prediction inside a moving rectangle and are background outside; a 255 border column, clip 5
    all background."""
    y = torch.zeros((B, T) + HW, dtype=torch.int64, device=pred.device)
    p = pred.view((B, T) + HW).long()
    for b in range(B):
        for t in range(T):
            sl = (b, t, slice(30 + 8 * t, 130 + 8 * t), slice(20 + 10 * b, 120 + 10 * b))
            y[sl] = p[sl]
    y[:, :, :, 0] = 255
    y[5] = 0
    return y


def reference_shaped_loop(logits, labels):
    """Per-class sums of IoU and F-score (beta^2 = 0.3) and the class frame counts, frame by frame on the host."""
    k = logits.shape[1]
    pred = torch.softmax(logits, dim=1).argmax(1) + 1
    target = labels.flatten(0, 1).float() + 1
    pred = pred.float() * (target > 0).float()
    hit = pred * (pred == target).float()
    ious, fscores, cls_count = torch.zeros(k), torch.zeros(k), torch.zeros(k)
    for n in range(pred.shape[0]):
        inter, area_p, area_t = (torch.histc(v[n].cpu(), bins=k, min=1, max=k) for v in (hit, pred, target))
        union = area_p + area_t - inter
        ious += inter / (2.220446049250313e-16 + union)
        cls_count[union != 0] += 1
        precision, recall = inter / area_p, inter / area_t
        f = (1 + 0.3) * precision * recall / (0.3 * precision + recall)
        fscores += torch.nan_to_num(f, nan=0.0)
    return ious, fscores, cls_count


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--out", default=os.path.join(REPO, "profiles", "semantic_validation_bench.jsonl"))
    a = ap.parse_args()
    from cavp_amd.cavp_model import CAVP
    from cavp_amd.hostinfo import cap_torch_threads
    from cavp_amd.synth import synth_inputs, synth_state_dict
    cap_torch_threads()
    N = B * T
    args = types.SimpleNamespace(seg_model="DeepLabV3Plus", last_three_dilation_stride=[False, True, True], audio_backbone="vgg",
                                 num_classes=K, batch_size=N, local_rank="cpu")
    m = CAVP(50, None, num_classes=K, args=args)
    m.load_state_dict(synth_state_dict({k: tuple(v.shape) for k, v in m.state_dict().items()}, seed=1), strict=True)
    m.eval().to(DEV).set_compute_dtype(torch.bfloat16)
    image, audio, _ = synth_inputs(N, HW, num_classes=K, seed=5)
    image, audio = image.to(DEV), audio.to(DEV)
    count = torch.full((B,), T, dtype=torch.int32, device=DEV)
    row = {"bench": "semantic_validation", "device": torch.cuda.get_device_name(0), "clips": B, "frames": T, "hw": list(HW), "K": K,
           "dtype": "bf16", "iters": a.iters, "rounds": a.rounds}

    lo = m.predict_lowres(image, audio)
    logits = ops.bilinear_to_nchw(lo, torch.empty((N, K) + HW, dtype=torch.float32, device=DEV), False)
    mask = m.predict(image, audio)
    labels = make_labels(mask)
    px = N * HW[0] * HW[1]
    lo_bytes = lo.shape[0] * lo.shape[1] * lo.shape[2] * lo.stride(2) * lo.element_size()
    row["bytes"] = {"update_logits": px * (4 * K + 8), "update_mask": px * (1 + 8), "update_lowres": lo_bytes + px * (1 + 1 + 8)}

    sv = MT.SemanticValidation(num_classes=K, max_frames=N, device=DEV)
    steps = {
        "update_logits": lambda: sv.update(logits, labels, count),
        "update_mask": lambda: sv.update(mask, labels, count),
        "update_lowres": lambda: sv.update_lowres(lo, labels, count),
        "forward_predict": lambda: m.predict(image, audio),
        "batched_mask": lambda: sv.update(m.predict(image, audio), labels, count),
        "forward_lowres": lambda: m.predict_lowres(image, audio),
        "batched_lowres": lambda: sv.update_lowres(m.predict_lowres(image, audio), labels, count),
    }
    for name, step in steps.items():
        row[f"us_{name}"] = replay_us(capture(step), a.iters, a.rounds)
    row["gbps"] = {k: round(v / row[f"us_{k}"]["median"] / 1e3, 1) for k, v in row["bytes"].items()}
    sv.check()
    sv.reset()
    sv.update(logits, labels, count)
    r = sv.results()
    row["results"] = {k: r[k] for k in ("miou", "fscore", "jf", "binary_miou")}
    dev_sums = [t.cpu() for t in sv.last_call()[:3]]

    row["us_loop_reference"], host_sums = wall_us(lambda: reference_shaped_loop(logits, labels), a.rounds)
    row["max_abs_diff_vs_loop"] = max(float((d - h).abs().max()) for d, h in zip(dev_sums, host_sums))
    row["speedup_logits_vs_loop"] = round(row["us_loop_reference"]["median"] / row["us_update_logits"]["median"], 1)
    print(json.dumps(row), flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "a") as f:
        f.write(json.dumps(row) + "\n")


if __name__ == "__main__":
    main()
