#!/usr/bin/env python3
"""Time the AVSBench object validation loop on the GPU: `VideoValidation.update` / `update_lowres` on a whole batch of videos
against the per-video loop (trainer_cavp_avs_obj.py:292-363) written with the per-call functions of cavp_amd.metrics: MIoU and
ForegroundDetect updates, mask_iou(argmax(vid_pred), labels), Eval_Fmeasure(vid_pred, labels) with its host read, two meters.

Workload: 8 videos x 5 frames at 224 x 224, C = K = 2, logits of the bf16 eval forward.  Every number is the median of `--rounds`
rounds (timing protocol of tools/bench_clip_validation.py: device events around `--iters` replays of a captured hipGraph; host wall
time for the loops, first round discarded):
  update_logits   one hipGraph: VideoValidation.update on the full-resolution f32 logits (two launches)
  update_lowres   one hipGraph: VideoValidation.update_lowres on the low-resolution logits (three launches)
  forward_lowres  one hipGraph: predict_lowres (B = 40) alone
  batched         one hipGraph: predict_lowres (B = 40) + update_lowres
  loop_metrics    the per-video loop on the same full-resolution logits: per video one MIoU.update and one
                  ForegroundDetect.update over its 5 frames, mask_iou on the int64 argmax, Eval_Fmeasure (logits form) and its
                  .item(); host wall time for the 8 videos (the metric calls only: the comparison with update_logits)
  loop_lowres     the same loop from the low-resolution logits: MIoU / ForegroundDetect.update_lowres, ops.seg_predict for
                  mask and probability, mask_iou on mask.long(), Eval_Fmeasure on the plane
The scores of the batched path and of the loop are compared (they read the same logits: equal counts, J and F within a few ulp).
One JSON line is appended to --out (profiles/video_validation_bench.jsonl).

usage: python tools/bench_video_validation.py [--iters 20] [--rounds 5] [--out profiles/video_validation_bench.jsonl]
"""
import argparse
import json
import os
import statistics
import sys
import time
import types

import torch

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)

from cavp_amd import metrics as MT  # noqa: E402
from cavp_amd import ops  # noqa: E402

DEV = "cuda:0"
K, B, T, HW = 2, 8, 5, (224, 224)


def spread(vals):
    return {"median": round(statistics.median(vals), 2), "min": round(min(vals), 2), "max": round(max(vals), 2)}


def capture(step):
    """step() eagerly, once on a side stream, then captured: the graph."""
    from cavp_amd.train import _no_gc_during_capture
    step()
    torch.cuda.synchronize()
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        step()
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with _no_gc_during_capture(), torch.cuda.graph(graph, capture_error_mode="thread_local"):
        step()
    return graph


def replay_us(graph, iters, rounds):
    out = []
    for _ in range(rounds):
        graph.replay()
        torch.cuda.synchronize()
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        for _ in range(iters):
            graph.replay()
        b.record()
        torch.cuda.synchronize()
        out.append(a.elapsed_time(b) * 1e3 / iters)
    return spread(out)


def make_labels():
    """Binary masks: one rectangle per frame that moves with the frame; video 3 has one empty frame, video 5 is all background."""
    y = torch.zeros((B, T) + HW, dtype=torch.int64)
    for b in range(B):
        for t in range(T):
            y[b, t, 30 + 8 * t:130 + 8 * t, 20 + 10 * b:120 + 10 * b] = 1
    y[3, 2] = 0
    y[5] = 0
    return y


def wall_us(fn, rounds):
    times = []
    for r in range(rounds + 1):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        out = fn()
        torch.cuda.synchronize()
        if r:                       # the first round warms up
            times.append((time.perf_counter() - t0) * 1e6)
    return spread(times), out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--out", default=os.path.join(REPO, "profiles", "video_validation_bench.jsonl"))
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
    labels = make_labels().to(DEV)
    count = torch.full((B,), T, dtype=torch.int32, device=DEV)
    row = {"bench": "video_validation", "device": torch.cuda.get_device_name(0), "videos": B, "frames": T, "hw": list(HW), "K": K,
           "dtype": "bf16", "iters": a.iters, "rounds": a.rounds}

    lo = m.predict_lowres(image, audio)
    logits = ops.bilinear_to_nchw(lo, torch.empty((N, K) + HW, dtype=torch.float32, device=DEV), False)

    # ---- batched: one update for all videos ----
    vv = MT.VideoValidation(num_classes=K, max_frames=N, max_videos=4096, device=DEV)
    row["us_update_logits"] = replay_us(capture(lambda: vv.update(logits, labels, count)), a.iters, a.rounds)
    row["us_update_lowres"] = replay_us(capture(lambda: vv.update_lowres(lo, labels, count)), a.iters, a.rounds)
    row["us_forward_lowres"] = replay_us(capture(lambda: m.predict_lowres(image, audio)), a.iters, a.rounds)
    row["us_batched"] = replay_us(capture(lambda: vv.update_lowres(m.predict_lowres(image, audio), labels, count)), a.iters, a.rounds)
    vv.check()                      # more than max_videos replays would have been reported here
    vv.reset()
    vv.update(logits, labels, count)
    (avs_miou, avs_f), perf = vv.results()
    J, F = (t.cpu() for t in vv.video_scores())
    row["batched_results"] = [float(avs_miou), float(avs_f)] + [float(v) for v in perf]

    # ---- the per-video loop with the per-call functions ----
    def loop_metrics():
        miou, fg = MT.MIoU(K, 255, 0), MT.ForegroundDetect(K)
        js, fs = [], []
        for b in range(B):
            vid_pred, y = logits[b * T:(b + 1) * T], labels[b]
            miou.update(vid_pred, y)
            fg.update(vid_pred, y)
            js.append(MT.mask_iou(torch.argmax(vid_pred, dim=1), y))
            fs.append(MT.Eval_Fmeasure(vid_pred, y))
        return torch.stack(js).cpu(), fs, MT.get_performance(miou, fg)

    mask = torch.empty((T,) + HW, dtype=torch.uint8, device=DEV)
    prob = torch.empty((T,) + HW, dtype=torch.float32, device=DEV)

    def loop_lowres():
        miou, fg = MT.MIoU(K, 255, 0), MT.ForegroundDetect(K)
        js, fs = [], []
        for b in range(B):
            lo_b, y = lo[b * T:(b + 1) * T], labels[b]
            miou.update_lowres(lo_b, y)
            fg.update_lowres(lo_b, y)
            ops.seg_predict(lo_b, HW, mask=mask, prob=prob, channel=1)
            js.append(MT.mask_iou(mask.long(), y))
            fs.append(MT.Eval_Fmeasure(prob, y))
        return torch.stack(js).cpu(), fs, MT.get_performance(miou, fg)

    row["us_loop_metrics"], (lj, lf, lperf) = wall_us(loop_metrics, a.rounds)
    row["us_loop_lowres"], (lj2, lf2, _) = wall_us(loop_lowres, a.rounds)
    row["perf_equal_loop"] = [float(v) for v in lperf] == [float(v) for v in perf]
    row["max_abs_dJ"] = max(float((J - lj).abs().max()), float((J - lj2).abs().max()))
    row["max_abs_dF"] = max(float((F - torch.tensor(lf)).abs().max()), float((F - torch.tensor(lf2)).abs().max()))
    row["speedup_logits_vs_loop"] = round(row["us_loop_metrics"]["median"] / row["us_update_logits"]["median"], 2)
    row["speedup_lowres_vs_loop"] = round(row["us_loop_lowres"]["median"] / row["us_update_lowres"]["median"], 2)
    print(json.dumps(row), flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "a") as f:
        f.write(json.dumps(row) + "\n")


if __name__ == "__main__":
    main()
