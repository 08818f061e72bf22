#!/usr/bin/env python3
"""Time the AVSS validation loop on the GPU: `CAVP.predict` + `ClipValidation.update` on a whole batch of clips against the
reference-shaped frame loop (trainer_cavp_avss_image.py:295-349) assembled from the per-frame pieces: one frame per forward,
MIoU / ForegroundDetect updates, torch.unique(return_counts=True) and the host read of the multi-source predicate.

Workload: 8 clips x 10 frames at 224 x 224, K = 71, bf16 compute.  Every number is the median of `--rounds` rounds:
  batched        one hipGraph: predict (B = 80) + ClipValidation.update; device events around `--iters` replays
  update_mask    one hipGraph: ClipValidation.update on the uint8 mask alone (three launches)
  update_logits  one hipGraph: ClipValidation.update on full-resolution f32 logits alone
  predict        one hipGraph: predict (B = 80) alone
  loop_graph     the frame loop at its best: per frame a captured B = 1 graph (predict_lowres + MIoU.update_lowres +
                 ForegroundDetect.update_lowres for ALL), torch.unique + the host read, a second captured graph for the two MS
                 accumulators when the frame is multi-source; host wall time for the 80 frames
  loop_eager     the same loop with eager launches
One JSON line is appended to --out (profiles/clip_validation_bench.jsonl).

usage: python tools/bench_clip_validation.py [--iters 20] [--rounds 5] [--out profiles/clip_validation_bench.jsonl]
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

DEV = "cuda:0"
K, B, T, HW = 71, 8, 10, (224, 224)


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


def make_labels(g):
    """Block labels: per frame 2 to 4 classes in horizontal bands plus an ignore stripe, so that about half the frames are
    multi-source; 2 % of the pixels are relabelled at random."""
    y = torch.zeros((B, T) + HW, dtype=torch.int64)
    for b in range(B):
        for t in range(T):
            n = 1 + (b + t) % 3
            for i in range(n):
                y[b, t, 40 * i + 20:40 * i + 50, 30:200] = 1 + (7 * b + 3 * t + 11 * i) % (K - 1)
            if t % 4 == 0:
                y[b, t, :, :2] = 255
    noise = torch.rand(y.shape, generator=g) < 0.02
    y[noise] = torch.randint(0, K, (int(noise.sum()),), generator=g)
    return y


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--out", default=os.path.join(REPO, "profiles", "clip_validation_bench.jsonl"))
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
    g = torch.Generator().manual_seed(0)
    labels = make_labels(g).to(DEV)
    count = torch.full((B,), T, dtype=torch.int32, device=DEV)
    row = {"bench": "clip_validation", "device": torch.cuda.get_device_name(0), "clips": B, "frames": T, "hw": list(HW), "K": K,
           "dtype": "bf16", "iters": a.iters, "rounds": a.rounds}

    # ---- batched: one forward, one update ----
    cv = MT.ClipValidation(num_classes=K, max_frames=N, device=DEV)
    row["us_batched"] = replay_us(capture(lambda: cv.update(m.predict(image, audio), labels, count)), a.iters, a.rounds)
    row["us_predict"] = replay_us(capture(lambda: m.predict(image, audio)), a.iters, a.rounds)
    mask = m.predict(image, audio)
    row["us_update_mask"] = replay_us(capture(lambda: cv.update(mask, labels, count)), a.iters, a.rounds)
    with torch.no_grad():
        logits = torch.cat([m(image[i:i + 16], audio[i:i + 16], eval_mode=True)[0].float() for i in range(0, N, 16)])
    row["us_update_logits"] = replay_us(capture(lambda: cv.update(logits, labels, count)), a.iters, a.rounds)
    del logits
    cv.reset()
    cv.update(mask, labels, count)
    row["frames_all_ms"] = list(cv.frames())
    batched_counts = cv.counts().clone()
    cv.check()

    # ---- the frame loop ----
    acc = [MT.MIoU(K, 255, 0), MT.ForegroundDetect(K), MT.MIoU(K, 255, 0), MT.ForegroundDetect(K)]
    x1, a1 = image[:1].clone(), audio[:1].clone()
    y1 = labels[0, :1].clone()
    lo = [None]

    def all_step():
        lo[0] = m.predict_lowres(x1, a1)
        acc[0].update_lowres(lo[0], y1)
        acc[1].update_lowres(lo[0], y1)

    def ms_step():
        acc[2].update_lowres(lo[0], y1)
        acc[3].update_lowres(lo[0], y1)

    all_step()
    ms_step()
    g_all = capture(all_step)           # (lo[0] is now the graph's static low-resolution buffer)
    g_ms = capture(ms_step)

    def frame_loop(run_all, run_ms):
        for b in range(B):
            mask_num = int(count[b].item())
            for t in range(mask_num):
                i = b * T + t
                x1.copy_(image[i:i + 1])
                a1.copy_(audio[i:i + 1])
                y1.copy_(labels[b, t:t + 1])
                run_all()
                uniq_id, cnt = y1.unique(return_counts=True)
                if uniq_id[cnt > 100].shape[0] > 2:
                    run_ms()

    for name, fns in (("loop_graph", (g_all.replay, g_ms.replay)), ("loop_eager", (all_step, ms_step))):
        times = []
        for r in range(a.rounds + 1):
            for o in acc:
                o.reset()
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            frame_loop(*fns)
            torch.cuda.synchronize()
            if r:                       # the first round warms up
                times.append((time.perf_counter() - t0) * 1e6)
        row["us_" + name] = spread(times)
    # The loop's labels have no negative values, so unique() on the raw label is the predicate ClipValidation evaluates: the MS
    # routing must agree (same row sums).  The predictions are those of two different bf16 forwards (B = 1 and B = 80 pick
    # different conv tiles), so a few near-tie pixels may land in another column: reported, not asserted (the f32 equality is
    # tests/test_gpu_clip_validation.py::test_predict_and_update_equal_the_frame_loop).
    loop_counts = torch.stack([acc[0].counts(), acc[2].counts()])
    row["routing_equal_loop"] = bool(torch.equal(batched_counts.sum(2), loop_counts.sum(2)))
    row["pixels_predicted_differently"] = [int(v) // 2 for v in (batched_counts - loop_counts).abs().sum((1, 2)).tolist()]
    row["pixels_counted"] = [int(v) for v in batched_counts.sum((1, 2)).tolist()]
    row["speedup_vs_loop_graph"] = round(row["us_loop_graph"]["median"] / row["us_batched"]["median"], 2)
    print(json.dumps(row), flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "a") as f:
        f.write(json.dumps(row) + "\n")


if __name__ == "__main__":
    main()
