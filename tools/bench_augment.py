"""The frame augmentation (cavp_amd.augment.FrameAugment: flip, rescale, ColorJitter, pad, crop, normalise on the GPU) as a trainer
would replay it, in one process:

  per configuration (crop 224 / 512, jitter on / off; B = 32, stage 640 x 640, every frame 480 rows x 640 columns, the seven-scale
  list): us per call as hipGraph replays - every replay draws afresh, so the figure averages over the scales - and us per kernel
  (plan, contrast_mean, render: each captured alone and replayed on the table the last full replay left), with the bytes the
  pass has to move (computed from that table: the source pixels it needs once, the outputs once) and bytes / time as a share of
  the 8 TB/s HBM peak;
  the captured training step (C1', bf16, B = 32, 224 x 224) without and with the augmentation as its `prologue`, alternating;
  tests/_augment_ref.ref_pil - the reference's chain as PIL calls - on one thread of this machine's CPU, the same frame size.

    python tools/bench_augment.py [--batch 32] [--iters 50] [--rounds 5] [--warmup 5] [--no-train-step] [--no-pil]
                                  [--out profiles/augment_bench.jsonl]

A round times `iters` back-to-back replays between two device events.  One JSON line per run is appended to --out.  Needs a GPU;
there is no fallback."""
import argparse
import json
import os
import statistics
import sys
import time
import types

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
import numpy as np
import torch

HBM_PEAK = 8.0e12
STAGE, FRAME = (640, 640), (480, 640)
SCALES = (0.5, 0.75, 1.0, 1.25, 1.5, 1.75, 2.0)


def timed(fn, iters):
    """us per call of fn over `iters` back-to-back calls between two device events"""
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(iters):
        fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b) * 1e3 / iters


def capture(fn):
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        fn()
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        fn()
    return graph


def pass_bytes(table, crop, jitter):
    """Bytes each pass has to move for the draws of `table` [B, 16]: contrast_mean reads every source pixel once; render reads the
    source window under the crop (+ the bicubic support) and its mask pixels, writes f32 x 3 + i64 per output pixel."""
    H, W = crop
    h, w = FRAME
    mean_b = render_b = 0
    for row in table:
        s = SCALES[int(row[1])]
        mean_b += (h * w * 3 + 8) if jitter else 0
        sup = 2 * int(np.ceil(2 * max(1 / s, 1.0))) + 1
        win_h, win_w = min(h, int(np.ceil(min(H, int(row[12])) / s)) + sup), min(w, int(np.ceil(min(W, int(row[13])) / s)) + sup)
        render_b += win_h * win_w * 3 + min(H * W, win_h * win_w) + H * W * (12 + 8)
    return mean_b, render_b


def bench_config(crop, jitter, B, a, dev, frames, masks, sizes):
    from cavp_amd.augment import AugResult, FrameAugment
    aug = FrameAugment(crop=crop, scales=SCALES, jitter=(.5, .5, .5, .25) if jitter else None, device=dev, max_batch=B, stage=STAGE)
    out = AugResult(B, crop, dev)
    graphs = {"call": capture(lambda: aug(frames, masks, sizes, out=out))}
    for name in ("plan", "mean", "render"):
        if name == "mean" and not jitter:
            continue
        graphs[name] = capture(lambda name=name: aug._run(frames, masks, sizes, None, out, False, launches=(name,)))
    for g in graphs.values():
        for _ in range(a.warmup):
            g.replay()
    times = {k: [] for k in graphs}
    shares = {"mean": [], "render": []}
    nbytes = {"mean": [], "render": []}
    for _ in range(a.rounds):
        times["call"].append(timed(graphs["call"].replay, a.iters))
        table = out.params.cpu().numpy()
        mb, rb = pass_bytes(table, crop, jitter)
        for k in graphs:
            if k == "call":
                continue
            if k == "plan":
                times[k].append(timed(graphs[k].replay, a.iters))
                graphs["call"].replay()          # the plan replays moved the table: a consistent one for the next two
                table = out.params.cpu().numpy()
                mb, rb = pass_bytes(table, crop, jitter)
                continue
            t = timed(graphs[k].replay, a.iters)
            times[k].append(t)
            nb = mb if k == "mean" else rb
            nbytes[k].append(nb)
            shares[k].append(nb / (t * 1e-6) / HBM_PEAK)
    aug.check()
    rec = {"crop": list(crop), "jitter": bool(jitter)}
    for k, v in times.items():
        rec[f"us_{k}"] = {"median": round(statistics.median(v), 2), "min": round(min(v), 2), "max": round(max(v), 2)}
    for k in ("mean", "render"):
        if shares[k]:
            rec[f"mbytes_{k}"] = round(statistics.median(nbytes[k]) / 1e6, 2)
            rec[f"hbm_share_{k}"] = round(statistics.median(shares[k]), 4)
    return rec


def build_model(B, dev):
    from cavp_amd.cavp_model import CAVP
    from cavp_amd.synth import synth_state_dict
    hyp = types.SimpleNamespace(seg_model="DeepLabV3Plus", last_three_dilation_stride=[False, False, False], audio_backbone="vgg",
                                num_classes=2, batch_size=B, local_rank=dev.index)
    m = CAVP(50, None, num_classes=2, args=hyp)
    m.load_state_dict(synth_state_dict({k: tuple(v.shape) for k, v in m.state_dict().items()}, seed=1))
    return m.train().to(dev).set_compute_dtype(torch.bfloat16)


def bench_train_step(B, a, dev, frames, masks, sizes):
    from cavp_amd.augment import AugResult, FrameAugment
    from cavp_amd.synth import synth_inputs
    image, audio, label = [t.to(dev) for t in synth_inputs(B, (224, 224), audio_batch=2 * B, num_classes=2, seed=0)]
    image2, label2 = image.clone(), label.clone()
    aug = FrameAugment(crop=(224, 224), scales=SCALES, device=dev, max_batch=B, stage=STAGE)
    res = AugResult(B, (224, 224), dev)

    def prologue():
        aug(frames, masks, sizes, out=res)
        image2.copy_(res.image)
        label2.copy_(res.label)

    m1, m2 = build_model(B, dev), build_model(B, dev)
    steps = {"plain": m1.capture_train_step(image, audio, label), "with_augment": m2.capture_train_step(image2, audio, label2, prologue=prologue)}
    for f in steps.values():
        for _ in range(a.warmup):
            f()
    torch.cuda.synchronize()
    times = {k: [] for k in steps}
    for _ in range(a.rounds):
        for k, f in steps.items():
            times[k].append(timed(f, max(a.iters // 2, 10)) / 1e3)
    aug.check()
    rec = {k: {"ms_median": round(statistics.median(v), 4), "ms_min": round(min(v), 4), "ms_max": round(max(v), 4)} for k, v in times.items()}
    rec["added_ms"] = round(rec["with_augment"]["ms_median"] - rec["plain"]["ms_median"], 4)
    rec["added_share_of_plain_step"] = round(rec["added_ms"] / rec["plain"]["ms_median"], 4)
    return rec


def bench_pil(frame, mask):
    """ms per image of ref_pil on one CPU thread: the chain with jitter at each of the seven scales, crops 224 and 512"""
    from tests import _augment_ref as R
    rec = {}
    for crop in ((224, 224), (512, 512)):
        per_scale = []
        for s in SCALES:
            ph, pw = R.padded_size(*R.scaled_size(*FRAME, s), crop)
            best = None
            for _ in range(2):
                t0 = time.perf_counter()
                R.ref_pil(frame, mask, crop, 1, s, (ph - crop[0]) // 2, (pw - crop[1]) // 2, ((0, 1, 2, 3), 1.2, 0.8, 1.3, 40))
                dt = (time.perf_counter() - t0) * 1e3
                best = dt if best is None else min(best, dt)
            per_scale.append(round(best, 2))
        rec[f"crop{crop[0]}"] = {"ms_per_scale": per_scale, "ms_mean": round(sum(per_scale) / len(per_scale), 2)}
    return rec


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=32)
    ap.add_argument("--iters", type=int, default=50)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--no-train-step", action="store_true")
    ap.add_argument("--no-pil", action="store_true")
    ap.add_argument("--out", default=os.path.join(REPO, "profiles", "augment_bench.jsonl"))
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_augment.py needs the GPU: a CPU run says nothing about these timings")
    from cavp_amd.hostinfo import cap_torch_threads
    cap_torch_threads()
    dev = torch.device("cuda", 0)
    B = a.batch
    rng = np.random.default_rng(0)
    host_frames = rng.integers(0, 256, (B,) + STAGE + (3,), dtype=np.uint8)
    host_masks = np.zeros((B,) + STAGE, np.uint8)
    host_masks[:, 100:300, 150:500] = 1
    frames, masks = torch.from_numpy(host_frames).to(dev), torch.from_numpy(host_masks).to(dev)
    sizes = torch.tensor([list(FRAME)] * B, dtype=torch.int32, device=dev)
    rec = {"bench": "augment", "device": torch.cuda.get_device_name(0), "batch": B, "stage": list(STAGE), "frame_hw": list(FRAME),
           "scales": list(SCALES), "iters": a.iters, "rounds": a.rounds, "configs": []}
    for crop in ((224, 224), (512, 512)):
        for jitter in (True, False):
            rec["configs"].append(bench_config(crop, jitter, B, a, dev, frames, masks, sizes))
            print(json.dumps(rec["configs"][-1]), flush=True)
    if not a.no_train_step:
        rec["train_step_c1p_bf16_224"] = bench_train_step(B, a, dev, frames, masks, sizes)
        print(json.dumps(rec["train_step_c1p_bf16_224"]), flush=True)
    if not a.no_pil:
        try:
            rec["ref_pil_one_thread"] = bench_pil(host_frames[0, :FRAME[0], :FRAME[1]], host_masks[0, :FRAME[0], :FRAME[1]])
        except ImportError as ex:
            rec["ref_pil_one_thread"] = f"not measured: {ex}"
    line = json.dumps(rec)
    print(line, flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "a") as f:
        f.write(line + "\n")


if __name__ == "__main__":
    main()
