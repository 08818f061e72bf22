#!/usr/bin/env python3
"""Time the preview stage on the GPU: `PreviewStage` on a whole batch against the reference-shaped upload route
(utils/tensor_board.py:90-139 as the four trainers call it), assembled from its pieces on the same inputs: four whole-tensor
.cpu() copies (image, labels, logits, torch.softmax(logits, 1)), the CPU argmax, the ignore overwrite and the per-frame picture
loop (de-normalise + byte cast + Image.fromarray, two palette pictures).

Workload: B = 32 frames at 224 x 224, K = 71 and K = 2, float32 logits.  One process, one GPU.  Every number is the median of
`--rounds` rounds; device times are device events around `--iters` replays of a captured hipGraph:
  us_panels_logits / us_panels_mask            the panels launch alone, logits resp. uint8 mask as the prediction source
  us_panels_logits_256 / us_panels_mask_256    the same with size=(256, 256): panels + the gather launch
  us_read / us_read_256                        host wall time of read(): one copy of the arena into pinned memory, one event wait,
                                               the PIL pictures built (us_read_copy: the same without the picture building)
  us_reference_route                           host wall time of the reference-shaped route, ending in the same pictures
Bytes, computed from the shapes: logits_bytes (what the logits source must read at least), floor_us_8TBs (logits + image + labels
+ panels over the 8 TB/s HBM peak), GBps_panels_logits (those bytes over the measured time), host_copy_bytes (the arena, 5 bytes
per pixel) and reference_copy_bytes (the four tensors).
One JSON line per K is appended to --out (profiles/preview_bench.jsonl).

usage: python tools/bench_preview.py [--iters 50] [--rounds 5] [--out profiles/preview_bench.jsonl]
"""
import argparse
import json
import os
import statistics
import sys
import time

import numpy as np
import torch

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)

from cavp_amd.augment import IMAGENET_MEAN, IMAGENET_STD  # noqa: E402
from cavp_amd.preview import PreviewStage  # noqa: E402

DEV = "cuda:0"
B, HW = 32, (224, 224)


def spread(vals):
    return {"median": round(statistics.median(vals), 2), "min": round(min(vals), 2), "max": round(max(vals), 2)}


def capture(step):
    """step() eagerly, once on a side stream, then captured: the graph."""
    step()
    torch.cuda.synchronize()
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        step()
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
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


def wall_us(fn, rounds):
    out = []
    for r in range(rounds + 1):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        if r:                           # the first round warms up
            out.append((time.perf_counter() - t0) * 1e6)
    return spread(out)


def reference_route(image, labels, logits, palette, Image):
    """What the trainers' upload call costs on these inputs: the four copies, then the host work, ending in the same pictures."""
    img, gt, pred, _score = image.cpu(), labels.cpu(), logits.cpu(), torch.softmax(logits, 1).cpu()
    frames = []
    for i in img:
        for t, m, s in zip(i, IMAGENET_MEAN, IMAGENET_STD):
            t.mul_(s).add_(m)
        frames.append(Image.fromarray(i.mul(255).byte().permute(1, 2, 0).numpy()))
    pred = torch.argmax(pred, dim=1)
    pred[gt == 255] = 255
    pics = []
    for arr in (pred.numpy(), gt.numpy()):
        for a in arr:
            p = Image.fromarray(a.astype(np.uint8)).convert("P")
            p.putpalette(palette)
            pics.append(p)
    return frames, pics


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=50)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--out", default=os.path.join(REPO, "profiles", "preview_bench.jsonl"))
    a = ap.parse_args()
    from PIL import Image
    from cavp_amd.hostinfo import cap_torch_threads
    cap_torch_threads()
    if not torch.cuda.is_available():
        raise SystemExit("bench_preview needs the GPU: a time taken elsewhere says nothing")
    g = torch.Generator().manual_seed(0)
    H, W = HW
    image = torch.randn(B, 3, H, W, generator=g).to(DEV)
    for K in (71, 2):
        logits = (torch.randn(B, K, H, W, generator=g) * 4).to(DEV)
        labels = torch.randint(0, K, (B, H, W), generator=g)
        labels[:, :4] = 255
        labels = labels.to(DEV)
        mask = logits.argmax(1).to(torch.uint8)
        n = B * H * W
        row = {"bench": "preview", "device": torch.cuda.get_device_name(0), "B": B, "hw": list(HW), "K": K, "iters": a.iters,
               "rounds": a.rounds, "logits_bytes": 4 * K * n, "host_copy_bytes": 5 * n,
               "reference_copy_bytes": (3 * 4 + 8 + 2 * 4 * K) * n}
        outs, stages = {}, {}
        for size, tag in ((None, ""), ((256, 256), "_256")):
            pv = PreviewStage(K, IMAGENET_MEAN, IMAGENET_STD, size=size, device=DEV, max_batch=B)
            for src, kw in (("logits", {"logits": logits}), ("mask", {"mask": mask})):
                out = pv(image, labels, **kw)
                row[f"us_panels_{src}{tag}"] = replay_us(capture(lambda: pv(image, labels, out=out, **kw)), a.iters, a.rounds)
                outs[src + tag] = out
            assert torch.equal(outs["logits" + tag].buffer, outs["mask" + tag].buffer)
            row["us_read" + tag] = wall_us(lambda: pv.read(outs["logits" + tag]), a.rounds)
            pv.check()
            stages[tag] = pv
        plain = stages[""]                      # the stage without a resize: the palette and the pictures compared below are its own
        pinned = torch.empty(5 * n, dtype=torch.uint8, pin_memory=True)
        row["us_read_copy"] = wall_us(lambda: pinned.copy_(outs["logits"].buffer.view(-1), non_blocking=True), a.rounds)
        moved = row["logits_bytes"] + (3 * 4 + 8 + 5) * n
        row["floor_us_8TBs"] = round(moved / 8e12 * 1e6, 2)
        row["GBps_panels_logits"] = round(moved / row["us_panels_logits"]["median"] / 1e3, 1)
        row["us_reference_route"] = wall_us(lambda: reference_route(image, labels, logits, plain.palette, Image), a.rounds)
        frames, pics = reference_route(image, labels, logits, plain.palette, Image)
        got = plain.read(outs["logits"])
        row["pictures_equal_reference_route"] = bool(
            all(np.array_equal(np.asarray(p), np.asarray(q)) for p, q in zip(frames + pics, got["x"] + got["y_tilde"] + got["y"])))
        row["speedup_device_plus_read_vs_reference_route"] = round(
            row["us_reference_route"]["median"] / (row["us_panels_logits"]["median"] + row["us_read"]["median"]), 1)
        print(json.dumps(row), flush=True)
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "a") as f:
            f.write(json.dumps(row) + "\n")
        del logits


if __name__ == "__main__":
    main()
