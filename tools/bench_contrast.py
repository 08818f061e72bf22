"""ContrastLoss forward + backward: host sampler against the device sampler (eager, and as one hipGraph replay).

    python tools/bench_contrast.py [--iters 200] [--warmup 20] [--rounds 5] [--out FILE]

Shapes: the config-#5 step (B = 30, 304 channels, 56 x 56 features from 224 x 224 binary labels, max_views = 512, max_classes = 1)
and one multi-class shape (same features, 8 foreground classes, max_classes = 8).  Every variant is warmed up on the shape it is
timed on; a round times `iters` back-to-back calls of each variant between two device synchronisations with a host clock, and the
variants alternate inside a round so that drift of the shared host hits all of them alike.  Reported: median and min / max over the
rounds of the per-call time.  The host-sampler path is the code this project had before the device sampler existed (it is not
touched by it), so its row is the baseline.  Needs a GPU; there is no fallback."""
import argparse
import json
import os
import statistics
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch

from cavp_amd.contrast import ContrastLoss


def make_inputs(B, C, hw, full, n_classes, dev, seed=0):
    g = torch.Generator().manual_seed(seed)
    em = torch.randn((B, hw[0], hw[1], C), generator=g).to(dev).permute(0, 3, 1, 2).requires_grad_(True)   # NHWC memory, as CAVP returns
    es = torch.randn((B, hw[0], hw[1], C), generator=g).to(dev).permute(0, 3, 1, 2).requires_grad_(True)
    gt = torch.zeros((B,) + full, dtype=torch.long)
    bh = full[0] // (n_classes + 1)
    for b in range(B):
        for k in range(1, n_classes + 1):          # one horizontal band per class, shifted per image; the rest is background
            r0 = (k * bh + 7 * b) % (full[0] - bh // 2)
            gt[b, r0:r0 + bh // 2, 16:full[1] - 16] = k
    gs = torch.roll(gt, 1, 0)
    return em, gt.to(dev), es, gs.to(dev)


def variants(shape, dev):
    em, gt, es, gs = make_inputs(shape["B"], 304, (56, 56), (224, 224), shape["classes"], dev)

    hcrit = ContrastLoss(0.1, 255, 512)

    def host_step():
        em.grad = es.grad = None
        hcrit(em, gt, es, gs).backward()

    dcrit = ContrastLoss(0.1, 255, 512).use_device_sampler(shape["max_classes"])

    def device_step():
        em.grad = es.grad = None
        dcrit(em, gt, es, gs).backward()

    gcrit = ContrastLoss(0.1, 255, 512).use_device_sampler(shape["max_classes"])
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        for _ in range(3):
            em.grad = es.grad = None
            gcrit(em, gt, es, gs).backward()
    torch.cuda.current_stream().wait_stream(side)
    em.grad = es.grad = None
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        gcrit(em, gt, es, gs).backward()
    torch.cuda.synchronize()
    return {"host sampler, eager": host_step, "device sampler, eager": device_step, "device sampler, graph replay": graph.replay}, dcrit


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=200)
    ap.add_argument("--warmup", type=int, default=20)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_contrast.py needs the GPU: a CPU run says nothing about these timings")
    dev = torch.device("cuda", 0)
    shapes = [{"name": "config #5 (binary labels)", "B": 30, "classes": 1, "max_classes": 1},
              {"name": "8 foreground classes", "B": 30, "classes": 8, "max_classes": 8}]
    lines = []
    for shape in shapes:
        fns, dcrit = variants(shape, dev)
        for f in fns.values():
            for _ in range(a.warmup):
                f()
        torch.cuda.synchronize()
        h = dcrit.last_plan()["header"].tolist()
        times = {k: [] for k in fns}
        for _ in range(a.rounds):
            for k, f in fns.items():
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                for _ in range(a.iters):
                    f()
                torch.cuda.synchronize()
                times[k].append((time.perf_counter() - t0) / a.iters * 1e3)
        cap = (shape["max_classes"] + 2) * 512
        for k, v in times.items():
            rec = {"shape": shape["name"], "variant": k, "n": h[0], "ncap": cap, "ms_median": round(statistics.median(v), 4),
                   "ms_min": round(min(v), 4), "ms_max": round(max(v), 4), "iters": a.iters, "rounds": a.rounds}
            lines.append(json.dumps(rec))
            print(lines[-1], flush=True)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
