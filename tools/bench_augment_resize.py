"""The resize variant of the frame augmentation (FrameAugment(resize=True)) and the label stage (cavp_amd.labels.LabelStage) as a
trainer would replay them, by the method of tools/bench_augment.py (hipGraph replays between two device events, median of
rounds), in one process:

  resize variant, B = 32, output 224 x 224, the AVS scale list: stage 640 x 640 with 480 x 640 frames, and stage 720 x 1280 with
  full frames; jitter off (the AVSS set-ups) and on; us per call and per launch (plan, contrast_mean, store, render; each captured
  alone and replayed on the table the last full replay left), and the test-time path eval_();
  the crop variant at the same stage, scale list and output in the same process;
  tests/_augment_resize_ref.ref_pil_resize - the reference's chain as PIL calls - on one thread of this machine's CPU;
  LabelStage at 32 x 224 x 224 and 8 x 512 x 512 (int64 labels, K = 71; plain, with a remap, with remap + binary) against the
  torch-op host route a data set takes today: the label to the host, the remap loop, unique + one_hot per image, img_label back.

    python tools/bench_augment_resize.py [--batch 32] [--iters 50] [--rounds 5] [--warmup 5] [--no-big] [--no-pil]
                                         [--out profiles/augment_resize_bench.jsonl]

One JSON line per run is appended to --out.  Needs a GPU; there is no fallback."""
import argparse
import json
import os
import statistics
import sys
import time

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
sys.path.insert(0, os.path.join(REPO, "tools"))
import numpy as np
import torch

from bench_augment import capture, timed  # noqa: E402

SCALES = (0.5, 0.75, 1.0)
OUT = (224, 224)


def stats(v, digits=2):
    return {"median": round(statistics.median(v), digits), "min": round(min(v), digits), "max": round(max(v), digits)}


def staged(B, stage, frame, dev, seed=0):
    rng = np.random.default_rng(seed)
    host_frames = rng.integers(0, 256, (B,) + stage + (3,), dtype=np.uint8)
    host_masks = np.zeros((B,) + stage, np.uint8)
    host_masks[:, stage[0] // 6:stage[0] // 2, stage[1] // 4:3 * stage[1] // 4] = 1
    sizes = torch.tensor([list(frame)] * B, dtype=torch.int32, device=dev)
    return host_frames, host_masks, (torch.from_numpy(host_frames).to(dev), torch.from_numpy(host_masks).to(dev), sizes)


def bench_variant(stage, frame, jitter, resize, B, a, dev, ins):
    from cavp_amd.augment import AugResult, FrameAugment
    aug = FrameAugment(crop=OUT, scales=SCALES, jitter=(.5, .5, .5, .25) if jitter else None, device=dev, max_batch=B, stage=stage,
                       resize=resize)
    out = AugResult(B, OUT, dev)
    graphs = {"call": capture(lambda: aug(*ins, out=out))}
    if resize:
        graphs["eval"] = capture(lambda: aug.eval_(*ins, out=out))
    for name in ("plan", "mean", "store", "render"):
        if (name == "mean" and not jitter) or (name == "store" and not resize):
            continue
        graphs[name] = capture(lambda name=name: aug._run(*ins, None, out, False, launches=(name,)))
    for g in graphs.values():
        for _ in range(a.warmup):
            g.replay()
    times = {k: [] for k in graphs}
    for _ in range(a.rounds):
        for k, g in graphs.items():
            if k in ("mean", "store", "render"):
                continue
            times[k].append(timed(g.replay, a.iters))
        graphs["call"].replay()          # the plan / eval replays moved the table: a consistent one for the passes
        for k in ("mean", "store", "render"):
            if k in graphs:
                times[k].append(timed(graphs[k].replay, a.iters))
    aug.check()
    rec = {"variant": "resize" if resize else "crop", "stage": list(stage), "frame_hw": list(frame), "out": list(OUT), "jitter": bool(jitter)}
    for k, v in times.items():
        rec[f"us_{k}"] = stats(v)
    return rec


def bench_pil(frame, mask):
    """ms per image of ref_pil_resize on one CPU thread at each AVS scale, without and with jitter"""
    from tests import _augment_resize_ref as RR
    rec = {}
    for name, jit in (("plain", None), ("jitter", ((0, 1, 2, 3), 1.2, 0.8, 1.3, 40))):
        per_scale = []
        for s in SCALES:
            best = None
            for _ in range(2):
                t0 = time.perf_counter()
                RR.ref_pil_resize(frame, mask, OUT, 1, s, jit)
                dt = (time.perf_counter() - t0) * 1e3
                best = dt if best is None else min(best, dt)
            per_scale.append(round(best, 2))
        rec[name] = {"ms_per_scale": per_scale, "ms_mean": round(sum(per_scale) / len(per_scale), 2)}
    return rec


def host_route(label, remap, K):
    """What a data set does today with a device label: to the host, the remap loop, unique + one_hot per image, img_label back."""
    import torch.nn.functional as F
    lab = label.cpu()
    vecs = []
    for b in range(lab.shape[0]):
        cur = lab[b]
        if remap is not None:
            values = torch.unique(cur)
            for v in values[(values != 0) & (values != 255)].tolist():
                cur[cur == v] = remap[v]
        vecs.append(F.one_hot(torch.unique(cur[cur != 255]), num_classes=K).sum(0))
    out = torch.stack(vecs).to(label.device)
    torch.cuda.synchronize()
    return out


def bench_labels(B, hw, a, dev):
    from cavp_amd.labels import LabelResult, LabelStage
    K = 71
    rng = np.random.default_rng(1)
    lab = np.zeros((B,) + hw, np.int64)
    for b in range(B):
        for v in rng.choice(np.arange(1, 60), size=3, replace=False):
            y, x = rng.integers(0, hw[0] // 2), rng.integers(0, hw[1] // 2)
            lab[b, y:y + hw[0] // 3, x:x + hw[1] // 3] = v
    lab[:, :4] = 255
    label = torch.from_numpy(lab).to(dev)
    remap = np.full(256, -1, np.int32)
    remap[1:60] = rng.integers(1, K, 59)
    rec = {"batch": B, "hw": list(hw), "K": K}
    for name, kw in (("plain", {}), ("remap", {"remap": remap}), ("remap_binary", {"remap": remap, "binary": True})):
        st = LabelStage(num_classes=K, device=dev, max_batch=B, **kw)
        out = LabelResult(B, K, hw, dev, st.changes_label)
        g = capture(lambda: st(label, out=out))
        for _ in range(a.warmup):
            g.replay()
        rec[f"us_{name}"] = stats([timed(g.replay, a.iters) for _ in range(a.rounds)])
        rec[f"launches_{name}"] = 3 if "remap" in kw else 2
        st.check()
    for name, rm in (("plain", None), ("remap", torch.from_numpy(remap.astype(np.int64)))):
        want = host_route(label, rm, K)
        t = []
        for _ in range(a.rounds):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            host_route(label, rm, K)
            t.append((time.perf_counter() - t0) * 1e6)
        rec[f"us_host_route_{name}"] = stats(t)
        st = LabelStage(num_classes=K, device=dev, max_batch=B, remap=None if rm is None else remap)
        assert torch.equal(st(label).img_label, want), name
    return rec


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=32)
    ap.add_argument("--iters", type=int, default=50)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--no-big", action="store_true", help="skip the 720 x 1280 stage")
    ap.add_argument("--no-pil", action="store_true")
    ap.add_argument("--out", default=os.path.join(REPO, "profiles", "augment_resize_bench.jsonl"))
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_augment_resize.py needs the GPU: a CPU run says nothing about these timings")
    from cavp_amd.hostinfo import cap_torch_threads
    cap_torch_threads()
    dev = torch.device("cuda", 0)
    B = a.batch
    rec = {"bench": "augment_resize", "device": torch.cuda.get_device_name(0), "batch": B, "scales": list(SCALES), "iters": a.iters,
           "rounds": a.rounds, "configs": [], "labels": []}
    pil_inputs = {}
    for stage, frame in (((640, 640), (480, 640)),) + (() if a.no_big else (((720, 1280), (720, 1280)),)):
        host_frames, host_masks, ins = staged(B, stage, frame, dev)
        pil_inputs[f"{frame[0]}x{frame[1]}"] = (host_frames[0, :frame[0], :frame[1]].copy(), host_masks[0, :frame[0], :frame[1]].copy())
        for resize, jitter in ((True, False), (True, True), (False, False), (False, True)):
            rec["configs"].append(bench_variant(stage, frame, jitter, resize, B, a, dev, ins))
            print(json.dumps(rec["configs"][-1]), flush=True)
        del ins
        torch.cuda.empty_cache()
    for Bl, hw in ((32, (224, 224)), (8, (512, 512))):
        rec["labels"].append(bench_labels(Bl, hw, a, dev))
        print(json.dumps(rec["labels"][-1]), flush=True)
    if not a.no_pil:
        torch.set_num_threads(1)
        try:
            rec["ref_pil_resize_one_thread"] = {k: bench_pil(*v) for k, v in pil_inputs.items()}
        except ImportError as ex:
            rec["ref_pil_resize_one_thread"] = f"not measured: {ex}"
    line = json.dumps(rec)
    print(line, flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "a") as f:
        f.write(line + "\n")


if __name__ == "__main__":
    main()
