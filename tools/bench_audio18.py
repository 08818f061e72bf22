#!/usr/bin/env python3
"""Time the ResNet-18 audio encoder (audio_backbone="18", eval forward).

  * stem rows: the fused launch (ops.audio_stem_pool: conv 7x7/2 + folded BatchNorm + ReLU + max pool 3/2, the stem map stays in LDS)
    against the two-launch route built from existing ops (ops.conv_smallcin_kxk 7/2/3 without bias, then ops.maxpool with scale / shift /
    ReLU) on [64, 2, 300, 64] and [64, 1, 300, 64], bf16 and f32.  The two variants alternate in one process in `--repeats` windows of
    `--iters` calls; per variant the median window, min, max and the spread (max - min).  The outputs are compared before anything is
    timed.  `bytes` is the compulsory traffic computed from the shapes: input + weights + pooled output, and for the two-launch route
    the stem map written once and read once on top.
  * encoder rows: the whole encoder ([64, 2, 300, 64] and [64, 1, 300, 64]) eager and as a graph replay, next to the VGGish encoder on
    [64, 1, 96, 64], bf16.
  * model rows (unless --no-model): the eval forward at the VPO-SS shape (512 x 512, output stride 8, 22 classes, bf16) with "18" on
    [B, 1, 300, 64] against the "vgg" plumbing variant on [B, 1, 96, 64], as graph replays, alternating.

Prints one JSON line per row; --jsonl appends them to a file.

usage: python tools/bench_audio18.py [--iters 50] [--repeats 7] [--batch 8] [--no-model] [--jsonl profiles/audio18_bench.jsonl]
"""
import argparse
import json
import os
import statistics
import sys
import types

import torch

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)

from cavp_amd import ops  # noqa: E402
from cavp_amd._lib import ACT_RELU  # noqa: E402

DEV = "cuda:0"
ROWS = []


def report(name, **fields):
    row = {"item": name, **fields}
    ROWS.append(row)
    print(json.dumps(row), flush=True)


def gpu_time(fn, iters, warmup=3):
    """Mean device time per call (microseconds) from events around `iters` back-to-back calls."""
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(iters):
        fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b) * 1e3 / iters


def alternate(variants, iters, repeats):
    """{name: [us per call, one per window]}: the variants take turns, window by window."""
    for fn in variants.values():
        gpu_time(fn, 5)
    us = {k: [] for k in variants}
    for _ in range(repeats):
        for k, fn in variants.items():
            us[k].append(gpu_time(fn, iters, warmup=1))
    return us


def stats(v, unit="us", nd=2):
    return {f"{unit}_median": round(statistics.median(v), nd), f"{unit}_min": round(min(v), nd), f"{unit}_max": round(max(v), nd),
            f"spread_{unit}": round(max(v) - min(v), nd)}


def capture(step):
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


def bench_stem(iters, repeats, N=64, T=300, Fq=64):
    g = torch.Generator(device="cpu").manual_seed(0)
    hs, ws = (T - 1) // 2 + 1, (Fq - 1) // 2 + 1
    hp, wp = (hs - 1) // 2 + 1, (ws - 1) // 2 + 1
    for cin in (2, 1):
        x = (torch.randn((N, cin, T, Fq), generator=g) * 0.5).to(DEV)
        w = (torch.randn((64, cin, 7, 7), generator=g) * (2.0 / (49 * cin)) ** 0.5).to(DEV)
        scale, shift = (torch.rand(64, generator=g) + 0.5).to(DEV), (torch.randn(64, generator=g) * 0.1).to(DEV)
        for dtype in (torch.bfloat16, torch.float32):
            es = 2 if dtype == torch.bfloat16 else 4
            stem = torch.empty((N, hs, ws, 64), dtype=dtype, device=DEV)
            y2 = torch.empty((N, hp, wp, 64), dtype=dtype, device=DEV)
            y1 = torch.empty_like(y2)

            def fused():
                ops.audio_stem_pool(x, w, scale, shift, y1)

            def two():
                ops.conv_smallcin_kxk(x, w, None, stem, 7, 2, 3)
                ops.maxpool(stem, y2, 3, 2, 1, scale=scale, shift=shift, act=ACT_RELU)

            fused()
            two()
            torch.cuda.synchronize()
            # (the two-launch route rounds the raw conv output to dtype BEFORE the BatchNorm: in bf16 the two differ by that rounding)
            err = float((y1.float() - y2.float()).abs().max())
            tol = (2e-4 if dtype == torch.float32 else 2.0 ** -6) * max(1.0, float(y2.float().abs().max()))
            if not err <= tol:
                raise SystemExit(f"fused stem differs from the two-launch route: {err} > {tol} (cin={cin}, {dtype})")
            common = x.numel() * 4 + w.numel() * 4 + y1.numel() * es
            us = alternate({"fused": fused, "two": two}, iters, repeats)
            tag = f"[{N}, {cin}, {T}, {Fq}] {str(dtype).split('.')[-1]}"
            report(f"stem fused {tag}", **stats(us["fused"]), bytes=common, windows=repeats, calls_per_window=iters)
            report(f"stem two-launch {tag}", **stats(us["two"]), bytes=common + 2 * stem.numel() * es, windows=repeats,
                   calls_per_window=iters)
            gain = statistics.median(us["two"]) - statistics.median(us["fused"])
            spread = max(max(v) - min(v) for v in us.values())
            report(f"stem two-launch - fused {tag}", delta_us_median=round(gain, 2), larger_spread_us=round(spread, 2),
                   fused_wins=bool(gain > spread), max_abs_diff=err)
            del stem, y1, y2


def _model(audio_backbone, in_plane, C, B, lds, dtype):
    from cavp_amd.cavp_model import CAVP
    from cavp_amd.synth import synth_state_dict
    args = types.SimpleNamespace(seg_model="DeepLabV3Plus", last_three_dilation_stride=lds, audio_backbone=audio_backbone,
                                 num_classes=C, batch_size=B, local_rank="cpu")
    m = CAVP(50, None, num_classes=C, args=args, in_plane=in_plane)
    m.load_state_dict(synth_state_dict({k: tuple(v.shape) for k, v in m.state_dict().items()}, seed=1), strict=True)
    return m.eval().to(DEV).set_compute_dtype(dtype)


def bench_encoder(iters, repeats, N=64):
    g = torch.Generator(device="cpu").manual_seed(1)
    rigs = {}
    for name, backbone, cin, T in (("resnet18 stereo [64, 2, 300, 64]", "18", 2, 300), ("resnet18 mono [64, 1, 300, 64]", "18", 1, 300),
                                   ("vggish [64, 1, 96, 64]", "vgg", 1, 96)):
        m = _model(backbone, cin, 2, N, [False, False, False], torch.bfloat16)
        audio = (torch.randn((N, cin, T, 64), generator=g) * 0.5).to(DEV)
        rigs[name] = (m, audio)
    with torch.no_grad():
        eager = {k: (lambda m=m, a=a: m._audio_hip(a, m.packed())) for k, (m, a) in rigs.items()}
        graphs = {k: capture(fn) for k, fn in eager.items()}
        us_e = alternate(eager, iters, repeats)
        us_g = alternate({k: gr.replay for k, gr in graphs.items()}, iters, repeats)
    for k in rigs:
        report(f"encoder eager bf16 {k}", **stats(us_e[k]), windows=repeats, calls_per_window=iters)
        report(f"encoder graph bf16 {k}", **stats(us_g[k]), windows=repeats, calls_per_window=iters)


def bench_model(iters, repeats, B):
    from cavp_amd.synth import synth_inputs
    C, hw, lds = 22, (512, 512), [False, True, True]   # output stride 8
    g = torch.Generator(device="cpu").manual_seed(2)
    image = synth_inputs(B, hw, num_classes=C, seed=5)[0].to(DEV)
    rigs = {"18 on [B, 1, 300, 64]": (_model("18", 1, C, B, lds, torch.bfloat16), (torch.randn((B, 1, 300, 64), generator=g) * 0.5).to(DEV)),
            "vgg on [B, 1, 96, 64]": (_model("vgg", 1, C, B, lds, torch.bfloat16), (torch.rand((B, 1, 96, 64), generator=g) * 2 - 1).to(DEV))}
    with torch.no_grad():
        graphs = {k: capture(lambda m=m, a=a: m(image, a, eval_mode=True)) for k, (m, a) in rigs.items()}
        us = alternate({k: gr.replay for k, gr in graphs.items()}, iters, repeats)
    for k in rigs:
        report(f"eval forward graph bf16 B{B} C{C} 512x512 OS8, audio {k}", **stats([u / 1e3 for u in us[k]], "ms", 4),
               windows=repeats, replays_per_window=iters)
    a, b = (statistics.median(us[k]) / 1e3 for k in rigs)
    report("eval forward 18 - vgg", delta_ms_median=round(a - b, 4))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=50)
    ap.add_argument("--repeats", type=int, default=7)
    ap.add_argument("--batch", type=int, default=8)
    ap.add_argument("--no-model", action="store_true")
    ap.add_argument("--jsonl", default="")
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_audio18 needs the GPU: there is nothing to time without one")
    from cavp_amd.hostinfo import cap_torch_threads
    cap_torch_threads()
    bench_stem(a.iters, a.repeats)
    bench_encoder(a.iters, a.repeats)
    if not a.no_model:
        bench_model(max(5, a.iters // 5), a.repeats, a.batch)
    if a.jsonl:
        os.makedirs(os.path.dirname(os.path.abspath(a.jsonl)), exist_ok=True)
        with open(a.jsonl, "a") as f:
            for row in ROWS:
                f.write(json.dumps(row) + "\n")


if __name__ == "__main__":
    main()
