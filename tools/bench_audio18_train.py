#!/usr/bin/env python3
"""Time the training of the ResNet-18 audio encoder (audio_backbone="18", CAVP.use_audio18_training).  Protocol of
tools/bench_audio18.py: device events around back-to-back calls, the variants of a comparison alternating in one process in
`--repeats` windows of `--iters` calls; per variant the median window, min, max and the spread (max - min).

  * stem rows: the one launch (cavp_audio_stem_train: conv 7x7/2 raw + the BatchNorm tile statistics of its output) against the two
    launches it replaces (ops.conv_smallcin_kxk 7/2/3, then train_ops.col_tile_stats over the map) on [64, 2, 300, 64] and
    [64, 1, 300, 64], bf16 and f32.  The maps and the statistics the two tables give are compared before anything is timed.  The keep
    rule: the one launch stays only if it wins by more than the larger run-to-run spread (`fused_wins`).
  * encoder rows: forward + backward of the encoder alone on a TrainPass tape (pack, forward, an upstream gradient, backward), eager and
    as a graph replay, stereo and mono [64, ., 300, 64] next to the VGGish encoder on [64, 1, 96, 64], bf16.
  * step rows (unless --no-model): the captured training step at the VPO-SS shape (512 x 512, output stride 8, 22 classes, B = 8,
    bf16) with "18" on [2B, 1, 300, 64] against the "vgg" plumbing variant on [2B, 1, 96, 64], replays alternating.

Prints one JSON line per row; --jsonl appends them to a file.

usage: python tools/bench_audio18_train.py [--iters 30] [--repeats 7] [--batch 8] [--no-model] [--jsonl profiles/audio18_train_bench.jsonl]
"""
import argparse
import json
import os
import statistics
import sys

import torch

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
sys.path.insert(0, os.path.join(REPO, "tools"))

from bench_audio18 import DEV, ROWS, alternate, capture, report, stats  # noqa: E402
from cavp_amd import train_ops as T  # noqa: E402


def bench_stem(iters, repeats, N=64, Tm=300, Fq=64):
    g = torch.Generator(device="cpu").manual_seed(0)
    hs, ws = (Tm - 1) // 2 + 1, (Fq - 1) // 2 + 1
    rows = N * hs * ws
    ones, zeros = torch.ones(64, device=DEV), torch.zeros(64, device=DEV)
    for cin in (2, 1):
        x = (torch.randn((N, cin, Tm, Fq), generator=g) * 0.5).to(DEV)
        w = (torch.randn((64, cin, 7, 7), generator=g) * (2.0 / (49 * cin)) ** 0.5).to(DEV)
        for dtype in (torch.bfloat16, torch.float32):
            es = 2 if dtype == torch.bfloat16 else 4
            z1 = torch.empty((N, hs, ws, 64), dtype=dtype, device=DEV)
            z2 = torch.empty_like(z1)

            def fused():
                return T.audio_stem_train(x, w, z1, fused=True)

            def two():
                return T.audio_stem_train(x, w, z2, fused=False)

            res = []
            for tab in (fused(), two()):
                f = lambda: torch.empty(64, device=DEV)   # noqa: E731
                sc, sh, mean, rstd = f(), f(), f(), f()
                T.bn_finalize_tiles(tab[0], tab[1], tab[2], rows, ones, zeros, 1e-5, 0.1, None, None, sc, sh, mean, rstd)
                res.append((tab[1], tab[2], mean, rstd))
            torch.cuda.synchronize()
            if res[0][1] == 128 and res[0][0] == res[1][0]:
                raise SystemExit("the one launch declined this shape: nothing to compare")
            err = float((z1.float() - z2.float()).abs().max())
            tol = (2e-4 if dtype == torch.float32 else 2.0 ** -7) * max(1.0, float(z2.float().abs().max()))
            d_mean = float((res[0][2] - res[1][2]).abs().max())
            d_rstd = float(((res[0][3] - res[1][3]).abs() / res[1][3]).max())
            if not (err <= tol and d_mean <= 1e-5 and d_rstd <= 1e-5):
                raise SystemExit(f"one-launch stem differs from the two-launch route: map {err}, mean {d_mean}, rstd {d_rstd} (cin={cin}, {dtype})")
            common = x.numel() * 4 + w.numel() * 4 + z1.numel() * es
            us = alternate({"fused": fused, "two": two}, iters, repeats)
            tag = f"[{N}, {cin}, {Tm}, {Fq}] {str(dtype).split('.')[-1]}"
            report(f"train stem one launch {tag}", **stats(us["fused"]), bytes=common, tiles=res[0][0], rows_per_tile=res[0][1],
                   windows=repeats, calls_per_window=iters)
            report(f"train stem two launches {tag}", **stats(us["two"]), bytes=common + z1.numel() * es, tiles=res[1][0],
                   rows_per_tile=res[1][1], windows=repeats, calls_per_window=iters)
            gain = statistics.median(us["two"]) - statistics.median(us["fused"])
            spread = max(max(v) - min(v) for v in us.values())
            report(f"train stem two launches - one launch {tag}", delta_us_median=round(gain, 2), larger_spread_us=round(spread, 2),
                   fused_wins=bool(gain > spread), max_abs_diff=err, mean_diff=d_mean, rstd_rel_diff=d_rstd)
            del z1, z2


def _model(audio_backbone, in_plane, C, B, lds, dtype):
    import types

    from cavp_amd.cavp_model import CAVP
    from cavp_amd.synth import synth_state_dict
    args = types.SimpleNamespace(seg_model="DeepLabV3Plus", last_three_dilation_stride=lds, audio_backbone=audio_backbone,
                                 num_classes=C, batch_size=B, local_rank="cpu")
    m = CAVP(50, None, num_classes=C, args=args, in_plane=in_plane)
    m.load_state_dict(synth_state_dict({k: tuple(v.shape) for k, v in m.state_dict().items()}, seed=1), strict=True)
    m.train().to(DEV).set_compute_dtype(dtype)
    if audio_backbone == "18":
        m.use_audio18_training()
    return m


def _encoder_pass(m, audio, g):
    """pack + forward + backward of the audio encoder alone on a tape of its own (what CAVPStageFunction runs for forward_audio), the
    gradients landing in the model's flat arena as in the native step"""
    from cavp_amd.train import TrainPass, _audio_stage, _pack_audio, bump_counters
    arena = m.grad_arena(DEV)

    def run():
        arena.zero()
        tp = TrainPass(m, m.compute_dtype, arena=arena)
        _pack_audio(tp, m)
        tp.flush_packs()
        fea = _audio_stage(tp, audio)
        if tp._nbt:
            bump_counters(m, tp._nbt)
            tp._nbt = []
        fea.set_g(g.clone())
        tp.backward()
        tp.finish_padded()
    return run


def bench_encoder(iters, repeats, N=64):
    g = torch.Generator(device="cpu").manual_seed(1)
    rigs = {}
    for name, backbone, cin, Tm in (("resnet18 stereo [64, 2, 300, 64]", "18", 2, 300), ("resnet18 mono [64, 1, 300, 64]", "18", 1, 300),
                                    ("vggish [64, 1, 96, 64]", "vgg", 1, 96)):
        m = _model(backbone, cin, 2, N, [False, False, False], torch.bfloat16)
        audio = (torch.randn((N, cin, Tm, 64), generator=g) * 0.5).to(DEV)
        up = torch.randn((N, m.latent_dim), generator=g).to(DEV).to(torch.bfloat16)
        rigs[name] = _encoder_pass(m, audio, up)
    with torch.no_grad():
        graphs = {k: capture(fn) for k, fn in rigs.items()}
        us_e = alternate(rigs, max(3, iters // 5), repeats)
        us_g = alternate({k: gr.replay for k, gr in graphs.items()}, iters, repeats)
    for k in rigs:
        report(f"encoder fwd+bwd eager bf16 {k}", **stats(us_e[k]), windows=repeats, calls_per_window=max(3, iters // 5))
        report(f"encoder fwd+bwd graph bf16 {k}", **stats(us_g[k]), windows=repeats, calls_per_window=iters)


def bench_step(iters, repeats, B):
    from cavp_amd.synth import synth_inputs
    C, hw, lds = 22, (512, 512), [False, True, True]   # output stride 8
    g = torch.Generator(device="cpu").manual_seed(2)
    image, _, label = (t.to(DEV) for t in synth_inputs(B, hw, audio_batch=2 * B, num_classes=C, seed=5))
    audios = {"18 on [2B, 1, 300, 64]": ("18", (torch.randn((2 * B, 1, 300, 64), generator=g) * 0.5).to(DEV)),
              "vgg on [2B, 1, 96, 64]": ("vgg", (torch.rand((2 * B, 1, 96, 64), generator=g) * 2 - 1).to(DEV))}
    replays = {}
    for k, (backbone, audio) in audios.items():
        m = _model(backbone, 1, C, B, lds, torch.bfloat16)
        replays[k] = m.capture_train_step(image, audio, label)
    us = alternate(replays, iters, repeats)
    for k in replays:
        report(f"captured train step bf16 B{B} C{C} 512x512 OS8, audio {k}", **stats([u / 1e3 for u in us[k]], "ms", 4),
               windows=repeats, replays_per_window=iters)
    a, b = (statistics.median(us[k]) / 1e3 for k in replays)
    report("captured train step 18 - vgg", delta_ms_median=round(a - b, 4))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=30)
    ap.add_argument("--repeats", type=int, default=7)
    ap.add_argument("--batch", type=int, default=8)
    ap.add_argument("--no-model", action="store_true")
    ap.add_argument("--jsonl", default="")
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_audio18_train needs the GPU: there is nothing to time without one")
    from cavp_amd.hostinfo import cap_torch_threads
    cap_torch_threads()
    bench_stem(a.iters, a.repeats)
    bench_encoder(a.iters, a.repeats)
    if not a.no_model:
        bench_step(max(5, a.iters // 3), a.repeats, a.batch)
    if a.jsonl:
        os.makedirs(os.path.dirname(os.path.abspath(a.jsonl)), exist_ok=True)
        with open(a.jsonl, "a") as f:
            for row in ROWS:
                f.write(json.dumps(row) + "\n")


if __name__ == "__main__":
    main()
