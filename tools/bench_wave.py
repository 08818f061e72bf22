"""The wave stage (cavp_amd.wave.WaveStage: resample to 16 kHz, crop_audio, channel mean, source sum) on two batches, and what it
replaces and costs:

  gpu          one WaveStage call per batch, `iters` back-to-back calls between two device synchronisations, the batches alternating
               inside a round;
  cpu          the same batches the reference's way - float32 conv1d over the WHOLE clip (tests/_wave_ref.py::resample_conv1d_f32,
               the published algorithm; the filter table is rebuilt per item, as the reference does), crop, mean / sum -
               on ONE CPU thread of the same box;
  --step       the stage inside the captured training step: two hipGraphs of the synthetic trainer's iteration at --batch
               (FrameAugment -> LabelStage -> PairBuilder -> MelFrontEnd -> forward, CE + contrast, backward, optimiser), one fed a
               16 kHz clip buffer (the parent step), one with WaveStage on 44.1 kHz int16 stereo PCM at the head of its prologue;
               the two replay alternately, each timed with device events.

Batches (B = 32, audio_len = 1.0):
  stereo_44k1  one 10 s 44.1 kHz stereo source per row (int16);
  mixed_3src   three mono sources per row at 48 / 44.1 / 22.05 / 16 / 8 kHz mixed, 3 .. 10 s (float32).

    python tools/bench_wave.py [--batch 32] [--iters 50] [--rounds 5] [--warmup 5] [--step] [--out profiles/wave_bench.jsonl]

One JSON line per run is appended to --out.  Needs a GPU; there is no fallback."""
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

RATES = (16000, 8000, 22050, 44100, 48000)


def make_batches(B):
    rng = np.random.default_rng(0)
    L = 441000
    a = {"name": "stereo_44k1", "raw": rng.integers(-20000, 20000, (B, 1, 2, L)).astype(np.int16), "length": np.full((B, 1), L, np.int32),
         "rate_idx": np.full((B, 1), RATES.index(44100), np.int32), "n_ch": np.full((B, 1), 2, np.int32)}
    rate_idx = rng.integers(0, len(RATES), (B, 3)).astype(np.int32)
    secs = rng.uniform(3.0, 10.0, (B, 3))
    length = np.minimum((secs * np.array(RATES)[rate_idx]).astype(np.int32), 480000)
    b = {"name": "mixed_3src", "raw": rng.uniform(-0.5, 0.5, (B, 3, 1, 480000)).astype(np.float32), "length": length, "rate_idx": rate_idx,
         "n_ch": np.ones((B, 3), np.int32)}
    return [a, b]


def cpu_route(batch, sample_len, R):
    """The reference's per-item steps on host tensors: whole-clip f32 conv1d, crop, mean over channels, sum over sources."""
    raw = batch["raw"]
    out = torch.zeros(raw.shape[0], 1, sample_len)
    for b in range(raw.shape[0]):
        wave_list = []
        for s in range(raw.shape[1]):
            L, nc = int(batch["length"][b, s]), int(batch["n_ch"][b, s])
            x = torch.from_numpy(raw[b, s, :nc, :L])
            x = x.to(torch.float32) / 32768.0 if x.dtype == torch.int16 else x
            y = R.resample_conv1d_f32(x, RATES[int(batch["rate_idx"][b, s])])
            wave_list.append(torch.mean(R.crop_audio_literal(y, sample_len), dim=0).unsqueeze(0))
        out[b] = torch.stack(wave_list).sum(0)
    return out


def bench_step(a, dev):
    """The training step with and without WaveStage at the head of its captured prologue, replayed alternately."""
    from cavp_amd.audio_frontend import MelFrontEnd
    from cavp_amd.augment import COCO_SCALES, AugResult, FrameAugment
    from cavp_amd.cavp_model import CAVP
    from cavp_amd.contrast import ContrastLoss
    from cavp_amd.labels import LabelResult, LabelStage
    from cavp_amd.optim import FusedSGDAdam
    from cavp_amd.pairs import PairBuilder, PairResult
    from cavp_amd.synth import synth_state_dict
    from cavp_amd.wave import WaveResult, WaveStage
    B, hw, K, L = a.batch, 224, 2, 441000
    hyp = types.SimpleNamespace(seg_model="DeepLabV3Plus", last_three_dilation_stride=[False, False, False], audio_backbone="vgg",
                                num_classes=K, batch_size=B, local_rank=0, audio_len=1.0, spec_min=-100, spec_max=100, allow_random_pvt=True)
    model = CAVP(50, None, num_classes=K, args=hyp)
    model.load_state_dict(synth_state_dict({k: tuple(v.shape) for k, v in model.state_dict().items()}, seed=1))
    model.train().to(dev).set_compute_dtype(torch.bfloat16)
    front = MelFrontEnd(hyp, device=dev)
    crit = ContrastLoss(0.1, 255, 512).use_device_sampler(1, seed=1234)
    pairs = PairBuilder(num_classes=K, bank_slots=B, wave_len=16000, ow_rate=0.5, seed=1234, device=dev, max_batch=B)
    stage = (hw + hw // 2,) * 2
    aug = FrameAugment(crop=(hw, hw), scales=COCO_SCALES, jitter=(.5, .5, .5, .25), seed=1234, device=dev, max_batch=B, stage=stage)
    remap = torch.full((256,), -1, dtype=torch.int32)
    remap[11:10 + K] = torch.arange(1, K, dtype=torch.int32)
    stage_labels = LabelStage(num_classes=K, mode="multi_hot", remap=remap, device=dev, max_batch=B)
    ws = WaveStage(audio_len=1.0, rates=(44100,), max_sources=1, max_channels=2, max_len=L, device=dev, max_batch=B)
    g = torch.Generator().manual_seed(0)
    s_frames = torch.randint(0, 256, (B,) + stage + (3,), dtype=torch.uint8, generator=g).to(dev)
    masks = torch.zeros((B,) + stage, dtype=torch.uint8)
    masks[:, 40:150, 60:200] = 11
    s_masks = masks.to(dev)
    s_sizes = torch.tensor([list(stage)] * B, dtype=torch.int32, device=dev)
    s_wave = (torch.randn(B, 1, 16000, generator=g) * 0.1).to(dev)
    s_pcm = torch.randint(-3277, 3278, (B, 1, 2, L), dtype=torch.int16, generator=g).to(dev)
    s_len = torch.full((B, 1), L, dtype=torch.int32, device=dev)
    s_rate, s_nch = torch.zeros((B, 1), dtype=torch.int32, device=dev), torch.full((B, 1), 2, dtype=torch.int32, device=dev)
    s_image = torch.zeros(B, 3, hw, hw, device=dev)
    s_label = torch.zeros(B, hw, hw, dtype=torch.int64, device=dev)
    s_img_label = torch.zeros(B, K, dtype=torch.int64, device=dev)
    s_audio = torch.zeros(2 * B, 1, front.n_frames, front.n_mels, device=dev)
    s_shuf = torch.zeros_like(s_label)
    built, cut = PairResult(B, 16000, K, (hw, hw), dev), WaveResult(B, 16000, dev)
    augmented, labelled = AugResult(B, (hw, hw), dev), LabelResult(B, K, (hw, hw), dev, True)
    opt = FusedSGDAdam(model, model.grad_arena(dev), 1e-3, momentum=0.9, weight_decay=1e-4)
    opt.use_device_schedule(1e-3, 0.9, 100000, 0)

    def prologue_of(raw_audio):
        def prologue():
            if raw_audio:
                ws(s_pcm, s_len, s_rate, s_nch, out=cut)
            aug(s_frames, s_masks, s_sizes, out=augmented)
            stage_labels(augmented.label, out=labelled)
            s_image.copy_(augmented.image)
            s_label.copy_(labelled.label)
            s_img_label.copy_(labelled.img_label)
            pairs(cut.waveform if raw_audio else s_wave, s_label, s_img_label, True, out=built)
            s_audio.copy_(front(built.waveforms))
            s_shuf.copy_(built.label_shuffle)
        return prologue
    reps = {k: model.capture_train_step(s_image, s_audio, s_label, contrast=crit, label_shuffle=s_shuf, contrast_weight=1.0, optimizer=opt,
                                        prologue=prologue_of(k == "with_wave_stage")) for k in ("parent_step", "with_wave_stage")}
    for _ in range(a.warmup):
        for rep in reps.values():
            rep()
    torch.cuda.synchronize()
    times = {k: [] for k in reps}
    for _ in range(a.step_iters):
        for k, rep in reps.items():
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            rep()
            e1.record()
            e1.synchronize()
            times[k].append(e0.elapsed_time(e1))
    ws.check()
    res = {k: {"ms_median": round(statistics.median(v), 4), "ms_min": round(min(v), 4), "ms_max": round(max(v), 4)} for k, v in times.items()}
    res["overhead_ms_median"] = round(res["with_wave_stage"]["ms_median"] - res["parent_step"]["ms_median"], 4)
    res["replays_each"] = a.step_iters
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=32)
    ap.add_argument("--iters", type=int, default=50)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--cpu-rounds", type=int, default=1)
    ap.add_argument("--step", action="store_true", help="also time the captured training step with and without the stage")
    ap.add_argument("--step-iters", type=int, default=30)
    ap.add_argument("--out", default=os.path.join(REPO, "profiles", "wave_bench.jsonl"))
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_wave.py needs the GPU: a CPU run says nothing about these timings")
    from cavp_amd.hostinfo import cap_torch_threads
    from cavp_amd.wave import WaveResult, WaveStage
    from tests import _wave_ref as R
    cap_torch_threads()
    dev = torch.device("cuda", 0)
    B, sample_len = a.batch, 16000
    batches = make_batches(B)
    fns, keep = {}, []
    for bt in batches:
        ws = WaveStage(audio_len=1.0, rates=RATES, max_sources=bt["raw"].shape[1], max_channels=bt["raw"].shape[2],
                       max_len=bt["raw"].shape[3], device=dev, max_batch=B)
        ins = [torch.from_numpy(bt[k]).to(dev) for k in ("raw", "length", "rate_idx", "n_ch")]
        out = WaveResult(B, sample_len, dev)
        fns[bt["name"]] = (lambda ws=ws, ins=ins, out=out: ws(*ins, out=out))
        keep.append((ws, out))
    for f in fns.values():
        for _ in range(a.warmup):
            f()
    torch.cuda.synchronize()
    times = {k: [] for k in fns}
    for _ in range(a.rounds):
        for k, f in fns.items():
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            for _ in range(a.iters):
                f()
            torch.cuda.synchronize()
            times[k].append((time.perf_counter() - t0) / a.iters * 1e3)
    rec = {"bench": "wave", "device": torch.cuda.get_device_name(0), "batch": B, "sample_len": sample_len, "iters": a.iters, "rounds": a.rounds,
           "gpu": {}, "cpu_one_thread": {}}
    for k, v in times.items():
        rec["gpu"][k] = {"ms_median": round(statistics.median(v), 4), "ms_min": round(min(v), 4), "ms_max": round(max(v), 4)}
    torch.set_num_threads(1)
    for bt, (ws, out) in zip(batches, keep):
        ws.check()
        cpu_ms = []
        for _ in range(a.cpu_rounds):
            t0 = time.perf_counter()
            ref = cpu_route(bt, sample_len, R)
            cpu_ms.append((time.perf_counter() - t0) * 1e3)
        rec["cpu_one_thread"][bt["name"]] = {"ms_median": round(statistics.median(cpu_ms), 1), "rounds": a.cpu_rounds,
                                             "max_abs_diff_to_gpu": float((out.waveform.cpu() - ref).abs().max()),
                                             "rms": round(float(ref.square().mean().sqrt()), 5)}
    if a.step:
        rec["step"] = bench_step(a, dev)
    line = json.dumps(rec)
    print(line, flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "a") as f:
        f.write(line + "\n")


if __name__ == "__main__":
    main()
