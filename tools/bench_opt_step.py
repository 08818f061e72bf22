"""What recording the optimiser step in the training graph costs or saves, two ways in one process:

  (a) replay + eager step   the captured training step (forward, CE, backward: one hipGraph) followed by the host-scheduled
                            FusedSGDAdam.step(sched(it)): a schedule value computed on the host and one eager launch per iteration;
  (b) replay, step recorded the same capture with optimizer= (FusedSGDAdam.use_device_schedule): the schedule launch and the update
                            are the graph's last two nodes, the iteration is one replay;
  (c) optimiser alone       the two launches of the device-scheduled step(), eager, nothing else on the GPU: their time and the
                            bytes of the job table (SGD: 3 reads + 2 writes, Adam: 4 reads + 3 writes of 4 bytes per element)
                            over it.

    python tools/bench_opt_step.py [--batch 32] [--hw 224] [--dtype bf16] [--iters 20] [--rounds 5] [--warmup 5]
                                   [--out profiles/opt_sched_bench.jsonl]

Default shape: c1p (ResNet-50 224 x 224 OS16, VGGish audio, 2 classes), B = 32, bf16.  A round times `iters` back-to-back iterations of
each variant between two device synchronisations with a host clock; the variants alternate inside a round (the protocol of
tools/bench_pairs.py).  All variants update the same model, so the weights drift over the run; the kernels' work does not depend on
the values.  One JSON line per run is appended to --out.  Needs a GPU; there is no fallback."""
import argparse
import json
import os
import statistics
import sys
import time
import types

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch

HBM_PEAK_GBS = 8000.0   # MI355X: 8 TB/s


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=32)
    ap.add_argument("--hw", type=int, default=224)
    ap.add_argument("--dtype", choices=["bf16", "f32"], default="bf16")
    ap.add_argument("--lr", type=float, default=1e-4)
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--out", default=os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "profiles", "opt_sched_bench.jsonl"))
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_opt_step.py needs the GPU: a CPU run says nothing about these timings")
    from cavp_amd.cavp_model import CAVP
    from cavp_amd.hostinfo import cap_torch_threads
    from cavp_amd.optim import FusedSGDAdam, warmup_poly_lr
    from cavp_amd.synth import synth_inputs, synth_state_dict
    cap_torch_threads()
    dev = torch.device("cuda", 0)
    B, total_iters = a.batch, 100000     # (the run takes a few hundred steps: the rate stays in the poly range)
    hyp = types.SimpleNamespace(seg_model="DeepLabV3Plus", last_three_dilation_stride=[False, False, False], audio_backbone="vgg",
                                num_classes=2, batch_size=B, local_rank="cpu")
    model = CAVP(50, None, num_classes=2, args=hyp)
    model.load_state_dict(synth_state_dict({k: tuple(v.shape) for k, v in model.state_dict().items()}, seed=1))
    model.train().to(dev).set_compute_dtype(torch.bfloat16 if a.dtype == "bf16" else torch.float32)
    image, audio, label = [t.to(dev) for t in synth_inputs(B, (a.hw, a.hw), audio_batch=2 * B, num_classes=2, seed=0)]

    arena = model.grad_arena(dev)
    opt_host = FusedSGDAdam(model, arena, a.lr)
    opt_dev = FusedSGDAdam(model, arena, a.lr).use_device_schedule(a.lr, 0.9, total_iters)
    sched = warmup_poly_lr(a.lr, 0.9, total_iters, 0)
    replay_plain = model.capture_train_step(image, audio, label)
    replay_opt = model.capture_train_step(image, audio, label, optimizer=opt_dev)
    it_host = [0]

    def variant_a():
        replay_plain()
        it = it_host[0]
        opt_host.step(sched(it - 1) if it > 0 else a.lr)
        it_host[0] = it + 1

    fns = {"a_replay_then_eager_step": variant_a, "b_replay_with_recorded_step": replay_opt, "c_optimizer_alone": opt_dev.step}
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

    audio_ids = {id(p) for p in model.audio_backbone.parameters()}
    n_adam = sum(p.numel() for p in opt_dev.params if id(p) in audio_ids)
    n_sgd = sum(p.numel() for p in opt_dev.params if id(p) not in audio_ids)
    nbytes = 20 * n_sgd + 28 * n_adam
    rec = {"bench": "opt_step", "device": torch.cuda.get_device_name(0), "config": "c1p", "batch": B, "hw": a.hw, "dtype": a.dtype,
           "iters": a.iters, "rounds": a.rounds, "tensors": opt_dev.njobs, "workgroups": opt_dev.total_blocks, "sgd_elements": n_sgd,
           "adam_elements": n_adam, "optimizer_bytes": nbytes, "device_steps_taken": opt_dev.iteration(), "variants": {}}
    for k, v in times.items():
        rec["variants"][k] = {"ms_median": round(statistics.median(v), 4), "ms_min": round(min(v), 4), "ms_max": round(max(v), 4)}
    ms_opt = rec["variants"]["c_optimizer_alone"]["ms_median"]
    rec["optimizer_gb_per_s"] = round(nbytes / (ms_opt * 1e-3) / 1e9, 1)
    rec["optimizer_frac_of_hbm_peak"] = round(rec["optimizer_gb_per_s"] / HBM_PEAK_GBS, 3)
    va, vb = rec["variants"]["a_replay_then_eager_step"], rec["variants"]["b_replay_with_recorded_step"]
    rec["b_minus_a_ms_median"] = round(vb["ms_median"] - va["ms_median"], 4)
    rec["spread_ms"] = round(max(va["ms_max"] - va["ms_min"], vb["ms_max"] - vb["ms_min"]), 4)
    line = json.dumps(rec)
    print(line, flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "a") as f:
        f.write(line + "\n")


if __name__ == "__main__":
    main()
