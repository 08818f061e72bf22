"""What drawing PVT's DropPath masks on the device costs or saves in the captured training step, two ways in one process:

  (a) host refresh     today's default: before every replay the host draws one torch.rand((B, 1, 1)) per branch from the default CPU
                       generator, stages the rows in pinned memory (waiting on the previous upload's event) and enqueues one
                       asynchronous copy into the buffer the graph reads (pvt_train.refresh_drop_path);
  (b) device sampler   model.use_device_drop_path(): one launch of cavp_drop_path_draw inside the graph, replay() is the bare replay.

    python tools/bench_droppath.py [--batch 8] [--hw 512] [--dtype bf16] [--iters 20] [--rounds 7] [--warmup 5]
                                   [--out profiles/droppath_bench.jsonl]

Default shape: config #4 (PVTv2-B5, 512 x 512, 71 classes, VGGish audio), B = 8, bf16.  A round times `iters` back-to-back replays of
each variant between two device synchronisations with a host clock, and inside that window the host time spent in the replay()
calls themselves (wall clock and this thread's CPU time); the variants alternate inside a round (the protocol of
tools/bench_pairs.py).  The spread is the host variant's own max - min over the rounds; the device variant is accepted when its
median is not above the host variant's by more than that.  No update is recorded, so the weights stay put.  One JSON line per run
is appended to --out.  Needs a GPU; there is no fallback."""
import argparse
import json
import os
import statistics
import sys
import time
import types

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=8)
    ap.add_argument("--hw", type=int, default=512)
    ap.add_argument("--num-classes", type=int, default=71)
    ap.add_argument("--dtype", choices=["bf16", "f32"], default="bf16")
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--out", default=os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "profiles", "droppath_bench.jsonl"))
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_droppath.py needs the GPU: a CPU run says nothing about these timings")
    from cavp_amd.cavp_model import CAVP
    from cavp_amd.hostinfo import cap_torch_threads
    from cavp_amd.synth import synth_inputs, synth_state_dict
    cap_torch_threads()
    dev = torch.device("cuda", 0)
    B, K = a.batch, a.num_classes
    hyp = types.SimpleNamespace(seg_model="PVT", last_three_dilation_stride=[False, False, False], audio_backbone="vgg",
                                num_classes=K, batch_size=B, local_rank="cpu", allow_random_pvt=True)
    model = CAVP(50, None, num_classes=K, args=hyp)
    model.load_state_dict(synth_state_dict({k: tuple(v.shape) for k, v in model.state_dict().items()}, seed=1))
    model.train().to(dev).set_compute_dtype(torch.bfloat16 if a.dtype == "bf16" else torch.float32)
    image, audio, label = [t.to(dev) for t in synth_inputs(B, (a.hw, a.hw), audio_batch=2 * B, num_classes=K, seed=0)]

    replay_host = model.capture_train_step(image, audio, label)          # captured without a sampler: replay() refreshes on the host
    dp = model.use_device_drop_path(seed=0)
    replay_dev = model.capture_train_step(image, audio, label)           # the draw is a node of this graph
    n_branches = int(model.backbone._dp_buf.shape[0])
    fns = {"a_host_refresh": replay_host, "b_device_sampler": replay_dev}
    for f in fns.values():
        for _ in range(a.warmup):
            f()
    torch.cuda.synchronize()
    off0 = dp.offset()
    ms = {k: [] for k in fns}
    wall_us = {k: [] for k in fns}
    cpu_us = {k: [] for k in fns}
    for _ in range(a.rounds):
        for k, f in fns.items():
            torch.cuda.synchronize()
            in_call = in_cpu = 0.0
            t0 = time.perf_counter()
            for _ in range(a.iters):
                w0, c0 = time.perf_counter(), time.thread_time()
                f()
                in_call += time.perf_counter() - w0
                in_cpu += time.thread_time() - c0
            torch.cuda.synchronize()
            ms[k].append((time.perf_counter() - t0) / a.iters * 1e3)
            wall_us[k].append(in_call / a.iters * 1e6)
            cpu_us[k].append(in_cpu / a.iters * 1e6)
    if dp.offset() - off0 != a.rounds * a.iters:
        raise SystemExit(f"the device sampler drew {dp.offset() - off0} times in {a.rounds * a.iters} replays")

    def stat(v, nd):
        return {"median": round(statistics.median(v), nd), "min": round(min(v), nd), "max": round(max(v), nd)}
    rec = {"bench": "droppath", "device": torch.cuda.get_device_name(0), "config": "c4", "batch": B, "hw": a.hw, "num_classes": K,
           "dtype": a.dtype, "iters": a.iters, "rounds": a.rounds, "branches": n_branches, "variants": {}}
    for k in fns:
        rec["variants"][k] = {"ms_per_iter": stat(ms[k], 4), "host_us_in_replay_call": stat(wall_us[k], 1),
                              "host_cpu_us_in_replay_call": stat(cpu_us[k], 1)}
    va, vb = rec["variants"]["a_host_refresh"], rec["variants"]["b_device_sampler"]
    rec["b_minus_a_ms_median"] = round(vb["ms_per_iter"]["median"] - va["ms_per_iter"]["median"], 4)
    rec["host_spread_ms"] = round(va["ms_per_iter"]["max"] - va["ms_per_iter"]["min"], 4)     # run-to-run spread of the host variant itself
    rec["device_not_slower_than_host_by_more_than_spread"] = rec["b_minus_a_ms_median"] <= rec["host_spread_ms"]
    line = json.dumps(rec)
    print(line, flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "a") as f:
        f.write(line + "\n")


if __name__ == "__main__":
    main()
