"""What gradient accumulation costs in the captured iteration, in one process:

  (a) the accumulate launch alone on the model's real arena, eager and back to back, with the state block's k pinned:
        a_k0     k = 0       acc <- g          1 read + 1 write per element
        a_add    0 < k < N-1 acc <- acc + g    2 reads + 1 write
        a_close  k = N-1     g <- acc + g      2 reads + 1 write
      and beside it, on the same two buffers, torch's `acc.copy_(g)` and `acc.add_(g)` (they move the whole flat arena, the
      launch the elements of the optimiser's job table: both byte counts are in the record).  The acceptance rule: the HIP launch
      is not slower than the torch op that moves the same bytes by more than that op's min-to-max spread over the rounds.
  (b) the captured step with `optimizer=` as without this feature, against the same step with `accumulate=` at N (default 8), in
      ms per replay; next to them the eager update alone (u) and the accumulator's micro-step launches alone (s).  The expectation
      the record checks: accumulating replay ~ plain replay + (a) - (N - 1) / N of the update's time.

    python tools/bench_accumulate.py [--batch 32] [--hw 224] [--dtype bf16] [--micro-steps 8] [--iters 24] [--rounds 5]
                                     [--warmup 8] [--out profiles/accumulate_bench.jsonl]

Default shape: c1p (ResNet-50 224 x 224 OS16, VGGish audio, 2 classes), B = 32, bf16 - bench.py's headline shape; the protocol of
tools/bench_step_guard.py (host clock around `iters` back-to-back calls between two synchronisations, the variants alternating
inside each of `rounds` rounds; --iters is rounded up to a multiple of N so that every timed stretch holds whole windows).  One JSON
line per run is appended to --out.  Needs a GPU; there is no fallback."""
import argparse
import ctypes as C
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
    ap.add_argument("--batch", type=int, default=32)
    ap.add_argument("--hw", type=int, default=224)
    ap.add_argument("--dtype", choices=["bf16", "f32"], default="bf16")
    ap.add_argument("--lr", type=float, default=1e-4)
    ap.add_argument("--micro-steps", type=int, default=8)
    ap.add_argument("--iters", type=int, default=24)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=8)
    ap.add_argument("--out", default=os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "profiles", "accumulate_bench.jsonl"))
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_accumulate.py needs the GPU: a CPU run says nothing about these timings")
    from cavp_amd import _lib
    from cavp_amd.accumulate import AccumState, GradAccumulator
    from cavp_amd.cavp_model import CAVP
    from cavp_amd.hostinfo import cap_torch_threads
    from cavp_amd.ops import _ptr, _stream
    from cavp_amd.optim import FusedSGDAdam
    from cavp_amd.synth import synth_inputs, synth_state_dict
    cap_torch_threads()
    dev = torch.device("cuda", 0)
    B, N, total_iters = a.batch, a.micro_steps, 100000
    iters = (a.iters + N - 1) // N * N
    hyp = types.SimpleNamespace(seg_model="DeepLabV3Plus", last_three_dilation_stride=[False, False, False], audio_backbone="vgg",
                                num_classes=2, batch_size=B, local_rank="cpu")
    model = CAVP(50, None, num_classes=2, args=hyp)
    model.load_state_dict(synth_state_dict({k: tuple(v.shape) for k, v in model.state_dict().items()}, seed=1))
    model.train().to(dev).set_compute_dtype(torch.bfloat16 if a.dtype == "bf16" else torch.float32)
    image, audio, label = [t.to(dev) for t in synth_inputs(B, (a.hw, a.hw), audio_batch=2 * B, num_classes=2, seed=0)]
    arena = model.grad_arena(dev)

    def optimiser():
        return FusedSGDAdam(model, arena, a.lr).use_device_schedule(a.lr, 0.9, total_iters)
    opt_plain, opt_acc, opt_alone = optimiser(), optimiser(), optimiser()
    acc, acc_alone = GradAccumulator(opt_acc, N), GradAccumulator(opt_alone, max(N, 3))
    replay_plain = model.capture_train_step(image, audio, label, optimizer=opt_plain)
    replay_acc = model.capture_train_step(image, audio, label, optimizer=opt_acc, accumulate=acc)

    lib = _lib.load()
    tab, nj, nb = _ptr(opt_alone.table), opt_alone.njobs, opt_alone.total_blocks
    n_alone = acc_alone.micro_steps

    def launch_alone():
        lib.cavp_grad_accumulate(tab, nj, nb, _ptr(arena.flat), _ptr(acc_alone.flat), _ptr(acc_alone._state), C.c_void_p(_stream()))

    def pinned(k):
        def f():
            launch_alone()
        f.k = k
        return f

    fns = {"a_k0_launch_alone": pinned(0), "a_add_launch_alone": pinned(1), "a_close_launch_alone": pinned(n_alone - 1),
           "t_torch_copy": lambda: acc_alone.flat.copy_(arena.flat), "t_torch_add": lambda: acc_alone.flat.add_(arena.flat),
           "b_replay_plain": replay_plain, "b_replay_accumulate": replay_acc, "u_update_alone": opt_plain.step,
           "s_micro_step_launches_alone": acc_alone.step}

    def prepare(f):
        arena.flat.normal_(0.0, 1e-3)   # random data, as a run has (an all-zero buffer can clock differently); small enough
        acc_alone.flat.normal_(0.0, 1e-3)   # that the repeated adds of a timed stretch stay finite
        if hasattr(f, "k"):
            acc_alone._set_k(f.k)     # only the accumulate launch follows, so k stays where it is put
        elif f is fns["s_micro_step_launches_alone"]:
            acc_alone.reset()
    for f in fns.values():
        prepare(f)
        for _ in range(max(a.warmup, N)):
            f()
    torch.cuda.synchronize()
    times = {k: [] for k in fns}
    for _ in range(a.rounds):
        for k, f in fns.items():
            prepare(f)
            if f is replay_acc:
                acc.reset()
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            for _ in range(iters):
                f()
            torch.cuda.synchronize()
            times[k].append((time.perf_counter() - t0) / iters * 1e3)

    table_elems = sum(p.numel() for p in opt_alone.params)
    flat_elems = arena.flat.numel()
    rec = {"bench": "accumulate", "device": torch.cuda.get_device_name(0), "config": "c1p", "batch": B, "hw": a.hw, "dtype": a.dtype,
           "micro_steps": N, "iters": iters, "rounds": a.rounds, "tensors": nj, "workgroups": nb, "table_elements": table_elems,
           "arena_elements": flat_elems, "accumulator_bytes": acc.nbytes, "state_bytes": C.sizeof(AccumState),
           "launches_per_micro_step": acc.launch_names(), "windows_closed_by_b": acc.read()["windows"], "variants": {}}
    for k, v in times.items():
        rec["variants"][k] = {"ms_median": round(statistics.median(v), 4), "ms_min": round(min(v), 4), "ms_max": round(max(v), 4)}
    med = {k: v["ms_median"] for k, v in rec["variants"].items()}
    spread = {k: round(v["ms_max"] - v["ms_min"], 4) for k, v in rec["variants"].items()}
    bytes_of = {"a_k0_launch_alone": 8 * table_elems, "a_add_launch_alone": 12 * table_elems, "a_close_launch_alone": 12 * table_elems,
                "t_torch_copy": 8 * flat_elems, "t_torch_add": 12 * flat_elems}
    rec["bytes"] = bytes_of
    rec["gb_per_s"] = {k: round(b / (med[k] * 1e-3) / 1e9, 1) for k, b in bytes_of.items()}
    rec["us"] = {k: round(med[k] * 1e3, 2) for k in bytes_of}
    rec["spread_ms"] = spread
    rec["k0_minus_torch_copy_ms"] = round(med["a_k0_launch_alone"] - med["t_torch_copy"], 4)
    rec["add_minus_torch_add_ms"] = round(med["a_add_launch_alone"] - med["t_torch_add"], 4)
    rec["close_minus_torch_add_ms"] = round(med["a_close_launch_alone"] - med["t_torch_add"], 4)
    rec["k0_within_torch_spread"] = bool(rec["k0_minus_torch_copy_ms"] <= spread["t_torch_copy"])
    rec["add_within_torch_spread"] = bool(rec["add_minus_torch_add_ms"] <= spread["t_torch_add"])
    rec["close_within_torch_spread"] = bool(rec["close_minus_torch_add_ms"] <= spread["t_torch_add"])
    # (b): per window one copy, N - 2 adds and one close; the update's share of a replay falls from 1 to 1 / N
    per_replay_accumulate = (med["a_k0_launch_alone"] + (N - 2) * med["a_add_launch_alone"] + med["a_close_launch_alone"]) / N \
        if N > 1 else 0.0
    rec["accumulate_minus_plain_ms_median"] = round(med["b_replay_accumulate"] - med["b_replay_plain"], 4)
    rec["expected_difference_ms"] = round(per_replay_accumulate - (N - 1) / N * med["u_update_alone"], 4)
    print(json.dumps(rec), flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "a") as f:
        f.write(json.dumps(rec) + "\n")


if __name__ == "__main__":
    main()
