"""What the step guard costs in the captured iteration, in one process:

  (a) replay, update recorded            the parent's captured step: forward, CE, backward, schedule launch, update launch;
  (b) the same with a guard              StepGuard(max_norm=None): block partials, combine, guarded schedule, guarded update;
  (c) the same with clipping             StepGuard(max_norm=...) with a bound below the gradient norm, so every step clips;
  (d) the guard's four launches alone    eager, nothing else on the GPU;
  (e) / (f) / (g)                        the partials launch, the guarded update launch and the combine launch alone, each back to
                                         back: the bytes of the gradient arena over (e) and the update's bytes over (f) are the two
                                         bandwidths the acceptance rule compares.

    python tools/bench_step_guard.py [--batch 32] [--hw 224] [--dtype bf16] [--iters 20] [--rounds 5] [--warmup 5]
                                     [--launch-floor-us 6] [--out profiles/step_guard_bench.jsonl]

Default shape: c1p (ResNet-50 224 x 224 OS16, VGGish audio, 2 classes), B = 32, bf16; the protocol of tools/bench_opt_step.py (host clock
around `iters` back-to-back iterations between two synchronisations, the variants alternating inside each of `rounds` rounds).  All
variants update the same model; the kernels' work does not depend on the values.  The allowance for (b) - (a) that the record carries:
arena bytes / the bandwidth of (f), plus three dependent small launches at --launch-floor-us (4.5 .. 6 us), plus the
min-to-max spread of (a).  One JSON line per run is appended to --out.  Needs a GPU; there is no fallback."""
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
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--launch-floor-us", type=float, default=6.0)
    ap.add_argument("--out", default=os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "profiles", "step_guard_bench.jsonl"))
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_step_guard.py needs the GPU: a CPU run says nothing about these timings")
    from cavp_amd import _lib
    from cavp_amd.cavp_model import CAVP
    from cavp_amd.hostinfo import cap_torch_threads
    from cavp_amd.ops import _ptr, _stream
    from cavp_amd.optim import FusedSGDAdam, StepGuard
    from cavp_amd.synth import synth_inputs, synth_state_dict
    cap_torch_threads()
    dev = torch.device("cuda", 0)
    B, total_iters = a.batch, 100000
    hyp = types.SimpleNamespace(seg_model="DeepLabV3Plus", last_three_dilation_stride=[False, False, False], audio_backbone="vgg",
                                num_classes=2, batch_size=B, local_rank="cpu")
    model = CAVP(50, None, num_classes=2, args=hyp)
    model.load_state_dict(synth_state_dict({k: tuple(v.shape) for k, v in model.state_dict().items()}, seed=1))
    model.train().to(dev).set_compute_dtype(torch.bfloat16 if a.dtype == "bf16" else torch.float32)
    image, audio, label = [t.to(dev) for t in synth_inputs(B, (a.hw, a.hw), audio_batch=2 * B, num_classes=2, seed=0)]

    arena = model.grad_arena(dev)

    def optimiser(guard):
        o = FusedSGDAdam(model, arena, a.lr).use_device_schedule(a.lr, 0.9, total_iters)
        return o.use_step_guard(guard) if guard is not None else o
    g_idle, g_clip, g_alone = StepGuard(max_norm=None), StepGuard(max_norm=1e-3), StepGuard(max_norm=None)
    opt_a, opt_b, opt_c, opt_d = optimiser(None), optimiser(g_idle), optimiser(g_clip), optimiser(g_alone)
    replay_a = model.capture_train_step(image, audio, label, optimizer=opt_a)
    replay_b = model.capture_train_step(image, audio, label, optimizer=opt_b)
    replay_c = model.capture_train_step(image, audio, label, optimizer=opt_c)

    lib = _lib.load()
    tab, nj, nb = _ptr(opt_d.table), opt_d.njobs, opt_d.total_blocks

    def partials_alone():
        lib.cavp_grad_guard_partials(tab, nj, nb, _ptr(g_alone._partials), C.c_void_p(_stream()))

    def finish_alone():
        lib.cavp_grad_guard_finish(tab, nj, nb, _ptr(g_alone._partials), _ptr(g_alone._buf), C.c_void_p(_stream()))

    def update_alone():
        lib.cavp_optimizer_step_guarded(tab, nj, nb, C.c_float(opt_d.momentum), C.c_float(opt_d.eps), _ptr(opt_d._sched),
                                        _ptr(g_alone._buf), C.c_void_p(_stream()))

    fns = {"a_replay_update_recorded": replay_a, "b_replay_with_guard": replay_b, "c_replay_with_clipping": replay_c,
           "d_guard_four_launches_alone": opt_d.step, "e_partials_launch_alone": partials_alone,
           "f_guarded_update_launch_alone": update_alone, "g_combine_launch_alone": finish_alone}
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
    n_adam = sum(p.numel() for p in opt_d.params if id(p) in audio_ids)
    n_sgd = sum(p.numel() for p in opt_d.params if id(p) not in audio_ids)
    update_bytes, arena_bytes = 20 * n_sgd + 28 * n_adam, 4 * (n_sgd + n_adam)
    seen = g_clip.read()
    rec = {"bench": "step_guard", "device": torch.cuda.get_device_name(0), "config": "c1p", "batch": B, "hw": a.hw, "dtype": a.dtype,
           "iters": a.iters, "rounds": a.rounds, "tensors": nj, "workgroups": nb, "sgd_elements": n_sgd, "adam_elements": n_adam,
           "update_bytes": update_bytes, "arena_bytes": arena_bytes, "launch_floor_us": a.launch_floor_us,
           "clipped_share_of_c": round(float(seen["clipped"].mean()), 3) if len(seen["t"]) else None,
           "skipped_total": {"b": int(g_idle.last()["skipped_total"].item()), "c": int(g_clip.last()["skipped_total"].item())},
           "variants": {}}
    for k, v in times.items():
        rec["variants"][k] = {"ms_median": round(statistics.median(v), 4), "ms_min": round(min(v), 4), "ms_max": round(max(v), 4)}
    med = {k: v["ms_median"] for k, v in rec["variants"].items()}
    va = rec["variants"]["a_replay_update_recorded"]
    rec["partials_gb_per_s"] = round(arena_bytes / (med["e_partials_launch_alone"] * 1e-3) / 1e9, 1)
    rec["update_gb_per_s"] = round(update_bytes / (med["f_guarded_update_launch_alone"] * 1e-3) / 1e9, 1)
    rec["b_minus_a_ms_median"] = round(med["b_replay_with_guard"] - med["a_replay_update_recorded"], 4)
    rec["c_minus_a_ms_median"] = round(med["c_replay_with_clipping"] - med["a_replay_update_recorded"], 4)
    rec["spread_a_ms"] = round(va["ms_max"] - va["ms_min"], 4)
    rec["allowance_ms"] = round(arena_bytes / (rec["update_gb_per_s"] * 1e9) * 1e3 + 3 * a.launch_floor_us * 1e-3 + rec["spread_a_ms"], 4)
    rec["within_allowance"] = bool(rec["b_minus_a_ms_median"] <= rec["allowance_ms"])
    line = json.dumps(rec)
    print(line, flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "a") as f:
        f.write(line + "\n")


if __name__ == "__main__":
    main()
