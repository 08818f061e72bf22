"""What the step rollback costs, in one process:

  (a) replay, guarded update recorded      the parent's captured step: forward, CE, backward, the guard's four launches;
  (b) the same with rollback=              + save() first and restore_if_skipped(guard) last (model ranges + a config-#5-sized bank);
  (c) / (d) save / forced restore alone    model ranges only (BatchNorm running statistics and counters);
  (e) / (f) save / forced restore alone    model ranges + the config-#5-sized bank (K = 2, S = 30, A = 16000);
  (g) / (h) save / forced restore alone    model ranges + the mono trainer's bank (K = 24, S = 32, A = 16000: the one group with traffic);
  (i) restore_if_skipped, word clear       the launch every clean iteration pays: one load per workgroup.

    python tools/bench_rollback.py [--batch 32] [--hw 224] [--dtype bf16] [--iters 20] [--rounds 5] [--warmup 5]
                                   [--copy-tb-per-s 6.29] [--out profiles/rollback_bench.jsonl]

Default shape: c1p (ResNet-50 224 x 224 OS16, VGGish audio, 2 classes), B = 32, bf16; the protocol of tools/bench_step_guard.py (host
clock around `iters` back-to-back iterations between two synchronisations, the variants alternating inside each of `rounds` rounds).
(a) runs the parent's code path in the same process, so (b) - (a) is the feature's price in the step.  The alone launches are compared
with 2 x bytes / the copy bandwidth a float4 copy reaches on this chip (--copy-tb-per-s, read + write bytes per second).  One JSON line per
run is appended to --out.  Needs a GPU; there is no fallback."""
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
    ap.add_argument("--batch", type=int, default=32)
    ap.add_argument("--hw", type=int, default=224)
    ap.add_argument("--dtype", choices=["bf16", "f32"], default="bf16")
    ap.add_argument("--lr", type=float, default=1e-4)
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--copy-tb-per-s", type=float, default=6.29, help="read + write bytes per second of a float4 copy on this chip")
    ap.add_argument("--out", default=os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "profiles", "rollback_bench.jsonl"))
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_rollback.py needs the GPU: a CPU run says nothing about these timings")
    from cavp_amd.cavp_model import CAVP
    from cavp_amd.hostinfo import cap_torch_threads
    from cavp_amd.optim import FusedSGDAdam, StepGuard
    from cavp_amd.pairs import PairBuilder
    from cavp_amd.rollback import StepRollback
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

    def optimiser():
        guard = StepGuard(max_norm=None)
        return FusedSGDAdam(model, arena, a.lr).use_device_schedule(a.lr, 0.9, total_iters).use_step_guard(guard), guard

    def bank(K, S):
        return PairBuilder(num_classes=K, bank_slots=S, wave_len=16000, ow_rate=0.5, device=dev, max_batch=B)
    # a model's buffers can be registered once per rollback only in the sense of one table each: the tables below share the live
    # ranges (never used concurrently) and own a shadow arena each
    rb_model = StepRollback(dev).add_model(model).freeze()
    rb_cfg5 = StepRollback(dev).add_model(model).add(bank(2, 30)).freeze()
    rb_mono = StepRollback(dev).add_model(model).add(bank(24, 32)).freeze()
    rb_step = StepRollback(dev).add_model(model).add(bank(2, 30)).freeze()
    (opt_a, guard_a), (opt_b, guard_b) = optimiser(), optimiser()
    replay_a = model.capture_train_step(image, audio, label, optimizer=opt_a)
    replay_b = model.capture_train_step(image, audio, label, optimizer=opt_b, rollback=rb_step)

    fns = {"a_replay_guarded": replay_a, "b_replay_guarded_rollback": replay_b,
           "c_save_model": rb_model.save, "d_restore_model": rb_model.restore,
           "e_save_model_bank_cfg5": rb_cfg5.save, "f_restore_model_bank_cfg5": rb_cfg5.restore,
           "g_save_model_bank_mono": rb_mono.save, "h_restore_model_bank_mono": rb_mono.restore,
           "i_restore_if_skipped_word_clear": lambda: rb_cfg5.restore_if_skipped(guard_a)}
    for rb in (rb_model, rb_cfg5, rb_mono):
        rb.save()   # every forced restore below puts back what is there now
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

    rec = {"bench": "rollback", "device": torch.cuda.get_device_name(0), "config": "c1p", "batch": B, "hw": a.hw, "dtype": a.dtype,
           "iters": a.iters, "rounds": a.rounds, "copy_tb_per_s": a.copy_tb_per_s,
           "registered_bytes": {"model": rb_model.registered_bytes(), "model_bank_cfg5": rb_cfg5.registered_bytes(),
                                "model_bank_mono": rb_mono.registered_bytes()},
           "ranges": {"model": len(rb_model._entries), "model_bank_cfg5": len(rb_cfg5._entries)},
           "blocks": {"model": rb_model.total_blocks, "model_bank_cfg5": rb_cfg5.total_blocks, "model_bank_mono": rb_mono.total_blocks},
           "stats_b": rb_step.stats(), "skipped_total_b": int(guard_b.last()["skipped_total"].item()), "variants": {}}
    for k, v in times.items():
        rec["variants"][k] = {"ms_median": round(statistics.median(v), 4), "ms_min": round(min(v), 4), "ms_max": round(max(v), 4)}
    med = {k: v["ms_median"] for k, v in rec["variants"].items()}
    va = rec["variants"]["a_replay_guarded"]
    rec["b_minus_a_ms_median"] = round(med["b_replay_guarded_rollback"] - med["a_replay_guarded"], 4)
    rec["spread_a_ms"] = round(va["ms_max"] - va["ms_min"], 4)
    rec["copy_floor_ms"] = {name: round(2 * sum(rb.registered_bytes().values()) / (a.copy_tb_per_s * 1e12) * 1e3, 5)
                            for name, rb in (("model", rb_model), ("model_bank_cfg5", rb_cfg5), ("model_bank_mono", rb_mono))}
    mono_bytes = sum(rb_mono.registered_bytes().values())
    rec["mono_save_tb_per_s"] = round(2 * mono_bytes / (med["g_save_model_bank_mono"] * 1e-3) / 1e12, 3)
    rec["mono_restore_tb_per_s"] = round(2 * mono_bytes / (med["h_restore_model_bank_mono"] * 1e-3) / 1e12, 3)
    line = json.dumps(rec)
    print(line, flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "a") as f:
        f.write(line + "\n")


if __name__ == "__main__":
    main()
