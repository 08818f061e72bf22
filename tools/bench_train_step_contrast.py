"""One training step with the reference trainers' full objective, `l_ce + w * l_ctr`, three ways in one process:

  (a) autograd route   model on the graphed autograd node (CAVP.enable_graphed_autograd), F.cross_entropy on the full-resolution
                       prediction and ContrastLoss (device sampler) on the f32 fusion map, `(l_ce + w * l_ctr).backward()`:
                       the fastest route to this objective before the native step took the contrast term;
  (b) native step      CAVP.capture_train_step(contrast=...): CE + contrast + backward as one hipGraph;
  (c) CE only          CAVP.capture_train_step(): the native step without the contrast term, the floor.

    python tools/bench_train_step_contrast.py [--batch 30] [--hw 224] [--dtype bf16] [--max-views 512] [--iters 20] [--rounds 5]
                                              [--warmup 5] [--out profiles/train_step_contrast_bench.jsonl]

Default shape: config #5's (B = 30 frames of 224 x 224, bf16, max_views = 512, binary labels).  Every variant is warmed up on the
shape it is timed on.  A round times `iters` back-to-back steps of each variant between two device synchronisations with a host
clock; the variants alternate inside a round, so drift of a shared host hits all of them alike.  Reported per variant: median and
min / max over the rounds of the per-step time, and the kernel dispatches of one eager step of the same route (torch.profiler, after
the timed rounds; the profiler does not list the kernels inside a graph replay).  One JSON line per run is appended to --out.  Needs a GPU; there is no fallback."""
import argparse
import json
import os
import statistics
import sys
import time
import types

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch
import torch.nn.functional as F


def build_model(B, dtype, dev):
    from cavp_amd.cavp_model import CAVP
    from cavp_amd.synth import synth_state_dict
    hyp = types.SimpleNamespace(seg_model="DeepLabV3Plus", last_three_dilation_stride=[False, False, False], audio_backbone="vgg",
                                num_classes=2, batch_size=B, local_rank=dev.index)
    m = CAVP(50, None, num_classes=2, args=hyp)
    m.load_state_dict(synth_state_dict({k: tuple(v.shape) for k, v in m.state_dict().items()}, seed=1))
    return m.train().to(dev).set_compute_dtype(dtype)


def make_labels(B, hw, dev):
    """binary labels: one foreground band per image, shifted from image to image; shuffle labels = labels with the second half of
    the batch set to 0"""
    gt = torch.zeros((B, hw, hw), dtype=torch.long)
    bh = hw // 2
    for b in range(B):
        r0 = (bh + 7 * b) % (hw - bh // 2)
        gt[b, r0:r0 + bh // 2, 16:hw - 16] = 1
    gs = gt.clone()
    gs[B // 2:] = 0
    return gt.to(dev), gs.to(dev)


def count_dispatches(fn):
    """kernel dispatches of one call of fn (device-side kernel events of torch.profiler), or None with the reason"""
    try:
        from torch.autograd import DeviceType
        from torch.profiler import ProfilerActivity, profile
        torch.cuda.synchronize()
        with profile(activities=[ProfilerActivity.CUDA]) as prof:
            fn()
            torch.cuda.synchronize()
        names = [e.name for e in prof.events() if e.device_type == DeviceType.CUDA]
        return sum(1 for n in names if not n.lower().startswith(("memcpy", "memset", "copy"))), None
    except Exception as ex:  # noqa: BLE001 - the count is a by-product: the timings stand without it
        return None, f"{type(ex).__name__}: {ex}"


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=30)
    ap.add_argument("--hw", type=int, default=224)
    ap.add_argument("--dtype", choices=["bf16", "f32"], default="bf16")
    ap.add_argument("--max-views", type=int, default=512)
    ap.add_argument("--contrast-weight", type=float, default=1.0)
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--no-dispatch-count", action="store_true")
    ap.add_argument("--out", default=os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "profiles",
                                                  "train_step_contrast_bench.jsonl"))
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_train_step_contrast.py needs the GPU: a CPU run says nothing about these timings")
    from cavp_amd.contrast import ContrastLoss
    from cavp_amd.hostinfo import cap_torch_threads
    from cavp_amd.synth import synth_inputs
    cap_torch_threads()
    dev = torch.device("cuda", 0)
    dtype = torch.bfloat16 if a.dtype == "bf16" else torch.float32
    B, w = a.batch, a.contrast_weight
    image, audio, _ = [t.to(dev) for t in synth_inputs(B, (a.hw, a.hw), audio_batch=2 * B, num_classes=2, seed=0)]
    label, shuf = make_labels(B, a.hw, dev)

    def crit():
        return ContrastLoss(0.1, 255, a.max_views).use_device_sampler(1)

    # (a) the autograd route
    m_a, c_a = build_model(B, dtype, dev), crit()
    m_a.enable_graphed_autograd()
    params_a = [p for p in m_a.parameters() if p.requires_grad]
    last = {}

    def step_a():
        for p in params_a:
            p.grad = None
        out, fus, _ = m_a(image, audio, None, False)
        l_ctr = c_a(fus[:B], label, fus[B:], shuf)
        l_ce = F.cross_entropy(out[:B] + out[B:] * 0.0, label, ignore_index=255)
        (l_ce + w * l_ctr).backward()
        last["a"] = (l_ce.detach(), l_ctr.detach())

    # (b) the native step with the contrast term, (c) without
    m_b, c_b = build_model(B, dtype, dev), crit()
    step_b = m_b.capture_train_step(image, audio, label, contrast=c_b, label_shuffle=shuf, contrast_weight=w)
    m_c = build_model(B, dtype, dev)
    step_c = m_c.capture_train_step(image, audio, label)
    fns = {"a_autograd_route": step_a, "b_native_ce_contrast": step_b, "c_native_ce_only": step_c}

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
    rec = {"bench": "train_step_contrast", "device": torch.cuda.get_device_name(0), "batch": B, "hw": a.hw, "dtype": a.dtype,
           "max_views": a.max_views, "contrast_weight": w, "iters": a.iters, "rounds": a.rounds,
           "anchors": int(c_b.last_plan()["header"][0]), "graphs_b": len(m_b._train_graph), "variants": {}}
    for k, v in times.items():
        med = statistics.median(v)
        rec["variants"][k] = {"ms_median": round(med, 4), "ms_min": round(min(v), 4), "ms_max": round(max(v), 4),
                              "frames_per_s": round(B / med * 1e3, 1)}
    rec["loss_a_ce_ctr"] = [round(float(t.item()), 5) for t in last["a"]]
    rec["loss_b_ce_ctr"] = [round(float(t.item()), 5) for t in m_b._last_losses]
    if not a.no_dispatch_count:
        # counted on the EAGER form of each step: the profiler does not list the kernels inside a hipGraph replay.  The contrast
        # chain issues the same launches eagerly and captured, so (b) - (c) is what the term adds to the step.
        m_a.enable_graphed_autograd(False)
        eager = {"a_autograd_route": step_a,
                 "b_native_ce_contrast": lambda: m_b.train_step(image, audio, label, contrast=c_b, label_shuffle=shuf, contrast_weight=w),
                 "c_native_ce_only": lambda: m_c.train_step(image, audio, label)}
        for k, f in eager.items():
            f()
            n, why = count_dispatches(f)
            rec["variants"][k]["dispatches_eager"] = n
            if why:
                rec["variants"][k]["dispatches_note"] = why
    line = json.dumps(rec)
    print(line, flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "a") as f:
        f.write(line + "\n")


if __name__ == "__main__":
    main()
