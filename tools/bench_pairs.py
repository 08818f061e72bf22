"""Building the mismatched audio-visual pairs of one training step (shuffle, overwrite from the sound bank, bank update, shuffle
labels), three ways in one process:

  (a) host route       the rules of trainer_cavp_vpo_mono.py:87-115,148-181 written with torch ops on GPU tensors plus the existing
                       cavp_amd.cavp_model.SoundBank: what a ported reference trainer runs (one host synchronisation per row in
                       update_bank, `.item()` in the overwrite loop, a torch.cat of [S, A] per queued clip);
  (b) builder, eager   cavp_amd.pairs.PairBuilder: four launches, nothing read by the host;
  (c) builder + mel    PairBuilder + MelFrontEnd captured as one hipGraph, one replay per step (includes the 2B-clip log-mel, which
                       (a) and (b) do not: it is the unit a captured trainer replays, not a like-for-like of (a)).

    python tools/bench_pairs.py [--batch 32] [--classes 24] [--slots 32] [--wave-len 16000] [--hw 224] [--ow-rate 0.5]
                                [--iters 20] [--rounds 5] [--warmup 5] [--out profiles/pairs_bench.jsonl]

Default shape: the mono trainer's (B = 32, 24 classes, 1-second clips, a bank of 32 slots per class, 224 x 224 labels).  The batch
(about two thirds single-source rows) stays the same; the banks fill during the warm-up, overwrite is on.  A round times `iters`
back-to-back calls of each variant between two device synchronisations with a host clock; the variants alternate inside a round.
One JSON line per run is appended to --out.  Needs a GPU; there is no fallback."""
import argparse
import json
import os
import statistics
import sys
import time
import types

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch


def make_batch(B, K, A, hw, dev):
    g = torch.Generator().manual_seed(0)
    img = torch.zeros(B, K, dtype=torch.int64)
    img[torch.arange(B), torch.randint(1, K, (B,), generator=g)] = 1
    two = torch.rand(B, generator=g) < 0.3
    img[two, torch.randint(1, K, (int(two.sum()),), generator=g)] = 1
    img[:, 0] = torch.randint(0, 2, (B,), generator=g)
    wav = torch.randn(B, 1, A, generator=g) * 0.1
    pix = torch.randint(0, K, (B, hw, hw), generator=g)
    return wav.to(dev), pix.to(dev), img.to(dev)


class HostRoute:
    """The reference trainers' block with torch ops on device tensors and the host SoundBank."""

    def __init__(self, K, S, A, ow_rate, dev):
        from cavp_amd.cavp_model import SoundBank
        self.bank = SoundBank(out_dim=A, args=types.SimpleNamespace(num_classes=K, batch_size=S), device=dev)
        self.ow_rate, self.dev = ow_rate, dev

    def overwrite_miss_match(self, if_match, shuffle_img_label, img_label):
        no_bg = img_label.clone()
        no_bg[:, 0] = 0
        multi = torch.where(no_bg.sum(1) != 1)[0]
        false_list = (if_match == 0).nonzero(as_tuple=True)[0]
        n_false = false_list.shape[0]
        pick = torch.randperm(n_false)[: int(n_false * self.ow_rate)].to(self.dev)
        change = false_list[pick]
        change = change[~torch.isin(change, multi)]
        mod = {}
        for idx in change:
            idx = idx.item()
            if_match[idx] = True
            shuffle_img_label[idx] = img_label[idx]
            mod[idx] = int(no_bg[idx].nonzero()[0].item())
        return if_match, shuffle_img_label, mod

    def __call__(self, waveform, pix_label, img_label, overwrite):
        B = waveform.shape[0]
        perm = torch.randperm(B).to(self.dev)
        shuffle_img_label = img_label[perm]
        if_match = torch.all(torch.eq(img_label, shuffle_img_label), dim=1)
        shuffle_audio = waveform[perm]
        if overwrite:
            if_match, shuffle_img_label, mod = self.overwrite_miss_match(if_match, shuffle_img_label, img_label)
            shuffle_audio = self.bank.overwrite_audio_feature(shuffle_audio, waveform, mod)
        self.bank.update_bank(waveform, img_label.clone())          # (update_bank zeroes column 0 of what it is given)
        waveforms = torch.cat((waveform, shuffle_audio))
        label_shuffle = torch.where(if_match[:, None, None], pix_label, torch.zeros_like(pix_label))
        return waveforms, label_shuffle


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=32)
    ap.add_argument("--classes", type=int, default=24)
    ap.add_argument("--slots", type=int, default=32)
    ap.add_argument("--wave-len", type=int, default=16000)
    ap.add_argument("--hw", type=int, default=224)
    ap.add_argument("--ow-rate", type=float, default=0.5)
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--out", default=os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "profiles", "pairs_bench.jsonl"))
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_pairs.py needs the GPU: a CPU run says nothing about these timings")
    from cavp_amd.audio_frontend import MelFrontEnd
    from cavp_amd.hostinfo import cap_torch_threads
    from cavp_amd.pairs import PairBuilder
    cap_torch_threads()
    dev = torch.device("cuda", 0)
    B, K, S, A = a.batch, a.classes, a.slots, a.wave_len
    wav, pix, img = make_batch(B, K, A, a.hw, dev)

    host = HostRoute(K, S, A, a.ow_rate, dev)
    pb_b = PairBuilder(num_classes=K, bank_slots=S, wave_len=A, ow_rate=a.ow_rate, device=dev, max_batch=B)
    pb_c = PairBuilder(num_classes=K, bank_slots=S, wave_len=A, ow_rate=a.ow_rate, device=dev, max_batch=B)
    mel = MelFrontEnd(None, device=dev)
    out_b = pb_b(wav, pix, img, True)
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        out_c = pb_c(wav, pix, img, True)
        mel(out_c.waveforms)
    torch.cuda.current_stream().wait_stream(side)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        pb_c(wav, pix, img, True, out=out_c)
        spec = mel(out_c.waveforms)
    fns = {"a_host_route": lambda: host(wav, pix, img, True), "b_builder_eager": lambda: pb_b(wav, pix, img, True, out=out_b),
           "c_builder_mel_graph": graph.replay}

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
    plan = pb_b.last_plan()
    rec = {"bench": "pairs", "device": torch.cuda.get_device_name(0), "batch": B, "classes": K, "slots": S, "wave_len": A, "hw": a.hw,
           "ow_rate": a.ow_rate, "iters": a.iters, "rounds": a.rounds, "n_false": plan["n_false"], "q": plan["q"],
           "n_overwritten": plan["n_overwritten"], "n_written": plan["n_written"], "spec_shape": list(spec.shape), "variants": {}}
    for k, v in times.items():
        rec["variants"][k] = {"ms_median": round(statistics.median(v), 4), "ms_min": round(min(v), 4), "ms_max": round(max(v), 4)}
    line = json.dumps(rec)
    print(line, flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "a") as f:
        f.write(line + "\n")


if __name__ == "__main__":
    main()
