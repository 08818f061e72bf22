"""The resident data set (cavp_amd.store: DeviceStore + BatchFeeder) against what it replaces: the batch put together on the host
and pushed to the device every iteration.  One batch is B = 32 rows of a 640 x 640 uint8 frame, its mask and 10 s of 44.1 kHz
stereo int16 PCM - about 110 MB.

  host_copy     the parent's route: the batch gathered on the host from the decoded items (torch.stack into fresh tensors) and pushed
                with the pageable, blocking `dst.copy_(src)` calls tools/train_synth.py uses; `copy_only` is the same without the
                gather (the batch already lies in four host tensors);
  pinned_copy   the same from pinned staging tensors with copy_(non_blocking=True) and one synchronisation; `copy_only` likewise;
  feed_eager    BatchFeeder.feed(out=res): two launches, `--feed-iters` back-to-back calls between two synchronisations;
  feed_graph    the same two launches captured once and replayed;
  --step        the captured training step of tools/train_synth.py --graph --augment --raw-audio (batch --batch, 224 x 224 crops from
                336 x 336 staging slots) with and without --resident, replayed alternately, host wall-clock per iteration.  The
                parent's iteration is "copy the four raw tensors in, replay, synchronise" from host batches that are already
                gathered (no host draw is charged to it); the resident one is "replay, synchronise".

Two stores are fed: `full` (every item fills its slot: a frame is one contiguous run) and `ragged` (sides 320 .. 640, 5 .. 10 s: rows
of 3 w bytes at arbitrary alignment).  The four routes alternate inside each of --rounds rounds; medians are reported.  For the feeds
the bytes gathered per call and per second are reported next to the chip's measured float4 copy rate (6.29 TB/s, read plus written
bytes: compare it with `traffic_TBps` = 2 x gathered bytes per second).  That is a reference point, not a target.

  --clips T     instead of the above: the clip store (cavp_amd.clips: ClipStore + ClipFeeder) beside the single-frame store in one
                process.  Clip i holds T frames of item i's size (its frame 0 IS item i's frame) and item i's PCM, so ClipFeeder.feed
                gathers what BatchFeeder.feed gathers - the same bytes per batch, plus one Philox call per row in the plan - and
                feed_clips gathers T frames and masks per row.  feed / clip_feed / clip_eval, eager and captured, alternate inside
                each round; per store kind the record holds the medians, `clip_feed_over_feed` (ratio of the medians) next to
                `feed_round_spread` ((max - min) / median of feed's own rounds), and for the eval feed the read-plus-written rate
                against the same copy-rate figure.

    python tools/bench_store.py [--batch 32] [--items 64] [--rounds 5] [--host-iters 3] [--feed-iters 200] [--step | --clips T]
                                [--out FILE]

One JSON line per run is appended to --out (default profiles/store_bench.jsonl).  Needs a GPU; there is no fallback."""
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

STAGE, RAW_LEN, COPY_RATE_TBPS = (640, 640), 441000, 6.29


def make_items(n, ragged, stage=STAGE, raw_len=RAW_LEN, seed=0):
    """n decoded items as CPU tensors: (frame u8 [h, w, 3], mask u8 [h, w], pcm i16 [2, len])"""
    g = torch.Generator().manual_seed(seed)
    items = []
    for _ in range(n):
        h, w, ln = stage[0], stage[1], raw_len
        if ragged:
            h, w = (int(torch.randint(stage[k] // 2, stage[k] + 1, (), generator=g)) for k in (0, 1))
            ln = int(torch.randint(raw_len // 2, raw_len + 1, (), generator=g))
        items.append((torch.randint(0, 256, (h, w, 3), dtype=torch.uint8, generator=g), torch.randint(0, 4, (h, w), dtype=torch.uint8, generator=g),
                      torch.randint(-3277, 3278, (2, ln), dtype=torch.int16, generator=g)))
    return items


def make_store(items, dev, stage=STAGE, raw_len=RAW_LEN):
    from cavp_amd.store import DeviceStore
    st = DeviceStore(stage=stage, max_sources=1, max_channels=2, max_len=raw_len, pcm_dtype=torch.int16, device=dev)
    for f, m, p in items:
        st.append(f, m, [(p, 0)])
    return st.freeze()


def item_bytes(it):
    return it[0].numel() + it[1].numel() + 2 * it[2].numel()


def med(v, nd=4):
    return {"ms_median": round(statistics.median(v), nd), "ms_min": round(min(v), nd), "ms_max": round(max(v), nd)}


def bench_routes(a, dev):
    from cavp_amd.store import BatchFeeder, FeedResult
    B = a.batch
    rec = {}
    for kind in ("full", "ragged"):
        items = make_items(a.items, kind == "ragged")
        store = make_store(items, dev)
        feeder = BatchFeeder(store, batch=B, seed=1)
        res = FeedResult(B, store, dev)
        mean_bytes = sum(item_bytes(it) for it in items) / len(items) * B
        # ---- the device routes
        feeder.feed(out=res)
        graph, side = torch.cuda.CUDAGraph(), torch.cuda.Stream()
        side.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(side):
            with torch.cuda.graph(graph, stream=side):
                feeder.feed(out=res)
        torch.cuda.current_stream().wait_stream(side)
        # ---- the host routes (only the full store: the parent stages whole slots)
        routes = {"feed_eager": (lambda: feeder.feed(out=res), a.feed_iters), "feed_graph": (graph.replay, a.feed_iters)}
        if kind == "full":
            dst = [res.frames, res.masks, res.pcm, res.length]
            order = np.random.default_rng(0).permutation(len(items))

            def gather(k, out=None):
                idx = [int(order[(k * B + i) % len(items)]) for i in range(B)]
                o = out or [None] * 4
                return [torch.stack([items[i][0] for i in idx], out=o[0]), torch.stack([items[i][1] for i in idx], out=o[1]),
                        torch.stack([items[i][2] for i in idx], out=o[2]), torch.full((B, 1), RAW_LEN, dtype=torch.int32)]
            ready = gather(0)
            ready[2] = ready[2].view(B, 1, 2, RAW_LEN)
            pinned = [t.clone().pin_memory() for t in ready]
            pinned_views = [pinned[0], pinned[1], pinned[2].view(B, 2, RAW_LEN), pinned[3]]
            step = [0]

            def host_copy():
                step[0] += 1
                src = gather(step[0])
                src[2] = src[2].view(B, 1, 2, RAW_LEN)
                for d, s in zip(dst, src):
                    d.copy_(s)

            def host_copy_only():
                for d, s in zip(dst, ready):
                    d.copy_(s)

            def pinned_copy():
                step[0] += 1
                gather(step[0], out=pinned_views[:3])
                for d, s in zip(dst, pinned):
                    d.copy_(s, non_blocking=True)

            def pinned_copy_only():
                for d, s in zip(dst, pinned):
                    d.copy_(s, non_blocking=True)
            routes.update({"host_copy": (host_copy, a.host_iters), "host_copy_only": (host_copy_only, a.host_iters),
                           "pinned_copy": (pinned_copy, a.host_iters), "pinned_copy_only": (pinned_copy_only, a.host_iters)})
        for f, _ in routes.values():        # warm-up
            f()
        torch.cuda.synchronize()
        times = {k: [] for k in routes}
        for _ in range(a.rounds):
            for k, (f, iters) in routes.items():
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                for _ in range(iters):
                    f()
                torch.cuda.synchronize()
                times[k].append((time.perf_counter() - t0) / iters * 1e3)
        feeder.check()
        out = {k: med(v) for k, v in times.items()}
        for k in ("feed_eager", "feed_graph"):
            s = out[k]["ms_median"] * 1e-3
            out[k].update({"gathered_TBps": round(mean_bytes / s / 1e12, 3), "traffic_TBps": round(2 * mean_bytes / s / 1e12, 3),
                           "share_of_copy_rate": round(2 * mean_bytes / s / 1e12 / COPY_RATE_TBPS, 3)})
        out.update({"bytes_per_batch": int(mean_bytes), "store_bytes": store.nbytes, "items": len(items)})
        rec[kind] = out
        del store, feeder, res, graph
    return rec


def make_clip_store(items, T, dev):
    """Clip i: T frames of item i's size (frame 0 is item i's, the others are rolled copies: the content does not matter here), a mask
    on every frame, item i's PCM."""
    from cavp_amd.clips import ClipStore
    st = ClipStore(stage=STAGE, max_frames=T, max_sources=1, max_channels=2, max_len=RAW_LEN, pcm_dtype=torch.int16, device=dev)
    for f, m, p in items:
        st.append([torch.roll(f, k, 0) for k in range(T)], [torch.roll(m, k, 0) for k in range(T)], [(p, 0)])
    return st.freeze()


def capture(fn):
    graph, side = torch.cuda.CUDAGraph(), torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        with torch.cuda.graph(graph, stream=side):
            fn()
    torch.cuda.current_stream().wait_stream(side)
    return graph


def bench_clips(a, dev):
    """The train and the eval clip feed against feed() on a single-frame store of the same items, alternating inside each round."""
    from cavp_amd.clips import ClipEvalResult, ClipFeeder, ClipFeedResult
    from cavp_amd.store import BatchFeeder, FeedResult
    B, T = a.batch, a.clips
    rec = {}
    for kind in ("full", "ragged"):
        items = make_items(a.items, kind == "ragged")
        store, cstore = make_store(items, dev), make_clip_store(items, T, dev)
        feeder, cfeeder = BatchFeeder(store, batch=B, seed=1), ClipFeeder(cstore, batch=B, seed=1)
        res, cres, ev = FeedResult(B, store, dev), ClipFeedResult(B, cstore, dev), ClipEvalResult(B, cstore, dev)
        fns = {"feed": lambda: feeder.feed(out=res), "clip_feed": lambda: cfeeder.feed(out=cres), "clip_eval": lambda: cfeeder.feed_clips(out=ev)}
        for f in fns.values():              # the code objects are loaded outside the captures
            f()
        routes = {}
        for k, f in fns.items():
            routes[k + "_eager"] = f
            routes[k + "_graph"] = capture(f).replay
        for f in routes.values():
            f()
        torch.cuda.synchronize()
        times = {k: [] for k in routes}
        for _ in range(a.rounds):
            for k, f in routes.items():
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                for _ in range(a.feed_iters):
                    f()
                torch.cuda.synchronize()
                times[k].append((time.perf_counter() - t0) / a.feed_iters * 1e3)
        feeder.check()
        cfeeder.check()
        out = {k: med(v) for k, v in times.items()}
        n = len(items)
        train_bytes = sum(item_bytes(it) for it in items) / n * B
        eval_bytes = sum(T * (it[0].numel() + it[1].numel()) + 2 * it[2].numel() for it in items) / n * B
        for k, nbytes in (("feed", train_bytes), ("clip_feed", train_bytes), ("clip_eval", eval_bytes)):
            for mode in ("_eager", "_graph"):
                sec = out[k + mode]["ms_median"] * 1e-3
                out[k + mode].update({"traffic_TBps": round(2 * nbytes / sec / 1e12, 3),
                                      "share_of_copy_rate": round(2 * nbytes / sec / 1e12 / COPY_RATE_TBPS, 3)})
        for mode in ("eager", "graph"):
            f = out[f"feed_{mode}"]
            out[f"clip_feed_over_feed_{mode}"] = round(out[f"clip_feed_{mode}"]["ms_median"] / f["ms_median"], 4)
            out[f"feed_round_spread_{mode}"] = round((f["ms_max"] - f["ms_min"]) / f["ms_median"], 4)
        out.update({"bytes_per_batch": int(train_bytes), "eval_bytes_per_batch": int(eval_bytes), "store_bytes": store.nbytes,
                    "clip_store_bytes": cstore.nbytes, "items": n, "steps_per_epoch": cfeeder.steps_per_epoch,
                    "steps_per_pass": cfeeder.steps_per_pass})
        rec[kind] = out
        del store, cstore, feeder, cfeeder, res, cres, ev, routes, fns
    return rec


def bench_step(a, dev):
    """The captured training step with and without the feeder at the head of its prologue, replayed alternately."""
    from cavp_amd.audio_frontend import MelFrontEnd
    from cavp_amd.augment import COCO_SCALES, AugResult, FrameAugment
    from cavp_amd.cavp_model import CAVP
    from cavp_amd.contrast import ContrastLoss
    from cavp_amd.labels import LabelResult, LabelStage
    from cavp_amd.optim import FusedSGDAdam
    from cavp_amd.pairs import PairBuilder, PairResult
    from cavp_amd.store import BatchFeeder, FeedResult
    from cavp_amd.synth import synth_state_dict
    from cavp_amd.wave import WaveResult, WaveStage
    B, hw, K, L = a.batch, 224, 2, RAW_LEN
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
    items = make_items(2 * B, False, stage=stage, seed=1)
    for _, m, _ in items:
        m.zero_()
        m[40:150, 60:200] = 11
    store = make_store(items, dev, stage=stage)
    feeder = BatchFeeder(store, batch=B, seed=1234)
    fed = FeedResult(B, store, dev)
    # the parent's static buffers and two host batches that are already gathered
    host = [[torch.stack([items[h * B + i][k] for i in range(B)]) for k in range(3)] for h in (0, 1)]
    for hb in host:
        hb[2] = hb[2].view(B, 1, 2, L)
    s_frames, s_masks, s_pcm = (torch.zeros_like(t, device=dev) for t in host[0])
    s_sizes = torch.tensor([list(stage)] * B, dtype=torch.int32, device=dev)
    s_len, h_len = torch.full((B, 1), L, dtype=torch.int32, device=dev), torch.full((B, 1), L, dtype=torch.int32)
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

    def prologue_of(resident):
        def prologue():
            if resident:
                feeder.feed(out=fed)
                ws(fed.pcm, fed.length, fed.rate_idx, fed.n_ch, out=cut)
                aug(fed.frames, fed.masks, fed.sizes, out=augmented)
            else:
                ws(s_pcm, s_len, s_rate, s_nch, out=cut)
                aug(s_frames, s_masks, s_sizes, out=augmented)
            stage_labels(augmented.label, out=labelled)
            s_image.copy_(augmented.image)
            s_label.copy_(labelled.label)
            s_img_label.copy_(labelled.img_label)
            pairs(cut.waveform, s_label, s_img_label, True, out=built)
            s_audio.copy_(front(built.waveforms))
            s_shuf.copy_(built.label_shuffle)
        return prologue
    reps = {k: model.capture_train_step(s_image, s_audio, s_label, contrast=crit, label_shuffle=s_shuf, contrast_weight=1.0, optimizer=opt,
                                        prologue=prologue_of(k == "resident")) for k in ("parent", "resident")}
    n = [0]

    def parent_iteration():
        n[0] += 1
        hb = host[n[0] % 2]
        for d, s in ((s_frames, hb[0]), (s_masks, hb[1]), (s_pcm, hb[2]), (s_len, h_len)):
            d.copy_(s)
        reps["parent"]()
    its = {"parent": parent_iteration, "resident": reps["resident"]}
    for _ in range(a.warmup):
        for f in its.values():
            f()
    torch.cuda.synchronize()
    times = {k: [] for k in its}
    for _ in range(a.step_iters):
        for k, f in its.items():
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            f()
            torch.cuda.synchronize()
            times[k].append((time.perf_counter() - t0) * 1e3)
    ws.check()
    aug.check()
    feeder.check()
    res = {k: med(v, 3) for k, v in times.items()}
    res["saved_ms_median"] = round(res["parent"]["ms_median"] - res["resident"]["ms_median"], 3)
    res.update({"iterations_each": a.step_iters, "raw_bytes_per_batch": sum(item_bytes(it) for it in items[:B]), "stage": list(stage)})
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=32)
    ap.add_argument("--items", type=int, default=64)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--host-iters", type=int, default=3)
    ap.add_argument("--feed-iters", type=int, default=200)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--step", action="store_true", help="also time the captured training step with and without the resident store")
    ap.add_argument("--step-iters", type=int, default=20)
    ap.add_argument("--clips", type=int, default=None, metavar="T", help="the clip store's train and eval feed against feed(), T frames per clip")
    ap.add_argument("--out", default=os.path.join(REPO, "profiles", "store_bench.jsonl"))
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_store.py needs the GPU: a CPU run says nothing about these timings")
    from cavp_amd.hostinfo import cap_torch_threads
    cap_torch_threads()
    dev = torch.device("cuda", 0)
    rec = {"bench": "store", "device": torch.cuda.get_device_name(0), "batch": a.batch, "stage": list(STAGE), "raw_len": RAW_LEN,
           "rounds": a.rounds, "host_iters": a.host_iters, "feed_iters": a.feed_iters, "copy_rate_TBps": COPY_RATE_TBPS}
    if a.clips is not None:
        if a.step or not 1 <= a.clips <= 32 or a.batch * a.clips > 1024:
            raise SystemExit("--clips T: 1 <= T <= 32, batch * T <= 1024, and not together with --step")
        rec.update({"bench": "store_clips", "clips": a.clips})
        rec.update(bench_clips(a, dev))
    else:
        rec.update(bench_routes(a, dev))
        if a.step:
            rec["step"] = bench_step(a, dev)
    line = json.dumps(rec)
    print(line, flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "a") as f:
        f.write(line + "\n")


if __name__ == "__main__":
    main()
