#!/usr/bin/env python3
"""Synthetic-data training driver on the MI355X path: the counterpart of the reference's main_vpo_mono.py +
trainer_cavp_vpo_mono.py::train loop (SURVEY.md §8f row f3 "synthetic-data train driver") with every stage on HIP:

    waveform --MelFrontEnd--> log-mel  \
    image ----------------------------> CAVP.train_step (forward_train + CE + backward, one flat gradient arena,
                                         one RCCL all-reduce) --> FusedSGDAdam.step(poly lr)

One process per GPU (python -m torch.distributed.run --nproc-per-node N tools/train_synth.py ...), 127.0.0.1 rendezvous.
There is no dataset here (no network): images / waveforms / labels are seeded random tensors of the config_avss_binary
shapes; the point is the plumbing and its throughput, not accuracy.

usage: python tools/train_synth.py [--steps 20] [--batch 32] [--dtype bf16|f32] [--num-classes 2] [--from-waveform]
                                   [--contrast [--contrast-weight W]] [--pairs] [--graph [--augment [--resize] [--raw-audio]
                                   [--resident [--store-items N] [--clips T [--validate-every K]]]]
                                   [--guard [--max-norm X] [--rollback]] [--accumulate N]] [--preview DIR]
                                   [--seg-model DeepLabV3Plus|PVT [--device-droppath]]

--contrast: the reference trainers' full objective, l_ce + W * l_ctr (trainer_cavp_vpo_mono.py:183-189), inside the native step:
ContrastLoss with the device sampler on the fusion map; the shuffle labels are the labels with the second half of the batch set to 0.

--pairs (with --from-waveform --contrast): the mismatched pairs are built as the reference trainers build them
(trainer_cavp_vpo_mono.py:148-181), on the device: B clips and synthetic multi-hot image labels go through cavp_amd.pairs.PairBuilder
(shuffle, overwrite from the sound bank from step 1 on, bank update), its 2B clips through MelFrontEnd, its label_shuffle into the step.

--graph (with --from-waveform --contrast --pairs): the whole iteration as one hipGraph - pair builder, log-mel, forward, CE + contrast,
backward and the optimiser step with the learning-rate schedule on the device (FusedSGDAdam.use_device_schedule,
CAVP.capture_train_step(optimizer=, prologue=)).  Two captures share the optimiser's device state: one without the sound-bank
overwrite for step 0, one with it for the rest.  The loop is "copy the batch into the static buffers, replay".

--augment (with --graph): the batch is raw material - synthetic uint8 frames and masks with a few class blobs in raw (data-set)
class indices - and the captured prologue is the whole input chain FrameAugment -> LabelStage -> PairBuilder -> MelFrontEnd: the
image labels the pair builder sees are computed on the device from the augmented, remapped mask, as the reference's data sets
compute them after their transform.  --resize: the AVSS set-ups' variant (the AVS scale list, no jitter, a resize to --hw instead
of pad + crop).  --raw-audio: the clips are raw material too - 10 s of synthetic 44.1 kHz int16 stereo PCM per row - and
cavp_amd.wave.WaveStage (resample to 16 kHz, centre crop to one second, channel mean) stands at the head of the prologue.

--resident (with --augment): the raw material is a data set that lives on the device - --store-items synthetic items (frame, mask and,
with --raw-audio, one PCM clip each) are appended to a cavp_amd.store.DeviceStore once, and BatchFeeder.feed stands at the head of the
prologue: the sampler (RandomSampler / DistributedSampler semantics, one shared store and a rank of its own per process) and the gather
into the staging buffers are two more launches of the graph, and the loop body is replay() - no host draw, no host copy.  (Without
--raw-audio the 16 kHz clip is still drawn and copied by the host.)

--clips T (with --resident): the items are clips, as in the AVSBench / AVSS data sets - T frames (the last one without a mask in
every third clip) and, with --raw-audio, one PCM clip each in a cavp_amd.clips.ClipStore.  ClipFeeder.feed draws the clip and one
of its frames on the device and gathers only that frame; the chain is ClipFeeder.feed -> FrameAugment -> LabelStage ->
WaveStage(segments=T, select=fed.select) -> PairBuilder -> MelFrontEnd, all inside the captured prologue (the wave stage then
crops T seconds and keeps the drawn frame's second).  --validate-every K (with --clips and --raw-audio): after every K steps one
validation pass over the store - feed_clips -> FrameAugment.eval_ -> LabelStage -> WaveStage (all T segments) -> MelFrontEnd ->
model.predict -> ClipValidation.update, batch // T clips per step, nothing copied to the host - and its ten numbers are printed.

--guard (with --graph): a cavp_amd.optim.StepGuard on the recorded update - global gradient norm, --max-norm clipping, the whole
update skipped when a gradient or a loss is not finite.  The loop then reads no loss back per step: every 5 steps one guard.read()
returns the records written since (step, rate, both losses, gradient norm, coefficient, skipped / clipped) and they are printed.

--rollback (with --guard): a cavp_amd.rollback.StepRollback over the model's BatchNorm state, the pair builder, the sampler and, with
--augment, the frame augmentation, handed to both captures: a skipped step also undoes what its forward wrote, and the captures undo
their own warm-up passes, so nothing is reloaded or reseeded behind them.  At the end the rollback's restore count is printed next to
the guard's skipped count; the run fails if the two differ.

--accumulate N (with --graph, one process, not with --rollback): a cavp_amd.accumulate.GradAccumulator on the recorded update - N
replays of --batch frames per optimiser update, the arithmetic of N data-parallel ranks with local BatchNorm.  --steps and
--total-iters then count WINDOWS (the loop replays --steps x N times), and so do the printed lines: with --guard one record per
window (its losses are the window's means), otherwise the closing replay's loss.

--device-droppath (with --seg-model PVT; an error otherwise): the backbone's DropPath masks are drawn on the device
(model.use_device_drop_path(seed=1234 + rank), cavp_amd/droppath.py) - one launch per forward, inside the graph with --graph, where
the host no longer draws or uploads anything before a replay; with --rollback the sampler's {seed, offset} joins the rollback.

--preview DIR: after training, the reference trainers' image upload (Tensorboard.upload_wandb_image) without its whole-tensor host
copies: eval mode, model.predict on the last batch, cavp_amd.preview.PreviewStage on image, label and mask, one 5-byte-per-pixel copy,
and the x / y / y_tilde pictures of the first frames written to DIR as PNG files (needs PIL).
"""
import argparse
import os
import sys
import time
import types

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def main():
    from cavp_amd.hostinfo import cap_torch_threads
    cap_torch_threads()   # (container CPU quota: cavp_amd/hostinfo.py)
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--batch", type=int, default=32, help="frames per GPU per step")
    ap.add_argument("--dtype", choices=["bf16", "f32"], default="bf16")
    ap.add_argument("--num-classes", type=int, default=2)
    ap.add_argument("--hw", type=int, default=224)
    ap.add_argument("--lr", type=float, default=1e-3)            # config_avss_binary.py:52-57
    ap.add_argument("--lr-power", type=float, default=0.9)
    ap.add_argument("--momentum", type=float, default=0.9)
    ap.add_argument("--weight-decay", type=float, default=1e-4)
    ap.add_argument("--total-iters", type=int, default=1000)
    ap.add_argument("--seg-model", choices=["DeepLabV3Plus", "PVT"], default="DeepLabV3Plus", help="PVT = config #4's PVTv2-B5 backbone")
    ap.add_argument("--device-droppath", action="store_true", help="with --seg-model PVT: draw the DropPath masks on the device "
                    "(one launch per forward, in the graph with --graph) instead of on the host before every step")
    ap.add_argument("--fixed-batch", action="store_true", help="train on ONE batch (over-fit sanity: the loss must fall)")
    ap.add_argument("--from-waveform", action="store_true", help="start from 16 kHz waveforms (HIP log-mel front-end)")
    ap.add_argument("--contrast", action="store_true", help="add the pixel-level contrastive term to the native step (device sampler)")
    ap.add_argument("--contrast-weight", type=float, default=1.0, help="W in l_ce + W * l_ctr (the reference's args.loss_w)")
    ap.add_argument("--max-views", type=int, default=512)
    ap.add_argument("--pairs", action="store_true", help="build the shuffled half of the batch and its labels with PairBuilder")
    ap.add_argument("--ow-rate", type=float, default=0.5, help="share of the mismatched rows overwritten from the sound bank")
    ap.add_argument("--graph", action="store_true", help="one hipGraph per iteration: pairs, log-mel, step and optimiser (device schedule)")
    ap.add_argument("--guard", action="store_true", help="with --graph: StepGuard on the recorded update (gradient norm, non-finite skip); "
                    "the progress lines come from guard.read(), one synchronisation per 5 steps instead of .item() reads")
    ap.add_argument("--max-norm", type=float, default=None, help="with --guard: clip the global gradient norm to this bound")
    ap.add_argument("--rollback", action="store_true", help="with --guard: a StepRollback over the model's BatchNorm state and every enabled "
                    "stage, so a skipped step also undoes its forward; the capture then leaves no trace and nothing is reseeded")
    ap.add_argument("--accumulate", type=int, default=None, metavar="N", help="with --graph: N micro-batches of --batch frames per update "
                    "(GradAccumulator); --steps and --total-iters count windows")
    ap.add_argument("--augment", action="store_true", help="with --graph: raw uint8 frames / masks through FrameAugment and LabelStage in the prologue")
    ap.add_argument("--resize", action="store_true", help="with --augment: the resize_flag variant (AVS scales, no jitter, resize to --hw)")
    ap.add_argument("--raw-audio", action="store_true", help="with --augment: 44.1 kHz int16 stereo PCM through WaveStage at the head of the prologue")
    ap.add_argument("--resident", action="store_true", help="with --augment: frames, masks and (with --raw-audio) PCM come from a device-resident "
                    "DeviceStore through BatchFeeder.feed at the head of the prologue; the loop body is replay()")
    ap.add_argument("--store-items", type=int, default=None, help="with --resident: items in the store (default 4 x --batch x world)")
    ap.add_argument("--clips", type=int, default=None, metavar="T", help="with --resident: the store is a ClipStore of T-frame clips; "
                    "ClipFeeder.feed draws clip and frame on the device")
    ap.add_argument("--validate-every", type=int, default=None, metavar="K", help="with --clips and --raw-audio: a validation pass "
                    "(feed_clips -> eval_ -> predict -> ClipValidation) after every K steps")
    ap.add_argument("--preview", metavar="DIR", default=None, help="after training: x / y / y_tilde PNGs of the last batch through PreviewStage")
    a = ap.parse_args()
    if a.raw_audio and not a.augment:
        ap.error("--raw-audio needs --augment")
    if a.resident and not a.augment:
        ap.error("--resident needs --augment (with --graph)")
    if a.store_items is not None and not a.resident:
        ap.error("--store-items needs --resident")
    if a.clips is not None and (not a.resident or not 1 <= a.clips <= 32 or a.batch < a.clips):
        ap.error("--clips T needs --resident, 1 <= T <= 32 and --batch >= T")
    if a.validate_every is not None and (a.clips is None or not a.raw_audio or a.validate_every < 1):
        ap.error("--validate-every K needs --clips and --raw-audio, K >= 1")
    if a.augment and not a.graph:
        ap.error("--augment needs --graph (with --from-waveform --contrast --pairs)")
    if a.resize and not a.augment:
        ap.error("--resize needs --augment")
    if a.pairs and not (a.from_waveform and a.contrast):
        ap.error("--pairs needs --from-waveform and --contrast")
    if a.guard and not a.graph:
        ap.error("--guard needs --graph: the guard lives beside the device schedule of the recorded update")
    if a.max_norm is not None and not a.guard:
        ap.error("--max-norm needs --guard")
    if a.rollback and not a.guard:
        ap.error("--rollback needs --guard: the guard's skip word decides the restore")
    if a.accumulate is not None and (not a.graph or a.rollback or a.accumulate < 1 or int(os.environ.get("WORLD_SIZE", "1")) > 1):
        ap.error("--accumulate N needs --graph, N >= 1, one process and no --rollback (a window spans several replays)")
    if a.graph and not a.pairs:
        ap.error("--graph needs --from-waveform --contrast --pairs")
    if a.device_droppath and a.seg_model != "PVT":
        ap.error("--device-droppath needs --seg-model PVT: only the PVT backbone has DropPath")

    world = int(os.environ.get("WORLD_SIZE", "1"))
    rank = int(os.environ.get("RANK", "0"))
    local = int(os.environ.get("LOCAL_RANK", "0"))
    torch.cuda.set_device(local)
    dev = torch.device("cuda", local)
    if world > 1:
        import torch.distributed as dist
        os.environ.setdefault("MASTER_ADDR", "127.0.0.1")
        os.environ.setdefault("MASTER_PORT", "29511")
        dist.init_process_group("nccl", rank=rank, world_size=world, device_id=dev)

    from cavp_amd.audio_frontend import MelFrontEnd
    from cavp_amd.cavp_model import CAVP
    from cavp_amd.optim import FusedSGDAdam, warmup_poly_lr
    from cavp_amd.synth import synth_state_dict

    hyp = types.SimpleNamespace(seg_model=a.seg_model, last_three_dilation_stride=[False, False, False],
                                audio_backbone="vgg", num_classes=a.num_classes, batch_size=a.batch, local_rank=local,
                                audio_len=1.0, spec_min=-100, spec_max=100, allow_random_pvt=True)
    model = CAVP(50, None, num_classes=a.num_classes, args=hyp)
    model.load_state_dict(synth_state_dict({k: tuple(v.shape) for k, v in model.state_dict().items()}, seed=1))
    model.train().to(dev).set_compute_dtype(torch.bfloat16 if a.dtype == "bf16" else torch.float32)
    drop_path = model.use_device_drop_path(seed=1234 + rank) if a.device_droppath else None   # each rank its own stream of masks
    sched = warmup_poly_lr(a.lr, a.lr_power, a.total_iters, 0)
    front = MelFrontEnd(hyp, device=dev) if a.from_waveform else None
    crit = None
    if a.contrast:
        from cavp_amd.contrast import ContrastLoss
        crit = ContrastLoss(0.1, 255, a.max_views).use_device_sampler(min(max(a.num_classes - 1, 1), 254), seed=1234 + rank)

    pairs = None
    if a.pairs:
        from cavp_amd.pairs import PairBuilder
        K = max(a.num_classes, 2)
        pairs = PairBuilder(num_classes=K, bank_slots=a.batch, wave_len=16000, ow_rate=a.ow_rate, seed=1234 + rank, device=dev,
                            max_batch=a.batch)

    g = torch.Generator().manual_seed(1234 + rank)
    B = a.batch
    opt = None
    t0 = None
    first = None

    def draw_pairs_batch():
        """B clips and synthetic multi-hot image labels (host tensors)"""
        wave = torch.randn(B, 1, 16000, generator=g) * 0.1
        img_label = torch.zeros(B, pairs.K, dtype=torch.int64)
        img_label[torch.arange(B), torch.randint(1, pairs.K, (B,), generator=g)] = 1       # one source per frame ...
        two = torch.rand(B, generator=g) < 0.25                                             # ... a second one for a quarter
        img_label[two, torch.randint(1, pairs.K, (int(two.sum()),), generator=g)] = 1
        img_label[:, 0] = torch.randint(0, 2, (B,), generator=g)
        return wave, img_label

    RAW0 = 10          # --augment: the raw mask holds RAW0 + c where the model's class is c (a data set's own index space)

    def draw_raw_batch(stage):
        """B raw frames and masks (host uint8): noise with one or two rectangular blobs of a foreground class each"""
        frames = torch.randint(0, 256, (B,) + stage + (3,), dtype=torch.uint8, generator=g)
        masks = torch.zeros((B,) + stage, dtype=torch.uint8)
        for b in range(B):
            for _ in range(1 + int(torch.rand((), generator=g) < 0.25)):
                c = int(torch.randint(1, pairs.K, (), generator=g))
                y, x = (int(torch.randint(0, stage[k] // 2, (), generator=g)) for k in (0, 1))
                masks[b, y:y + stage[0] // 3, x:x + stage[1] // 3] = RAW0 + c
        return frames, masks

    RAW_RATE, RAW_LEN = 44100, 441000      # --raw-audio: 10 s of stereo PCM per row

    def draw_raw_audio():
        """B clips of int16 stereo PCM (host) and their lengths, 5 .. 10 s"""
        pcm = torch.randint(-3277, 3278, (B, 1, 2, RAW_LEN), dtype=torch.int16, generator=g)
        return pcm, torch.randint(RAW_LEN // 2, RAW_LEN + 1, (B, 1), dtype=torch.int32, generator=g)

    def build_store(stage, n_items):
        """n_items synthetic items of draw_raw_batch's / draw_raw_audio's kind in a frozen DeviceStore - the same store on every rank"""
        from cavp_amd.store import DeviceStore
        gs = torch.Generator().manual_seed(4321)
        store = DeviceStore(stage=stage, max_sources=1, max_channels=2, max_len=RAW_LEN if a.raw_audio else 1, pcm_dtype=torch.int16,
                            device=dev)
        for _ in range(n_items):
            frame = torch.randint(0, 256, stage + (3,), dtype=torch.uint8, generator=gs)
            mask = torch.zeros(stage, dtype=torch.uint8)
            for _ in range(1 + int(torch.rand((), generator=gs) < 0.25)):
                c = int(torch.randint(1, pairs.K, (), generator=gs))
                y, x = (int(torch.randint(0, stage[k] // 2, (), generator=gs)) for k in (0, 1))
                mask[y:y + stage[0] // 3, x:x + stage[1] // 3] = RAW0 + c
            sources = []
            if a.raw_audio:
                n = int(torch.randint(RAW_LEN // 2, RAW_LEN + 1, (), generator=gs))
                sources.append((torch.randint(-3277, 3278, (2, n), dtype=torch.int16, generator=gs), 0))
            store.append(frame, mask, sources)
        return store.freeze()

    def build_clip_store(stage, n_clips, T):
        """n_clips synthetic T-frame clips in a frozen ClipStore - the same store on every rank.  Every third clip has no mask on
        its last frame (T > 1), as the AVSS sets have frames beyond mask_num."""
        from cavp_amd.clips import ClipStore
        gs = torch.Generator().manual_seed(4321)
        store = ClipStore(stage=stage, max_frames=T, max_sources=1, max_channels=2, max_len=RAW_LEN if a.raw_audio else 1,
                          pcm_dtype=torch.int16, device=dev)
        for i in range(n_clips):
            frames, masks = [], []
            for k in range(T):
                frames.append(torch.randint(0, 256, stage + (3,), dtype=torch.uint8, generator=gs))
                mask = torch.zeros(stage, dtype=torch.uint8)
                for _ in range(1 + int(torch.rand((), generator=gs) < 0.25)):
                    c = int(torch.randint(1, pairs.K, (), generator=gs))
                    y, x = (int(torch.randint(0, stage[j] // 2, (), generator=gs)) for j in (0, 1))
                    mask[y:y + stage[0] // 3, x:x + stage[1] // 3] = RAW0 + c
                masks.append(mask)
            if T > 1 and i % 3 == 2:
                masks.pop()
            sources = []
            if a.raw_audio:
                n = int(torch.randint(RAW_LEN // 2, RAW_LEN + 1, (), generator=gs))
                sources.append((torch.randint(-3277, 3278, (2, n), dtype=torch.int16, generator=gs), 0))
            store.append(frames, masks, sources, tag=i % pairs.K)
        return store.freeze()

    replays = None
    rb = None
    aug = None
    wave_stage = None
    feeder = None
    if a.graph:
        from cavp_amd.pairs import PairResult
        s_image = torch.zeros(B, 3, a.hw, a.hw, device=dev)
        s_label = torch.zeros(B, a.hw, a.hw, dtype=torch.int64, device=dev)
        s_wave = torch.zeros(B, 1, 16000, device=dev)
        s_img_label = torch.zeros(B, pairs.K, dtype=torch.int64, device=dev)
        s_img_label[:, 1] = 1
        s_audio = torch.zeros(2 * B, 1, front.n_frames, front.n_mels, device=dev)
        s_shuf = torch.zeros_like(s_label)
        built = PairResult(B, 16000, pairs.K, (a.hw, a.hw), dev)
        opt = FusedSGDAdam(model, model.grad_arena(dev), a.lr, momentum=a.momentum, weight_decay=a.weight_decay)
        opt.use_device_schedule(a.lr, a.lr_power, a.total_iters, 0)
        guard = None
        if a.guard:
            from cavp_amd.optim import StepGuard
            guard = StepGuard(max_norm=a.max_norm, skip_nonfinite=True, history=64)
            opt.use_step_guard(guard)                           # before the captures: they record its four launches
        acc = None
        if a.accumulate is not None:
            from cavp_amd.accumulate import GradAccumulator
            acc = GradAccumulator(opt, a.accumulate)            # before the captures too: they record its gated launches
        start = {k: v.clone() for k, v in model.state_dict().items()}

        if a.augment:
            from cavp_amd.augment import AVS_SCALES, COCO_SCALES, AugResult, FrameAugment
            from cavp_amd.labels import LabelResult, LabelStage
            stage = (a.hw + a.hw // 2,) * 2
            aug = FrameAugment(crop=(a.hw, a.hw), scales=AVS_SCALES if a.resize else COCO_SCALES, jitter=None if a.resize else (.5, .5, .5, .25),
                               seed=1234 + rank, device=dev, max_batch=B, stage=stage, resize=a.resize)
            remap = torch.full((256,), -1, dtype=torch.int32)
            remap[RAW0 + 1:RAW0 + pairs.K] = torch.arange(1, pairs.K, dtype=torch.int32)
            stage_labels = LabelStage(num_classes=pairs.K, mode="multi_hot", remap=remap, device=dev, max_batch=B)
            s_frames = torch.zeros((B,) + stage + (3,), dtype=torch.uint8, device=dev)
            s_masks = torch.zeros((B,) + stage, dtype=torch.uint8, device=dev)
            s_sizes = torch.tensor([list(stage)] * B, dtype=torch.int32, device=dev)
            augmented, labelled = AugResult(B, (a.hw, a.hw), dev), LabelResult(B, pairs.K, (a.hw, a.hw), dev, True)
            if a.resident:                                      # the staging buffers are the feeder's: nothing is copied into them from here
                n_items = a.store_items if a.store_items is not None else 4 * B * world
                if a.clips is not None:                         # clips: the feeder draws the frame too, and gathers only that frame
                    from cavp_amd.clips import ClipFeeder, ClipFeedResult
                    store = build_clip_store(stage, n_items, a.clips)
                    feeder = ClipFeeder(store, batch=B, seed=1234, rank=rank, world=world)
                    fed = ClipFeedResult(B, store, dev)
                else:
                    from cavp_amd.store import BatchFeeder, FeedResult
                    store = build_store(stage, n_items)
                    feeder = BatchFeeder(store, batch=B, seed=1234, rank=rank, world=world)
                    fed = FeedResult(B, store, dev)
                s_frames, s_masks, s_sizes = fed.frames, fed.masks, fed.sizes
        if a.raw_audio:
            from cavp_amd.wave import WaveResult, WaveStage
            segments = a.clips if a.clips is not None else 1     # clips: T seconds are cropped, the drawn frame's second is kept
            wave_stage = WaveStage(audio_len=hyp.audio_len * segments, rates=(RAW_RATE,), max_sources=1, max_channels=2, max_len=RAW_LEN,
                                   segments=segments, device=dev, max_batch=B)
            wave_select = fed.select if segments > 1 else None
            s_pcm = torch.zeros((B, 1, 2, RAW_LEN), dtype=torch.int16, device=dev)
            s_pcm_len = torch.full((B, 1), RAW_LEN, dtype=torch.int32, device=dev)
            s_rate_idx = torch.zeros((B, 1), dtype=torch.int32, device=dev)
            s_n_ch = torch.full((B, 1), 2, dtype=torch.int32, device=dev)
            cut = WaveResult(B, 16000, dev)
            if feeder is not None:
                s_pcm, s_pcm_len, s_rate_idx, s_n_ch = fed.pcm, fed.length, fed.rate_idx, fed.n_ch

        def prologue_of(overwrite):
            def prologue():
                if feeder is not None:     # sampler + gather: this step's items into the staging buffers the two stages below read
                    feeder.feed(out=fed)
                if aug is not None:        # raw frames -> image, label -> remapped label, img_label: nothing returns to the host
                    aug(s_frames, s_masks, s_sizes, out=augmented)
                    stage_labels(augmented.label, out=labelled)
                    s_image.copy_(augmented.image)
                    s_label.copy_(labelled.label)
                    s_img_label.copy_(labelled.img_label)
                if wave_stage is not None:   # raw PCM -> the mono 16 kHz second the pair builder takes
                    wave_stage(s_pcm, s_pcm_len, s_rate_idx, s_n_ch, select=wave_select, out=cut)
                pairs(s_wave if wave_stage is None else cut.waveform, s_label, s_img_label, overwrite, out=built)
                s_audio.copy_(front(built.waveforms))
                s_shuf.copy_(built.label_shuffle)
            return prologue
        if a.rollback:                                          # everything an iteration's forward mutates, through whatever is enabled
            from cavp_amd.rollback import StepRollback
            rb = StepRollback(dev).add_model(model).add(pairs).add(crit)
            if aug is not None:
                rb.add(aug)
            if feeder is not None:
                rb.add(feeder)                                  # a skipped step sees the same batch again
            if drop_path is not None:
                rb.add(drop_path)                               # ... and the same DropPath masks
            rb.freeze()
        replays = []
        for ow in (False, True):
            rep = model.capture_train_step(s_image, s_audio, s_label, contrast=crit, label_shuffle=s_shuf,
                                           contrast_weight=a.contrast_weight, optimizer=opt, prologue=prologue_of(ow),
                                           **({"rollback": rb} if rb is not None else {}),
                                           **({"accumulate": acc} if acc is not None else {}))
            replays.append((rep, model._last_losses))           # (each graph has its own static loss buffers)
        if rb is None:
            # the warm-up passes of the captures ran the pair builder, the sampler and the BatchNorm statistics for real: start over
            # (with a rollback the captures undo their own passes and this is unnecessary)
            model.load_state_dict(start)
            if aug is not None:
                aug.manual_seed(1234 + rank)
            if feeder is not None:
                feeder.set_step(0)
            if drop_path is not None:
                drop_path.manual_seed(1234 + rank)
            pairs.manual_seed(1234 + rank)
            pairs.load_bank(torch.zeros(pairs.K, pairs.S, pairs.A, device=dev))
            crit.manual_seed(1234 + rank)

    validate = None
    if a.validate_every is not None:
        from cavp_amd.clips import ClipEvalResult
        from cavp_amd.metrics import ClipValidation
        T, Bv = a.clips, B // a.clips                           # Bv * T <= B frames per step: the stages' max_batch holds
        val_feeder = ClipFeeder(store, batch=Bv, rank=rank, world=world)
        ev = ClipEvalResult(Bv, store, dev)
        cv = ClipValidation(num_classes=pairs.K, ignore_index=255, max_frames=Bv * T, device=dev)
        # an augmentation stage of its own: eval_ draws nothing but advances the stage's call counter, and the training stream
        # must not depend on whether a validation pass ran
        val_aug = FrameAugment(crop=(a.hw, a.hw), jitter=None, device=dev, max_batch=Bv * T, stage=stage, resize=a.resize)
        v_aug, v_lab = AugResult(Bv * T, (a.hw, a.hw), dev), LabelResult(Bv * T, pairs.K, (a.hw, a.hw), dev, True)
        v_cut = WaveResult(Bv, 16000 * T, dev)

        def validate():
            """One pass over this rank's share of the store; every launch reads device values only"""
            model.eval()
            cv.reset()
            for _ in range(val_feeder.steps_per_pass):
                val_feeder.feed_clips(out=ev)
                val_aug.eval_(ev.frames.view(Bv * T, *stage, 3), ev.masks.view(Bv * T, *stage), ev.sizes, out=v_aug)
                stage_labels(v_aug.label, out=v_lab)
                if T > 1:
                    wave_stage(ev.pcm, ev.length, ev.rate_idx, ev.n_ch, out=v_cut)
                    audio = front(v_cut.waveform.view(Bv * T, 1, 16000))
                else:
                    audio = front(wave_stage(ev.pcm, ev.length, ev.rate_idx, ev.n_ch).waveform)
                cv.update(model.predict(v_aug.image, audio), v_lab.label.view(Bv, T, a.hw, a.hw), ev.count)
            model.train()
            val_aug.check()
            cv.check()
            return cv.results()

    N = a.accumulate or 1                                       # replays per update: the loop counts micro-steps, the prints windows
    total = a.steps * N
    for it in range(total):
        if validate is not None and it > 0 and it % a.validate_every == 0:
            all_, ms = validate()
            if rank == 0:
                fmt = lambda r: "mIoU {:.4f} acc {:.4f} fdr {:.4f} f1 {:.4f} f0.3 {:.4f}".format(*(float(v) for v in r))
                print(f"validation before step {it}: {val_feeder.steps_per_pass} steps of {Bv} clips x {T} frames;  ALL {fmt(all_)};  "
                      f"MS {fmt(ms)}", flush=True)
        if a.fixed_batch:
            g = torch.Generator().manual_seed(1234 + rank)      # the same batch every step
        if feeder is not None:                                  # resident: the batch is drawn and gathered inside the graph
            if a.fixed_batch:
                feeder.set_step(0)
            if wave_stage is None:
                s_wave.copy_(draw_pairs_batch()[0])
        else:
            image = torch.randn(B, 3, a.hw, a.hw, generator=g)
            label = torch.randint(0, a.num_classes, (B, a.hw, a.hw), generator=g)
        if replays is not None:                                 # copy the batch in, replay: nothing else is launched from here
            if feeder is None:
                wave, img_label = draw_pairs_batch()
            if feeder is not None:
                pass                                            # resident: nothing to draw, nothing to copy
            elif aug is not None:                               # raw material only: image, label and img_label come from the prologue
                frames, masks = draw_raw_batch(tuple(s_masks.shape[1:]))
                for dst, src in ((s_frames, frames), (s_masks, masks), (s_wave, wave)):
                    dst.copy_(src)
                if wave_stage is not None:
                    for dst, src in zip((s_pcm, s_pcm_len), draw_raw_audio()):
                        dst.copy_(src)
            else:
                for dst, src in ((s_image, image), (s_label, label), (s_wave, wave), (s_img_label, img_label)):
                    dst.copy_(src)
            rep, graph_terms = replays[1 if it >= 1 else 0]
            loss = rep()
            if it == 1:
                torch.cuda.synchronize()
                t0 = time.time()
            if guard is not None:                               # the display_iter pattern: one read per 5 steps, every step shown
                if it % 5 == 4 or it == total - 1:
                    rec = guard.read()
                    if first is None and len(rec["t"]):
                        first = float(rec["l_ce"][0] + a.contrast_weight * rec["l_ctr"][0])
                    for i in range(len(rec["t"]) if rank == 0 else 0):
                        mark = " SKIPPED" if rec["skipped"][i] else (" clipped" if rec["clipped"][i] else "")
                        print(f"step {int(rec['t'][i]):4d}  lr {rec['lr'][i]:.3e}  CE {rec['l_ce'][i]:.4f}  contrast {rec['l_ctr'][i]:.4f}  "
                              f"|g| {rec['grad_norm'][i]:.3e}  coef {rec['clip_coef'][i]:.3f}{mark}", flush=True)
                    if rec["dropped"]:
                        print(f"({rec['dropped']} records overwritten before this read)")
                continue
            if first is None:
                first = float(loss.item())
            if rank == 0 and (it + 1) % N == 0 and ((it // N) % 5 == 0 or it == total - 1):
                terms = "  (CE {:.4f}, contrast {:.4f})".format(*(float(t.item()) for t in graph_terms))
                print(f"iter {it // N:4d}  lr {float(opt.last_lr().item()):.3e}  loss {float(loss.item()):.4f}{terms}", flush=True)
            continue
        image, label = image.to(dev), label.to(dev)
        built = None
        if pairs is not None:                                   # B clips + image labels -> matched ‖ shuffled clips, shuffle labels
            wave, img_label = draw_pairs_batch()
            built = pairs(wave.to(dev), label, img_label.to(dev), overwrite=it >= 1)
            audio = front(built.waveforms)
        elif front is not None:                                 # matched clips ‖ shuffled clips = 2B (cavp_model.py:181)
            wave = (torch.randn(2 * B, 1, 16000, generator=g) * 0.1).to(dev)
            audio = front(wave)
        else:
            audio = (torch.rand(2 * B, 1, 96, 64, generator=g) * 2 - 1).to(dev)
        if built is not None:
            loss = model.train_step(image, audio, label, contrast=crit, label_shuffle=built.label_shuffle,
                                    contrast_weight=a.contrast_weight)
        elif crit is not None:
            shuf = label.clone()
            shuf[B // 2:] = 0
            loss = model.train_step(image, audio, label, contrast=crit, label_shuffle=shuf, contrast_weight=a.contrast_weight)
        else:
            loss = model.train_step(image, audio, label)
        if opt is None:
            opt = FusedSGDAdam(model, model._grad_arena, a.lr, momentum=a.momentum, weight_decay=a.weight_decay)
        # the reference sets the learning rate AFTER the optimiser step (trainer_cavp_vpo_mono.py:193-203): step `it` runs with
        # the rate computed at the end of step it - 1 (the configured start rate for the first one)
        opt.step(sched(it - 1) if it > 0 else a.lr)
        if it == 1:                                             # skip the first two (allocation / warm-up) steps
            torch.cuda.synchronize()
            t0 = time.time()
        if first is None:
            first = float(loss.item())
        if rank == 0 and (it % 5 == 0 or it == a.steps - 1):
            terms = "  (CE {:.4f}, contrast {:.4f})".format(*(float(t.item()) for t in model._last_losses)) if crit is not None else ""
            print(f"iter {it:4d}  lr {sched(it):.3e}  loss {float(loss.item()):.4f}{terms}", flush=True)
    torch.cuda.synchronize()
    if rank == 0 and t0 is not None and total > 2:
        dt = (time.time() - t0) / (total - 2)
        print(f"{B * world / dt:.1f} frames/s over {world} GPU(s) ({dt * 1e3:.1f} ms/step incl. host-side input generation, "
              f"{'one graph replay' if a.graph else 'eager launches, optimiser step'})")
    if rank == 0 and a.accumulate is not None:
        rd = acc.read()
        print(f"accumulate: {rd['windows']} windows of {N} replays ({rd['micro_total']} replays, effective batch {B * N}), "
              f"t = {opt.iteration()}, accumulator {acc.nbytes / 1e6:.1f} MB")
    if rb is not None:
        stats, skipped = rb.stats(), int(guard.last()["skipped_total"].item())
        if rank == 0:
            print(f"rollback: {stats['restores']} restores in {stats['saves']} iterations, the guard skipped {skipped} "
                  f"({sum(rb.registered_bytes().values())} bytes registered: {rb.registered_bytes()})")
        if stats["restores"] != skipped:
            raise SystemExit("rollback: the restores and the guard's skipped steps disagree")
    if rank == 0 and pairs is not None:
        plan = pairs.last_plan()
        print(f"pairs, last step: {int(plan['if_match'].sum())} of {B} rows matched, {plan['n_overwritten']} taken from the sound bank "
              f"(q = {plan['q']} of {plan['n_false']} mismatched), {plan['n_written']} clips queued")
    if rank == 0 and aug is not None:
        aug.check()
        stage_labels.check()
        print(f"input chain: {'resize' if a.resize else 'pad + crop'} augmentation, img_label from the augmented mask: "
              f"{labelled.img_label[:, 1:].sum(0).tolist()} frames per foreground class in the last batch")
    if rank == 0 and feeder is not None:
        feeder.check()
        print(f"resident: {len(store)} items, {store.nbytes / 1e6:.1f} MB on the device ({store.arena_bytes()}); step {feeder.step()} = epoch "
              f"{feeder.epoch_of(feeder.step())} of {feeder.steps_per_epoch} steps; items of the last batch {fed.index[:8].tolist()} ...")
        if a.clips is not None:
            print(f"clips: {a.clips} frames each, {store.total_frames} frames resident; frames drawn in the last batch "
                  f"{fed.select[:8].tolist()} ..." + (f"; the validation feeder stands at step {val_feeder.eval_step()}, the training "
                  f"feeder's eval counter at {feeder.eval_step()}" if validate is not None else ""))
    if rank == 0 and wave_stage is not None:
        wave_stage.check()
        print(f"raw audio: {RAW_LEN / RAW_RATE:.0f} s of {RAW_RATE} Hz int16 stereo per row -> [B, 1, 16000] by WaveStage; rms of the last batch "
              f"{float(cut.waveform.square().mean().sqrt()):.4f}")
    if rank == 0 and a.fixed_batch:
        print(f"fixed batch: loss {first:.4f} -> {float(loss.item()):.4f} after {a.steps} steps")
    if rank == 0 and a.preview and a.steps > 0:
        from cavp_amd.augment import IMAGENET_MEAN, IMAGENET_STD
        from cavp_amd.preview import PreviewStage
        last = (s_image, s_audio, s_label) if replays is not None else (image, audio, label)
        model.eval()
        mask = model.predict(last[0], last[1][:B].contiguous())            # the matched clips: the first half of the 2B
        pv = PreviewStage(max(a.num_classes, 2), IMAGENET_MEAN, IMAGENET_STD, device=dev, max_batch=B)
        panels = pv(last[0], last[2], mask=mask)
        pics = pv.read(panels)
        pv.check()
        os.makedirs(a.preview, exist_ok=True)
        shown = min(B, 4)
        for name, frames in pics.items():
            for b in range(shown):
                frames[b].save(os.path.join(a.preview, f"{name}_{b}.png"))
        print(f"preview: {3 * shown} PNG files in {a.preview} ({B} frames, {panels.buffer.numel()} bytes copied to the host; "
              f"classes predicted in frame 0: {sorted(set(pics['y_tilde'][0].tobytes()))[:8]})")
    if world > 1:
        import torch.distributed as dist
        dist.destroy_process_group()


if __name__ == "__main__":
    main()
