"""Host side of the step rollback (cavp_amd/rollback.py, csrc/rollback.hip): the ctypes mirrors of struct cavp_rollback_range /
cavp_rollback_state against the header and the library, the new prototypes beside an unchanged ABI number, the block prefix of a
mixed table against a plain-Python restatement, every refusal, and which buffers add_model finds.  No GPU needed."""
import ctypes
import os
import re
import types

import pytest
import torch
import torch.nn as nn

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = {"cavp_rollback_range_bytes": 0, "cavp_rollback_state_bytes": 0, "cavp_rollback_blocks": 2, "cavp_rollback_save": 5,
         "cavp_rollback_restore": 6}
C_TYPES = {"int64_t": ctypes.c_int64, "int32_t": ctypes.c_int32, "void*": ctypes.c_void_p}


def _header():
    return open(os.path.join(REPO, "include", "cavp_hip.h")).read()


# ------------------------------------------------------------------------------------------------------------ the mirrors
def test_rollback_structs_match_header_and_library():
    from cavp_amd import _lib, build
    from cavp_amd.rollback import ROLLBACK_SCRUB, RollbackRange, RollbackState
    build.build(verbose=False)
    hdr = _header()
    for struct, mirror in (("cavp_rollback_range", RollbackRange), ("cavp_rollback_state", RollbackState)):
        body = hdr[hdr.index("typedef struct %s {" % struct):hdr.index("} %s;" % struct)]
        body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
        fields = re.findall(r"\b(int64_t|int32_t|void\*)\s+([a-z0-9_]+)\s*;", body)
        assert [(n, C_TYPES[t]) for t, n in fields] == [(n, t) for n, t in mirror._fields_], struct
    lib = _lib.load()
    assert lib.cavp_rollback_range_bytes() == ctypes.sizeof(RollbackRange) == 32
    assert lib.cavp_rollback_state_bytes() == ctypes.sizeof(RollbackState) == 16
    assert int(re.search(r"#define CAVP_ROLLBACK_SCRUB +(\d+)", hdr).group(1)) == ROLLBACK_SCRUB


def test_rollback_prototypes_header_and_exports_agree():
    from cavp_amd import _lib, build
    build.build(verbose=False)
    hdr = re.sub(r"/\*.*?\*/", "", _header(), flags=re.S)
    raw = ctypes.CDLL(_lib.LIB_PATH)
    for name, nargs in NAMES.items():
        assert name in _lib.PROTOTYPES and len(_lib.PROTOTYPES[name][1]) == nargs, name
        assert hasattr(raw, name), name
        decl = re.search(r"\b%s\s*\(([^)]*)\)\s*;" % name, hdr)
        assert decl is not None, name
        params = [p for p in decl.group(1).split(",") if p.strip() and p.strip() != "void"]
        assert len(params) == nargs, (name, params)
    # additive: the ABI number is what it was, and header, exports and ctypes table still agree one to one
    assert _lib.ABI_VERSION == 16 and _lib.load().cavp_abi_version() == 16
    assert int(re.search(r"#define CAVP_ABI_VERSION (\d+)", hdr).group(1)) == 16
    declared = set(re.findall(r"\b(cavp_[a-z0-9_]+)\s*\(", _header()))
    assert declared == set(_lib.PROTOTYPES)
    assert "rollback.hip" in build.SOURCES


# ------------------------------------------------------------------------------------------------------- the block prefix
def _blocks(live, nbytes):
    """restatement: 1 KiB blocks on a grid that starts at the 16-byte boundary at or below the live address"""
    first = live - live % 16
    return (live + nbytes - first + 1023) // 1024


def test_block_prefix_of_a_mixed_table():
    from cavp_amd import _lib
    from cavp_amd.rollback import BLOCK_BYTES, ROLLBACK_SCRUB, SPAN_BLOCKS, build_table
    lib = _lib.load()
    assert BLOCK_BYTES == 1024 and SPAN_BLOCKS == 16
    for live, n in ((0, 4), (0, 1024), (0, 1028), (4, 1020), (4, 1024), (12, 1012), (12, 1016), (1 << 40, 1 << 30), (8, 0)):
        assert lib.cavp_rollback_blocks(live, n) == (_blocks(live, n) if n else 0), (live, n)
    span = BLOCK_BYTES * SPAN_BLOCKS
    base, cur, entries = 1 << 20, 0, []
    sizes = [4, 8, 12, 16, 20, 192, 256, 8192, span - 16, span, span + 4, 3 * span + 8, 8, 2048]
    for i, n in enumerate(sizes):
        mis = (0, 4, 8, 12)[i % 4]
        entries.append((base + cur + mis, n, ROLLBACK_SCRUB if i == 6 else 0))
        cur += (n + mis + 63) // 64 * 64
    shadow_base = 1 << 30
    tab, total, shadow_bytes = build_table(entries, shadow_base)
    blk, end = 0, 0
    for (live, n, flags), row in zip(entries, tab):
        assert (row.live, row.nbytes, row.flags, row.blk0) == (live, n, flags, blk)
        blk += _blocks(live, n)
        if flags & ROLLBACK_SCRUB:
            assert row.shadow is None
            continue
        off = row.shadow - shadow_base
        assert off >= end and off - end < 32 and row.shadow % 16 == live % 16     # packed, and on the live range's 16-byte phase
        end = off + n
    assert total == blk and shadow_bytes >= end and shadow_bytes % 16 == 0
    # the model's share: ~370 ranges of at most 8 KiB are a few dozen workgroup spans, not one workgroup each
    small = [(base + 512 * i * 17, n, 0) for i, n in enumerate([192, 192, 8] * 20 + [8192, 8192, 8] * 20)]
    _, total_small, _ = build_table(small, shadow_base)
    assert total_small == sum(_blocks(a, n) for a, n, _ in small) == 20 * 3 + 20 * 17
    assert (total_small + SPAN_BLOCKS - 1) // SPAN_BLOCKS < len(small) // 4
    empty, total0, bytes0 = build_table([], shadow_base)
    assert total0 == 0 and bytes0 == 0


# ------------------------------------------------------------------------------------------------------------ the refusals
def test_rollback_refusals():
    from cavp_amd._lib import CavpError
    from cavp_amd.contrast import ContrastLoss
    from cavp_amd.optim import StepGuard
    from cavp_amd.rollback import StepRollback
    with pytest.raises(CavpError):
        StepRollback("cpu")
    rb = StepRollback("cuda:0")
    with pytest.raises(CavpError, match="CPU tensor"):
        rb.add_tensor(torch.zeros(8))
    with pytest.raises(CavpError, match="CPU tensor"):
        rb.add_scrub(torch.zeros(8))
    with pytest.raises(CavpError, match="contiguous"):
        rb.add_tensor(torch.zeros(8, 8).t())
    with pytest.raises(CavpError, match="contiguous"):
        rb.add_scrub(torch.zeros(8, 8)[:, ::2])
    with pytest.raises(CavpError, match="tensor is required"):
        rb.add_tensor([1, 2, 3])
    with pytest.raises(CavpError, match="rollback_ranges"):
        rb.add(object())
    with pytest.raises(CavpError, match="use_device_sampler"):
        rb.add(ContrastLoss(0.1, 255, 8))                      # the host sampler keeps no device state
    # ranges: the address arithmetic needs no device
    for live, n in ((4096, 6), (4096, 2), (4098, 8), (4096, 0), (4096, -4)):
        with pytest.raises(CavpError, match="multiple of 4"):
            rb._add_raw(live, n, 0, "t")
    rb._add_raw(4096, 64, 0, "a")
    rb._add_raw(4160, 8, 0, "b")                               # adjacent is not overlapping
    with pytest.raises(CavpError, match="already registered"):
        rb._add_raw(4096, 64, 0, "c")
    with pytest.raises(CavpError, match="already registered"):
        rb._add_raw(4160, 8, 1, "c")                           # ... nor as a scrub range
    for live, n in ((4092, 8), (4100, 4), (4156, 8), (4000, 1000), (4164, 4)):
        with pytest.raises(CavpError, match="overlaps"):
            rb._add_raw(live, n, 0, "c")
    assert rb.registered_bytes() == {"a": 64, "b": 8}
    # use before freeze()
    for call in (rb.save, rb.restore, rb.stats, rb.reset_stats, rb.ranges):
        with pytest.raises(CavpError, match="freeze"):
            call()
    # guards: not a guard, not attached, on another device - all before the frozen check and before any launch
    with pytest.raises(CavpError, match="StepGuard"):
        rb.restore_if_skipped(object())
    with pytest.raises(CavpError, match="not attached"):
        rb.restore_if_skipped(StepGuard())
    elsewhere = StepGuard()
    elsewhere._buf = torch.zeros(64, dtype=torch.uint8)         # (a guard whose state block lives on another device)
    with pytest.raises(CavpError, match="the guard on"):
        rb.restore_if_skipped(elsewhere)


def test_capture_refuses_rollback_without_a_skipping_guard():
    """capture_train_step(rollback=): no optimiser, no guard, both skip rules off, not frozen - refused before any launch."""
    from cavp_amd._lib import CavpError
    from cavp_amd.cavp_model import CAVP
    from cavp_amd.optim import StepGuard
    from cavp_amd.rollback import StepRollback
    x = torch.zeros(1)

    def call(optimizer, rollback):
        return CAVP.capture_train_step(types.SimpleNamespace(), x, x, x, optimizer=optimizer, rollback=rollback)
    rb = StepRollback("cuda:0")
    with pytest.raises(CavpError, match="frozen"):
        call(None, rb)
    with pytest.raises(CavpError, match="frozen"):
        call(None, object())
    rb._frozen = True                                           # (freeze() itself needs the device)
    with pytest.raises(CavpError, match="StepGuard"):
        call(None, rb)
    arena = types.SimpleNamespace(flat=x)
    model = types.SimpleNamespace(_grad_arena=arena)
    opt = types.SimpleNamespace(_sched=x, _arena=arena, _guard=None)
    with pytest.raises(CavpError, match="StepGuard"):
        CAVP.capture_train_step(model, x, x, x, optimizer=opt, rollback=rb)
    opt._guard = StepGuard(skip_nonfinite=False, skip_nonfinite_loss=False)
    with pytest.raises(CavpError, match="both skip rules off"):
        CAVP.capture_train_step(model, x, x, x, optimizer=opt, rollback=rb)


# --------------------------------------------------------------------------------------------------------------- add_model
def _args(C=2):
    return types.SimpleNamespace(seg_model="DeepLabV3Plus", last_three_dilation_stride=[False, False, False], audio_backbone="vgg",
                                 num_classes=C, batch_size=2, local_rank="cpu")


def test_add_model_finds_every_tracking_batchnorm():
    from cavp_amd.cavp_model import CAVP
    from cavp_amd.rollback import bn_state_tensors
    m = CAVP(50, None, num_classes=2, args=_args())
    bns = [mod for mod in m.modules() if isinstance(mod, nn.modules.batchnorm._BatchNorm) and mod.track_running_stats]
    assert len(bns) > 50
    found = bn_state_tensors(m)
    assert len(found) == 3 * len(bns)
    sd = m.state_dict()
    assert {k for k, _ in found} == {k for k in sd if k.rsplit(".", 1)[-1] in ("running_mean", "running_var", "num_batches_tracked")}
    assert all(t.data_ptr() == sd[k].data_ptr() for k, t in found)                  # the buffers themselves, not copies
    assert len({t.data_ptr() for _, t in found}) == len(found)
    total = sum(t.numel() * t.element_size() for _, t in found)
    print(f"{len(bns)} tracking BatchNorm modules, {len(found)} ranges, {total} bytes")
    assert all(t.numel() * t.element_size() % 4 == 0 for _, t in found)
    # registration does not depend on .training: frozen layers are simply never written
    m.eval()
    assert [k for k, _ in bn_state_tensors(m)] == [k for k, _ in found]
    # a layer without running statistics is left out
    m.train()
    extra = nn.Sequential(nn.BatchNorm2d(8, track_running_stats=False), nn.BatchNorm1d(4), nn.GroupNorm(2, 4), nn.LayerNorm(4))
    assert [k for k, _ in bn_state_tensors(extra)] == ["1.running_mean", "1.running_var", "1.num_batches_tracked"]
    # SyncBatchNorm-converted: the same ranges under the same names
    sync = nn.SyncBatchNorm.convert_sync_batchnorm(m)
    assert any(isinstance(mod, nn.SyncBatchNorm) for mod in sync.modules())
    found_sync = bn_state_tensors(sync)
    assert [(k, tuple(t.shape), t.dtype) for k, t in found_sync] == [(k, tuple(t.shape), t.dtype) for k, t in found]
