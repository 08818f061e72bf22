"""The device preview stage (cavp_amd/preview.py, csrc/preview.hip) against tests/golden/preview.npz - the pictures the reference's
own functions made - and the numpy restatement of its specification (tests/_preview_ref.py, held to that fixture by
tests/test_preview_host.py).  Everything it produces is a byte: every comparison is exact equality.  B = 3 with 5 x 7 images (35
pixels: no 16-byte alignment of the second image, the element path) and 32 x 48 (the vector path; 1536 pixels hold every byte level
six times per channel)."""
import os

import numpy as np
import pytest
import torch

from tests import _preview_ref as R

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
MEAN, STD = (0.485, 0.456, 0.406), (0.229, 0.224, 0.225)
KS = (2, 24, 71, 256)
SHAPES = {"s": (5, 7), "v": (32, 48)}
_logits = {}


@pytest.fixture(scope="module")
def gold():
    with np.load(os.path.join(REPO, "tests", "golden", "preview.npz")) as z:
        return {k: z[k] for k in z.files}


def _stage(K, **kw):
    from cavp_amd.preview import PreviewStage
    kw.setdefault("max_batch", 8)
    return PreviewStage(K, MEAN, STD, device=DEV, **kw)


def _lg(K, tag):
    """The seeded fixture logits, made once per case (read only)."""
    if (K, tag) not in _logits:
        _logits[K, tag] = R.fixture_logits(K, SHAPES[tag])
    return _logits[K, tag]


def _dev(a, dtype=None):
    return None if a is None else torch.from_numpy(np.ascontiguousarray(a if dtype is None else a.astype(dtype))).to(DEV)


def _run(pv, image, labels, **pred):
    """One call; asserts that no input was modified and that the panels are views into the arena."""
    ins = [t for t in (image, labels) + tuple(pred.values()) if t is not None]
    keep = [t.clone() for t in ins]
    out = pv(image, labels, **pred)
    torch.cuda.synchronize()
    for t, k in zip(ins, keep):
        bits = (lambda v: v.view(torch.int32)) if t.is_floating_point() else (lambda v: v)      # a NaN equals itself bit for bit
        assert torch.equal(bits(t), bits(k)), "an input was modified"
    assert out.buffer.is_contiguous() and out.buffer.dtype == torch.uint8
    lo, hi = out.buffer.data_ptr(), out.buffer.data_ptr() + out.buffer.numel()
    for p in (out.x, out.y, out.y_tilde):
        assert p is None or (p.dtype == torch.uint8 and lo <= p.data_ptr() < hi)
    return out


def _np(t):
    return t.cpu().numpy()


@pytest.mark.parametrize("K", KS)
@pytest.mark.parametrize("ldt", [np.int64, np.uint8], ids=["i64", "u8"])
@pytest.mark.parametrize("source", ["logits", "mask"])
@pytest.mark.parametrize("tag", SHAPES)
def test_fixture_panels(gold, tag, source, ldt, K):
    """The reference's x, y and y_tilde bytes: int8-quantised logits with many exact ties and one NaN, labels with 255, -1, 259 and
    300, image 1 all 255; the mask source is the argmax as seg_predict would write it."""
    lg = _lg(K, tag)
    pred = {"logits": _dev(lg)} if source == "logits" else {"mask": _dev(R.argmax_first(lg))}
    pv = _stage(K)
    for _ in range(2):
        out = _run(pv, _dev(gold[f"image_{tag}"]), _dev(gold[f"labels_{tag}"], ldt), **pred)
        h, w = SHAPES[tag]
        assert tuple(out.x.shape) == (3, h, w, 3) and tuple(out.y.shape) == (3, h, w) == tuple(out.y_tilde.shape)
        assert tuple(out.buffer.shape) == (3, 5 * h * w)
        assert np.array_equal(_np(out.x), gold[f"x_{tag}"])
        assert np.array_equal(_np(out.y), gold[f"y_{tag}"])
        yt = gold[f"yt_{tag}_K{K}_{'i64' if ldt is np.int64 else 'u8'}"]
        assert np.array_equal(_np(out.y_tilde), yt)
        # per image the arena holds x, then y, then y_tilde
        want = np.concatenate([gold[f"x_{tag}"].reshape(3, -1), gold[f"y_{tag}"].reshape(3, -1), yt.reshape(3, -1)], axis=1)
        assert np.array_equal(_np(out.buffer), want)
        pv.check()


@pytest.mark.parametrize("tag", SHAPES)
def test_dropped_panels_and_label_shapes(gold, tag):
    """labels=None: no y panel and no propagation (generate_image); image=None: no x panel; labels as [B, 1, H, W]."""
    K = 24
    lg, img, lab = _dev(_lg(K, tag)), _dev(gold[f"image_{tag}"]), _dev(gold[f"labels_{tag}"])
    h, w = SHAPES[tag]
    pv = _stage(K)
    out = _run(pv, img, None, logits=lg)
    assert out.y is None and tuple(out.buffer.shape) == (3, 4 * h * w)
    assert np.array_equal(_np(out.x), gold[f"x_{tag}"]) and np.array_equal(_np(out.y_tilde), R.argmax_first(_lg(K, tag)))
    out = _run(pv, None, lab[:, None], logits=lg)
    assert out.x is None and tuple(out.buffer.shape) == (3, 2 * h * w)
    assert np.array_equal(_np(out.y), gold[f"y_{tag}"]) and np.array_equal(_np(out.y_tilde), gold[f"yt_{tag}_K{K}_i64"])
    out = _run(pv, None, None, mask=_dev(R.argmax_first(_lg(K, tag))))
    assert out.x is None and out.y is None and np.array_equal(_np(out.buffer).reshape(3, h, w), R.argmax_first(_lg(K, tag)))
    out = _run(_stage(K, ignore_index=5), img, lab, logits=lg)
    exp = R.preview(gold[f"image_{tag}"], gold[f"labels_{tag}"], logits=_lg(K, tag), mean=MEAN, std=STD, ignore=5)
    assert (exp["y_tilde"] != gold[f"yt_{tag}_K{K}_i64"]).any() and np.array_equal(_np(out.y_tilde), exp["y_tilde"])
    pv.check()


@pytest.mark.parametrize("tag", SHAPES)
def test_image_values_outside_the_unit_range_and_bad_values(tag):
    """Values far outside [0, 1] wrap as torch's CPU cast does; a NaN, an infinity and 1e12 write 0, are counted, and check() raises
    once and then is clear."""
    from cavp_amd._lib import CavpError
    h, w = SHAPES[tag]
    rs = np.random.RandomState(5)
    img = ((rs.rand(3, 3, h, w) * 12 - 6)).astype(np.float32)               # de-normalised: about [-1, 2] -> bytes wrap both ways
    img[0, 0, 0, :7] = np.array([-1.5, -0.3, 255.9, 256.7, 300, 511.2, -255.5], dtype=np.float32)
    exp = R.preview(img, None, mask=np.zeros((3, h, w), np.uint8), mean=MEAN, std=STD)
    ref = torch.stack([torch.stack([t.mul(s).add(m) for t, m, s in zip(i, MEAN, STD)]) for i in torch.from_numpy(img.copy())]).mul(255)
    assert exp["bad"] == 0 and np.array_equal(exp["x"], ref.byte().permute(0, 2, 3, 1).numpy())
    assert (ref < 0).any() and (ref >= 256).any()
    pv = _stage(2)
    mask = torch.zeros((3, h, w), dtype=torch.uint8, device=DEV)
    out = _run(pv, _dev(img), None, mask=mask)
    assert np.array_equal(_np(out.x), exp["x"])
    pv.check()
    img[1, 2, h - 1, w - 1], img[2, 0, 1, 1], img[0, 1, 0, 0] = np.nan, np.inf, 1e12
    exp = R.preview(img, None, mask=np.zeros((3, h, w), np.uint8), mean=MEAN, std=STD)
    assert exp["bad"] == 3 and exp["x"][1, h - 1, w - 1, 2] == 0
    out = _run(pv, _dev(img), None, mask=mask)
    assert np.array_equal(_np(out.x), exp["x"])
    with pytest.raises(CavpError, match="3 image value"):
        pv.check()
    pv.check()               # the counter was cleared by the report


def test_mask_route_equals_logits_route():
    """seg_predict's mask of low-resolution logits, then this stage, equals this stage on the full-resolution logits the repository's
    bilinear op makes of them: the low-resolution path never needs the [B, C, H, W] tensor."""
    from cavp_amd import ops
    B, C, hi, wi, H, W = 3, 24, 8, 12, 32, 48
    g = torch.Generator().manual_seed(3)
    lo = (torch.randn(B, hi, wi, C, generator=g) * 4).to(DEV)
    full = ops.bilinear_to_nchw(lo, torch.empty((B, C, H, W), dtype=torch.float32, device=DEV), False)
    mask = torch.full((B, H, W), 255, dtype=torch.uint8, device=DEV)
    ops.seg_predict(lo, (H, W), mask=mask)
    lab = torch.randint(0, C, (B, H, W), generator=g)
    lab[:, :3] = 255
    lab, img = lab.to(DEV), torch.randn(B, 3, H, W, generator=g).to(DEV)
    pv = _stage(C)
    a, b = _run(pv, img, lab, logits=full), _run(pv, img, lab, mask=mask)
    assert torch.equal(a.buffer, b.buffer) and len(a.y_tilde.unique()) > 4
    assert np.array_equal(_np(a.y_tilde), R.y_tilde_panel(R.argmax_first(_np(full)), _np(lab)))


@pytest.mark.parametrize("rname,size", [("r256", (256, 256)), ("r9x13", (9, 13))])
@pytest.mark.parametrize("ldt", [np.int64, np.uint8], ids=["i64", "u8"])
@pytest.mark.parametrize("tag", SHAPES)
def test_resized_panels(gold, tag, ldt, rname, size):
    """size=(256, 256), the reference's resize=True, and an odd size: PIL's NEAREST pictures of the fixture."""
    K = 71
    pv = _stage(K, size=size)
    out = _run(pv, _dev(gold[f"image_{tag}"]), _dev(gold[f"labels_{tag}"], ldt), logits=_dev(_lg(K, tag)))
    assert tuple(out.buffer.shape) == (3, 5 * size[0] * size[1]) and tuple(out.x.shape) == (3,) + size + (3,)
    assert np.array_equal(_np(out.x), gold[f"x_{tag}_{rname}"]) and np.array_equal(_np(out.y), gold[f"y_{tag}_{rname}"])
    yt = gold[f"yt_{tag}_K71_i64_{rname}"] if ldt is np.int64 else R.resize(gold[f"yt_{tag}_K71_u8"], size)
    assert np.array_equal(_np(out.y_tilde), yt)
    out = _run(pv, None, None, mask=_dev(R.argmax_first(_lg(K, tag))))          # the gather with the y_tilde panel alone
    assert np.array_equal(_np(out.y_tilde), R.resize(R.argmax_first(_lg(K, tag)), size))
    pv.check()


@pytest.mark.parametrize("guard", [64, 67], ids=["aligned", "odd_base"])
@pytest.mark.parametrize("size", [None, (9, 13), (12, 16)], ids=["same", "9x13", "12x16"])
@pytest.mark.parametrize("tag", SHAPES)
def test_nothing_is_written_outside_the_arena(gold, tag, size, guard):
    """out= carved from sentinel-filled buffers (the arena and, with a resize, the staging arena): the bytes around them are untouched.
    odd_base: the arenas start 3 bytes off a dword, so 32 x 48 and 12 x 16 take the element paths as well."""
    from cavp_amd.preview import PreviewResult
    K = 71
    h, w = SHAPES[tag]
    oh, ow = size or (h, w)
    pv = _stage(K, size=size)
    out = PreviewResult(3, (h, w), (oh, ow), True, True, torch.device(DEV))
    bufs = []
    for name, n in (("buffer", 15 * oh * ow),) + ((("_staging", 15 * h * w),) if size else ()):
        buf = torch.full((n + 2 * guard,), 0xA5, dtype=torch.uint8, device=DEV)
        setattr(out, name, buf[guard:guard + n].view(3, -1))
        bufs.append((buf, n))
    out._carve(True, True)
    got = pv(_dev(gold[f"image_{tag}"]), _dev(gold[f"labels_{tag}"]), logits=_dev(_lg(K, tag)), out=out)
    torch.cuda.synchronize()
    assert got is out
    exp = R.preview(gold[f"image_{tag}"], gold[f"labels_{tag}"], logits=_lg(K, tag), mean=MEAN, std=STD, size=size)
    for k in ("x", "y", "y_tilde"):
        assert np.array_equal(_np(getattr(out, k)), exp[k]), k
    for buf, n in bufs:
        assert (buf[:guard] == 0xA5).all() and (buf[guard + n:] == 0xA5).all()
    pv.check()


def test_out_made_for_other_shapes_is_refused(gold):
    from cavp_amd._lib import CavpError
    pv = _stage(71)
    img, lab, lg = _dev(gold["image_s"]), _dev(gold["labels_s"]), _dev(_lg(71, "s"))
    out = pv(img, lab, logits=lg)
    with pytest.raises(CavpError, match="out="):
        pv(None, lab, logits=lg, out=out)
    with pytest.raises(CavpError, match="out="):
        _stage(71, size=(9, 13))(img, lab, logits=lg, out=out)
    assert pv(img, lab, logits=lg, out=out) is out


def test_graph_capture_seg_predict_then_preview():
    """seg_predict -> PreviewStage (with the resize gather) captured in one torch.cuda.graph on one stream (capture raises if anything
    synchronises): three replays with fresh inputs equal the eager chain and the restatement."""
    from cavp_amd import ops
    B, C, hi, wi, H, W, size = 3, 24, 8, 12, 32, 48, (40, 36)
    pv_cap, pv_eager = _stage(C, size=size), _stage(C, size=size)

    def staged(k):
        g = torch.Generator().manual_seed(50 + k)
        lab = torch.randint(0, C, (B, H, W), generator=g)
        lab[:, k:k + 2] = 255
        return [(torch.randn(B, hi, wi, C, generator=g) * 4).to(DEV), torch.randn(B, 3, H, W, generator=g).to(DEV), lab.to(DEV)]

    def chain(pv, ins, mask, out=None):
        ops.seg_predict(ins[0], (H, W), mask=mask)
        return pv(ins[1], ins[2], mask=mask, out=out)

    ins = staged(0)
    mask_cap = torch.zeros((B, H, W), dtype=torch.uint8, device=DEV)
    mask_eager = torch.zeros_like(mask_cap)
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        out = chain(pv_cap, ins, mask_cap)                  # warm-up: allocates the device state, the tables and the out= buffers
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        chain(pv_cap, ins, mask_cap, out)
    for k in range(3):
        for dst, src in zip(ins, staged(k + 1)):
            dst.copy_(src)
        out.buffer.fill_(0x5A)
        graph.replay()
        torch.cuda.synchronize()
        eager = chain(pv_eager, ins, mask_eager)
        torch.cuda.synchronize()
        assert torch.equal(out.buffer, eager.buffer), k
        exp = R.preview(_np(ins[1]), _np(ins[2]), mask=_np(mask_eager), mean=MEAN, std=STD, size=size)
        for name in ("x", "y", "y_tilde"):
            assert np.array_equal(_np(getattr(out, name)), exp[name]), (k, name)
        pv_cap.check()


@pytest.mark.parametrize("size", [None, (256, 256)], ids=["same", "256"])
def test_read_returns_the_reference_pictures(gold, size):
    """read(): modes, sizes, getpalette() and bytes of the PIL pictures equal the fixture's."""
    pytest.importorskip("PIL")
    K, tag = 71, "s"
    h, w = size or SHAPES[tag]
    suffix = "_r256" if size else ""
    pv = _stage(K, size=size)
    out = pv(_dev(gold[f"image_{tag}"]), _dev(gold[f"labels_{tag}"]), logits=_dev(_lg(K, tag)))
    for _ in range(2):                                       # the second read reuses the pinned buffer
        pics = pv.read(out)
        assert sorted(pics) == ["x", "y", "y_tilde"] and all(len(v) == 3 for v in pics.values())
        for k, key, mode in zip(("x", "y", "y_tilde"), (f"x_{tag}", f"y_{tag}", f"yt_{tag}_K{K}_i64"), gold["modes"].tolist()):
            for b, pic in enumerate(pics[k]):
                assert pic.mode == mode and pic.size == (w, h)
                assert np.array_equal(np.asarray(pic), gold[key + suffix][b]), (k, b)
                if mode == "P":
                    assert pic.getpalette() == gold[f"palette_K{K}"].tolist() == pv.palette
    only = pv.read(pv(None, None, logits=_dev(_lg(K, tag))))
    assert sorted(only) == ["y_tilde"] and only["y_tilde"][0].size == (w, h)
