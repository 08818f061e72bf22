#!/usr/bin/env python3
"""Generate tests/golden/preview.npz by running the REFERENCE's own picture functions - get_pallete, colorize_mask and DeNormalize,
a read-only import of utils/tensor_board.py from a checkout of the reference (--reference DIR) - through lines 94-130 of
Tensorboard.upload_wandb_image, restated here around those functions (the method itself needs a wandb run), on the CPU.

Authoring-container only, on the recipe of tools/make_golden_clipval.py: the stub packages of tools/_shims stand in for the
reference's module-scope imports.  torchvision is not installed, so ToPILImage is restated as its published float path,
pic.mul(255).byte() followed by the CHW -> HWC transpose; everything else is the reference's code or PIL's.

Two shapes, B = 3: "s" 5 x 7 (35 pixels) and "v" 32 x 48 (1536 pixels: every byte level six times per channel).  Stored per shape:
  image_*     float32 [3, 3, H, W]: uint8 frames through ToTensor + Normalize(ImageNet mean / std);
  labels_*    int64 [3, H, W] with 255, -1, 259 and 300 (a value >= every K); image 1 is all 255;
  x_*         uint8 [3, H, W, 3]: the bytes of the x pictures;    y_*: uint8 [3, H, W], the bytes (palette indices) of the y pictures;
  yt_*_K{K}_{i64,u8}  the bytes of the y_tilde pictures for K in {2, 24, 71, 256}, with the label tensor int64 resp. uint8 (a -1 that
              became 255 then propagates); the logits are tests/_preview_ref.fixture_logits(K, (H, W)), of which crc_*_K{K} is the CRC-32;
  *_r256, *_r9x13   x, y and yt_*_K71_i64 through Image.resize(NEAREST) to 256 x 256 (the reference's resize=True) and to 9 rows x 13 columns.
And palette_K{K}: getpalette() of a y_tilde picture; modes: the picture modes ("RGB", "P", "P").

The tool asserts that the "v" image holds, in each channel, a level that the truncation lowers and a level where a fused multiply-add
would give another byte.

usage: python tools/make_golden_preview.py --reference DIR [--out tests/golden]
"""
import argparse
import os
import sys
import zlib

sys.dont_write_bytecode = True
HERE = os.path.dirname(os.path.abspath(__file__))
REPO = os.path.dirname(HERE)

MEAN, STD = (0.485, 0.456, 0.406), (0.229, 0.224, 0.225)
KS = (2, 24, 71, 256)
SHAPES = {"s": (5, 7), "v": (32, 48)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reference", required=True, help="a checkout of the reference project (read only)")
    ap.add_argument("--out", default=os.path.join(REPO, "tests", "golden"))
    a = ap.parse_args()
    sys.path[:0] = [os.path.join(HERE, "_shims"), a.reference, REPO]

    import numpy as np
    import torch
    from PIL import Image

    import utils.tensor_board as TB
    from tests import _preview_ref as R

    denorm = TB.DeNormalize(MEAN, STD)

    def restore(t):
        """restore_transform: DeNormalize (in place, on the caller's copy), then ToPILImage's float path."""
        return Image.fromarray(np.ascontiguousarray(denorm(t).mul(255).byte().permute(1, 2, 0).numpy()))

    def pictures(K, image, gt, logits, resize=None):
        """Per frame the (x, y, y_tilde) pictures the upload hands to wandb.Image (utils/tensor_board.py:94-130), made by the
        reference's functions on CPU tensors: the argmax with the ignore overwrite, colorize_mask over one shared palette list,
        the restored frame through an int array and back to uint8, and the optional NEAREST resize of all three."""
        colours = TB.get_pallete(K)
        index = torch.argmax(logits, dim=1).long()
        index[gt == 255] = 255
        out = []
        for frame, label, guess in zip(image, gt.numpy(), index.numpy()):
            x = Image.fromarray(np.asarray(restore(frame.squeeze()), dtype=int).astype(np.uint8))
            trio = (x, TB.colorize_mask(label, colours), TB.colorize_mask(guess, colours))
            out.append(tuple(p.resize(resize, Image.NEAREST) for p in trio) if resize else trio)
        return out

    def stack(pics, k):
        return np.stack([np.asarray(p[k]) for p in pics]).astype(np.uint8)

    mean_t, std_t = (torch.tensor(v, dtype=torch.float32).view(3, 1, 1) for v in (MEAN, STD))
    out, modes = {}, None
    rs = np.random.RandomState(77)
    for tag, (H, W) in SHAPES.items():
        n = H * W
        if n % 256 == 0:
            frames = np.stack([np.stack([rs.permutation(np.tile(np.arange(256), n // 256)) for _ in range(3)]) for _ in range(3)])
        else:
            frames = rs.randint(0, 256, size=(3, 3, n))
        frames = frames.reshape(3, 3, H, W).astype(np.uint8)
        image = torch.from_numpy(frames).float().div(255).sub_(mean_t).div_(std_t)          # ToTensor + Normalize
        labels = rs.choice(np.array([0, 1, 5, 23, 70, 255]), size=(3, H, (W + 2) // 3))
        labels = np.ascontiguousarray(np.repeat(labels, 3, axis=2)[:, :, :W]).astype(np.int64)
        labels[1] = 255
        labels[0, 0, :4] = [-1, 259, 300, 255]
        labels[2, H - 1, W - 4:] = [255, 300, -1, 259]
        out[f"image_{tag}"], out[f"labels_{tag}"] = image.numpy().copy(), labels
        for K in KS:
            lg = R.fixture_logits(K, (H, W))
            out[f"crc_{tag}_K{K}"] = np.array(zlib.crc32(lg.tobytes()), dtype=np.int64)
            for name, gt in (("i64", torch.from_numpy(labels)), ("u8", torch.from_numpy(labels.astype(np.uint8)))):
                pics = pictures(K, image.clone(), gt.clone(), torch.from_numpy(lg))
                out[f"yt_{tag}_K{K}_{name}"] = stack(pics, 2)
                if name == "i64":
                    x, y = stack(pics, 0), stack(pics, 1)
                    assert np.array_equal(out.setdefault(f"x_{tag}", x), x) and np.array_equal(out.setdefault(f"y_{tag}", y), y)
                    out[f"palette_K{K}"] = np.array(pics[0][2].getpalette(), dtype=np.int64)
                    assert out[f"palette_K{K}"].shape == (768,)
                    modes = [p.mode for p in pics[0]]
            if K == 71:
                for rname, size in (("r256", (256, 256)), ("r9x13", (9, 13))):
                    pics = pictures(K, image.clone(), torch.from_numpy(labels.copy()), torch.from_numpy(lg), resize=size[::-1])
                    assert pics[0][0].size == size[::-1]                                    # PIL sizes are (width, height)
                    out[f"x_{tag}_{rname}"], out[f"y_{tag}_{rname}"] = stack(pics, 0), stack(pics, 1)
                    out[f"yt_{tag}_K71_i64_{rname}"] = stack(pics, 2)
        if tag == "v":
            # what the image must be able to show: per channel a level that comes back one lower, and one where an FMA differs
            x = out["x_v"].astype(np.int64)
            f = frames.transpose(0, 2, 3, 1).astype(np.int64)
            t64 = image.numpy().astype(np.float64)
            s64, m64 = (np.asarray(v, np.float32).astype(np.float64).reshape(1, 3, 1, 1) for v in (STD, MEAN))
            fused = ((t64 * s64 + m64).astype(np.float32) * np.float32(255)).astype(np.int64).transpose(0, 2, 3, 1) & 255
            for c in range(3):
                lowered, differs = int((x[..., c] == f[..., c] - 1).sum()), int((fused[..., c] != x[..., c]).sum())
                assert lowered > 0 and differs > 0, (c, lowered, differs)
                assert ((x[..., c] == f[..., c]) | (x[..., c] == f[..., c] - 1)).all()
                print(f"channel {c}: {lowered} pixels one level lower, {differs} where a fused multiply-add differs")
    out["modes"] = np.array(modes)
    assert modes == ["RGB", "P", "P"], modes
    path = os.path.join(a.out, "preview.npz")
    np.savez_compressed(path, **out)
    print(path, os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()
