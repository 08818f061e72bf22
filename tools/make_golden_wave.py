#!/usr/bin/env python3
"""Generate tests/golden/wave_crop.npz by running the REFERENCE's own crop_audio (read-only import, the recipe of
tools/make_pairs_golden.py: stub packages in tools/_shims, the reference tree on sys.path, stand-in modules for what is not
installed, unbound calls on a SimpleNamespace that carries audio_len).

Authoring-container only; nothing here is imported by the product or the tests.  What runs is `crop_audio` of the three data-set
files - dataset/vpo_mono/multi_source/audio/audio_dataset.py, dataset/avss/audio/audio_dataset.py and dataset/avsbench_ms.py - and,
around it, the statements of their __getitem__ that are no function that could be called: torch.stack(wave_list).sum(0) (VPO),
torch.mean(wave_, dim=0).unsqueeze(0) (AVSS), and mean + view(1, 10, -1)[:, img_id - 1, :] (AVSBench training items).  The inputs
are 16 kHz already, so the stand-in torchaudio is never called (Resample returns its input at equal rates).

The inputs are tests/_wave_ref.py::golden_input (int16 PCM of a short period, v / 32768 exact in float32); only the outputs are
stored, and they compress to a few KB.  sample_len 400 (audio_len 0.025) and 16000 (audio_len 1.0), one clip length per crop
regime (tests/_wave_ref.py::golden_lengths).

usage: python tools/make_golden_wave.py [--out tests/golden]
"""
import argparse
import importlib
import os
import sys
import types

sys.dont_write_bytecode = True
HERE = os.path.dirname(os.path.abspath(__file__))
REPO = os.path.dirname(HERE)
sys.path[:0] = [os.path.join(HERE, "_shims"), "/root/reference", REPO]

import numpy as np  # noqa: E402
import torch  # noqa: E402

from tests import _wave_ref as R  # noqa: E402


class _Anything:
    """Attribute of a stand-in module: callable, subscriptable, and every attribute of it is another one."""

    def __call__(self, *a, **k):
        return self

    def __getattr__(self, name):
        return self


def _stand_in(name):
    m = types.ModuleType(name)
    m.__path__ = []
    m.__getattr__ = lambda attr: _Anything()
    sys.modules[name] = m


def _import(module):
    """Import a module of the reference; whatever it imports that is not installed here becomes an empty stand-in."""
    for _ in range(64):
        try:
            return importlib.import_module(module)
        except ModuleNotFoundError as e:
            if not e.name or e.name == module or module.startswith(e.name + "."):
                raise
            _stand_in(e.name)
    raise RuntimeError(f"{module} of the reference does not import")


def drive():
    vpo = _import("dataset.vpo_mono.multi_source.audio.audio_dataset").AudioDataset
    avss = _import("dataset.avss.audio.audio_dataset").AudioDataset
    avsb = _import("dataset.avsbench_ms").MS3Dataset
    rec = {}
    for sample_len in R.GOLDEN_SAMPLE_LENS:
        self_ = types.SimpleNamespace(audio_len=R.GOLDEN_AUDIO_LEN[sample_len])
        assert int(self_.audio_len * 16000) == sample_len
        for name, (kind, sources, img_id) in R.golden_cases(sample_len).items():
            waves = [torch.from_numpy(R.golden_input(*src).astype(np.float32) / 32768.0) for src in sources]
            if kind == "vpo":
                wave_list = []
                for wave_ in waves:
                    wave_ = vpo.crop_audio(self_, wave_)
                    wave_list.append(wave_)
                out = torch.stack(wave_list).sum(0)
            elif kind == "avss":
                wave_ = avss.crop_audio(self_, waves[0])
                out = torch.mean(wave_, dim=0).unsqueeze(0)
            else:
                audio_wav = avsb.crop_audio(self_, waves[0])
                audio_wav = torch.mean(audio_wav, dim=0).unsqueeze(0)
                audio_wav = audio_wav.view(1, R.GOLDEN_SEGMENTS, -1)
                out = audio_wav[:, img_id - 1, :]
            rec[name] = out.numpy().astype(np.float32)
    return rec


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(REPO, "tests", "golden"))
    a = ap.parse_args()
    rec = drive()
    path = os.path.join(a.out, "wave_crop.npz")
    np.savez_compressed(path, **rec)
    print(f"wrote {path}: {len(rec)} arrays, {os.path.getsize(path)} bytes")


if __name__ == "__main__":
    main()
