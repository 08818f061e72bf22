"""Plumbing of the BatchNorm combine-inside-apply entry points (no GPU): prototypes, header, ABI version."""
import os
import re

from cavp_amd import _lib

HDR = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "cavp_hip.h")).read()
NAMES = ("cavp_bn_tiles_scale_shift_act", "cavp_bn_tiles_bwd_apply")


def _header_args(name):
    m = re.search(r"\bint " + name + r"\(([^;]*?)\);", HDR, re.S)
    assert m, f"{name} is not declared in include/cavp_hip.h"
    return [a.strip() for a in m.group(1).split(",")]


def test_prototypes_present():
    for n in NAMES:
        assert n in _lib.PROTOTYPES, n
        assert _lib.PROTOTYPES[n][0] is _lib.PROTOTYPES["cavp_scale_shift_act"][0]   # int status like every launch


def test_argument_counts_match_header():
    for n in NAMES:
        args = _header_args(n)
        assert len(args) == len(_lib.PROTOTYPES[n][1]), (n, len(args), len(_lib.PROTOTYPES[n][1]))
        assert args[-1] == "void* stream"


def test_argument_kinds_match_header():
    """pointer arguments are void pointers in the prototype, int64_t / float arguments keep their width"""
    vp = _lib.PROTOTYPES["cavp_scale_shift_act"][1][1]
    i64 = _lib.PROTOTYPES["cavp_scale_shift_act"][1][6]
    for n in NAMES:
        for decl, ct in zip(_header_args(n), _lib.PROTOTYPES[n][1]):
            assert ("*" in decl) == (ct is vp), (n, decl)
            assert decl.startswith("int64_t") == (ct is i64), (n, decl)


def test_abi_version_unchanged():
    assert int(re.search(r"#define CAVP_ABI_VERSION (\d+)", HDR).group(1)) == 16


def test_wrappers_keep_their_names():
    """the launch timer of the benchmark wraps these two names: the one-launch route is reached through keyword arguments"""
    import inspect
    from cavp_amd import train_ops as T
    assert "bn_tiles" in inspect.signature(T.scale_shift_act).parameters
    assert "tile_partials" in inspect.signature(T.bn_act_bwd_apply).parameters
    assert inspect.signature(T.scale_shift_act).parameters["bn_tiles"].default is None
    assert inspect.signature(T.bn_act_bwd_apply).parameters["tile_partials"].default is None
