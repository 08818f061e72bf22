"""Host side of the device-resident optimiser schedule: the ctypes mirror of struct cavp_opt_state against the library and the
header, and the new prototypes.  No GPU needed."""
import ctypes
import os
import re

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

C_TYPES = {"int64_t": ctypes.c_int64, "int32_t": ctypes.c_int32, "double": ctypes.c_double, "float": ctypes.c_float}


def test_state_struct_size_matches_library():
    from cavp_amd import _lib, build
    from cavp_amd.optim import OptState
    build.build(verbose=False)
    lib = _lib.load()
    assert lib.cavp_optimizer_state_bytes() == ctypes.sizeof(OptState)
    assert ctypes.sizeof(OptState) % 8 == 0


def test_state_struct_fields_match_header():
    """Same field names, order and C types as the header's struct."""
    from cavp_amd.optim import OptState
    hdr = open(os.path.join(REPO, "include", "cavp_hip.h")).read()
    body = hdr[hdr.index("typedef struct cavp_opt_state {"):hdr.index("} cavp_opt_state;")]
    body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
    fields = re.findall(r"\b(int64_t|int32_t|double|float)\s+([a-z0-9_]+)\s*;", body)
    assert [(n, C_TYPES[t]) for t, n in fields] == [(n, t) for n, t in OptState._fields_]
    for name in ("t", "start_lr", "lr_power", "total_iters", "warmup_steps", "end_lr", "base_lr", "beta1", "beta2", "lr_sgd",
                 "lr_adam", "bc1", "bc2_sqrt", "first_step"):
        assert hasattr(OptState, name), name
    assert OptState.t.offset == 0 and OptState.lr_sgd.offset % 4 == 0


def test_new_prototypes_are_declared():
    from cavp_amd import _lib
    for name in ("cavp_optimizer_state_bytes", "cavp_optimizer_schedule", "cavp_optimizer_step_dev"):
        assert name in _lib.PROTOTYPES, name
    assert len(_lib.PROTOTYPES["cavp_optimizer_schedule"][1]) == 2
    assert len(_lib.PROTOTYPES["cavp_optimizer_step_dev"][1]) == 7
    assert _lib.ABI_VERSION == 16
