"""The device PMI publish without a GPU: the new entry points are declared in include/uavtrack.h and bound in
uavtrack/_lib.py with matching argument counts, struct uavtrack_pmi_tensors mirrors the header, publish_pmi's argument
validation raises ValueError before any library handle is touched, and the exponent-field floor the block scales use equals
floor(log2(.)) wherever a correctly rounded log2 is unambiguous.

(The register budget of pmi_score_t3_kernel<128> after the scalars moved to memory -- 246 vector + 228 accumulation
registers, no scratch -- is recorded in DESIGN.md 4.11 from `hipcc -S`; compiling pmi_kernel.hip takes minutes, too long for
this suite.)"""
import ctypes as C
import math
import os
import re

import numpy as np
import pytest
import torch

from uavtrack import _lib
from uavtrack.env import BatchedUavEnv
from uavtrack.pmi import make_pmi_net

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ("uavtrack_publish_pmi_weights", "uavtrack_pmi_trainer_publish", "uavtrack_get_pmi_blob", "uavtrack_pmi_blob_floats",
       "uavtrack_pmi_publish_info")


def _header():
    return open(os.path.join(ROOT, "include", "uavtrack.h")).read()


@pytest.mark.parametrize("name", NEW)
def test_declared_and_bound_with_matching_argument_counts(name):
    m = re.search(r"\bint\s+" + name + r"\s*\(([^;]*)\)\s*;", _header())
    assert m, f"{name} is not declared in include/uavtrack.h"
    n_args = len([a for a in m.group(1).split(",") if a.strip()])
    assert name in _lib.SIGNATURES, f"{name} is not bound in uavtrack/_lib.py"
    res, args = _lib.SIGNATURES[name]
    assert res is C.c_int and len(args) == n_args, (name, n_args, len(args))


def test_tensor_struct_mirrors_the_header():
    m = re.search(r"typedef struct uavtrack_pmi_tensors \{(.*?)\} uavtrack_pmi_tensors;", _header(), re.S)
    assert m
    body = m.group(1)
    per_block = re.search(r"const float ([^;]*);\s*\} block\[4\];", body, re.S).group(1).count("*")
    tail = re.search(r"block\[4\];\s*const float ([^;]*);", body, re.S).group(1).count("*")
    assert 4 * per_block + tail == 26 == len(_lib.PMI_STATE_KEYS)
    assert C.sizeof(_lib.PmiTensors) == 26 * C.sizeof(C.c_void_p)
    # the order is the reference state_dict's float entries
    floats = [k for k, v in make_pmi_net(8).state_dict().items() if v.dtype == torch.float32]
    assert tuple(floats) == _lib.PMI_STATE_KEYS


def test_publish_validation_raises_before_any_handle():
    sd = {k: v for k, v in make_pmi_net(16).state_dict().items()}
    check = BatchedUavEnv._pmi_publish_tensors
    with pytest.raises(ValueError, match="cuda:0"):
        check(sd, 0)                                           # CPU tensors
    with pytest.raises(ValueError, match="lacks"):
        check({k: v for k, v in sd.items() if k != "fc2.bias"}, 0)
    with pytest.raises(ValueError, match="float32"):
        check({k: v.double() if v.is_floating_point() else v for k, v in sd.items()}, 0)
    with pytest.raises(ValueError, match="float32"):
        check({k: np.zeros(3, np.float32) for k in _lib.PMI_STATE_KEYS}, 0)


def _scale_exponent(bound, target):
    """csrc/pmi_pack.h, pmi_scale_for: the floor from the quotient's exponent field."""
    if not bound > 0.0:
        return 15
    r = target / bound
    if not r > 0.0:
        return -6
    if math.isinf(r):
        return 15
    e = math.frexp(r)[1] - 1
    return max(-6, min(15, e))


def test_exponent_floor_equals_log2_floor_away_from_powers_of_two():
    rng = np.random.RandomState(0)
    for target in (512.0, 32000.0):
        for bound in np.exp(rng.uniform(-40, 40, 2000)):
            r = target / bound
            if abs(r / 2.0 ** round(math.log2(r)) - 1.0) < 1e-12:
                continue
            assert _scale_exponent(bound, target) == max(-6, min(15, math.floor(math.log2(r))))
    assert _scale_exponent(0.0, 512.0) == 15 and _scale_exponent(float("nan"), 512.0) == 15
    assert _scale_exponent(float("inf"), 512.0) == -6
    assert _scale_exponent(512.0, 512.0) == 0 and _scale_exponent(np.nextafter(512.0, 1e9), 512.0) == -1
