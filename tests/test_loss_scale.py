"""Dynamic loss scaling, everything that needs no GPU: the C-ABI of the new entries (header, ctypes mirror and library agree), the update rule
restated in Python -- `scaler_update_ref`, the reference tests/test_gpu_loss_scale.py holds the device to -- against hand-computed
sequences, and the public switches (Architecture(loss_scale=...), train.py --loss_scale)."""
import ctypes
import os
import re
import subprocess

import numpy as np
import pytest

from deepdenoiser_amd import _lib
from deepdenoiser_amd import loss_scale as LS

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW_ENTRIES = ("dd_grads_nonfinite", "dd_adam_step_scaled", "dd_scaler_update", "dd_loss_head_dscale", "dd_loss_msssim_bwd_dscale")
FIELDS = ("scale", "good_steps", "found_nonfinite", "adam_t", "skipped_total")


def scaler_update_ref(state, growth=2.0, backoff=0.5, growth_interval=2000, min_scale=1.0, max_scale=float(2 ** 24)):
    """dd_scaler_update (include/dd_hip.h) restated: state is a dict of FIELDS with found_nonfinite already set or clear; returns the new
    dict.  The scale is float32 arithmetic as on the device."""
    f32 = np.float32
    st = dict(state)
    if st["found_nonfinite"]:
        st["scale"] = float(max(f32(st["scale"]) * f32(backoff), f32(min_scale)))
        st["good_steps"] = 0
        st["skipped_total"] += 1
    else:
        st["adam_t"] += 1
        st["good_steps"] += 1
        if st["good_steps"] == growth_interval:
            st["scale"] = float(min(f32(st["scale"]) * f32(growth), f32(max_scale)))
            st["good_steps"] = 0
    st["found_nonfinite"] = 0
    return st


def run_ref(scale, overflows, **settings):
    """The states after each step of a scripted overflow pattern (True: the step's gradients held an inf / NaN)."""
    st = {"scale": float(scale), "good_steps": 0, "found_nonfinite": 0, "adam_t": 0, "skipped_total": 0}
    out = []
    for o in overflows:
        st = scaler_update_ref(dict(st, found_nonfinite=int(o)), **settings)
        out.append(st)
    return out


# ---------------------------------------------------------------------------------------------------------------- C-ABI
def _declared():
    text = open(os.path.join(ROOT, "include", "dd_hip.h")).read()
    text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    return set(re.findall(r"\b(dd_[a-z0-9_]+)\s*\(", text))


def test_new_entries_in_header_mirror_and_library(lib):
    declared = _declared()
    for name in NEW_ENTRIES:
        assert name in declared, name + " is not declared in include/dd_hip.h"
        assert name in _lib.SYMBOLS, name + " is not in _lib.SYMBOLS"
        assert hasattr(lib, name), name + " is not exported by libdd_hip.so"
        assert getattr(lib, name).argtypes, name + " has no argtypes"
    exported = subprocess.check_output(["nm", "-D", "--defined-only", _lib.LIB_PATH], text=True)
    for name in NEW_ENTRIES:
        assert re.search(r"\bT %s$" % name, exported, flags=re.M), name


def test_scaler_state_size_and_layout_match_the_header(tmp_path):
    src = r'''
#include <stdio.h>
#include <stddef.h>
#include "dd_hip.h"
int main(void){ printf("%zu %zu %zu %zu %zu %zu\n", sizeof(dd_scaler_state), offsetof(dd_scaler_state, scale), offsetof(dd_scaler_state, good_steps),
  offsetof(dd_scaler_state, found_nonfinite), offsetof(dd_scaler_state, adam_t), offsetof(dd_scaler_state, skipped_total)); return 0; }
'''
    c, exe = str(tmp_path / "t.c"), str(tmp_path / "t")
    open(c, "w").write(src)
    subprocess.check_call(["gcc", "-I", os.path.join(ROOT, "include"), c, "-o", exe])
    got = [int(x) for x in subprocess.check_output([exe]).split()]
    S = _lib.ScalerState
    assert tuple(n for n, _ in S._fields_) == FIELDS == LS.FIELDS
    assert got == [ctypes.sizeof(S)] + [getattr(S, n).offset for n in FIELDS] == [20, 0, 4, 8, 12, 16]


def test_invalid_arguments_are_refused_without_a_launch(lib):
    assert lib.dd_grads_nonfinite(None, 4, None, None) == -1
    assert lib.dd_grads_nonfinite(ctypes.c_void_p(4), 4, ctypes.c_void_p(64), None) == -1 and b"aligned" in lib.dd_last_error()
    assert lib.dd_adam_step_scaled(None, None, None, None, 0, 1e-3, 0.9, 0.999, 1e-8, 1.0, None, None) == -1
    assert lib.dd_scaler_update(None, 2.0, 0.5, 2000, 1.0, 2.0 ** 24, None) == -1
    st = ctypes.c_void_p(64)      # never dereferenced: validation fails first
    assert lib.dd_scaler_update(st, 2.0, 0.5, 0, 1.0, 2.0 ** 24, None) == -1
    assert lib.dd_scaler_update(st, 0.5, 0.5, 3, 1.0, 2.0 ** 24, None) == -1
    assert lib.dd_scaler_update(st, 2.0, 0.5, 3, 4.0, 2.0, None) == -1
    assert lib.dd_loss_head_dscale(None, 1, 8, 8, None, None, None) == -1
    assert lib.dd_loss_msssim_bwd_dscale(None, 1, 48, 48, None, None, None) == -1


def test_new_kernels_are_on_the_no_scratch_list():
    from deepdenoiser_amd import build
    assert "dd_loss_scale.hip" in build.SOURCES
    assert set(build.NO_SCRATCH["dd_loss_scale.hip"]) == {"grads_nonfinite_kernel", "adam_scaled_kernel", "scaler_update_kernel"}


# ---------------------------------------------------------------------------------------------------------------- the update rule
def test_overflow_at_step_1():
    (st,) = run_ref(65536.0, [True])
    assert st == {"scale": 32768.0, "good_steps": 0, "found_nonfinite": 0, "adam_t": 0, "skipped_total": 1}


def test_growth_exactly_at_the_interval():
    a, b, c, d = run_ref(1024.0, [False] * 4, growth_interval=3)
    assert (a["scale"], a["good_steps"], a["adam_t"]) == (1024.0, 1, 1)
    assert (b["scale"], b["good_steps"], b["adam_t"]) == (1024.0, 2, 2)
    assert (c["scale"], c["good_steps"], c["adam_t"]) == (2048.0, 0, 3)
    assert (d["scale"], d["good_steps"], d["adam_t"]) == (2048.0, 1, 4)
    # an overflow restarts the count: two good steps, a skip, then three more are needed
    seq = run_ref(1024.0, [False, False, True, False, False, False], growth_interval=3)
    assert [s["scale"] for s in seq] == [1024.0, 1024.0, 512.0, 512.0, 512.0, 1024.0]
    assert [s["good_steps"] for s in seq] == [1, 2, 0, 1, 2, 0]
    assert [s["adam_t"] for s in seq] == [1, 2, 2, 3, 4, 5] and seq[-1]["skipped_total"] == 1


def test_clamps_at_min_and_max():
    seq = run_ref(3.0, [True, True, True], min_scale=1.0)
    assert [s["scale"] for s in seq] == [1.5, 1.0, 1.0] and seq[-1]["skipped_total"] == 3
    seq = run_ref(float(2 ** 23) * 1.5, [False, False], growth_interval=1)
    assert [s["scale"] for s in seq] == [float(2 ** 24)] * 2
    # the INITIAL scale is not clamped: the clamps apply when the scale changes
    assert run_ref(2.0 ** 40, [True])[0]["scale"] == 2.0 ** 39
    assert run_ref(2.0 ** 40, [False], growth_interval=1)[0]["scale"] == 2.0 ** 24


# ---------------------------------------------------------------------------------------------------------------- public switches
def test_train_parser_accepts_dynamic_and_numbers():
    from deepdenoiser_amd import train
    p = train.parser()
    assert p.parse_args(["t.json"]).loss_scale is None
    assert p.parse_args(["t.json", "--loss_scale", "dynamic"]).loss_scale == "dynamic"
    assert p.parse_args(["t.json", "--loss_scale", "1024"]).loss_scale == 1024.0
    for bad in ("0", "-4", "nan", "inf", "sometimes"):
        with pytest.raises(SystemExit):
            p.parse_args(["t.json", "--loss_scale", bad])


def test_architecture_accepts_the_dynamic_setting():
    from deepdenoiser_amd import configs
    from deepdenoiser_amd.architecture import Architecture
    aj = configs.cfg1_small_unet()
    for dtype, init in (("f16", 65536.0), ("bf16", 1.0), ("f32", 1.0)):
        arch = Architecture(aj, device="cpu", dtype=dtype, loss_scale="dynamic")
        assert arch.loss_scale == "dynamic" and arch.loss_scaler is None
        assert LS.parse(arch.loss_scale, dtype) == {"init": init, "growth": 2.0, "backoff": 0.5, "growth_interval": 2000, "min_scale": 1.0,
                                                    "max_scale": float(2 ** 24)}
    arch = Architecture(aj, device="cpu", dtype="f16", loss_scale={"init": 2.0 ** 40, "growth_interval": 7})
    cfg = LS.parse(arch.loss_scale, "f16")
    assert cfg["init"] == 2.0 ** 40 and cfg["growth_interval"] == 7 and cfg["backoff"] == 0.5
    for bad in ("static", {"initial": 4.0}, {"init": 0.0}, {"backoff": 2.0}, {"growth_interval": 0}, {"min_scale": 8.0, "max_scale": 4.0}, True):
        with pytest.raises(ValueError):
            Architecture(aj, device="cpu", dtype="f16", loss_scale=bad)


def test_static_settings_build_the_attributes_they_always_did():
    from deepdenoiser_amd import configs
    from deepdenoiser_amd.architecture import Architecture
    aj = configs.cfg1_small_unet()
    assert Architecture(aj, device="cpu", dtype="f16").loss_scale is None
    assert Architecture(aj, device="cpu", dtype="f16", loss_scale=None).loss_scale is None
    assert Architecture(aj, device="cpu", dtype="f16", loss_scale=1024).loss_scale == 1024
    assert Architecture(aj, device="cpu", dtype="bf16", loss_scale=0.5).loss_scale == 0.5
    for setting in (None, 1024, 4096.0):
        assert LS.parse(setting, "f16") is None and not LS.is_dynamic(setting)
