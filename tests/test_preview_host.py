"""The preview kernel's own source (csrc/dd_preview.hip with csrc/dd_loss_common.h) compiled as host C++ against tests/preview_host/dd_common.h
and run thread by thread on the CPU, against tests/preview_ref.py: the arithmetic, the output indexing and the argument checks of
dd_loss_previews on a machine without a GPU.  tests/test_gpu_previews.py is the test of the device build; this one needs a host C++
compiler (the clang++ of the ROCm installation, or any on the PATH) and is skipped without one."""
import ctypes as C
import os
import shutil
import subprocess

import numpy as np
import pytest

import preview_ref as PR
from deepdenoiser_amd import _lib as L
from deepdenoiser_amd import metrics as M

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "deepdenoiser_amd", "csrc")
THR = M.preview_thresholds()
SENTINEL = 0xAB


def _compiler():
    rocm = os.environ.get("ROCM_PATH", "/opt/rocm")
    for c in (os.path.join(rocm, "lib", "llvm", "bin", "clang++"), os.path.join(rocm, "llvm", "bin", "clang++"), shutil.which("clang++"), shutil.which("g++")):
        if c and os.path.exists(c):
            return c
    return None


@pytest.fixture(scope="module")
def host(tmp_path_factory):
    cxx = _compiler()
    if cxx is None:
        pytest.skip("no host C++ compiler")
    d = tmp_path_factory.mktemp("preview_host")
    shutil.copy(os.path.join(CSRC, "dd_preview.hip"), d / "dd_preview.cpp")      # (next to the stand-in dd_common.h, not the real one)
    shutil.copy(os.path.join(CSRC, "dd_loss_common.h"), d / "dd_loss_common.h")
    shutil.copy(os.path.join(ROOT, "tests", "preview_host", "dd_common.h"), d / "dd_common.h")
    so = str(d / "libpreview_host.so")
    # -ffp-contract=off: the device build forms these values with contraction off; -Wno-unknown-pragmas: g++ does not know `#pragma clang fp`
    p = subprocess.run([cxx, "-std=c++17", "-O1", "-ffp-contract=off", "-Wno-unknown-pragmas", "-fPIC", "-shared", "-x", "c++", "-I", os.path.join(ROOT, "include"),
                        "-o", so, str(d / "dd_preview.cpp")], capture_output=True, text=True)
    assert p.returncode == 0, p.stderr[-3000:]
    lib = C.CDLL(so)
    vp, i, f = C.c_void_p, C.c_int, C.c_float
    lib.dd_loss_previews.argtypes = [C.POINTER(L.LossDesc), C.POINTER(vp), C.POINTER(i), i, i, i, C.POINTER(i), i, C.POINTER(i), i, i, vp, f, f, vp, vp]
    lib.dd_last_error.restype = C.c_char_p
    return lib


class _Op:
    """host arrays and the descriptor of one case, laid out as tests/test_gpu_previews.py lays them out on the device"""

    def __init__(self, lib, case, sides, kind="SMAPE", pred_ld=3, pred_offset=0):
        self.lib, self.case, self.keep = lib, case, []
        d = self.d = L.LossDesc()
        d.n_features, d.kind, d.epsilon = len(case["nch"]), PR.KINDS[kind], PR.EPSILON
        self.source, self.source_ld = (C.c_void_p * L.MAX_FEATURES)(), (C.c_int * L.MAX_FEATURES)()
        for f, n in enumerate(case["nch"]):
            d.nch[f] = n
            d.pred[f], d.pred_ld[f] = self._array(sides["prediction"][f], max(pred_ld, n), pred_offset), max(pred_ld, n)
            d.target[f], d.target_ld[f] = self._array(sides["target"][f], 3, 0), 3
            self.source[f], self.source_ld[f] = self._array(sides["source"][f], n, 0), n
        d.n_combined = len(case["combined"])
        for k, triple in enumerate(case["combined"]):
            for j in range(3):
                d.comb[k][j] = triple[j]
        img = case.get("image") or {"combined": [], "features": []}
        d.n_image_combined, d.n_image_features = len(img["combined"]), len(img["features"])
        for j, k in enumerate(img["combined"]):
            d.image_combined[j] = k
        for j, f in enumerate(img["features"]):
            d.image_features[j] = f

    def _array(self, a, ld, offset):
        a = np.asarray(a)
        flat = np.full(offset + a.shape[0] * a.shape[1] * a.shape[2] * ld, 7.0, dtype=np.float32)
        flat[offset:].reshape(a.shape[0], a.shape[1], a.shape[2], ld)[..., :a.shape[3]] = a.astype(np.float32)
        self.keep.append(flat)
        return flat.ctypes.data + 4 * offset

    def call(self, out_ptr, slots, mask, images, thr_ptr, exposure=1.0, gain=1.0, source=True):
        c = self.case
        img, sl = (C.c_int * max(len(images), 1))(*images), (C.c_int * max(len(slots), 1))(*slots)
        return self.lib.dd_loss_previews(C.byref(self.d), self.source if source else None, self.source_ld if source else None, c["B"], c["H"], c["W"], img,
                                         len(images), sl, len(slots), mask, thr_ptr, exposure, gain, out_ptr, None)

    def run(self, slots, mask, images, exposure=1.0, gain=1.0, guard=64):
        c = self.case
        shape = (len(slots), len(images) * c["H"], bin(mask).count("1") * c["W"], 3)
        n = int(np.prod(shape))
        buf = np.full(guard + n + guard + 3, SENTINEL, dtype=np.uint8)
        buf = buf[(-buf.ctypes.data) % 4:]      # a 4-byte aligned start: `guard` decides where the mosaics begin, as on the device
        assert self.call(buf.ctypes.data + guard, slots, mask, images, THR.ctypes.data, exposure, gain) == 0, self.lib.dd_last_error()
        assert (buf[:guard] == SENTINEL).all() and (buf[guard + n:] == SENTINEL).all(), "bytes outside the mosaics were written"
        return buf[guard:guard + n].reshape(shape)


def test_dyadic_every_byte(host):
    for B, H, W, images, kind, guard in ((1, 1, 1, [0], "SMAPE", 64), (2, 5, 7, [1, 0], "ABSOLUTE", 61), (2, 16, 20, [0, 1], "SQUARED", 64),
                                         (2, 33, 35, [1, 1, 0], "SMAPE", 63)):
        c = PR.case(PR.SMALL, B, H, W)
        sides = PR.dyadic_sides(c, seed=H * 1000 + W)
        slots = PR.slots_of(c)
        got = _Op(host, c, sides, kind).run(slots, 15, images, gain=0.5, guard=guard)
        assert np.array_equal(got, PR.mosaics(c, sides, slots, 15, images, THR, kind=kind, error_gain=0.5)), (H, W)


def test_layouts_masks_and_kinds(host):
    c = PR.case(PR.TWO_TRIPLES, 3, 6, 9)
    sides = PR.dyadic_sides(c, seed=7)
    slots = [PR.IMAGE_SLOT, 3, PR.MAX_FEATURES + 1, 0, PR.MAX_FEATURES, 3]
    want = PR.mosaics(c, sides, slots, 15, [2, 0, 2], THR, kind="SMOOTH_ABSOLUTE", exposure=0.75)
    for kw in ({}, {"pred_ld": 4}, {"pred_offset": 1}, {"pred_ld": 4, "pred_offset": 1}):
        assert np.array_equal(_Op(host, c, sides, "SMOOTH_ABSOLUTE", **kw).run(slots, 15, [2, 0, 2], exposure=0.75, guard=62), want), kw
    c = PR.case(PR.SMALL, 2, 5, 7)
    sides = PR.dyadic_sides(c, seed=3)
    slots = PR.slots_of(c)
    for mask in range(1, 16):
        got = _Op(host, c, sides, "SMAPE").run(slots, mask, [0, 1], gain=2.0, guard=64 + mask)
        assert np.array_equal(got, PR.mosaics(c, sides, slots, mask, [0, 1], THR, kind="SMAPE", error_gain=2.0)), mask
    for kind in PR.KINDS:
        got = _Op(host, c, sides, kind).run(slots, 15, [1], gain=0.25)
        assert np.array_equal(got, PR.mosaics(c, sides, slots, 15, [1], THR, kind=kind, error_gain=0.25)), kind


def test_continuous_and_specials(host):
    c = PR.case(PR.SMALL, 2, 16, 20)
    sides = PR.radiance_sides(c, 1)
    slots = PR.slots_of(c)
    values = np.stack([PR.mosaic_values(c, sides, s, 7, [0, 1], exposure=1.7) for s in slots])
    want, near = np.stack([PR.quantise(v, THR) for v in values]), PR.near_threshold(values, THR, 1e-5)
    got = _Op(host, c, sides).run(slots, 7, [0, 1], exposure=1.7, guard=61)
    feature = np.array([s < PR.MAX_FEATURES for s in slots])
    assert np.array_equal(got[feature], want[feature])
    diff = got[~feature].astype(np.int64) - want[~feature].astype(np.int64)
    assert np.abs(diff).max() <= 1 and not (diff != 0)[~near[~feature]].any()
    c = PR.case(PR.SMALL, 1, 2, 5)
    sides = PR.dyadic_sides(c, seed=5)
    for side in PR.PANELS[:3]:
        sides[side][0][0, 0, 0] = [np.nan, 0.5, 0.5]
        sides[side][0][0, 0, 1] = [np.inf, -np.inf, 0.25]
        sides[side][0][0, 0, 2] = [-3.0, 17.0, 1.0]
        sides[side][4][0, 1, 0] = [np.nan]
    sides["target"][0][0, 0, 1] = [np.inf, np.inf, 0.25]
    got = _Op(host, c, sides, "ABSOLUTE").run(PR.slots_of(c), 15, [0], guard=61)
    assert np.array_equal(got, PR.mosaics(c, sides, PR.slots_of(c), 15, [0], THR, kind="ABSOLUTE"))
    assert got[0][0, :3].tolist() == [[255, 0, 255], [255, 0, int(np.searchsorted(THR, 0.25, side="right"))], [0, 255, 255]]
    assert got[0][0, 15 + 1].tolist() == [255, 0, 255] and got[6][1, 0].tolist() == [255, 0, 255]
    # every threshold and its fp32 neighbours, through a feature slot (255 x 3 values as one row of 255 pixels)
    c = PR.case({"nch": [3], "combined": [], "image": None}, 1, 1, 255)
    edge = np.stack([np.nextafter(THR, np.float32(-1)), THR, np.nextafter(THR, np.float32(2))], axis=1).astype(np.float64)
    sides = {side: [edge.reshape(1, 1, 255, 3)] for side in PR.PANELS[:3]}
    got = _Op(host, c, sides).run([0], 7, [0])
    assert np.array_equal(got, PR.mosaics(c, sides, [0], 7, [0], THR))
    assert got[0][0, :255].tolist() == [[k, k + 1, k + 1] for k in range(255)]


def test_refused_arguments(host):
    c = PR.case(PR.SMALL, 2, 4, 4)
    op = _Op(host, c, PR.dyadic_sides(c, seed=1))
    out = np.full(4096, SENTINEL, dtype=np.uint8)
    t, o = THR.ctypes.data, out.ctypes.data
    for call, word in ((lambda: op.call(o, [5], 7, [0], t), b"does not have"), (lambda: op.call(o, [PR.MAX_FEATURES + 1], 7, [0], t), b"does not have"),
                       (lambda: op.call(o, [0], 7, [], t), b"n_images"), (lambda: op.call(o, [0], 7, [0] * 17, t), b"n_images"),
                       (lambda: op.call(o, [0], 7, [2], t), b"batch index"), (lambda: op.call(o, [], 7, [0], t), b"n_slots"),
                       (lambda: op.call(o, [0] * 42, 7, [0], t), b"n_slots"), (lambda: op.call(o, [0], 0, [0], t), b"panels"),
                       (lambda: op.call(o, [0], 16, [0], t), b"panels"), (lambda: op.call(o, [0], 3, [0], t, source=False), b"source"),
                       (lambda: op.call(o, [0], 7, [0], None), b"table"), (lambda: op.call(None, [0], 7, [0], t), b"null")):
        assert call() < 0 and word in host.dd_last_error(), host.dd_last_error()
    assert (out == SENTINEL).all()
    assert op.call(o, [0], 6, [0], t, source=False) == 0
