"""-m gpu: image summaries on the device -- dd_loss_previews (csrc/dd_preview.hip) against tests/preview_ref.py, Program.previews() against
the same reference on the program's own tensors, and the training command line's event files.

Gates.  Dyadic inputs (every value k / 16, |k| <= 32): every derived value is exact in fp32, so every byte equals the reference's.
Continuous non-negative radiances: a feature slot's only arithmetic is the fp32 exposure multiply, which the reference repeats, so it is
exact; a combined or image slot is formed in fp32 where the reference has float64, so a byte may differ by 1 -- only where the float64 value
lies within a relative 1e-5 of a threshold (a product and a sum of up to 7 non-negative terms: under 10 roundings of 2^-24 each, 6e-7,
with a margin), and the test first checks on the reference alone that at most 1 % of the values are that close."""
import ctypes as C
import json
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import preview_ref as PR
import test_gpu_metrics as TM
from deepdenoiser_amd import _lib as L
from deepdenoiser_amd import configs, summaries
from deepdenoiser_amd import metrics as M
from deepdenoiser_amd.naming import Naming

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
THR = M.preview_thresholds()
SENTINEL = 0xAB
BAND = 1e-5


def _stream():
    return torch.cuda.current_stream().cuda_stream


@pytest.fixture(scope="module")
def thr_dev():
    TM._need_gpu()
    return torch.from_numpy(THR).cuda()


class _Op:
    """Device tensors and the descriptor of one case.  Predictions live in pixels of `pred_ld` floats, `pred_offset` floats into their
    allocation; targets in pixels of 3 floats (a 1-channel pass in channel 0, as Program keeps them); raw sources densely.  Every float
    that must not be read is 7.0."""

    def __init__(self, case, sides, kind="SMAPE", pred_ld=3, pred_offset=0):
        self.case, self.keep = case, []
        d = self.d = L.LossDesc()
        d.n_features, d.kind, d.epsilon = len(case["nch"]), PR.KINDS[kind], PR.EPSILON
        self.source, self.source_ld = (C.c_void_p * L.MAX_FEATURES)(), (C.c_int * L.MAX_FEATURES)()
        for f, n in enumerate(case["nch"]):
            d.nch[f] = n
            d.pred[f], d.pred_ld[f] = self._dev(sides["prediction"][f], max(pred_ld, n), pred_offset), max(pred_ld, n)
            d.target[f], d.target_ld[f] = self._dev(sides["target"][f], 3, 0), 3
            self.source[f], self.source_ld[f] = self._dev(sides["source"][f], n, 0), n
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

    def _dev(self, a, ld, offset):
        a = np.asarray(a)
        flat = torch.full((offset + a.shape[0] * a.shape[1] * a.shape[2] * ld,), 7.0, dtype=torch.float32)
        flat[offset:].view(a.shape[0], a.shape[1], a.shape[2], ld)[..., :a.shape[3]] = torch.from_numpy(a.astype(np.float32))
        flat = flat.cuda()
        self.keep.append(flat)
        return flat.data_ptr() + 4 * offset

    def call(self, out_ptr, slots, mask, images, thr_ptr, exposure=1.0, gain=1.0, source=True):
        c = self.case
        img, sl = (C.c_int * max(len(images), 1))(*images), (C.c_int * max(len(slots), 1))(*slots)
        return L.load().dd_loss_previews(C.byref(self.d), self.source if source else None, self.source_ld if source else None, c["B"], c["H"], c["W"], img,
                                         len(images), sl, len(slots), mask, thr_ptr, exposure, gain, out_ptr, _stream())

    def run(self, slots, mask, images, thr_dev, exposure=1.0, gain=1.0, guard=64):
        """the mosaics [slots, images * H, P * W, 3] as a host array; the `guard` bytes on either side of them must stay untouched"""
        c = self.case
        shape = (len(slots), len(images) * c["H"], bin(mask).count("1") * c["W"], 3)
        n = int(np.prod(shape))
        buf = torch.full((guard + n + guard,), SENTINEL, dtype=torch.uint8, device="cuda")
        L.check(self.call(buf.data_ptr() + guard, slots, mask, images, thr_dev.data_ptr(), exposure, gain))
        torch.cuda.synchronize()
        host = buf.cpu().numpy()
        assert (host[:guard] == SENTINEL).all() and (host[guard + n:] == SENTINEL).all(), "bytes outside the mosaics were written"
        return host[guard:guard + n].reshape(shape)


def _exact(name, got, want):
    bad = int((got != want).sum())
    print("%-40s %d bytes, %d differ" % (name, want.size, bad))
    assert got.shape == want.shape and bad == 0, (name, bad, np.argwhere(got != want)[:5].tolist())


# ---------------------------------------------------------------------------------------------------------------- dyadic: every byte
# (B, H, W, images, kind, guard): 1 x 1; rows of 21 bytes per panel; a multiple of the 4-pixel group; odd and more than one workgroup; 16 images
# of 128 x 128.  An odd guard puts `out` itself off a 4-byte boundary.
DYADIC = [(1, 1, 1, [0], "SMAPE", 64), (2, 5, 7, [1, 0], "ABSOLUTE", 61), (2, 16, 20, [0, 1], "SQUARED", 64), (2, 33, 35, [1, 1, 0], "SMAPE", 63),
          (16, 128, 128, list(range(15, -1, -1)), "SMAPE", 64)]


@pytest.mark.parametrize("B,H,W,images,kind,guard", DYADIC, ids=["%dx%d" % (c[1], c[2]) for c in DYADIC])
def test_dyadic_every_byte(B, H, W, images, kind, guard, thr_dev):
    """all four panels, all three kinds of slot (5 features with a 1-channel pass, a combined feature, the image)"""
    c = PR.case(PR.SMALL, B, H, W)
    sides = PR.dyadic_sides(c, seed=H * 1000 + W)
    slots = PR.slots_of(c)
    op = _Op(c, sides, kind)
    got = op.run(slots, 15, images, thr_dev, gain=0.5, guard=guard)
    want = PR.mosaics(c, sides, slots, 15, images, THR, kind=kind, error_gain=0.5)
    _exact("dyadic %dx%d %s" % (H, W, kind), got, want)
    assert len(np.unique(want)) > (2 if H * W == 1 else 100)      # (not a degenerate picture: values above 1 and below 0 clamp, the rest spread)
    if H == 33:
        assert np.array_equal(got, op.run(slots, 15, images, thr_dev, gain=0.5, guard=guard)), "two runs differ"


def test_dyadic_layouts(thr_dev):
    """B = 3 with images [2, 0, 2]; predictions in pixels of 4 floats; prediction pointers 4 bytes into their allocation; a 1-channel pass as
    the colour of a triple; slots in any order, repeated"""
    c = PR.case(PR.TWO_TRIPLES, 3, 6, 9)
    sides = PR.dyadic_sides(c, seed=7)
    slots = [PR.IMAGE_SLOT, 3, PR.MAX_FEATURES + 1, 0, PR.MAX_FEATURES, 3]
    want = PR.mosaics(c, sides, slots, 15, [2, 0, 2], THR, kind="SMOOTH_ABSOLUTE", exposure=0.75)
    assert np.array_equal(want[1], want[5]) and np.array_equal(want[:, :6], want[:, 12:]) and (want[1][..., 0] == want[1][..., 2]).all()
    for name, kw in (("plain", {}), ("pred_ld 4", {"pred_ld": 4}), ("pred offset by 4 bytes", {"pred_offset": 1}),
                     ("pred_ld 4, offset", {"pred_ld": 4, "pred_offset": 1})):
        got = _Op(c, sides, "SMOOTH_ABSOLUTE", **kw).run(slots, 15, [2, 0, 2], thr_dev, exposure=0.75, guard=62)
        _exact(name, got, want)


def test_dyadic_every_panel_mask_and_loss_kind(thr_dev):
    c = PR.case(PR.SMALL, 2, 5, 7)
    sides = PR.dyadic_sides(c, seed=3)
    slots = PR.slots_of(c)
    op = _Op(c, sides, "SMAPE")
    for mask in range(1, 16):
        want = PR.mosaics(c, sides, slots, mask, [0, 1], THR, kind="SMAPE", error_gain=2.0)
        assert want.shape[2] == bin(mask).count("1") * 7
        _exact("panel mask %d" % mask, op.run(slots, mask, [0, 1], thr_dev, gain=2.0, guard=64 + mask), want)
    seen = []
    for kind in PR.KINDS:
        for mask in (8, 15):
            want = PR.mosaics(c, sides, slots, mask, [1], THR, kind=kind, error_gain=0.25)
            _exact("%s, mask %d" % (kind, mask), _Op(c, sides, kind).run(slots, mask, [1], thr_dev, gain=0.25), want)
        seen.append(want[:, :, -7:])
    assert all(not np.array_equal(seen[0], s) for s in seen[1:]), "the loss kinds must give different difference panels"


# ---------------------------------------------------------------------------------------------------------------- continuous
@pytest.mark.parametrize("H,W,seed,exposure", [(16, 20, 1, 1.0), (33, 35, 2, 1.7)])
def test_continuous_radiances(H, W, seed, exposure, thr_dev):
    c = PR.case(PR.SMALL, 2, H, W)
    sides = PR.radiance_sides(c, seed)
    slots = PR.slots_of(c)
    values = np.stack([PR.mosaic_values(c, sides, s, 7, [0, 1], exposure=exposure) for s in slots])
    want = np.stack([PR.quantise(v, THR) for v in values])
    near = PR.near_threshold(values, THR, BAND)
    print("%dx%d: %.3f %% of the reference's values lie within a relative %g of a threshold" % (H, W, 100.0 * near.mean(), BAND))
    assert near.mean() <= 0.005
    got = _Op(c, sides).run(slots, 7, [0, 1], thr_dev, exposure=exposure, guard=61)
    feature = np.array([s < PR.MAX_FEATURES for s in slots])
    _exact("feature slots", got[feature], want[feature])
    diff = got[~feature].astype(np.int64) - want[~feature].astype(np.int64)
    print("combined and image slots: %d of %d bytes differ, all by at most %d" % ((diff != 0).sum(), diff.size, np.abs(diff).max()))
    assert np.abs(diff).max() <= 1 and not (diff != 0)[~near[~feature]].any()


# ---------------------------------------------------------------------------------------------------------------- specials
def test_specials(thr_dev):
    """NaN -> the whole pixel magenta, +inf -> 255, -inf -> 0, values below 0 and above 1 clamp, through a feature, a combined product and the
    image sum; every threshold and its fp32 neighbours land on the right side"""
    c = PR.case(PR.SMALL, 1, 4, 9)
    sides = PR.dyadic_sides(c, seed=5)
    nan, inf = np.nan, np.inf
    for side in ("source", "prediction", "target"):
        f0 = sides[side][0]
        f0[0, 0, 0] = [nan, 0.5, 0.5]
        f0[0, 0, 1] = [0.5, 0.5, nan]
        f0[0, 0, 2] = [inf, -inf, 0.25]
        f0[0, 0, 3] = [-3.0, 17.0, 1.0]
        f0[0, 0, 4] = [0.0, -0.0, -1.0 / 16]
        sides[side][4][0, 1, 0] = [nan]
        sides[side][4][0, 1, 1] = [inf]
        sides[side][3][0, 2, 0] = [inf, 1.0, 1.0]      # the image: inf + finite
        sides[side][1][0, 3, 0] = [inf, 0.0, 0.0]      # the triple: colour x (inf + finite)
    sides["target"][0][0, 0, 2] = [inf, inf, 0.25]     # difference: inf - inf = NaN in channel 0
    slots = PR.slots_of(c)
    got = _Op(c, sides, "ABSOLUTE").run(slots, 15, [0], thr_dev, guard=61)
    _exact("specials", got, PR.mosaics(c, sides, slots, 15, [0], THR, kind="ABSOLUTE"))
    for p in range(3):      # slot 0 = feature 0, panel p
        row = got[0][0, p * 9:p * 9 + 5].tolist()
        assert row[0] == [255, 0, 255] and row[1] == [255, 0, 255]
        assert row[2] == [255, 0 if p < 2 else 255, int(np.searchsorted(THR, 0.25, side="right"))]
        assert row[3] == [0, 255, 255] and row[4] == [0, 0, 0]
    assert got[0][0, 27 + 2].tolist() == [255, 0, 255]                       # |inf - inf| is NaN: magenta in the gray panel too
    assert got[4][1, 0].tolist() == [255, 0, 255] and got[4][1, 1].tolist() == [255, 255, 255]
    assert got[6][1, 0].tolist() == [255, 0, 255] and got[6][2, 0, 0] == 255
    # every threshold and its fp32 neighbours, through a feature slot (a row of 255 pixels), and the smallest normal and denormal values
    c = PR.case({"nch": [3, 3], "combined": [], "image": None}, 1, 1, 255)
    edge = np.stack([np.nextafter(THR, np.float32(-1)), THR, np.nextafter(THR, np.float32(2))], axis=1).astype(np.float64).reshape(1, 1, 255, 3)
    tiny = np.zeros((1, 1, 255, 3))
    tiny[0, 0, 0] = [float(np.float32(1e-30)), float(np.float32(1e-45)), -float(np.float32(1e-45))]
    sides = {side: [edge, tiny] for side in PR.PANELS[:3]}
    got = _Op(c, sides).run([0, 1], 7, [0], thr_dev)
    _exact("thresholds", got, PR.mosaics(c, sides, [0, 1], 7, [0], THR))
    assert got[0][0, :255].tolist() == [[k, k + 1, k + 1] for k in range(255)] and not got[1].any()


# ---------------------------------------------------------------------------------------------------------------- bad arguments
def test_bad_arguments_return_a_status(thr_dev):
    c = PR.case(PR.SMALL, 2, 4, 4)
    op = _Op(c, PR.dyadic_sides(c, seed=1))
    lib = L.load()
    out = torch.full((4096,), SENTINEL, dtype=torch.uint8, device="cuda")
    t, o = thr_dev.data_ptr(), out.data_ptr()
    no_image = _Op(PR.case({"nch": [3, 3, 3], "combined": [(0, 1, 2)], "image": None}, 2, 4, 4),
                   PR.dyadic_sides(PR.case({"nch": [3, 3, 3], "combined": [(0, 1, 2)], "image": None}, 2, 4, 4), seed=1))
    cases = [
        ("a feature the descriptor does not have", lambda: op.call(o, [5], 7, [0], t), b"does not have"),
        ("a combined feature it does not have", lambda: op.call(o, [PR.MAX_FEATURES + 1], 7, [0], t), b"does not have"),
        ("the image of a descriptor without one", lambda: no_image.call(o, [PR.IMAGE_SLOT], 7, [0], t), b"does not have"),
        ("a negative slot", lambda: op.call(o, [-1], 7, [0], t), b"does not have"),
        ("no images", lambda: op.call(o, [0], 7, [], t), b"n_images"),
        ("17 images", lambda: op.call(o, [0], 7, [0] * 17, t), b"n_images"),
        ("an image index past the batch", lambda: op.call(o, [0], 7, [2], t), b"batch index"),
        ("no slots", lambda: op.call(o, [], 7, [0], t), b"n_slots"),
        ("42 slots", lambda: op.call(o, [0] * 42, 7, [0], t), b"n_slots"),
        ("no panels", lambda: op.call(o, [0], 0, [0], t), b"panels"),
        ("panel bits past the fourth", lambda: op.call(o, [0], 16, [0], t), b"panels"),
        ("a null source with the source bit", lambda: op.call(o, [0], 3, [0], t, source=False), b"source"),
        ("no table", lambda: op.call(o, [0], 7, [0], None), b"table"),
        ("no output", lambda: op.call(None, [0], 7, [0], t), b"null"),
    ]
    for name, call, word in cases:
        rc = call()
        assert rc < 0, name
        assert word in lib.dd_last_error(), (name, lib.dd_last_error())
    assert lib.dd_loss_previews(None, None, None, 2, 4, 4, None, 1, None, 1, 7, t, 1.0, 1.0, o, _stream()) < 0
    torch.cuda.synchronize()
    assert (out == SENTINEL).all(), "a refused call wrote"
    # without the source bit a null source is fine, and the launch after the refusals is clean
    L.check(op.call(o, [0], 6, [0], t, source=False))
    torch.cuda.synchronize()
    want = PR.mosaics(c, PR.dyadic_sides(c, seed=1), [0], 6, [0], THR)
    assert np.array_equal(out[:want.size].cpu().numpy().reshape(want.shape), want) and (out[want.size:] == SENTINEL).all()


# ---------------------------------------------------------------------------------------------------------------- whole program
def _program(seed=2):
    from deepdenoiser_amd.architecture import Architecture
    B, H, W = 4, 32, 32
    aj, tj = configs.architecture(filters=(16, 24), convs=1), configs.training()
    arch = Architecture(aj, device="cuda", dtype="f32", seed=seed)
    prog = arch.program(B, H, W, training_json=tj)
    feats, labels = TM._program_inputs(arch, B, H, W)
    prog.set_inputs(feats, labels)
    return arch, tj, prog, labels


def test_program_previews_against_the_reference():
    """the 17-pass network, B = 4, 32 x 32, f32: previews() against the reference evaluated on Program.raw, prediction_dictionaries()[0] and
    the labels; feature slots exact, combined and image slots within the band rule of the continuous family"""
    TM._need_gpu()
    arch, tj, prog, labels = _program()
    B, H, W = prog.B, prog.H, prog.W
    n_fwd = len(prog.g.fwd_ops)
    prog.zero_grads()
    prog.forward()
    images = [3, 0]
    shown = prog.previews(images=images, which="all")
    with_diff = prog.previews(images=images, which="all", panels=("prediction", "difference"), error_gain=4.0)
    torch.cuda.synchronize()
    assert len(prog.g.fwd_ops) == n_fwd, "previews() must not add to the forward program"
    plan = M.preview_plan(arch, tj, "all")
    assert [t for t, _ in shown] == [t for e in plan for t in M.preview_tags(e.name, 2)] == [t for t, _ in with_diff]
    assert [e.source[0] for e in plan] == ["image"] + ["combined"] * 4 + ["feature"] * 17
    assert all(a.shape == (H, 3 * W, 3) and a.dtype == np.uint8 for _, a in shown) and all(a.shape == (H, 2 * W, 3) for _, a in with_diff)
    # the case of the reference, from the program's own tensors
    head = prog.head
    preds = prog.prediction_dictionaries()[0]
    sides = {"source": [prog.raw[f.name].cpu().numpy().astype(np.float64) for f in head],
             "prediction": [preds[Naming.feature_prediction_name(f.name)].cpu().numpy().astype(np.float64) for f in head],
             "target": [labels[Naming.target_feature_name(f.name)].cpu().numpy().astype(np.float64) for f in head]}
    triples = M.combined_triples(arch)
    cidx = {cn: k for k, (cn, _) in enumerate(triples)}
    c = {"B": B, "H": H, "W": W, "nch": [f.number_of_channels for f in head],
         "combined": [tuple(prog.head_index[n] for n in names) for _, names in triples],
         "image": {"combined": [cidx[n] for n in ("Diffuse", "Glossy", "Subsurface", "Transmission")],
                   "features": [prog.head_index[n] for n in ("Volume Direct", "Volume Indirect", "Emission", "Environment")]}}
    slot_of = {("feature", f.name): i for i, f in enumerate(head)}
    slot_of.update({("combined", cn): PR.MAX_FEATURES + k for cn, k in cidx.items()})
    slot_of[("image", "Combined")] = PR.IMAGE_SLOT
    got = dict(shown)
    moved = total = close = 0
    for e in plan:
        slot = slot_of[e.source]
        values = PR.mosaic_values(c, sides, slot, 7, images)
        want, near = PR.quantise(values, THR), PR.near_threshold(values, THR, BAND)
        for k, tag in enumerate(M.preview_tags(e.name, 2)):
            g, w, n = got[tag], want[k * H:(k + 1) * H], near[k * H:(k + 1) * H]
            if e.source[0] == "feature":
                assert np.array_equal(g, w), tag
                d = dict(with_diff)[tag]
                wd = PR.quantise(PR.mosaic_values(c, sides, slot, 10, [images[k]], kind=tj["loss_difference"], error_gain=4.0), THR)
                assert np.array_equal(d, wd), tag
            else:
                diff = g.astype(np.int64) - w.astype(np.int64)
                assert np.abs(diff).max() <= 1 and not (diff != 0)[~n].any(), tag
                moved, total, close = moved + int((diff != 0).sum()), total + diff.size, close + int(n.sum())
    print("combined and image previews: %d of %d bytes differ by 1; %d values lie within a relative %g of a threshold" % (moved, total, close, BAND))
    assert close <= 0.01 * total
    a = got["previews/combined/image/0"]
    assert len(np.unique(a)) > 50 and (a[:12, :12] == 0).all()      # (the black corner of _program_inputs, in all three panels' first)
    again = prog.previews(images=images, which="all")
    assert all(np.array_equal(x, y) for (_, x), (_, y) in zip(shown, again)), "two runs differ"
    with pytest.raises(ValueError):
        prog.previews(which="some")
    with pytest.raises(RuntimeError):
        prog.previews(images=[4])


CHILD = r"""
import sys, torch
sys.path.insert(0, %(root)r)
sys.path.insert(0, %(tests)r)
import test_gpu_previews as TP
out = []
for with_previews in (False, True):
    arch, tj, prog, labels = TP._program()
    if with_previews:
        prog.zero_grads(); prog.forward()
        assert len(prog.previews(which="all", panels=("source", "prediction", "target", "difference"))) == 22 * 3
    prog.zero_grads(); prog.forward()
    torch.cuda.synchronize()
    out.append((prog.loss_buf.clone(), prog.predictions[0].buf.clone()))
print("RESULT loss=%%d predictions=%%d value=%%r" %% (int(torch.equal(out[0][0], out[1][0])), int(torch.equal(out[0][1], out[1][1])), float(out[0][0].sum())))
"""


def test_previews_leave_the_forward_alone():
    """loss_buf and the predictions after forward() are bit-identical with and without a previews() call before it (DD_DETERMINISTIC=1 in
    a child process: the loss kernels' atomics are not ordered otherwise)"""
    TM._need_gpu()
    env = dict(os.environ, DD_DETERMINISTIC="1")
    p = subprocess.run([sys.executable, "-c", CHILD % {"root": ROOT, "tests": os.path.join(ROOT, "tests")}], env=env, cwd=ROOT,
                       capture_output=True, text=True, timeout=300)
    assert p.returncode == 0, p.stdout[-2000:] + p.stderr[-3000:]
    line = [ln for ln in p.stdout.splitlines() if ln.startswith("RESULT")][0]
    r = dict(kv.split("=") for kv in line.split()[1:])
    assert r["loss"] == "1" and r["predictions"] == "1" and float(r["value"]) > 0, line


# ---------------------------------------------------------------------------------------------------------------- command line
def _cli_setup(tmp_path, modes):
    from deepdenoiser_amd.architecture import Architecture
    aj = configs.architecture(filters=(16, 24), convs=1, flag_mode="NONE", combined=TM.NO_ALPHA)
    aj["model_directory"] = "model"
    tj = configs.training(learning_rate=2e-3, batch_size=4)
    tj.update({"architecture": "architecture.json", "base_tfrecords_directory": "data", "modes": modes, "number_of_source_index_tuples": 1})
    tj["data_augmentation"] = {"use_rotate_90": True, "use_flip_left_right": False, "use_rgb_permutation": True, "use_normal_rotation": False}
    json.dump(aj, open(tmp_path / "architecture.json", "w"))
    json.dump(tj, open(tmp_path / "training.json", "w"))
    arch = Architecture(aj, device="cpu")
    for k, mode in enumerate(modes):
        TM._write_dataset(str(tmp_path / "data"), arch, mode, 2 if mode == "training" else 1, 4, k)
    return arch, tj


def _train(tmp_path, *flags):
    p = subprocess.run([sys.executable, "-m", "deepdenoiser_amd.train", str(tmp_path / "training.json"), "--dtype", "f32"] + list(flags),
                       env=dict(os.environ, PYTHONPATH=ROOT), cwd=ROOT, capture_output=True, text=True, timeout=600)
    assert p.returncode == 0, p.stdout[-2000:] + p.stderr[-3000:]
    return p.stdout


def test_cli_writes_image_summaries(tmp_path):
    """two epochs of two steps with validation, --image_steps 2 --image_count 2 --image_difference: image events of their own at steps 2 and
    4 in the training file, the validation previews at the same global steps in eval_validation/"""
    TM._need_gpu()
    arch, tj = _cli_setup(tmp_path, ["training", "validation"])
    # (--image_exposure 1/16: the radiances of this data set are a + b*y + c*x with a, b, c in [0, 1) per pass, so the combined image, a sum
    # of eight members, lies near 6 .. 25 and would be one white tile at exposure 1; at 1/16 every tile spreads over 50 or more byte values)
    out = _train(tmp_path, "--train_epochs", "2", "--summary_steps", "1", "--image_steps", "2", "--image_count", "2", "--image_difference",
                 "--image_exposure", "0.0625")
    assert "epoch 2: global_step 4" in out and "epoch 2: validation loss " in out, out
    names = [e.name for e in M.metric_plan(arch, tj, out=lambda *a: None)]
    plan = M.preview_plan(arch, tj, "combined")
    tags = [t for e in plan for t in M.preview_tags(e.name, 2)]
    assert len(plan) == 5 and tags[0] == "previews/combined/image/0" and tags[-1] == "previews/combined_transmission/image/1"
    model = str(tmp_path / "model")
    (train_file,) = summaries.event_files(model)
    events = [e for e in summaries.read_events(train_file) if e["file_version"] is None]
    # the image event of a step comes in front of its scalar event and holds only images
    assert [(e["step"], bool(e["images"])) for e in events] == [(1, False), (2, True), (2, False), (3, False), (4, True), (4, False)]
    for e in events:
        if e["images"]:
            assert e["tags"] == tags and not e["scalars"] and not e["histograms"]
        else:
            assert e["tags"] == ["loss", "learning_rate", "batch_size"] + names
    images = summaries.read_images(train_file)
    assert [(s, t) for s, t, _ in images] == [(s, t) for s in (2, 4) for t in tags]
    for _, tag, im in images:
        a = summaries.decode_png(im["png"])
        assert a.shape == (TM.T_, 4 * TM.T_, 3) == (im["height"], im["width"], im["colorspace"]), tag
        panels = [a[:, k * TM.T_:(k + 1) * TM.T_] for k in range(4)]
        assert all(len(np.unique(p)) > 4 for p in panels[:3]), tag      # smooth ramps with noise, not a blank tile
        assert (panels[3][..., 0] == panels[3][..., 1]).all() and not np.array_equal(panels[0], panels[2])
    (eval_file,) = summaries.event_files(os.path.join(model, "eval_validation"))
    shown = summaries.read_images(eval_file)
    assert [(s, t) for s, t, _ in shown] == [(s, t) for s in (2, 4) for t in tags]
    by = {(s, t): summaries.decode_png(im["png"]) for s, t, im in shown}
    for t in tags:      # the validation stream is not shuffled: the same tiles every epoch (source and target panels), another prediction
        a, b = by[(2, t)], by[(4, t)]
        assert a.shape == (TM.T_, 4 * TM.T_, 3)
        assert np.array_equal(a[:, :TM.T_], b[:, :TM.T_]) and np.array_equal(a[:, 2 * TM.T_:3 * TM.T_], b[:, 2 * TM.T_:3 * TM.T_]), t
    assert any(not np.array_equal(by[(2, t)][:, TM.T_:2 * TM.T_], by[(4, t)][:, TM.T_:2 * TM.T_]) for t in tags)
    evs = [e for e in summaries.read_events(eval_file) if e["file_version"] is None]
    assert [(e["step"], bool(e["images"])) for e in evs] == [(2, False), (2, True), (4, False), (4, True)]
    assert all(e["tags"] == (tags if e["images"] else ["loss"] + names) for e in evs)


def test_cli_without_the_flag_writes_what_it_wrote(tmp_path):
    """--image_steps 0 (the default): one event per step with loss, learning_rate, batch_size and the tracked scalars, as before images existed,
    no image value, nothing else new"""
    TM._need_gpu()
    arch, tj = _cli_setup(tmp_path, ["training"])
    out = _train(tmp_path, "--train_epochs", "1", "--summary_steps", "1")
    assert "epoch 1: global_step 2" in out, out
    names = [e.name for e in M.metric_plan(arch, tj, out=lambda *a: None)]
    (train_file,) = summaries.event_files(str(tmp_path / "model"))
    events = summaries.read_events(train_file)
    assert [(e["step"], e["file_version"]) for e in events] == [(0, summaries.FILE_VERSION), (1, None), (2, None)]
    for e in events[1:]:
        assert e["tags"] == ["loss", "learning_rate", "batch_size"] + names and not e["images"] and not e["histograms"]
        assert [t for t, _ in e["scalars"]] == e["tags"]
    assert summaries.read_images(train_file) == []
    assert not os.path.exists(os.path.join(str(tmp_path / "model"), "eval_validation"))
