"""-m gpu: dd_nonfinite_scan / dd_nonfinite_repair through the C-ABI against tests/nonfinite_ref.py, the Predictor's nonfinite= modes and the
command line's --nonfinite options.

Op level.  Every plane lies between guard floats (a NaN pattern: a read past either end would be counted) and every mask plane between
guard bytes inside a buffer pre-filled with a sentinel; both must come back untouched.  Gates: masks and counts equal; every value at an
unmasked position -- guards and the unused channel of an ld = 4 plane included -- bit-identical to the input; repaired values bit-equal on
the dyadic family (every finite value k/16 with |k| <= 32: every window sum is exact in any order and the one division is correctly rounded
on both sides) and within gpu_util.ROUND["f32"] on the continuous family (randn)."""
import ctypes
import json
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import nonfinite_ref as R
from deepdenoiser_amd import _lib, configs, openexr
from deepdenoiser_amd.naming import Naming
from gpu_util import ROUND, check

pytestmark = pytest.mark.gpu

GUARD = 64                                    # floats (and mask bytes) either side of a plane
GUARD_BITS = 0x7fc12345                       # a NaN
SENTINEL = 0xAB
BAD_BITS = (0x7f800000, 0xff800000, 0x7fc00000, 0xffc00000, 0x7f800001, 0xff800001, 0x7fffffff, 0xffbfffff)      # +-inf, quiet and signalling NaNs


def _need_gpu():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")


def _values(rng, shape, family):
    if family == "dyadic":
        return (rng.integers(-32, 33, size=shape).astype(np.float32) / np.float32(16.0)).astype(np.float32)
    return rng.standard_normal(shape).astype(np.float32)


def _plant(rng, plane, C, family, fraction=0.01, block=None):
    """plane: [N,H,W,ld]; the first C channels receive ~1 % non-finite values of every bit pattern, plus the placements the kernels can get
    wrong: the four corners, a whole edge, the rows and columns either side of the border between two images, a block larger than the window."""
    N, H, W, _ = plane.shape
    u = plane.view(np.uint32)
    # finite patterns that must NOT be masked: -0, and the smallest denormal (continuous family only: it is not k/16).  +-FLT_MAX are in
    # test_finite_extremes_are_left_alone, away from every window: a window sum that holds them overflows
    u[N - 1, H // 2, W // 2, 0] = 0x80000000
    if family == "continuous":
        u[0, H // 2, W // 3, 0] = 0x00000001
    k = max(1, int(round(fraction * N * H * W * C)))
    pick = rng.choice(N * H * W * C, size=k, replace=False)
    n, y, x, c = np.unravel_index(pick, (N, H, W, C))
    u[n, y, x, c] = np.array(BAD_BITS, dtype=np.uint32)[np.arange(k) % len(BAD_BITS)]
    if H * W > 1:
        for yy, xx in ((0, 0), (0, W - 1), (H - 1, 0), (H - 1, W - 1)):
            u[0, yy, xx, 0] = BAD_BITS[2]
        u[0, 0, :, C - 1] = BAD_BITS[0]                       # the whole top edge of image 0
        for i in range(N - 1):                                # facing rows / pixels of neighbouring images
            u[i, H - 1, :, 0] = BAD_BITS[1]
            u[i + 1, 0, ::2, 0] = BAD_BITS[4]
    if block is not None:
        y0, x0, size = block
        u[N - 1, y0:y0 + size, x0:x0 + size, :C] = BAD_BITS[3]


class Case:
    """planes: (C, ld, data offset in floats past the aligned base, mask offset in bytes past the aligned base)"""

    def __init__(self, name, N, H, W, planes, radius, fraction=0.01, block=None, clean=(), all_bad=False):
        self.name, self.N, self.H, self.W, self.planes, self.radius = name, N, H, W, planes, radius
        self.fraction, self.block, self.clean, self.all_bad = fraction, block, clean, all_bad

    def build(self, family, seed=0):
        """-> per plane: (host float buffer with guards, offset of the plane in it, [N,H,W,ld] view of the plane)"""
        rng = np.random.default_rng(seed)
        out = []
        for i, (C, ld, off, _) in enumerate(self.planes):
            n = self.N * self.H * self.W * ld
            buf = np.full(GUARD + off + n + GUARD, GUARD_BITS, dtype=np.uint32).view(np.float32)
            plane = buf[GUARD + off:GUARD + off + n].reshape(self.N, self.H, self.W, ld)
            plane[...] = _values(rng, plane.shape, family)
            if ld > C:
                plane[..., C:].view(np.uint32)[::2] = BAD_BITS[2]      # the channels past C are not the kernels' business, NaN or not
            if self.all_bad:
                plane[..., :C].view(np.uint32)[...] = BAD_BITS[i % len(BAD_BITS)]
            elif i not in self.clean:
                _plant(rng, plane, C, family, self.fraction, self.block)
            out.append((buf, GUARD + off, plane))
        return out


P1, P3 = (1, 1, 0, 0), (3, 3, 0, 0)
CASES = [
    Case("1x1_everything_bad", 1, 1, 1, [P1, P3], 2, all_bad=True),
    Case("1x37_one_plane", 1, 1, 37, [P3], 1),
    Case("37x1", 1, 37, 1, [P1, P3], 2),
    Case("5x7_radius_4", 1, 5, 7, [P3, P1], 4),
    Case("35x257", 1, 35, 257, [P3, P1, (3, 4, 0, 0)], 2, block=(11, 100, 9)),
    Case("35x257_radius_1", 1, 35, 257, [P3], 1, block=(20, 3, 9)),
    Case("35x257_misaligned", 1, 35, 257, [(3, 3, 1, 0), (1, 1, 1, 0), (3, 3, 0, 1), (1, 1, 3, 2)], 2, block=(0, 0, 9)),
    Case("3_images_13x10", 3, 13, 10, [P3, P1, (3, 4, 0, 0)], 4),
    Case("3_images_6x5_radius_1", 3, 6, 5, [P1, P3], 1),
    Case("32_planes_mixed", 2, 9, 13, [(3, 3, 0, 0), (1, 1, 0, 0), (3, 4, 0, 0), (1, 2, 0, 0)] * 8, 2),
    Case("clean_sibling", 1, 35, 257, [P3, P3, P1, P1], 2, clean=(0, 2)),
    Case("1572864_pixels", 1, 1024, 1536, [P3, P1], 2, fraction=0.01, block=(500, 700, 9)),
]


def _reference(case, built):
    want = []
    for (C, ld, _, _), (buf, off, plane) in zip(case.planes, built):
        mask, values, pixels = R.scan(plane[..., :C])
        fixed = plane.copy()
        fixed[..., :C] = R.repair(plane[..., :C], mask, case.radius)
        want.append((mask, values, pixels, fixed))
    return want


def _launch(lib, case, built):
    """one scan + one repair of the whole table -> per plane (float buffer, mask buffer) on the host, and the counts"""
    npix = case.N * case.H * case.W
    data = [torch.from_numpy(buf.copy()).cuda() for buf, _, _ in built]
    masks = [torch.full((GUARD + moff + npix + GUARD,), SENTINEL, dtype=torch.uint8, device="cuda") for (_, _, _, moff) in case.planes]
    counts = torch.zeros((len(built), 2), dtype=torch.int64, device="cuda")
    d = _lib.NonfiniteDesc()
    d.n_planes = len(built)
    for i, ((C, ld, _, moff), (_, off, _)) in enumerate(zip(case.planes, built)):
        d.plane[i].data, d.plane[i].C, d.plane[i].ld = data[i].data_ptr() + 4 * off, C, ld
        d.plane[i].mask = masks[i].data_ptr() + GUARD + moff
    stream = torch.cuda.current_stream().cuda_stream
    _lib.check(lib.dd_nonfinite_scan(ctypes.byref(d), case.N, case.H, case.W, counts.data_ptr(), stream))
    scanned = counts.clone()
    _lib.check(lib.dd_nonfinite_repair(ctypes.byref(d), case.N, case.H, case.W, case.radius, counts.data_ptr(), stream))
    after = torch.zeros_like(counts)
    masks2 = [m.clone() for m in masks]
    for i, (_, _, _, moff) in enumerate(case.planes):
        d.plane[i].mask = masks2[i].data_ptr() + GUARD + moff
    _lib.check(lib.dd_nonfinite_scan(ctypes.byref(d), case.N, case.H, case.W, after.data_ptr(), stream))
    torch.cuda.synchronize()
    return data, masks, scanned.cpu().tolist(), after.cpu().tolist()


@pytest.mark.parametrize("family", ["dyadic", "continuous"])
@pytest.mark.parametrize("case", CASES, ids=[c.name for c in CASES])
def test_scan_and_repair_match_the_reference(lib, case, family):
    _need_gpu()
    built = case.build(family)
    want = _reference(case, built)
    data, masks, counts, after = _launch(lib, case, built)
    again = _launch(lib, case, built)
    npix = case.N * case.H * case.W
    total_bad = 0
    for i, ((C, ld, _, moff), (buf, off, plane), (mask, values, pixels, fixed)) in enumerate(zip(case.planes, built, want)):
        tag = "%s/%s plane %d" % (case.name, family, i)
        total_bad += values
        assert counts[i] == [values, pixels], tag
        assert after[i] == [0, 0], tag + ": a second scan after the repair"
        got_mask = masks[i].cpu().numpy()
        lo = GUARD + moff
        assert np.array_equal(got_mask[lo:lo + npix].reshape(mask.shape), mask), tag
        assert (got_mask[:lo] == SENTINEL).all() and (got_mask[lo + npix:] == SENTINEL).all(), tag + ": mask guard bytes"
        got = data[i].cpu().numpy()
        expect = buf.copy()
        expect[off:off + plane.size] = fixed.reshape(-1)
        bad = np.zeros(buf.shape, dtype=bool)
        sel = np.zeros(plane.shape, dtype=bool)
        for c in range(C):
            sel[..., c] = ((mask >> c) & 1) == 1
        bad[off:off + plane.size] = sel.reshape(-1)
        # everything that is not masked -- guards, the channels past C, every finite value -- is bit-identical to the input
        assert torch.equal(torch.from_numpy(got.view(np.int32)[~bad]), torch.from_numpy(buf.view(np.int32)[~bad])), tag
        if i in case.clean:
            assert values == 0 and not got_mask[lo:lo + npix].any() and np.array_equal(got.view(np.int32), buf.view(np.int32)), tag
        if values:
            if family == "dyadic":
                assert torch.equal(torch.from_numpy(got.view(np.int32)[bad]), torch.from_numpy(expect.view(np.int32)[bad])), tag
            else:
                check(tag + " repaired values", torch.from_numpy(got[bad]), torch.from_numpy(expect[bad]), ROUND["f32"])
        # the same launches on a copy of the same input: the same bits
        assert torch.equal(again[0][i].view(torch.int32), data[i].view(torch.int32)) and torch.equal(again[1][i], masks[i]), tag
    assert again[2] == counts
    assert total_bad > 0
    if case.all_bad:      # no usable value anywhere: every replacement is 0
        assert all((d.cpu().numpy()[GUARD:GUARD + C] == 0.0).all() for d, (C, _, _, _) in zip(data, case.planes))


def test_finite_extremes_are_left_alone(lib):
    """+-FLT_MAX, denormals and -0 are finite: not masked, not counted, not written; every non-finite pattern next to them is."""
    _need_gpu()
    fine = (0x7f7fffff, 0xff7fffff, 0x00000001, 0x80000001, 0x80000000)
    case = Case("patterns", 1, 1, 64, [P1], 1)
    buf = np.full(GUARD + 64 + GUARD, GUARD_BITS, dtype=np.uint32).view(np.float32)
    plane = buf[GUARD:GUARD + 64].reshape(1, 1, 64, 1)
    plane[...] = 1.0
    u = plane.view(np.uint32)
    for i, bits in enumerate(fine):
        u[0, 0, 4 * i, 0] = bits                              # 0, 4, .. 16: no bad value within radius 1
    for i, bits in enumerate(BAD_BITS):
        u[0, 0, 30 + 3 * i, 0] = bits
    built = [(buf, GUARD, plane)]
    (mask, values, pixels, fixed), = _reference(case, built)
    assert (values, pixels) == (len(BAD_BITS), len(BAD_BITS)) and not mask[0, 0, :30].any()
    data, masks, counts, after = _launch(lib, case, built)
    assert counts == [[values, pixels]] and after == [[0, 0]]
    assert np.array_equal(masks[0].cpu().numpy()[GUARD:GUARD + 64].reshape(mask.shape), mask)
    expect = buf.copy()
    expect[GUARD:GUARD + 64] = fixed.reshape(-1)
    assert np.array_equal(data[0].cpu().numpy().view(np.int32), expect.view(np.int32))
    assert (fixed[0, 0, 30:54:3, 0] == 1.0).all()


def test_the_cases_cover_what_the_kernels_can_get_wrong():
    """(no device needed: the properties of the inputs the test above relies on)"""
    big = [c for c in CASES if c.N * c.H * c.W == 1572864]
    assert len(big) == 1 and any(len(c.planes) == 32 for c in CASES) and any(len(c.planes) == 1 for c in CASES)
    assert {c.radius for c in CASES} >= {1, 2, 4}
    assert any(c.N * c.H * c.W % 4 for c in CASES) and any(p[1] > p[0] for c in CASES for p in c.planes)
    case = next(c for c in CASES if c.name == "35x257")
    built = case.build("dyadic")
    mask, values, pixels, fixed = _reference(case, built)[0]
    assert mask[0, 0, 0] and mask[0, 0, 256] and mask[0, 34, 0] and mask[0, 34, 256] and mask[0, 0].all()
    assert (fixed[0, 13:18, 102:107, :3] == 0).all()                      # inside the 9 x 9 block: no usable value within radius 2
    frac = values / float(case.H * case.W * 3)
    assert 0.005 < frac < 0.2
    plane = built[0][2]
    finite = plane[np.isfinite(plane)]
    assert np.array_equal(finite * 16, np.round(finite * 16)) and np.abs(finite).max() <= 2.0


# ---------------------------------------------------------------------------------------------------- Predictor
H, W, T, O = 70, 90, 32, 4


def _arch(dtype):
    from deepdenoiser_amd.architecture import Architecture
    aj = configs.architecture(filters=(16, 16), convs=1, flag_mode="NONE")
    return Architecture(aj, device="cuda", dtype=dtype, seed=3)


def _frame(arch):
    """A dyadic frame (k/16) with a NaN, a +inf and a -inf in three pixels of two passes: one in an auxiliary pass, one inside a tile overlap."""
    rng = np.random.default_rng(9)
    frame = {}
    for f in arch.feature_predictions + arch.auxiliary_features:
        frame[Naming.source_feature_name(f.name, index=0)] = (rng.integers(0, 33, size=(H, W, f.number_of_channels)).astype(np.float32) / np.float32(16.0))
    head = Naming.source_feature_name(arch.feature_predictions[0].name, index=0)
    aux = Naming.source_feature_name(arch.auxiliary_features[0].name, index=0)
    assert head != aux
    from deepdenoiser_amd.tiling import tile_plan
    plan = tile_plan(H, W, T, O)
    x_overlap = plan.windows()[1][1] + 1                    # a column the second tile column shares with the first
    assert plan.windows()[1][1] < plan.windows()[0][1] + plan.tile
    bad = {k: v.copy() for k, v in frame.items()}
    bad[head][10, 12, 0] = np.nan
    bad[head][40, x_overlap, frame[head].shape[2] - 1] = np.inf
    bad[aux][33, 50, 0] = -np.inf
    want = {head: {"values": 2, "pixels": 2}, aux: {"values": 1, "pixels": 1}}
    return frame, bad, want


def _repaired_by_the_reference(arch, bad, radius=2):
    out = {}
    for k, v in bad.items():
        mask, _, _ = R.scan(v[None])
        out[k] = R.repair(v[None], mask, radius)[0]
    return out


def _tensors(frame, device="cpu"):
    return {k: torch.from_numpy(v.copy()).to(device) for k, v in frame.items()}


@pytest.mark.parametrize("dtype", ["f32", "f16"])
def test_predictor_modes(dtype, monkeypatch):
    _need_gpu()
    from deepdenoiser_amd.prediction import Predictor
    arch = _arch(dtype)
    clean, bad, want = _frame(arch)
    kw = dict(tile_size=T, tile_overlap_size=O, tiles_per_batch=5)

    def outputs(pred, frame):
        out = {k: v.clone() for k, v in pred.predict_frame(frame).items()}
        torch.cuda.synchronize()
        return out

    # keep: today's behaviour -- the non-finite samples run through the network
    keep = Predictor(arch, **kw)
    assert keep._scanner is None
    out_keep = outputs(keep, _tensors(bad))
    assert not all(bool(torch.isfinite(v).all()) for v in out_keep.values())
    assert keep._scanner is None and keep._scanners == {}

    # error: named passes with their counts, and no forward launch
    err = Predictor(arch, nonfinite="error", **kw)
    with pytest.raises(ValueError) as e:
        err.predict_frame(_tensors(bad))
    for k, v in want.items():
        assert "%s: %d values in %d pixels" % (k, v["values"], v["pixels"]) in str(e.value)
    assert err._graphs == {}
    assert {k: v for k, v in err.nonfinite_report().items() if v["values"]} == want
    out_err_clean = outputs(err, _tensors(clean))                      # a clean frame passes

    # repair == keep on the frame repaired by the reference
    reference = outputs(Predictor(arch, **kw), _tensors(_repaired_by_the_reference(arch, bad)))
    assert all(bool(torch.isfinite(v).all()) for v in reference.values())
    rep = Predictor(arch, nonfinite="repair", **kw)
    got = outputs(rep, _tensors(bad))
    assert {k: v for k, v in rep.nonfinite_report().items() if v["values"]} == want
    assert set(rep.nonfinite_report()) == set(arch.required_source_names())
    assert set(got) == set(reference)
    for k in got:
        assert torch.isfinite(got[k]).all() and torch.equal(got[k], reference[k]), k
    # ... a device-resident frame: the same outputs, and the caller's tensors still hold their NaN / inf
    resident = _tensors(bad, "cuda")
    before = {k: v.clone() for k, v in resident.items()}
    got = outputs(rep, resident)
    for k in got:
        assert torch.equal(got[k], reference[k]), k
    for k in resident:
        assert torch.equal(resident[k].view(torch.int32), before[k].view(torch.int32)), k
    assert sum(int((~torch.isfinite(v)).sum()) for v in resident.values()) == 3
    # ... through dd_extract_tiles instead of the in-place input assembly
    monkeypatch.setenv("DD_FRAME_INPUT", "0")
    tiles = Predictor(arch, nonfinite="repair", **kw)
    got = outputs(tiles, _tensors(bad))
    assert tiles._plans[(H, W)][1].frame_input is None
    for k in got:
        assert torch.equal(got[k], reference[k]), k
    monkeypatch.delenv("DD_FRAME_INPUT")
    # a clean frame: repair mode changes nothing
    out_clean = outputs(Predictor(arch, **kw), _tensors(clean))
    got = outputs(rep, _tensors(clean))
    assert all(v == {"values": 0, "pixels": 0} for v in rep.nonfinite_report().values())
    for k in got:
        assert torch.equal(got[k], out_clean[k]) and torch.equal(out_err_clean[k], out_clean[k]), k


def test_predictor_scans_a_wide_frame_with_the_channels_of_its_pass():
    _need_gpu()
    from deepdenoiser_amd.prediction import Predictor
    arch = _arch("f32")
    clean, bad, want = _frame(arch)
    kw = dict(tile_size=T, tile_overlap_size=O, tiles_per_batch=5)
    reference = {k: v.clone() for k, v in Predictor(arch, **kw).predict_frame(_tensors(_repaired_by_the_reference(arch, bad))).items()}
    f0 = arch.feature_predictions[0]
    k0 = Naming.source_feature_name(f0.name, index=0)
    wide = _tensors(bad)
    wide[k0] = torch.cat([wide[k0], torch.full((H, W, 1), float("nan"))], dim=2)      # a fourth channel the pass does not have, all NaN
    rep = Predictor(arch, nonfinite="repair", **kw)
    got = rep.predict_frame(wide)
    assert {k: v for k, v in rep.nonfinite_report().items() if v["values"]} == want
    for k in got:
        assert torch.equal(got[k], reference[k]), k


# ---------------------------------------------------------------------------------------------------- command line
def test_cli_nonfinite_options(tmp_path):
    _need_gpu()
    from deepdenoiser_amd import tf_checkpoint
    from deepdenoiser_amd.architecture import Architecture
    from deepdenoiser_amd.summaries import decode_png
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    aj = configs.architecture(filters=(16, 24), convs=1, flag_mode="NONE")
    aj["model_directory"] = "model"
    json.dump(aj, open(tmp_path / "architecture.json", "w"))
    arch = Architecture(aj, device="cuda", dtype="f32", seed=2)
    from deepdenoiser_amd.prediction import Predictor
    Predictor(arch, tile_size=32, tile_overlap_size=4).prepare(40, 72)              # (creates the parameters)
    tf_checkpoint.save_variables(arch, str(tmp_path / "model"), global_step=1)
    passes = {f.name: f.number_of_channels for f in arch.feature_predictions + arch.auxiliary_features if f.load_data}
    frame_dir = tmp_path / "frame_0001_16_0_0"
    frame_dir.mkdir()
    rng = np.random.default_rng(5)
    victim = next(n for n, ch in passes.items() if ch == 3)
    want_mask = np.zeros((40, 72, 3), dtype=np.uint8)
    for name, ch in passes.items():
        img = rng.random((40, 72, 3)).astype(np.float32)
        if ch == 1:
            img[...] = img[..., :1]
        if name == victim:
            img[17, 30, 1] = np.nan
            want_mask[17, 30, 1] = 255
        openexr.write_image(str(frame_dir / ("render_%s_0001.exr" % name)), img)
    env = dict(os.environ, PYTHONPATH=root)
    base = [sys.executable, "-m", "deepdenoiser_amd.predict", str(tmp_path / "architecture.json"), "--input", str(frame_dir),
            "--tile_size", "32", "--tile_overlap_size", "4", "--dtype", "f32"]
    p = subprocess.run(base + ["--nonfinite", "error"], env=env, cwd=root, capture_output=True, text=True, timeout=600)
    assert p.returncode != 0 and victim in p.stdout, p.stdout[-2000:] + p.stderr[-3000:]
    assert not [ln for ln in p.stdout.splitlines() if ln.endswith(".npy")]
    p = subprocess.run(base + ["--nonfinite", "repair", "--nonfinite_png"], env=env, cwd=root, capture_output=True, text=True, timeout=600)
    assert p.returncode == 0, p.stdout[-2000:] + p.stderr[-3000:]
    assert ("source_image/0/%s: 1 non-finite values in 1 pixels" % victim) in p.stdout, p.stdout
    written = [ln for ln in p.stdout.splitlines() if ln.endswith(".npy")]
    assert written and all(np.isfinite(np.load(w)).all() for w in written)
    pngs = sorted(n for n in os.listdir(frame_dir) if n.endswith("_nonfinite.png"))
    assert pngs == [victim + "_nonfinite.png"]
    assert np.array_equal(decode_png(open(frame_dir / pngs[0], "rb").read()), want_mask)
