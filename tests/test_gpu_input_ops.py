"""-m gpu: the kernels every network reads its input through, op by op through the C-ABI, against the float64 reference and error budget of
tests/input_ref.py: dd_prepare_feature, dd_gather_input, dd_assemble_input (the fused default) and dd_assemble_input_frames (inference).

THE GATE is elementwise on every written element: |got - ref| <= 2 * budget + r_T(ref) (input_ref.py: the budget is a first-order bound on
what ANY float32 evaluation of the formulas may be off by, carried through the reference's own intermediates; r_T is half an ulp of the storage
type, 0 for float32 and for std_out; the factor 2 covers second-order terms and the store of a value that is itself off by the budget).  The
worst error / gate of every case is printed and recorded (gpu_util.gate, bound 1).  tests/test_input_ref.py shows on the CPU, for these very
inputs, that an f32 evaluation stays within 1x the budget and that wrong borders, counts, taps, sources, epsilon, channel orders and dst_ch
offsets do not pass.  Everything a kernel must NOT write is pre-filled with a sentinel and compared for equality."""
import ctypes as C

import pytest
import torch

import input_ref as R
from deepdenoiser_amd import _lib as L
from gpu_util import gate, rel_l2

pytestmark = pytest.mark.gpu
SENTINEL = 12288.0      # exact in fp32, bf16 and fp16
DT = {"f32": (L.DD_F32, torch.float32, 4), "bf16": (L.DD_BF16, torch.bfloat16, 8), "f16": (L.DD_F16, torch.float16, 8)}


def _need_gpu():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")


def _stream():
    return torch.cuda.current_stream().cuda_stream


def _dev(t):
    return t.float().contiguous().cuda()


def _fp(fp):
    return L.FeatureParams(fp["use_log1p"], fp["mean"], fp["inv_std"], fp["use_variance"], fp["variance_before"], fp["mode_neighbor"],
                           fp["relative"], fp["compress"], fp["epsilon"])


def _table(records):
    """A ctypes array of entry records -> device bytes."""
    arr = (type(records[0]) * len(records))(*records)
    return torch.frombuffer(bytearray(bytes(arr)), dtype=torch.uint8).cuda()


def _gated(name, got, ref, err, dtype="f32"):
    got = got.double().cpu()
    assert tuple(got.shape) == tuple(ref.shape), (name, tuple(got.shape), tuple(ref.shape))
    assert bool(torch.isfinite(got).all()), name + ": non-finite values"
    w = R.worst_ratio(got, ref, err, dtype)
    print("%-70s worst error / gate %.3f" % (name, w))
    gate(name, w, 1.0)
    return w


def _untouched(t):
    return bool((t == SENTINEL).all())


# ---------------------------------------------------------------------------------------------------------------- dd_prepare_feature
@pytest.mark.parametrize("shape", R.SHAPES, ids=["%dx%dx%d" % s for s in R.SHAPES])
def test_prepare_feature_parity(shape):
    _need_gpu()
    lib = L.load()
    B, H, W = shape
    ran = set()
    for i, c in enumerate(R.PREPARE_CASES):
        if c["shape"] != shape:
            continue
        v, fp = R.prepare_inputs(i)
        ref, err = R.prepare_reference(i)
        n = ref.shape[3]
        assert n == 3 + R.n_variance_channels(fp, c["cs"])
        src, fps = _dev(v), _fp(fp)
        for ldd in sorted({n, 4, 8}):
            if ldd < n:
                continue
            dst = torch.full((B, H, W, ldd), SENTINEL, dtype=torch.float32, device="cuda")
            L.check(lib.dd_prepare_feature(src.data_ptr(), c["cs"], dst.data_ptr(), ldd, C.byref(fps), B, H, W, _stream()))
            torch.cuda.synchronize()
            got = dst.cpu()
            _gated("prepare %s ldd %d" % (c["name"], ldd), got[..., :n], ref, err)
            if c["branch"] == "identity":
                assert torch.equal(got[..., :3].double(), v.expand(-1, -1, -1, 3)), c["name"]
            if ldd == 4 and n == 3:      # the record leaves as one float4 whose fourth lane is 0
                assert not got[..., 3].any(), "%s: channel 3 of a float4 record without a variance is not 0" % c["name"]
            else:
                assert _untouched(got[..., n:]), "%s ldd %d: a channel past the record was written" % (c["name"], ldd)
            assert torch.equal(src.cpu().double(), v)
            ran.add((c["cs"], c["branch"], ldd == 4 and (n <= 4)))
    assert {(cs, br) for cs, br, _ in ran} == {(cs, br) for cs in (1, 3) for br in R.BRANCHES}


def test_prepare_feature_flat_planes_have_no_variance():
    """A constant plane (a pass that was not loaded): the relative variance is within budget of 0 -- and the budget there is small (below 1e-4
    even where mean^2 < epsilon and log1p's two ulp are divided by epsilon), not the cancellation noise of E[x^2] - E[x]^2 over epsilon."""
    _need_gpu()
    lib = L.load()
    for i, c in enumerate(R.PREPARE_CASES):
        v, fp = R.prepare_inputs(i)
        if c["family"] not in R.FLAT or not fp["use_variance"] or c["shape"] != (2, 17, 33):
            continue
        ref, err = R.prepare_reference(i)
        assert float(ref[..., 3:].abs().max()) < 1e-12 and float(err[..., 3:].max()) < 1e-4, c["name"]
        dst = torch.full(tuple(c["shape"]) + (8,), SENTINEL, dtype=torch.float32, device="cuda")
        L.check(lib.dd_prepare_feature(_dev(v).data_ptr(), c["cs"], dst.data_ptr(), 8, C.byref(_fp(fp)), *c["shape"], _stream()))
        torch.cuda.synchronize()
        worst = float(dst.cpu()[..., 3:ref.shape[3]].abs().max())
        print("%s: |variance| <= %.3e (budget %.3e)" % (c["name"], worst, float(err[..., 3:].max())))
        assert worst <= 2 * float(err[..., 3:].max())


def test_prepare_feature_refusals():
    _need_gpu()
    lib = L.load()
    B, H, W = 1, 5, 7
    src = torch.ones(B, H, W, 3, device="cuda")
    dst = torch.full((B, H, W, 8), SENTINEL, dtype=torch.float32, device="cuda")
    per_channel, compressed, none = (_fp(R.feature_params("signed", b)) for b in ("uniform_relative_per_channel", "default", "no_variance"))
    for cs, ldd, fps in ((3, 5, per_channel), (3, 3, compressed), (1, 3, per_channel), (3, 2, none), (2, 8, compressed), (0, 8, none), (4, 8, none)):
        rc = lib.dd_prepare_feature(src.data_ptr(), cs, dst.data_ptr(), ldd, C.byref(fps), B, H, W, _stream())
        torch.cuda.synchronize()
        assert rc != 0 and lib.dd_last_error(), (cs, ldd)
        assert _untouched(dst), (cs, ldd)


# ---------------------------------------------------------------------------------------------------------------- dd_gather_input
# (channels, pixel stride of the source plane, first channel inside it) in dst_ch order; 0 channels: skipped; "b": a broadcast vector
GATHER_ORDERS = {
    "even_then_odd": ([(4, 4, 0), (3, 8, 2), (6, 6, 0), ("b", 2), (0, 4, 0), (4, 5, 1)], 24, 32),      # dst_ch 0 4 7 13 15 15; 19 used
    "odd_first": ([(3, 3, 0), (6, 8, 1), (4, 4, 0), ("b", 3), (4, 8, 4)], 24, 24),                     # dst_ch 0 3 9 13 16; 20 used
    "one_group": ([(3, 4, 0)], 8, 16),
}


@pytest.mark.parametrize("dtype", list(DT))
@pytest.mark.parametrize("order", list(GATHER_ORDERS))
def test_gather_input_is_exact(order, dtype):
    _need_gpu()
    lib = L.load()
    code, tdt, _ = DT[dtype]
    specs, c_pad, ld = GATHER_ORDERS[order]
    for T in (1, 3):
        for B, H, W in ((1, 1, 1), (2, 17, 33), (1, 5, 50)):
            g = torch.Generator().manual_seed(B + H + W + T)
            want = torch.zeros(T * B, H, W, c_pad)
            keep, records, used = [], [], 0
            for t in range(T):
                dst_ch = 0
                for sp in specs:
                    if sp[0] == "b":
                        vec = (torch.randint(-16, 17, (sp[1],), generator=g).float() / 8).cuda()
                        keep.append(vec)
                        want[t * B:(t + 1) * B, ..., dst_ch:dst_ch + sp[1]] = vec.cpu()
                        records.append(L.GatherEntry(vec.data_ptr(), 0, 0, sp[1], dst_ch))
                        dst_ch += sp[1]
                        continue
                    nch, stride, first = sp
                    plane = (torch.randint(-16, 17, (B, H, W, stride), generator=g).float() / 8).cuda()      # k/8: exact in every storage type
                    keep.append(plane)
                    want[t * B:(t + 1) * B, ..., dst_ch:dst_ch + nch] = plane.cpu()[..., first:first + nch]
                    records.append(L.GatherEntry(plane.data_ptr() + 4 * first, stride, H * W, nch, dst_ch))
                    dst_ch += nch
                used = dst_ch
            table = _table(records)
            dst = torch.full((T * B, H, W, ld), SENTINEL, dtype=tdt, device="cuda")
            L.check(lib.dd_gather_input(table.data_ptr(), T, len(specs), dst.data_ptr(), ld, c_pad, B, H, W, code, _stream()))
            torch.cuda.synchronize()
            got = dst.cpu()
            assert torch.equal(got[..., :c_pad].double(), want.double()), (order, dtype, T, (B, H, W))
            assert used < c_pad and not got[..., used:c_pad].any() and _untouched(got[..., c_pad:])


def test_gather_input_refusals():
    _need_gpu()
    lib = L.load()
    plane = torch.ones(1, 4, 4, 4, device="cuda")
    table = _table([L.GatherEntry(plane.data_ptr(), 4, 16, 4, 0)])
    for dtype, c_pad, ld in (("f32", 6, 8), ("f32", 8, 10), ("bf16", 12, 16), ("f16", 12, 16), ("bf16", 8, 12), ("f16", 8, 12), ("f32", 16, 8)):
        code, tdt, _ = DT[dtype]
        dst = torch.full((1, 4, 4, 16), SENTINEL, dtype=tdt, device="cuda")
        rc = lib.dd_gather_input(table.data_ptr(), 1, 1, dst.data_ptr(), ld, c_pad, 1, 4, 4, code, _stream())
        torch.cuda.synchronize()
        assert rc != 0 and lib.dd_last_error() and _untouched(dst), (dtype, c_pad, ld)


# ---------------------------------------------------------------------------------------------------------------- dd_assemble_input
class Assembly:
    """Device buffers and the entry table of one dd_assemble_input / dd_assemble_input_frames launch.  tuples: per tuple the entries of
    input_ref.network_input() with a `std` field ((ld_std, byte offset of the pointer from a 16-byte boundary) or None).  frame: (origins
    [(y, x)], frame_h, frame_w) -- then the src of a pass is a whole frame [frame_h, frame_w, cs]."""

    def __init__(self, tuples, c_pad, ld, shape, dtype, frame=None):
        self.lib, self.shape, self.dtype, self.c_pad, self.ld, self.frame = L.load(), shape, dtype, c_pad, ld, frame
        self.T, self.n_entries = len(tuples), len(tuples[0])
        B, H, W = shape
        self.keep, self.std, records = [], {}, []
        for t, entries in enumerate(tuples):
            for k, en in enumerate(entries):
                src = _dev(en["src"]) if en["nch"] > 0 else None
                self.keep.append(src)
                rec = L.AssembleEntry(src.data_ptr() if src is not None else None, en.get("cs", 0), en["kind"], _fp(en["fp"]) if en["kind"] == 0 else L.FeatureParams(),
                                      en["nch"], en["dst_ch"], None, 0)
                if en.get("std"):
                    ld_std, offset = en["std"]
                    buf = torch.full((B * H * W * ld_std + 8,), SENTINEL, dtype=torch.float32, device="cuda")
                    assert buf.data_ptr() % 16 == 0
                    self.std[(t, k)] = (buf, ld_std, offset // 4)
                    rec.std_out, rec.ld_std = buf.data_ptr() + offset, ld_std
                records.append(rec)
        self.table = _table(records)
        self.dst = torch.full((self.T * B, H, W, ld), SENTINEL, dtype=DT[dtype][1], device="cuda")
        if frame:
            self.origins = torch.tensor(frame[0], dtype=torch.int32).cuda()

    def run(self):
        B, H, W = self.shape
        args = (self.table.data_ptr(), self.T, self.n_entries, self.dst.data_ptr(), self.ld, self.c_pad, B, H, W, DT[self.dtype][0])
        if self.frame:
            L.check(self.lib.dd_assemble_input_frames(*args, self.origins.data_ptr(), self.frame[1], self.frame[2], _stream()))
        else:
            L.check(self.lib.dd_assemble_input(*args, _stream()))
        torch.cuda.synchronize()
        return self

    def std_out(self, t, k):
        """-> (the [B,H,W,ld_std] view, everything of the buffer around it)"""
        buf, ld_std, first = self.std[(t, k)]
        B, H, W = self.shape
        n = B * H * W * ld_std
        flat = buf.cpu()
        return flat[first:first + n].view(B, H, W, ld_std), torch.cat([flat[:first], flat[first + n:]])


def _compare_assembly(tag, a, tuples, refs):
    """The network input and every std_out of a finished launch against the reference; -> the worst ratios (dst, std_out)."""
    B = a.shape[0]
    worst = [0.0, 0.0]
    got = a.dst.cpu()
    assert _untouched(got[..., a.c_pad:]), "%s: channels [c_pad, ld) were written" % tag
    for t, (entries, (val, err, records)) in enumerate(zip(tuples, refs)):
        mine = got[t * B:(t + 1) * B, ..., :a.c_pad]
        used = max(en["dst_ch"] + en["nch"] for en in entries if en["nch"] > 0)
        assert not mine[..., used:].any(), "%s tuple %d: padding channels [%d, %d) are not zero" % (tag, t, used, a.c_pad)
        worst[0] = max(worst[0], _gated("%s tuple %d" % (tag, t), mine, val, err, a.dtype))
        for k, en in enumerate(entries):
            if en["kind"] != 0:      # vectors and planes hold values every storage type represents: exact
                assert torch.equal(mine[..., en["dst_ch"]:en["dst_ch"] + en["nch"]].double(), val[..., en["dst_ch"]:en["dst_ch"] + en["nch"]]), (tag, t, k)
            if (t, k) not in a.std:
                continue
            rec, erec = records[k]
            view, around = a.std_out(t, k)
            n = min(rec.shape[3], view.shape[3])
            worst[1] = max(worst[1], _gated("%s tuple %d std_out of entry %d (ld_std %d)" % (tag, t, k, view.shape[3]), view[..., :n], rec[..., :n], erec[..., :n]))
            assert _untouched(view[..., n:]) and _untouched(around), "%s tuple %d entry %d: std_out written past min(3 + nv, ld_std)" % (tag, t, k)
    return worst


@pytest.mark.parametrize("dtype", list(DT))
@pytest.mark.parametrize("name", list(R.TABLES))
def test_assemble_input_parity(name, dtype):
    _need_gpu()
    _, c_pad, ld = R.TABLES[name]
    worst = [0.0, 0.0]
    for T in (1, 3):
        for shape in R.SHAPES:
            tuples = R.assemble_entries(name, T, shape)
            a = Assembly(tuples, c_pad, ld, shape, dtype).run()
            w = _compare_assembly("assemble %s %s T %d %dx%dx%d" % ((name, dtype, T) + shape), a, tuples, R.assemble_reference(name, T, shape))
            worst = [max(x, y) for x, y in zip(worst, w)]
    print("dd_assemble_input %s %s: worst error / gate %.3f (network input), %.3f (std_out)" % (name, dtype, worst[0], worst[1]))


@pytest.mark.parametrize("dtype", list(DT))
def test_assemble_input_without_std_out_and_twice(dtype):
    """std_out == NULL on every entry writes the same network input; two launches give the same bits."""
    _need_gpu()
    for name in R.TABLES:
        _, c_pad, ld = R.TABLES[name]
        shape = (2, 17, 33)
        tuples = R.assemble_entries(name, 3, shape)
        a, b = Assembly(tuples, c_pad, ld, shape, dtype).run(), Assembly(tuples, c_pad, ld, shape, dtype).run()
        assert torch.equal(a.dst, b.dst), name
        for key in a.std:
            assert torch.equal(a.std[key][0], b.std[key][0]), (name, key)
        bare = Assembly([[dict(en, std=None) for en in entries] for entries in tuples], c_pad, ld, shape, dtype).run()
        assert not bare.std and torch.equal(bare.dst, a.dst), name


def test_assemble_input_refusals():
    _need_gpu()
    lib = L.load()
    shape = (1, 5, 7)
    tuples = R.assemble_entries("single", 1, shape)
    for dtype, c_pad, ld in (("f32", 6, 8), ("bf16", 12, 16), ("f16", 8, 12), ("f32", 16, 8), ("f32", 0, 8)):
        a = Assembly(tuples, c_pad, 16, shape, dtype)
        rc = lib.dd_assemble_input(a.table.data_ptr(), 1, 1, a.dst.data_ptr(), ld, c_pad, *shape, DT[dtype][0], _stream())
        torch.cuda.synchronize()
        assert rc != 0 and lib.dd_last_error() and _untouched(a.dst) and _untouched(a.std[(0, 0)][0]), (dtype, c_pad, ld)


# ---------------------------------------------------------------------------------------------------------------- dd_assemble_input_frames
FRAME_H, FRAME_W = 37, 53
FRAME_SPECS = [R.P("radiance", 3, "default", (4, 0)), R.P("signed", 1, "uniform_absolute", (3, 0)), R.P("dyadic", 3, "neighbor_absolute_per_channel", (8, 4)),
               R.K2(2), R.P("signed_log1p", 3, "before_standardization", (4, 4)), R.V(2)]      # 4 + 4 + 6 + 2 + 4 + 2 = 22 of c_pad 24
# (H, W, origins): the top-left and the bottom-right corner, odd offsets, and two windows that overlap
WINDOWS = [(16, 16, [(0, 0), (FRAME_H - 16, FRAME_W - 16), (3, 5), (7, 11), (21, 1)]),
           (17, 20, [(0, 0), (FRAME_H - 17, FRAME_W - 20), (5, 7), (9, 13), (1, 33)])]


def _frame_entries(B, H, W, outside=None, window=None):
    """The entries of FRAME_SPECS with whole frames as the passes' src.  outside: the value of every frame pixel that is not in `window`."""
    entries, dst = [], 0
    for k, sp in enumerate(FRAME_SPECS):
        g = torch.Generator().manual_seed(900 + k)
        if sp["kind"] == 0:
            fp = R.feature_params(sp["family"], sp["branch"])
            frame = R.make_values(sp["family"], 1, FRAME_H, FRAME_W, sp["cs"], 900 + k)[0]
            if outside is not None:
                (oy, ox), inner = window, frame
                frame = torch.full_like(inner, outside)
                frame[oy:oy + H, ox:ox + W] = inner[oy:oy + H, ox:ox + W]
            en = dict(kind=0, src=frame, cs=sp["cs"], fp=fp, nch=3 + R.n_variance_channels(fp, sp["cs"]), dst_ch=dst, std=sp["std"])
        elif sp["kind"] == 1:
            en = dict(kind=1, src=torch.randint(-16, 17, (sp["nch"],), generator=g).double() / 8, nch=sp["nch"], dst_ch=dst, std=None)
        else:
            en = dict(kind=2, src=torch.randint(-16, 17, (B, H, W, sp["nch"]), generator=g).double() / 8, nch=sp["nch"], dst_ch=dst, std=None)
        dst += en["nch"]
        entries.append(en)
    return entries


def _cut(entries, origins, H, W):
    """The same entries with every pass's windows cut from its frame by slicing: what dd_assemble_input takes."""
    return [dict(en, src=torch.stack([en["src"][oy:oy + H, ox:ox + W] for oy, ox in origins])) if en["kind"] == 0 else en for en in entries]


@pytest.mark.parametrize("dtype", ["f32", "bf16"])
@pytest.mark.parametrize("H,W,origins", WINDOWS, ids=["16x16", "17x20"])
def test_assemble_input_frames_is_bit_identical_to_cut_windows(H, W, origins, dtype):
    _need_gpu()
    B = len(origins)
    entries = _frame_entries(B, H, W)
    cut = _cut(entries, origins, H, W)
    frames = Assembly([entries], 24, 32, (B, H, W), dtype, frame=(origins, FRAME_H, FRAME_W)).run()
    tiles = Assembly([cut], 24, 32, (B, H, W), dtype).run()
    assert torch.equal(frames.dst, tiles.dst)
    for key in tiles.std:
        assert torch.equal(frames.std[key][0], tiles.std[key][0]), key
    _compare_assembly("frames %dx%d %s" % (H, W, dtype), frames, [cut], [R.network_input(cut, B, H, W, 24)])
    # a frame that is 1e6 everywhere outside the window: a neighbourhood mirrored at the FRAME's border, or not mirrored at all, reads it
    for origin in origins:
        lone = _frame_entries(1, H, W, outside=1e6, window=origin)
        lone_cut = _cut(lone, [origin], H, W)
        a = Assembly([lone], 24, 32, (1, H, W), dtype, frame=([origin], FRAME_H, FRAME_W)).run()
        b = Assembly([lone_cut], 24, 32, (1, H, W), dtype).run()
        assert torch.equal(a.dst, b.dst), origin
        for key in b.std:
            assert torch.equal(a.std[key][0], b.std[key][0]), (origin, key)
        _compare_assembly("frames %dx%d %s, 1e6 outside the window at %s" % (H, W, dtype, origin), a, [lone_cut], [R.network_input(lone_cut, 1, H, W, 24)])


def test_assemble_input_frames_refusals():
    _need_gpu()
    lib = L.load()
    H, W, origins = 16, 16, [(0, 0)]
    a = Assembly([_frame_entries(1, H, W)], 24, 32, (1, H, W), "f32", frame=(origins, FRAME_H, FRAME_W))
    args = (a.table.data_ptr(), 1, a.n_entries, a.dst.data_ptr(), 32, 24, 1)
    for h, w, org, fh, fw in ((16, 16, None, FRAME_H, FRAME_W), (16, 16, a.origins.data_ptr(), 15, FRAME_W), (16, 16, a.origins.data_ptr(), FRAME_H, 15),
                              (FRAME_H + 1, 16, a.origins.data_ptr(), FRAME_H, FRAME_W), (16, FRAME_W + 1, a.origins.data_ptr(), FRAME_H, FRAME_W)):
        rc = lib.dd_assemble_input_frames(*args, h, w, L.DD_F32, org, fh, fw, _stream())
        torch.cuda.synchronize()
        assert rc != 0 and lib.dd_last_error() and _untouched(a.dst), (h, w, fh, fw)
        assert all(_untouched(buf) for buf, _, _ in a.std.values())


# ---------------------------------------------------------------------------------------------------------------- unfused against fused
@pytest.mark.parametrize("dtype", ["f32", "bf16"])
@pytest.mark.parametrize("name", ["usual", "odd", "late"])
def test_unfused_path_and_fused_path_meet_the_same_reference(name, dtype):
    """dd_prepare_feature + dd_gather_input (DD_FUSE_INPUT=0) and dd_assemble_input on one table: both within the gate of the same reference.
    Their mutual difference is printed, not gated: the unfused path divides where the fused one multiplies by a reciprocal."""
    _need_gpu()
    lib = L.load()
    _, c_pad, ld = R.TABLES[name]
    for shape in ((2, 17, 33), (1, 5, 50)):
        B, H, W = shape
        (entries,), ((val, err, _),) = R.assemble_entries(name, 1, shape), R.assemble_reference(name, 1, shape)
        keep, records = [], []
        for en in entries:
            if en["nch"] <= 0:
                records.append(L.GatherEntry(None, 0, 0, 0, en["dst_ch"]))
                continue
            src = _dev(en["src"])
            if en["kind"] == 0:
                plane = torch.full((B, H, W, 8), SENTINEL, dtype=torch.float32, device="cuda")
                L.check(lib.dd_prepare_feature(src.data_ptr(), en["cs"], plane.data_ptr(), 8, C.byref(_fp(en["fp"])), B, H, W, _stream()))
                records.append(L.GatherEntry(plane.data_ptr(), 8, H * W, en["nch"], en["dst_ch"]))
                keep.append(plane)
            elif en["kind"] == 1:
                records.append(L.GatherEntry(src.data_ptr(), 0, 0, en["nch"], en["dst_ch"]))
            else:
                records.append(L.GatherEntry(src.data_ptr(), en["nch"], H * W, en["nch"], en["dst_ch"]))
            keep.append(src)
        table = _table(records)
        dst = torch.full((B, H, W, ld), SENTINEL, dtype=DT[dtype][1], device="cuda")
        L.check(lib.dd_gather_input(table.data_ptr(), 1, len(records), dst.data_ptr(), ld, c_pad, B, H, W, DT[dtype][0], _stream()))
        torch.cuda.synchronize()
        tag = "%s %s %dx%dx%d" % ((name, dtype) + shape)
        _gated("unfused " + tag, dst.cpu()[..., :c_pad], val, err, dtype)
        fused = Assembly([entries], c_pad, ld, shape, dtype).run()
        _gated("fused " + tag, fused.dst.cpu()[..., :c_pad], val, err, dtype)
        assert _untouched(dst.cpu()[..., c_pad:])
        d = (dst.double() - fused.dst.double()).abs().cpu()[..., :c_pad]
        print("unfused vs fused %s: max |difference| %.3e, rel-L2 %.3e, %d of %d elements differ" % (
            tag, float(d.max()), rel_l2(dst[..., :c_pad], fused.dst[..., :c_pad]), int((d > 0).sum()), d.numel()))
