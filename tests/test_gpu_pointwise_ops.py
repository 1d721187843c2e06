"""-m gpu: the single-pass kernels of csrc/dd_pointwise.hip, op by op through the C ABI, against the float64 reference, the inputs
and the gates of tests/pointwise_ref.py: dd_maxpool_fwd / dd_maxpool_bwd, dd_masked_add, dd_zero_stuff / dd_zero_unstuff, dd_space_to_depth2,
dd_convert_channels, dd_compose_pack / dd_compose_blend_fwd / dd_compose_blend_bwd / dd_compose_unpack_bwd, dd_colsum / dd_colsum_segments,
dd_extract_tiles and dd_stitch.

Selection and copies are compared bit for bit (padding exactly +0), integer-valued cases of the adding kernels too (tests/test_pointwise_ref.py
proves for these very inputs that every fp32 sum is exact in any order), real-valued ones element by element against
r_T(ref) + (n - 1) 2^-24 sum |terms|; what depends on the blend's sigmoid and the real-valued column sums take gpu_util.ACC32 / ROUND.
Operands and outputs are channel views inside wider sentinel-filled rows (conv_ops_util.View / Guarded): neighbours and guard words must come
back untouched, inputs byte for byte.  Every comparison is recorded (gpu_util.gate / check); a bit-equal gate records the number of differing
elements against a bound of 0, the worst case of a loop under its name."""
import ctypes as C

import pytest
import torch

import pointwise_ref as R
from conv_ops_util import DT, SENTINEL, G, Guarded, View, stream
from deepdenoiser_amd import _lib as L
from gpu_util import ACC32, ROUND, check, gate

pytestmark = pytest.mark.gpu
assert SENTINEL == R.SENTINEL
ESZ = {"f32": 4, "bf16": 2, "f16": 2}
INT = {torch.float32: torch.int32, torch.bfloat16: torch.int16, torch.float16: torch.int16}
PAD0 = 7.0      # what a pad channel holds before a kernel that must zero it


def _need_gpu():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")


def _sync():
    torch.cuda.synchronize()


def _bits_differ(got, ref64):
    """Elements of `got` (storage type) whose bit pattern is not that of the float64 reference stored in that type (-0 is not +0)."""
    got = got.detach().cpu().contiguous()
    want = ref64.to(got.dtype).contiguous()
    assert tuple(got.shape) == tuple(want.shape), (tuple(got.shape), tuple(want.shape))
    return int((got.view(INT[got.dtype]) != want.view(INT[got.dtype])).sum())


def _off16(dtype, extra):
    """First channel of a view inside a row with `extra` spare channels: 16 bytes in when there is room."""
    return 0 if extra == 0 else 16 // ESZ[dtype]


def _inside(v):
    """The storage-type values of a View, on the host."""
    return v.buf[..., v.off:v.off + v.C].cpu()


def _f32_rows(vals, ld):
    """[..., 3] fp32 values as the leading channels of sentinel-filled rows of length ld, on the device."""
    t = torch.full(tuple(vals.shape[:-1]) + (ld,), SENTINEL, dtype=torch.float32, device="cuda")
    t[..., :vals.shape[-1]] = vals.float().cuda()
    return t


class Tally:
    """The worst value of every named comparison of a test, recorded once each (gpu_util.gate) when the test ends."""

    def __init__(self):
        self.worst = {}

    def put(self, name, value, bound, case):
        if name not in self.worst or value > self.worst[name][0]:
            self.worst[name] = (value, bound, case)

    def exact(self, name, case, got, ref64):
        self.put(name + " (differing elements)", float(_bits_differ(got, ref64)), 0.0, case)

    def bounded(self, name, case, got, ref64, bound):
        got = got.detach().cpu().to(torch.float64)
        assert bool(torch.isfinite(got).all()), (name, case)
        self.put(name + " (worst error / bound)", R.worst_ratio(got, ref64, bound), 1.0, case)

    def true(self, name, case, ok):
        self.put(name + " (violations)", 0.0 if ok else 1.0, 0.0, case)

    def flush(self):
        for name, (value, bound, case) in sorted(self.worst.items()):
            print("%-72s %.3f <= %g   [worst: %s]" % (name, value, bound, case))
        for name, (value, bound, case) in sorted(self.worst.items()):
            gate("%s [worst: %s]" % (name, case), value, bound)


# ---------------------------------------------------------------------------------------------------------------- max pooling
def _idx_plane(n, values=None):
    """n bytes of argmax plane between 16 guard bytes on either side (0xAB; the plane itself 0xEE or `values`)."""
    buf = torch.full((n + 32,), 0xAB, dtype=torch.uint8, device="cuda")
    buf[16:16 + n] = 0xEE if values is None else values.reshape(-1).to(torch.uint8).cuda()
    return buf


def _idx_guards_intact(buf):
    return bool((buf[:16] == 0xAB).all()) and bool((buf[-16:] == 0xAB).all())


@pytest.mark.parametrize("geometry", R.POOL_GEOMETRIES, ids=["pool%d_stride%d_%dx%d" % g for g in R.POOL_GEOMETRIES])
@pytest.mark.parametrize("dtype", R.DTYPES)
def test_maxpool_forward_then_backward_through_its_index_plane(dtype, geometry):
    """y bit-equal, the uint8 plane byte-equal to the reference codes (first maximum in row-major window order, 255 under relu_mask where the
    maximum is not > 0), dx from the forward's own plane AND from the reference plane (a forward error cannot mask a backward one)."""
    _need_gpu()
    lib, t = L.load(), Tally()
    pool, stride, H, W = geometry
    per16, code = R.PER16[dtype], DT[dtype][0]
    full = {}      # the reference at full size, once per switch combination; a case compares its leading images / channels
    for c in R.pool_cases(dtype, geometry):
        B, Cc, ld = c["B"], c["C"], c["ld"]
        case = "%s B%d C%d ld%d relu_mask%d mask_%s acc%d" % (c["kind"], B, Cc, ld, c["relu_mask"], c["mask"], c["acc"])
        off = _off16(dtype, ld - Cc)
        sw = (c["relu_mask"], c["mask"], c["acc"], c["kind"])
        if sw not in full:
            full[sw] = R.pool_reference(dtype, geometry, *sw)[:4]
        x, dy, old, m = (v[:B, ..., :Cc] for v in R.pool_inputs(dtype, geometry, c["relu_mask"], c["kind"]))
        y_ref, codes_ref, dx_ref, bound = (v[:B, ..., :Cc] for v in full[sw])
        OH, OW = y_ref.shape[1:3]
        xv = View((B, H, W), Cc, Cc, ld, off, dtype, x)
        yv = View((B, OH, OW), Cc, Cc, ld, off, dtype)
        n_idx = B * OH * OW * Cc
        idx = _idx_plane(n_idx)
        L.check(lib.dd_maxpool_fwd(xv.ptr, ld, yv.ptr, ld, idx.data_ptr() + 16, Cc, B, H, W, pool, stride, c["relu_mask"], code, stream()))
        _sync()
        t.exact("maxpool_fwd y", case, _inside(yv), y_ref)
        t.put("maxpool_fwd index plane (differing bytes)", float((idx[16:16 + n_idx].cpu().long() != codes_ref.reshape(-1)).sum()), 0.0, case)
        t.true("maxpool_fwd leaves neighbours, guards and x alone", case, yv.neighbours_intact() and _idx_guards_intact(idx) and xv.unchanged())
        for which, plane in (("own", idx), ("reference", _idx_plane(n_idx, codes_ref))):
            plane_before = plane.clone()
            dyv = View((B, OH, OW), Cc, Cc, ld, off, dtype, dy)
            dxv = View((B, H, W), Cc, Cc, ld, off, dtype, old if c["acc"] else None)
            mv = None
            if c["mask"] == "input":
                mptr, ldm = xv.ptr, ld
            elif c["mask"] == "unrelated":
                mv = View((B, H, W), Cc, Cc, Cc + 2 * per16, per16, dtype, m)
                mptr, ldm = mv.ptr, mv.ld
            else:
                mptr, ldm = None, 0
            L.check(lib.dd_maxpool_bwd(dyv.ptr, ld, plane.data_ptr() + 16, dxv.ptr, ld, mptr, ldm, Cc, B, H, W, pool, stride, c["acc"], code, stream()))
            _sync()
            got = _inside(dxv)
            if c["kind"] == "int":
                t.exact("maxpool_bwd dx, integer-valued, %s plane" % which, case, got, dx_ref)
            else:
                t.bounded("maxpool_bwd dx, real-valued, %s plane" % which, case, got, dx_ref, bound)
            t.true("maxpool_bwd leaves neighbours, dy, the plane and the mask alone", case, dxv.neighbours_intact() and dyv.unchanged()
                   and torch.equal(plane, plane_before) and xv.unchanged() and (mv is None or mv.unchanged()))
            if c["kind"] == "int" and c["mask"] == "none" and which == "reference":
                base = old if c["acc"] else torch.zeros_like(old)
                if c["relu_mask"]:      # an all-zero plane: every window's maximum is 0, not > 0 -> no gradient although dy is never 0 there
                    t.true("relu_mask = 1: a non-positive window passes no gradient", case, torch.equal(got[..., R.CH_ZERO].double(), base[..., R.CH_ZERO]))
                else:                   # an all-negative plane: every window passes its (never zero) gradient to a negative maximum
                    t.true("relu_mask = 0: a negative maximum passes its gradient", case,
                           float((got[..., R.CH_NEG].double() - base[..., R.CH_NEG]).abs().sum()) > 0 and int(codes_ref[..., R.CH_NEG].max()) < 255)
    t.flush()


@pytest.mark.parametrize("dtype", R.DTYPES)
def test_maxpool_forward_without_an_index_plane(dtype):
    """idx = NULL (inference graphs): the same y, nothing else written."""
    _need_gpu()
    lib, t = L.load(), Tally()
    for geometry in (R.POOL_GEOMETRIES[1], R.POOL_GEOMETRIES[6]):
        pool, stride, H, W = geometry
        x = R.pool_inputs(dtype, geometry, 1, "real")[0]
        y_ref = R.pool_reference(dtype, geometry, 1, "none", 0, "real")[0]
        B, _, _, Cc = x.shape
        ld = Cc + 2 * R.PER16[dtype]
        off = _off16(dtype, ld - Cc)
        xv, yv = View((B, H, W), Cc, Cc, ld, off, dtype, x), View(tuple(y_ref.shape[:3]), Cc, Cc, ld, off, dtype)
        L.check(lib.dd_maxpool_fwd(xv.ptr, ld, yv.ptr, ld, None, Cc, B, H, W, pool, stride, 1, DT[dtype][0], stream()))
        _sync()
        t.exact("maxpool_fwd y, idx = NULL", str(geometry), _inside(yv), y_ref)
        t.true("maxpool_fwd, idx = NULL, leaves neighbours and x alone", str(geometry), yv.neighbours_intact() and xv.unchanged())
    t.flush()


# ---------------------------------------------------------------------------------------------------------------- executor helpers
@pytest.mark.parametrize("dtype", R.DTYPES)
def test_masked_add(dtype):
    _need_gpu()
    lib, t = L.load(), Tally()
    code = DT[dtype][0]
    for Cc in R.MASKED_ADD_C:
        for extra in R.MASKED_ADD_EXTRA:
            ld, off = Cc + extra, _off16(dtype, extra)
            for npix in R.MASKED_ADD_NPIX:      # 257 pixels x (C / 4) threads: the last workgroup is ragged
                for kind in R.POOL_KINDS:
                    src, mask, old = R.masked_add_inputs(dtype, Cc, npix, kind)
                    for use_mask in (0, 1):
                        for acc in (0, 1):
                            case = "%s C%d ld%d npix%d mask%d acc%d" % (kind, Cc, ld, npix, use_mask, acc)
                            ref, bound, _ = R.masked_add(src, mask if use_mask else None, old if acc else None, dtype)
                            sv = View((1, 1, npix), Cc, Cc, ld, off, dtype, src)
                            mv = View((1, 1, npix), Cc, Cc, Cc + 8, _off16(dtype, 8), dtype, mask)      # a row length of its own
                            dv = View((1, 1, npix), Cc, Cc, ld, off, dtype, old if acc else None)
                            L.check(lib.dd_masked_add(dv.ptr, ld, sv.ptr, ld, mv.ptr if use_mask else None, mv.ld if use_mask else 0, Cc, npix, acc, code, stream()))
                            _sync()
                            if kind == "int" or not acc:
                                t.exact("masked_add, %s" % ("integer-valued" if kind == "int" else "no accumulate"), case, _inside(dv), ref)
                            else:
                                t.bounded("masked_add, real-valued accumulate", case, _inside(dv), ref, bound)
                            t.true("masked_add leaves neighbours, src and mask alone", case, dv.neighbours_intact() and sv.unchanged() and mv.unchanged())
    # dst == src: the in-place ReLU backward of engine.Graph (the gradient masked by the layer's own output)
    src, mask, _ = R.masked_add_inputs(dtype, 12, 257, "real")
    gv, mv = View((1, 1, 257), 12, 12, 20, _off16(dtype, 8), dtype, src), View((1, 1, 257), 12, 12, 12, 0, dtype, mask)
    L.check(lib.dd_masked_add(gv.ptr, 20, gv.ptr, 20, mv.ptr, 12, 12, 257, 0, code, stream()))
    _sync()
    t.exact("masked_add in place (dst == src)", "C12 ld20 npix257", _inside(gv), R.masked_add(src, mask, None, dtype)[0])
    t.true("masked_add in place leaves neighbours and mask alone", "C12 ld20 npix257", gv.neighbours_intact() and mv.unchanged())
    t.flush()


@pytest.mark.parametrize("dtype", R.DTYPES)
def test_zero_stuff_and_unstuff(dtype):
    _need_gpu()
    lib, t = L.load(), Tally()
    code, Cc = DT[dtype][0], R.STUFF_C
    for shape in R.STUFF_SHAPES:
        B, H, W = shape
        for extra in (0, 8):
            ld, off = Cc + extra, _off16(dtype, extra)
            for kind in R.POOL_KINDS:
                x, dy, mask, old = R.stuff_inputs(dtype, shape, kind)
                case = "%s %dx%dx%d ld%d" % (kind, B, H, W, ld)
                xv, yv = View((B, H, W), Cc, Cc, ld, off, dtype, x), View((B, 2 * H, 2 * W), Cc, Cc, ld, off, dtype)
                L.check(lib.dd_zero_stuff(xv.ptr, ld, yv.ptr, ld, Cc, B, H, W, code, stream()))
                _sync()
                got = _inside(yv)
                t.exact("zero_stuff", case, got, R.zero_stuff(x))
                for py, px in ((0, 0), (0, 1), (1, 0)):      # the three zero parities: every bit clear
                    t.true("zero_stuff: parity (%d, %d) exactly +0" % (py, px), case, not bool(got[:, py::2, px::2].contiguous().view(INT[got.dtype]).any()))
                t.true("zero_stuff leaves neighbours and x alone", case, yv.neighbours_intact() and xv.unchanged())
                for use_mask in (0, 1):
                    for acc in (0, 1):
                        sub = "%s mask%d acc%d" % (case, use_mask, acc)
                        ref, bound, _ = R.zero_unstuff(dy, mask if use_mask else None, old if acc else None, dtype)
                        gv = View((B, 2 * H, 2 * W), Cc, Cc, ld, off, dtype, dy)      # the three other parities hold the sentinel: it must not leak
                        mv = View((B, H, W), Cc, Cc, Cc + 8, _off16(dtype, 8), dtype, mask)
                        dv = View((B, H, W), Cc, Cc, ld, off, dtype, old if acc else None)
                        L.check(lib.dd_zero_unstuff(gv.ptr, ld, dv.ptr, ld, mv.ptr if use_mask else None, mv.ld if use_mask else 0, Cc, B, H, W, acc, code, stream()))
                        _sync()
                        if kind == "int" or not acc:
                            t.exact("zero_unstuff, %s" % ("integer-valued" if kind == "int" else "no accumulate"), sub, _inside(dv), ref)
                        else:
                            t.bounded("zero_unstuff, real-valued accumulate", sub, _inside(dv), ref, bound)
                        t.true("zero_unstuff leaves neighbours, dy and mask alone", sub, dv.neighbours_intact() and gv.unchanged() and mv.unchanged())
    t.flush()


@pytest.mark.parametrize("dtype", R.DTYPES)
def test_space_to_depth2(dtype):
    """ldy is the four-channel group that holds channel C - 1 and no more: the row's end is the allocation's end."""
    _need_gpu()
    lib, t = L.load(), Tally()
    B, H, W = R.S2D_SHAPE
    for Cc, cp in R.S2D_CHANNELS:
        y = R.s2d_input(dtype, Cc)
        ldy = y.shape[3]
        assert ldy == (Cc + 3) // 4 * 4
        ref = R.space_to_depth2(y, Cc, cp)
        for extra in (0, 8):
            lds, off = 4 * cp + extra, _off16(dtype, extra)
            case = "C%d cp%d ldy%d lds%d" % (Cc, cp, ldy, lds)
            yv = View((B, 2 * H, 2 * W), ldy, ldy, ldy, 0, dtype, y)
            sv = View((B, H, W), 4 * cp, 4 * cp, lds, off, dtype)
            L.check(lib.dd_space_to_depth2(yv.ptr, ldy, sv.ptr, lds, Cc, cp, B, H, W, DT[dtype][0], stream()))
            _sync()
            got = _inside(sv)
            t.exact("space_to_depth2", case, got, ref)
            pads = torch.cat([got[..., p * cp + Cc:(p + 1) * cp] for p in range(4)], dim=-1)
            t.true("space_to_depth2: channels C <= c < cp of every plane exactly +0", case, not bool(pads.contiguous().view(INT[got.dtype]).any()))
            t.true("space_to_depth2 leaves neighbours and y alone", case, sv.neighbours_intact() and yv.unchanged())
    t.flush()


@pytest.mark.parametrize("dst_dtype", R.DTYPES)
@pytest.mark.parametrize("src_dtype", R.DTYPES)
def test_convert_channels(src_dtype, dst_dtype):
    """Channels [3 j, 3 j + nch) of a 16-channel logits row into channels [3 j', ...) of another (Program._direct and its backward), rounded to
    nearest even; pads up to dst_pad +0, everything else untouched."""
    _need_gpu()
    lib, t = L.load(), Tally()
    npix = R.CONVERT_NPIX
    for nch in R.CONVERT_NCH:
        vals = R.convert_input(src_dtype, nch)
        for k, dst_pad in enumerate((nch, 4, 8)):
            for j in range(3):
                jd = (j + k) % 3
                case = "nch%d dst_pad%d src channel %d dst channel %d" % (nch, dst_pad, 3 * j, 3 * jd)
                ref = R.convert_channels(vals[:, 3 * j:3 * j + nch], nch, dst_pad, dst_dtype)
                sv = View((npix,), 9, 9, 16, 0, src_dtype, vals)
                dv = View((npix,), nch, max(nch, dst_pad), 16, 3 * jd, dst_dtype, pad=PAD0)
                L.check(lib.dd_convert_channels(sv.ptr + 3 * j * ESZ[src_dtype], DT[src_dtype][0], 16, dv.ptr, DT[dst_dtype][0], 16, nch, dst_pad, npix, stream()))
                _sync()
                t.exact("convert_channels %s -> %s" % (src_dtype, dst_dtype), case, dv.buf[:, dv.off:dv.off + dv.cv].cpu(), ref)
                t.true("convert_channels leaves neighbours and src alone", case, dv.neighbours_intact() and sv.unchanged())
    t.flush()


# ---------------------------------------------------------------------------------------------------------------- layer-wise compose path
@pytest.mark.parametrize("shape", R.COMPOSE_SHAPES, ids=["%dx%dx%d" % s for s in R.COMPOSE_SHAPES])
@pytest.mark.parametrize("dtype", R.DTYPES)
def test_compose_pack_and_unpack_bwd(dtype, shape):
    _need_gpu()
    lib, t = L.load(), Tally()
    N, H, W = shape
    code = DT[dtype][0]
    for ld3 in (3, 4):
        for kind in R.POOL_KINDS:
            small, fine, _, ds_old, df_old, _, dnet = R.compose_inputs(dtype, shape, kind)
            sm, fn = _f32_rows(small, ld3), _f32_rows(fine, ld3)
            for c_pad, ld in ((6, 8), (8, 8), (6, 16), (8, 16)):
                case = "%s fp32 ld%d c_pad%d ld%d" % (kind, ld3, c_pad, ld)
                pv = View((N, H, W), 6, c_pad, ld, 0, dtype, pad=PAD0)
                L.check(lib.dd_compose_pack(sm.data_ptr(), ld3, fn.data_ptr(), ld3, pv.ptr, ld, c_pad, N, H, W, code, stream()))
                _sync()
                t.exact("compose_pack", case, pv.buf[..., :c_pad].cpu(), R.compose_pack(small, fine, c_pad, dtype))
                t.true("compose_pack leaves neighbours, small and fine alone", case, pv.neighbours_intact() and torch.equal(sm, _f32_rows(small, ld3))
                       and torch.equal(fn, _f32_rows(fine, ld3)))
            for ld in (8, 16):
                case = "%s fp32 ld%d dnet ld%d" % (kind, ld3, ld)
                nv = View((N, H, W), 6, 6, ld, 0, dtype, dnet)
                dsm, dfn = _f32_rows(ds_old, ld3), _f32_rows(df_old, ld3)
                L.check(lib.dd_compose_unpack_bwd(nv.ptr, ld, dsm.data_ptr(), ld3, dfn.data_ptr(), ld3, N, H, W, code, stream()))
                _sync()
                (ds, bs, _), (df, bf, _) = R.compose_unpack_bwd(dnet, ds_old, df_old)
                if kind == "int":
                    t.exact("compose_unpack_bwd d_small, integer-valued", case, dsm[..., :3], ds)
                    t.exact("compose_unpack_bwd d_fine, integer-valued", case, dfn[..., :3], df)
                else:
                    t.bounded("compose_unpack_bwd d_small, real-valued", case, dsm[..., :3], ds, bs)
                    t.bounded("compose_unpack_bwd d_fine, real-valued", case, dfn[..., :3], df, bf)
                t.true("compose_unpack_bwd leaves the fourth channel and dnet alone", case, nv.unchanged() and bool((dsm[..., 3:] == SENTINEL).all())
                       and bool((dfn[..., 3:] == SENTINEL).all()))
    t.flush()


@pytest.mark.parametrize("shape", R.COMPOSE_SHAPES, ids=["%dx%dx%d" % s for s in R.COMPOSE_SHAPES])
@pytest.mark.parametrize("dtype", R.DTYPES)
def test_compose_blend_forward_and_backward(dtype, shape):
    """out, d_small, d_fine (fp32) by gpu_util.ACC32, dwl (storage type) by gpu_util.ROUND: they depend on the device's fast exponential."""
    _need_gpu()
    lib, t = L.load(), Tally()
    N, H, W = shape
    code = DT[dtype][0]
    small, fine, dout, ds_old, _, wl, _ = R.compose_inputs(dtype, shape)
    for ld3 in (3, 4):
        for ldw in (1, 8):
            case = "fp32 ld%d wl ld%d" % (ld3, ldw)
            sm, fn, go = _f32_rows(small, ld3), _f32_rows(fine, ld3), _f32_rows(dout, ld3)
            wv = View((N, H, W), 1, 1, ldw, 0, dtype, wl)
            out = torch.full((N, H, W, ld3), SENTINEL, dtype=torch.float32, device="cuda")
            L.check(lib.dd_compose_blend_fwd(sm.data_ptr(), ld3, fn.data_ptr(), ld3, wv.ptr, ldw, out.data_ptr(), ld3, N, H, W, code, stream()))
            _sync()
            check("compose_blend_fwd out, " + case, out[..., :3], R.compose_blend_fwd(small, fine, wl), ACC32[dtype])
            t.true("compose_blend_fwd leaves the fourth channel and its inputs alone", case, bool((out[..., 3:] == SENTINEL).all()) and wv.unchanged()
                   and torch.equal(sm, _f32_rows(small, ld3)) and torch.equal(fn, _f32_rows(fine, ld3)))
            for dw_pad in (1, 8):
                for acc in (0, 1):
                    sub = "%s dw_pad%d accumulate_small%d" % (case, dw_pad, acc)
                    lddw = 8 if dw_pad == 8 or ldw == 8 else 1
                    dsm = _f32_rows(ds_old, ld3)      # non-zero either way: overwritten (0) or added to (1)
                    dfn = torch.full((N, H, W, ld3), SENTINEL, dtype=torch.float32, device="cuda")
                    dv = View((N, H, W), 1, dw_pad, lddw, 0, dtype, pad=PAD0)
                    L.check(lib.dd_compose_blend_bwd(go.data_ptr(), ld3, sm.data_ptr(), ld3, fn.data_ptr(), ld3, wv.ptr, ldw, dsm.data_ptr(), ld3, acc,
                                                     dfn.data_ptr(), ld3, dv.ptr, lddw, dw_pad, N, H, W, code, stream()))
                    _sync()
                    d_small, d_fine, dwl = R.compose_blend_bwd(dout, small, fine, wl, ds_old, acc, dw_pad, dtype)
                    check("compose_blend_bwd d_small, " + sub, dsm[..., :3], d_small, ACC32[dtype])
                    check("compose_blend_bwd d_fine, " + sub, dfn[..., :3], d_fine, ACC32[dtype])
                    check("compose_blend_bwd dwl, " + sub, dv.buf[..., :1], dwl[..., :1], ROUND[dtype])
                    t.exact("compose_blend_bwd: pad channels of dwl +0", sub, dv.buf[..., 1:dw_pad].cpu(), dwl[..., 1:dw_pad])
                    # the ReLU gate: dwl is exactly +0 wherever wl is not > 0
                    t.true("compose_blend_bwd: dwl exactly 0 where wl = 0", sub, not bool(dv.buf[..., :1].cpu()[wl == 0].view(INT[DT[dtype][1]]).any()))
                    t.true("compose_blend_bwd leaves neighbours, fourth channels and inputs alone", sub, dv.neighbours_intact() and wv.unchanged()
                           and bool((dsm[..., 3:] == SENTINEL).all()) and bool((dfn[..., 3:] == SENTINEL).all()) and torch.equal(go, _f32_rows(dout, ld3))
                           and torch.equal(sm, _f32_rows(small, ld3)) and torch.equal(fn, _f32_rows(fine, ld3)))
    t.flush()


# ---------------------------------------------------------------------------------------------------------------- column sums
def _colsum_case(lib, t, what, dtype, c, ld, ch0, rows, kind):
    x = R.colsum_input(dtype, rows, ld, kind)      # every channel of the row holds data: a sum over the wrong channels cannot pass
    old = R.colsum_old((c,), rows, c)
    ref, _ = R.colsum(x[:, ch0:ch0 + c], old)
    xd = x.to(DT[dtype][1]).cuda()
    before = xd.clone()
    out = Guarded(c, old)
    case = "%s c%d ld%d first channel %d rows%d" % (dtype, c, ld, ch0, rows)
    L.check(lib.dd_colsum(xd.data_ptr() + ch0 * ESZ[dtype], ld, c, rows, out.ptr, DT[dtype][0], stream()))
    _sync()
    if kind == "int":
        t.exact("colsum %s, integer-valued" % what, case, out.buf[G:G + c], ref)
    else:
        check("colsum %s, real-valued, %s" % (what, case), out.values(), ref, ACC32[dtype])
    t.true("colsum %s leaves the guard words and x alone" % what, case, out.guards_intact() and torch.equal(xd, before))


@pytest.mark.parametrize("rows", R.COLSUM_ROWS)
def test_colsum_narrow_aligned_views(rows):
    """The shapes dd_colsum hands to colsum_segments_kernel (at most 8 vectors, 16-byte aligned rows); out holds non-zero integers: the launch adds."""
    _need_gpu()
    lib, t = L.load(), Tally()
    for dtype, c, ld, ch0, _ in R.COLSUM_VECTOR:
        for kind in R.POOL_KINDS:
            _colsum_case(lib, t, "vector route", dtype, c, ld, ch0, rows, kind)
    t.flush()


@pytest.mark.parametrize("rows", R.COLSUM_ROWS)
def test_colsum_wide_unaligned_or_odd_rows(rows):
    """The shapes only the per-channel-lane colsum_kernel takes: more than 8 vectors, a view that does not start on a 16-byte vector (it reads
    single elements), a row that is no whole number of vectors; 4100 rows make its grid-stride loop wrap (1024 workgroups x 4 row lanes)."""
    _need_gpu()
    lib, t = L.load(), Tally()
    for dtype, c, ld, ch0, _ in R.COLSUM_LANE:
        for kind in R.POOL_KINDS:
            _colsum_case(lib, t, "per-channel-lane route", dtype, c, ld, ch0, rows, kind)
    t.flush()


@pytest.mark.parametrize("case_index", range(len(R.COLSUM_SEGMENTS)))
def test_colsum_segments(case_index):
    """1, 3 and 64 segments; two segments aimed at the same output row add up; out_ld > c with the columns past c and the guard words untouched."""
    _need_gpu()
    lib, t = L.load(), Tally()
    dtype, c, ld, ch0, nseg, rows, out_row, out_ld = R.COLSUM_SEGMENTS[case_index]
    nrow = max(out_row) + 1
    for kind in R.POOL_KINDS:
        x = R.colsum_input(dtype, nseg * rows, ld, kind, nseg)
        old = R.colsum_old((nrow, c), nseg, rows)
        ref, _ = R.colsum_segments(x[:, ch0:ch0 + c], rows, out_row, old)
        xd = x.to(DT[dtype][1]).cuda()
        before = xd.clone()
        init = torch.full((nrow, out_ld), PAD0, dtype=torch.float64)
        init[:, :c] = old
        out = Guarded(nrow * out_ld, init)
        tab = (C.c_int * nseg)(*out_row)
        case = "%s c%d ld%d segments%d rows%d out_ld%d" % (dtype, c, ld, nseg, rows, out_ld)
        L.check(lib.dd_colsum_segments(xd.data_ptr() + ch0 * ESZ[dtype], ld, c, rows, nseg, out.ptr, out_ld, tab, DT[dtype][0], stream()))
        _sync()
        got = out.buf[G:G + nrow * out_ld].reshape(nrow, out_ld)
        if kind == "int":
            t.exact("colsum_segments, integer-valued", case, got[:, :c], ref)
        else:
            check("colsum_segments, real-valued, " + case, got[:, :c], ref, ACC32[dtype])
        t.true("colsum_segments leaves the columns past c, the guard words and x alone", case, bool((got[:, c:] == PAD0).all()) and out.guards_intact()
               and torch.equal(xd, before))
    t.flush()


# ---------------------------------------------------------------------------------------------------------------- tiles
@pytest.mark.parametrize("Cc", R.TILE_C)
def test_extract_tiles_and_stitch(Cc):
    """Bit-exact copies, 37 x 41 frame, 16 x 16 tiles: even and odd origins and every (ldf, ldt) in {C, C + 1}^2 (the float4 walk needs C == ldf
    == ldt and a 16-byte aligned source row, everything else takes the scalar walk), the last tile flush with the frame's last row and column;
    dd_stitch with whole tiles, crops and empty crops into a sentinel-filled frame whose untouched part is compared."""
    _need_gpu()
    lib, t = L.load(), Tally()
    frame = R.frame_input(Cc)
    n, ts = len(R.TILE_ORIGINS), R.TILE
    tiles_ref = R.extract_tiles(frame, R.TILE_ORIGINS, ts)
    origins = torch.tensor(R.TILE_ORIGINS, dtype=torch.int32).reshape(-1).cuda()
    table = (L.StitchEntry * len(R.STITCH_ENTRIES))(*[L.StitchEntry(*e) for e in R.STITCH_ENTRIES])
    table_d = torch.frombuffer(bytearray(bytes(table)), dtype=torch.uint8).cuda()
    for ldf in (Cc, Cc + 1):
        for ldt in (Cc, Cc + 1):
            case = "C%d ldf%d ldt%d" % (Cc, ldf, ldt)
            fr = _f32_rows(frame, ldf)
            tl = torch.full((n, ts, ts, ldt), SENTINEL, dtype=torch.float32, device="cuda")
            L.check(lib.dd_extract_tiles(fr.data_ptr(), R.FRAME_H, R.FRAME_W, ldf, Cc, tl.data_ptr(), ts, ldt, origins.data_ptr(), n, stream()))
            _sync()
            t.exact("extract_tiles", case, tl[..., :Cc], tiles_ref)
            t.true("extract_tiles leaves the spare channel and the frame alone", case, bool((tl[..., Cc:] == SENTINEL).all()) and torch.equal(fr, _f32_rows(frame, ldf)))
            out = torch.full((1, R.FRAME_H, R.FRAME_W, ldf), SENTINEL, dtype=torch.float32, device="cuda")
            src = _f32_rows(tiles_ref, ldt)
            L.check(lib.dd_stitch(src.data_ptr(), ts, ldt, out.data_ptr(), R.FRAME_H, R.FRAME_W, ldf, Cc, table_d.data_ptr(), len(R.STITCH_ENTRIES), stream()))
            _sync()
            want = R.stitch(tiles_ref, R.STITCH_ENTRIES, torch.full((1, R.FRAME_H, R.FRAME_W, Cc), SENTINEL, dtype=torch.float64))
            t.exact("stitch (untouched border included)", case, out[..., :Cc], want)
            t.true("stitch leaves the spare channel and the tiles alone", case, bool((out[..., Cc:] == SENTINEL).all()) and torch.equal(src, _f32_rows(tiles_ref, ldt)))
    t.flush()
