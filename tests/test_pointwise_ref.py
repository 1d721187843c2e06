"""CPU: the float64 reference of tests/pointwise_ref.py is (1) the oracle's -- oracle.tf_ops and torch autograd on the case tables the GPU test
uses, (2) reachable -- an honest float32 evaluation of every adding formula stays within 1x the per-element bound, (3) sharp -- every named
mutant fails the gate of at least one case -- and (4) the integer-valued inputs behind the bit-equal gates really make every fp32 sum exact."""
import pytest
import torch

import pointwise_ref as R
from gpu_util import ACC32, ROUND
from oracle import tf_ops as T

F64, F32 = torch.float64, torch.float32
CASE_DTYPES = R.DTYPES


def _pool_all(dtypes=CASE_DTYPES):
    for dt in dtypes:
        for g in R.POOL_GEOMETRIES:
            for c in R.pool_switches():
                yield dt, g, c


# ---------------------------------------------------------------------------------------------------------------- (1) the oracle
@pytest.mark.parametrize("kind", R.POOL_KINDS)
def test_maxpool_reference_is_the_oracles_max_pool_and_its_autograd_gradient(kind):
    """y = oracle max_pool_same; dx (forward's own codes) = autograd's gradient -- on the tie-saturated integer inputs too: both give a tied
    maximum's gradient to the FIRST maximum in row-major window order, as TF does.  With relu_mask the gradient is autograd's times (x > 0)."""
    ties = 0
    for dt in CASE_DTYPES:
        for g in R.POOL_GEOMETRIES:
            pool, stride = g[:2]
            for relu_mask in (0, 1):
                x, dy, old, _ = R.pool_inputs(dt, g, relu_mask, kind)
                xo = x.clone().requires_grad_(True)
                yo = T.max_pool_same(xo, pool, stride)
                (gx,) = torch.autograd.grad((yo * dy).sum(), [xo])
                y, codes, dx, _, _ = R.pool_reference(dt, g, relu_mask, "none", 0, kind)
                assert torch.equal(y, yo.detach()), (dt, g, relu_mask)
                assert torch.equal(dx, gx * (x > 0) if relu_mask else gx), (dt, g, relu_mask)
                _, _, dxa, _, _ = R.pool_reference(dt, g, relu_mask, "unrelated", 1, kind)
                m = R.pool_inputs(dt, g, relu_mask, kind)[3]
                assert torch.equal(dxa, old + (gx * (x > 0) if relu_mask else gx) * (m > 0)), (dt, g, relu_mask)
                assert int(codes.max()) in (255,) + tuple(range(pool * pool)) and (relu_mask or int(codes.max()) < pool * pool)
                # windows whose maximum is met more than once inside the image
                cnt = torch.zeros_like(y)
                OH, pby = R.same_pad(g[2], pool, stride)
                OW, pbx = R.same_pad(g[3], pool, stride)
                for oy in range(OH):
                    for ox in range(OW):
                        for a in range(pool):
                            for b in range(pool):
                                sy, sx = oy * stride + a - pby, ox * stride + b - pbx
                                if 0 <= sy < g[2] and 0 <= sx < g[3]:
                                    cnt[:, oy, ox] += (x[:, sy, sx] == y[:, oy, ox]).to(F64)
                ties += int((cnt > 1).sum())
    print("%s inputs: %d windows with a tied maximum" % (kind, ties))
    assert kind != "int" or ties > 1000


def test_maxpool_codes_follow_the_documented_numbering():
    """Known answers: 3x3 / stride 2 on a 2 x 2 image pads one cell AFTER (pad_before 0): cell (a, b) of the window is pixel (a, b)."""
    x = torch.tensor([[1.0, 5.0], [5.0, 2.0]], dtype=F64).reshape(1, 2, 2, 1)
    y, codes = R.maxpool_fwd(x, 3, 2, 0)
    assert y.reshape(-1).tolist() == [5.0] and codes.reshape(-1).tolist() == [1]      # first of the two fives: (0, 1) -> 0 * 3 + 1
    # a 1 x 1 image: total padding 2, one cell before -> the pixel is cell (1, 1), code 4; non-positive under relu_mask -> 255
    for v, rm, want in ((3.0, 1, 4), (0.0, 1, 255), (-2.0, 1, 255), (-2.0, 0, 4)):
        _, codes = R.maxpool_fwd(torch.full((1, 1, 1, 1), v, dtype=F64), 3, 2, rm)
        assert codes.item() == want
    dx, _, _ = R.maxpool_bwd(torch.full((1, 1, 1, 1), 7.0, dtype=F64), torch.tensor(4).reshape(1, 1, 1, 1), (1, 1, 1, 1), 3, 2)
    assert dx.item() == 7.0
    dx, _, _ = R.maxpool_bwd(torch.full((1, 1, 1, 1), 7.0, dtype=F64), torch.tensor(255).reshape(1, 1, 1, 1), (1, 1, 1, 1), 3, 2)
    assert dx.item() == 0.0


def test_zero_stuff_is_the_transposed_conv_with_an_identity_kernel():
    for shape in R.STUFF_SHAPES:
        x = R.stuff_inputs("f32", shape, "real")[0]
        C = x.shape[3]
        k = torch.zeros(3, 3, C, C, dtype=F64)
        k[1, 1] = torch.eye(C, dtype=F64)
        xo = x.clone().requires_grad_(True)
        yo = T.conv2d_transpose_s2(xo, k)
        assert torch.equal(R.zero_stuff(x), yo.detach())
        dy = R.reals(yo.shape, "f32", 99, *shape)
        (gx,) = torch.autograd.grad((yo * dy).sum(), [xo])
        assert torch.equal(R.zero_unstuff(dy)[0], gx)


def test_space_to_depth_planes_are_the_output_parities():
    y = R.s2d_input("f32", 5)
    s = R.space_to_depth2(y, 5, 8)
    for py in range(2):
        for px in range(2):
            assert torch.equal(s[..., (py * 2 + px) * 8:(py * 2 + px) * 8 + 5], y[:, py::2, px::2, :5])
            assert not s[..., (py * 2 + px) * 8 + 5:(py * 2 + px + 1) * 8].any()


@pytest.mark.parametrize("shape", R.COMPOSE_SHAPES)
def test_blend_reference_is_compose_scales_and_its_autograd(shape):
    small, fine, dout, ds_old, _, wl, _ = R.compose_inputs("bf16", shape)
    so, fo, zo = small.clone().requires_grad_(True), fine.clone().requires_grad_(True), wl.clone().requires_grad_(True)
    wts = torch.sigmoid(torch.relu(zo))      # (the 1x1 conv before the sigmoid ends in a ReLU: wl is its output, dwl the gradient before it)
    low = T.resize_nearest_x2(T.avg_pool_same(fo, 2))
    out = fo - wts * low + wts * T.resize_nearest_x2(so)
    gs, gf, gz = torch.autograd.grad((out * dout).sum(), [so, fo, zo])
    assert R.rel_l2(R.compose_blend_fwd(small, fine, wl), out.detach()) < 1e-15
    d_small, d_fine, dwl = R.compose_blend_bwd(dout, small, fine, wl, ds_old, 1, 1, "f32")
    assert R.rel_l2(d_small, gs + ds_old) < 1e-14 and R.rel_l2(d_fine, gf) < 1e-14
    assert R.rel_l2(dwl, R.rne(gz, "f32")) < 1e-7
    assert R.rel_l2(R.compose_blend_bwd(dout, small, fine, wl, ds_old, 0, 1, "f32")[0], gs) < 1e-14
    # the pack is cat([resize(small), fine]) stored in the storage type; unpack_bwd the gradient of that cat
    packed = R.compose_pack(small, fine, 8, "bf16")
    assert torch.equal(packed[..., :6], torch.cat([T.resize_nearest_x2(small), fine], dim=3).to(torch.bfloat16).to(F64)) and not packed[..., 6:].any()
    dnet = R.compose_inputs("bf16", shape)[6]
    (gs2, gf2) = torch.autograd.grad((torch.cat([T.resize_nearest_x2(so), fo], dim=3) * dnet).sum(), [so, fo])
    (ds, _, _), (df, _, _) = R.compose_unpack_bwd(dnet, torch.zeros_like(gs2), torch.zeros_like(gf2))
    assert R.rel_l2(ds, gs2) < 1e-15 and torch.equal(df, gf2)


def test_tiles_and_stitch_round_trip():
    frame = R.frame_input(3)
    tiles = R.extract_tiles(frame, R.TILE_ORIGINS, R.TILE)
    assert tuple(tiles.shape) == (len(R.TILE_ORIGINS), R.TILE, R.TILE, 3)
    assert max(oy for oy, _ in R.TILE_ORIGINS) + R.TILE == R.FRAME_H and max(ox for _, ox in R.TILE_ORIGINS) + R.TILE == R.FRAME_W
    assert {ox % 2 for _, ox in R.TILE_ORIGINS} == {0, 1}
    old = torch.full((1, R.FRAME_H, R.FRAME_W, 3), R.SENTINEL, dtype=F64)
    out = R.stitch(tiles, R.STITCH_ENTRIES, old)
    written = torch.zeros(R.FRAME_H, R.FRAME_W, dtype=torch.int64)
    for t, y0, y1, x0, x1, _, dy, dx in R.STITCH_ENTRIES:      # destinations never overlap (workgroups of one launch write them)
        written[dy:dy + y1 - y0, dx:dx + x1 - x0] += 1
        assert 0 <= dy and dy + y1 - y0 <= R.FRAME_H and 0 <= dx and dx + x1 - x0 <= R.FRAME_W
    assert int(written.max()) == 1 and int(written[-1, -1]) == 1
    assert bool((out[0][written == 0] == R.SENTINEL).all()) and not bool((out[0][written == 1] == R.SENTINEL).any())


# ---------------------------------------------------------------------------------------------------------------- (2) float32 stays within 1x
def _store(v, dtype):
    """What a kernel stores of an fp32 value."""
    return R.rne(v, dtype)


def test_a_float32_evaluation_stays_within_the_bound():
    worst = {}

    def see(name, got, ref, bound):
        worst[name] = max(worst.get(name, 0.0), R.worst_ratio(got, ref, bound))

    for dt, g, c in _pool_all():
        _, codes, dx, bound, _ = R.pool_reference(dt, g, c["relu_mask"], c["mask"], c["acc"], c["kind"])
        dx32 = R.pool_reference(dt, g, c["relu_mask"], c["mask"], c["acc"], c["kind"], eval_dtype=F32)[2]
        see("maxpool_bwd", _store(dx32, dt), dx, bound)
    for dt in CASE_DTYPES:
        for C in R.MASKED_ADD_C:
            for npix in R.MASKED_ADD_NPIX:
                for kind in R.POOL_KINDS:
                    src, mask, old = R.masked_add_inputs(dt, C, npix, kind)
                    for mk in (None, mask):
                        for o in (None, old):
                            ref, bound, _ = R.masked_add(src, mk, o, dt)
                            see("masked_add", _store(R.masked_add(src, mk, o, dt, eval_dtype=F32)[0], dt), ref, bound)
        for shape in R.STUFF_SHAPES:
            for kind in R.POOL_KINDS:
                _, dy, mask, old = R.stuff_inputs(dt, shape, kind)
                for mk in (None, mask):
                    for o in (None, old):
                        ref, bound, _ = R.zero_unstuff(dy, mk, o, dt)
                        see("zero_unstuff", _store(R.zero_unstuff(dy, mk, o, dt, eval_dtype=F32)[0], dt), ref, bound)
        for shape in R.COMPOSE_SHAPES:
            for kind in R.POOL_KINDS:
                _, _, _, ds_old, df_old, _, dnet = R.compose_inputs(dt, shape, kind)
                (ds, bs, _), (df, bf, _) = R.compose_unpack_bwd(dnet, ds_old, df_old)
                (ds32, _, _), (df32, _, _) = R.compose_unpack_bwd(dnet, ds_old, df_old, eval_dtype=F32)
                see("compose_unpack_bwd d_small", ds32, ds, bs)
                see("compose_unpack_bwd d_fine", df32, df, bf)
    for name, w in sorted(worst.items()):
        print("float32 evaluation of %-28s worst error / bound %.3f" % (name, w))
        assert w <= 1.0, name


def test_a_float32_evaluation_of_the_blend_and_the_column_sums_passes_the_rel_l2_gates():
    """... with 1 - w formed as e * w.  The subtraction 1.f - w cancels for a large wl (w(1 - w) at wl = 8 is off by up to 2e-4 relative); where such
    a pixel carries the gradient (the 2 x 2 case: wl = 0, 8 and two draws) an fp32 evaluation of THAT form misses the fp32 gate of dwl, which is
    why compose_blend_bwd_kernel forms e * w (printed, and asserted to be over the gate, so that the case keeps telling the two apart)."""
    worst = {}
    sub = 0.0
    for dt in CASE_DTYPES:
        for shape in R.COMPOSE_SHAPES:
            small, fine, dout, ds_old, _, wl, _ = R.compose_inputs(dt, shape)
            pairs = [("blend out", R.compose_blend_fwd(small, fine, wl, eval_dtype=F32), R.compose_blend_fwd(small, fine, wl), ACC32[dt])]
            ref = R.compose_blend_bwd(dout, small, fine, wl, ds_old, 1, 1, dt)
            got = R.compose_blend_bwd(dout, small, fine, wl, ds_old, 1, 1, dt, eval_dtype=F32)
            pairs += [("blend d_small", got[0], ref[0], ACC32[dt]), ("blend d_fine", got[1], ref[1], ACC32[dt]), ("blend dwl " + dt, got[2], ref[2], ROUND[dt])]
            for name, a, b, tol in pairs:
                worst[name] = max(worst.get(name, (0.0, tol))[0], R.rel_l2(a, b)), tol
            if dt == "f32":
                sub = max(sub, R.rel_l2(R.compose_blend_bwd(dout, small, fine, wl, ds_old, 1, 1, dt, eval_dtype=F32, one_minus_w="1-w")[2], ref[2]))
        for rows in R.COLSUM_ROWS:
            x = R.colsum_input(dt, rows, 64, "real")
            old = R.colsum_old((64,), rows)
            worst["colsum real"] = max(worst.get("colsum real", (0.0, 0.0))[0], R.rel_l2(R.colsum(x, old, eval_dtype=F32)[0], R.colsum(x, old)[0])), ACC32[dt]
    for name, (e, tol) in sorted(worst.items()):
        print("float32 evaluation of %-16s rel-L2 %.3e (gate %.1e)" % (name, e, tol))
        assert e <= tol, name
    print("float32 evaluation of blend dwl f32 with 1.f - w: rel-L2 %.3e (gate %.1e)" % (sub, ROUND["f32"]))
    assert sub > ROUND["f32"]


# ---------------------------------------------------------------------------------------------------------------- (3) mutants
def _differs(a, b):
    return not torch.equal(a, b)


def _fails(got, ref, bound, exact):
    return _differs(got, ref) if exact else R.worst_ratio(got, ref, bound) > 1.0


def _pool_fwd_mutant_fails(m):
    for dt, g, c in _pool_all(("bf16",)):
        y, codes = R.pool_reference(dt, g, c["relu_mask"], c["mask"], c["acc"], c["kind"])[:2]
        ym, cm = R.pool_reference(dt, g, c["relu_mask"], c["mask"], c["acc"], c["kind"], mut={m})[:2]
        if tuple(ym.shape) != tuple(y.shape) or _differs(ym, y) or _differs(cm, codes):
            return True
    return False


def _pool_bwd_mutant_fails(m):
    """The backward mutant decodes the REFERENCE codes (a forward error cannot hide a backward one, nor make one up)."""
    for dt, g, c in _pool_all(("bf16",)):
        _, codes, dx, bound, _ = R.pool_reference(dt, g, c["relu_mask"], c["mask"], c["acc"], c["kind"])
        x, dy, old, mm = R.pool_inputs(dt, g, c["relu_mask"], c["kind"])
        mk = {"none": None, "input": x, "unrelated": mm}[c["mask"]]
        dxm = R.maxpool_bwd(dy, codes, x.shape, g[0], g[1], mk, old if c["acc"] else None, dt, {m})[0]
        if _fails(_store(dxm, dt), dx, bound, c["kind"] == "int"):
            return True
    return False


def _masked_add_mutant_fails(m):
    for dt in CASE_DTYPES:
        for kind in R.POOL_KINDS:
            src, mask, old = R.masked_add_inputs(dt, 12, 7, kind)
            ref, bound, _ = R.masked_add(src, mask, old, dt)
            if _fails(_store(R.masked_add(src, mask, old, dt, {m})[0], dt), ref, bound, kind == "int"):
                return True
    return False


def _unstuff_mutant_fails(m):
    for dt in CASE_DTYPES:
        for kind in R.POOL_KINDS:
            _, dy, mask, old = R.stuff_inputs(dt, (2, 3, 5), kind)
            ref, bound, _ = R.zero_unstuff(dy, mask, old, dt)
            if _fails(_store(R.zero_unstuff(dy, mask, old, dt, {m})[0], dt), ref, bound, kind == "int"):
                return True
    return False


def _unpack_mutant_fails(m):
    for kind in R.POOL_KINDS:
        _, _, _, ds_old, df_old, _, dnet = R.compose_inputs("bf16", (2, 4, 6), kind)
        (ds, bs, _), (df, bf, _) = R.compose_unpack_bwd(dnet, ds_old, df_old)
        (dsm, _, _), (dfm, _, _) = R.compose_unpack_bwd(dnet, ds_old, df_old, {m})
        if _fails(dsm, ds, bs, kind == "int") and _fails(dfm, df, bf, kind == "int"):
            return True
    return False


def _stuff_mutant_fails(m):
    x = R.stuff_inputs("bf16", (2, 3, 5), "real")[0]
    return _differs(R.zero_stuff(x, {m}), R.zero_stuff(x))


def _s2d_mutant_fails(m):
    return all(_differs(R.space_to_depth2(R.s2d_input("bf16", C), C, cp, {m}), R.space_to_depth2(R.s2d_input("bf16", C), C, cp)) for C, cp in R.S2D_CHANNELS
               if m != "pads_unwritten" or cp > C)


def _convert_mutant_fails(m):
    src = R.convert_input("f32", 3)
    return all(_differs(R.convert_channels(src, 3, 8, dt, {m}), R.convert_channels(src, 3, 8, dt)) for dt in ("bf16", "f16"))


def _pack_mutant_fails(m):
    small, fine = R.compose_inputs("bf16", (2, 4, 6))[:2]
    return all(_differs(R.compose_pack(small, fine, 8, dt, {m}), R.compose_pack(small, fine, 8, dt)) for dt in ("bf16", "f16"))


def _segments_mutant_fails(m):
    for kind in R.POOL_KINDS:
        dt, c, ld, ch0, nseg, rows, out_row, out_ld = R.COLSUM_SEGMENTS[1]
        x = R.colsum_input(dt, nseg * rows + 1, ld, kind, nseg)[:, ch0:ch0 + c]
        old = R.colsum_old((max(out_row) + 1, c), nseg, rows)
        ref = R.colsum_segments(x, rows, out_row, old)[0]
        got = R.colsum_segments(x, rows, out_row, old, {m})[0]
        if not (_differs(got, ref) if kind == "int" else R.rel_l2(got, ref) > ACC32[dt]):
            return False
    return True


def _blend_misses(m):
    """(rel-L2 / gate) of the mutant for every output it touches, in every storage type: the largest over the compose shapes (a mutant has to
    fail on at least one case; on a 2 x 2 image `low` or the zeros of wl can be small or few by chance), the smallest over outputs and types."""
    least = float("inf")
    for dt in CASE_DTYPES:
        most = {}
        for shape in R.COMPOSE_SHAPES:
            small, fine, dout, ds_old, _, wl, _ = R.compose_inputs(dt, shape)
            ref = (R.compose_blend_fwd(small, fine, wl),) + R.compose_blend_bwd(dout, small, fine, wl, ds_old, 1, 8, dt)
            got = (R.compose_blend_fwd(small, fine, wl, {m}),) + R.compose_blend_bwd(dout, small, fine, wl, ds_old, 1, 8, dt, {m})
            tols = (ACC32[dt], ACC32[dt], ACC32[dt], ROUND[dt])
            touched = {"low_not_quarter": (0, 3), "wl_gate_dropped": (3,), "dsmall_overwrites": (1,), "pads_unwritten": (3,)}[m]
            for i in touched:
                most[i] = max(most.get(i, 0.0), R.rel_l2(got[i], ref[i]) / tols[i])
        least = min(least, min(most.values()))
    return least


# mutant -> the checks that must ALL report a failure
MUTANT_CHECKS = {
    "last_max_wins": (_pool_fwd_mutant_fails,),
    "pad_before": (_pool_fwd_mutant_fails,),
    "padded_cells_win": (_pool_fwd_mutant_fails,),
    "relu_mask_ignored": (_pool_fwd_mutant_fails,),
    "offset2_as_1": (_pool_bwd_mutant_fails,),
    "out_of_image_window": (_pool_bwd_mutant_fails,),
    "mask_after_accumulate": (_pool_bwd_mutant_fails, _masked_add_mutant_fails, _unstuff_mutant_fails),
    "accumulate_dropped": (_pool_bwd_mutant_fails, _masked_add_mutant_fails, _unstuff_mutant_fails, _unpack_mutant_fails),
    "parity_swapped": (_s2d_mutant_fails,),
    "stuffed_even": (_stuff_mutant_fails, _unstuff_mutant_fails),
    "x_not_halved": (_pack_mutant_fails,),
    "low_not_quarter": (),
    "wl_gate_dropped": (),
    "dsmall_overwrites": (),
    "pads_unwritten": (_s2d_mutant_fails, _convert_mutant_fails, _pack_mutant_fails),
    "truncate": (_convert_mutant_fails, _pack_mutant_fails),
    "segment_shifted": (_segments_mutant_fails,),
}


@pytest.mark.parametrize("mutant", sorted(R.MUTANTS))
def test_every_mutant_fails_its_gate(mutant):
    assert set(MUTANT_CHECKS) == set(R.MUTANTS)
    assert MUTANT_CHECKS[mutant] or mutant in R.BLEND_MUTANTS
    for chk in MUTANT_CHECKS[mutant]:
        assert chk(mutant), "%s (%s) passes %s" % (mutant, R.MUTANTS[mutant], chk.__name__)
    if mutant in R.BLEND_MUTANTS:
        least = _blend_misses(mutant)
        print("%s: misses the rel-L2 gate by at least %.3g x" % (mutant, least))
        assert least >= 100.0, mutant


def test_the_unmutated_reference_passes_every_mutant_check():
    """The checks above are not trivially true: with no mutation each of them reports no failure."""
    for chk in {c for cs in MUTANT_CHECKS.values() for c in cs}:
        assert not chk("no_such_mutant"), chk.__name__


# ---------------------------------------------------------------------------------------------------------------- (4) exact inputs
def test_the_integer_cases_make_every_fp32_sum_exact():
    n = 0
    for dt, g, c in _pool_all():
        if c["kind"] == "int":
            x, dy, old, m = R.pool_inputs(dt, g, c["relu_mask"], "int")
            _, _, dx, _, gabs = R.pool_reference(dt, g, c["relu_mask"], c["mask"], c["acc"], "int")
            assert all(torch.equal(R.rne(t, dt), t) for t in (x, dy, old, m)) and R.exact_in_fp32(dx, gabs, dt), (dt, g, c)
            n += 1
    for dt in CASE_DTYPES:
        for C in R.MASKED_ADD_C:
            for npix in R.MASKED_ADD_NPIX:
                src, mask, old = R.masked_add_inputs(dt, C, npix, "int")
                ref, _, ab = R.masked_add(src, mask, old, dt)
                assert R.exact_in_fp32(ref, ab, dt)
        for shape in R.STUFF_SHAPES:
            _, dy, mask, old = R.stuff_inputs(dt, shape, "int")
            ref, _, ab = R.zero_unstuff(dy, mask, old, dt)
            assert R.exact_in_fp32(ref, ab, dt)
        for shape in R.COMPOSE_SHAPES:
            _, _, _, ds_old, df_old, _, dnet = R.compose_inputs(dt, shape, "int")
            assert torch.equal(R.rne(dnet, dt), dnet)
            for ref, _, ab in R.compose_unpack_bwd(dnet, ds_old, df_old):
                assert R.exact_in_fp32(ref, ab, "f32")
    for dt, c, ld, ch0, mis in R.COLSUM_VECTOR + R.COLSUM_LANE:
        for rows in R.COLSUM_ROWS:
            x = R.colsum_input(dt, rows, ld, "int")
            ref, ab = R.colsum(x[:, ch0:ch0 + c], R.colsum_old((c,), rows, c))
            assert torch.equal(R.rne(x, dt), x) and R.exact_in_fp32(ref, ab, "f32")
    for dt, c, ld, ch0, nseg, rows, out_row, out_ld in R.COLSUM_SEGMENTS:
        x = R.colsum_input(dt, nseg * rows, ld, "int", nseg)
        ref, ab = R.colsum_segments(x[:, ch0:ch0 + c], rows, out_row, R.colsum_old((max(out_row) + 1, c), nseg, rows))
        assert torch.equal(R.rne(x, dt), x) and R.exact_in_fp32(ref, ab, "f32")
    assert n == 3 * len(R.POOL_GEOMETRIES) * 12


def test_case_tables_cover_what_they_claim():
    """Every switch with every (B, C, ld) on every geometry; the column-sum routes as dd_colsum decides them."""
    for dt in CASE_DTYPES:
        for g in R.POOL_GEOMETRIES:
            cs = R.pool_cases(dt, g)
            assert len(cs) == 24 * 8 == len({tuple(sorted(c.items())) for c in cs})
            assert {(c["B"], c["C"], c["ld"] - c["C"]) for c in cs} == set(R.POOL_BCL[dt]) and len(R.POOL_BCL[dt]) == 8
            assert R.POOL_B == max(c["B"] for c in cs) and R.POOL_C[dt] == max(c["C"] for c in cs)

    def vector_route(dt, c, ld, ch0):
        per16, esz = (4, 4) if dt == "f32" else (8, 2)
        nv = 1
        while nv * per16 < c:
            nv *= 2
        return nv <= 8 and (c + per16 - 1) // per16 * per16 <= ld and ld % per16 == 0 and (ch0 * esz) % 16 == 0 and (ld * esz) % 16 == 0

    assert all(vector_route(dt, c, ld, ch0) for dt, c, ld, ch0, _ in R.COLSUM_VECTOR)
    assert not any(vector_route(dt, c, ld, ch0) for dt, c, ld, ch0, _ in R.COLSUM_LANE)
    for dt, c, ld, ch0, _ in R.COLSUM_VECTOR + R.COLSUM_LANE:
        assert ch0 + c <= ld
    assert {n for _, _, _, _, n, _, _, _ in R.COLSUM_SEGMENTS} == {1, 3, 64}
    assert any(len(set(r)) < len(r) for _, _, _, _, _, _, r, _ in R.COLSUM_SEGMENTS) and any(o > c for _, c, _, _, _, _, _, o in R.COLSUM_SEGMENTS)
