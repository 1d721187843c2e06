"""CPU proof that the gates of tests/compose_ref.py are sound and sharp, on the very inputs tests/test_gpu_compose_ops.py launches (the smaller
shapes, where every product is materialised):
  sound   every layer evaluated in fp32 with its terms added in four different orders (one in blocks of 16, as an MFMA K-step) stays within the
          gates with worst error / gate < 1, for both kernels' bias handling and both storage types;
  sharp   each of seventeen plausible mistakes of a kernel, injected into the restated kernel, exceeds a gate on at least one shape;
  and the conditions on the inputs and the geometry coverage of the GPU shape list hold."""
import pytest
import torch

import compose_ref as R

plan, PLAN_KEYS, coverage_lost = R.plan, R.PLAN_KEYS, R.coverage_lost


@pytest.mark.parametrize("dtype", R.DTYPES)
@pytest.mark.parametrize("kernel", ["stream", "tile"])
def test_fp32_evaluation_in_any_order_stays_within_the_gates(dtype, kernel):
    worst = {}
    for shape in R.SMALL_SHAPES[:4] + [(1, 6, 260)]:
        for kind in R.KINDS:
            inp = R.compose_inputs(shape, dtype, 0, kind)
            for order in R.ORDERS:
                for s, w in R.worst(inp, R.simulate(inp, kernel, order=order), kernel).items():
                    worst[s] = max(worst.get(s, 0.0), w)
    print("fp32 orders, worst error / gate (%s, %s): %s" % (dtype, kernel, " ".join("%s %.3f" % kv for kv in worst.items())))
    assert R.within(worst), worst
    # the float64 restatement itself: the one rounding only -- at most half an ulp of the gate's ulp / 2 + E
    inp = R.compose_inputs((2, 10, 50), dtype, 0)
    w64 = R.worst(inp, R.simulate(inp, kernel), kernel)
    assert all(w <= 1.0 for w in w64.values()), w64


@pytest.mark.parametrize("dtype", R.DTYPES)
@pytest.mark.parametrize("mistake", R.MISTAKES)
def test_every_mistake_exceeds_a_gate(lib, dtype, mistake):
    caught = []
    for shape in R.SMALL_SHAPES:
        inp = R.compose_inputs(shape, dtype, 0)
        got = R.simulate(inp, "stream", mistake=mistake, plan=plan(lib, shape), layer=1)
        w = R.worst(inp, got, "stream")
        if max(w.values()) > 1.0:
            caught.append((R.shape_id(shape), max(w, key=w.get), max(w.values())))
    print("%-24s %-5s caught on %s" % (mistake, dtype, caught))
    assert caught, "%s (%s) passes every gate on every shape" % (mistake, dtype)


def test_mistakes_in_every_3x3_layer_are_caught(lib):
    """The layer-bound mistakes, in each of the four 3x3 layers (bf16, the wider gate)."""
    shape = (1, 16, 130)
    inp = R.compose_inputs(shape, "bf16", 0)
    for layer in range(4):
        for mistake in ("tap_dropped", "taps_transposed", "frame_padding", "seam_left_zeroed", "seam_right_zeroed", "bias_dropped"):
            w = R.worst(inp, R.simulate(inp, "stream", mistake=mistake, plan=plan(lib, shape), layer=layer), "stream")
            assert max(w.values()) > 1.0, (layer, mistake, w)


def test_ulp_of_the_storage_types():
    z = torch.tensor([0.0, 1.0, 1.5, 2.0, -3.0, 2.0 ** -14, 2.0 ** -15, 2.0 ** -24, 1e-9, 65504.0], dtype=torch.float64)
    assert R.ulp(z, "f16").tolist() == [2.0 ** -24, 2.0 ** -10, 2.0 ** -10, 2.0 ** -9, 2.0 ** -9, 2.0 ** -24, 2.0 ** -24, 2.0 ** -24, 2.0 ** -24, 32.0]
    assert R.ulp(z, "bf16")[:5].tolist() == [2.0 ** -133, 2.0 ** -7, 2.0 ** -7, 2.0 ** -6, 2.0 ** -6]
    for dtype in R.DTYPES:      # against the type itself: the distance to the next number
        t = (torch.rand(4096, dtype=torch.float64) * 2.0 ** torch.randint(-20, 10, (4096,)).double()).to(R.TDT[dtype])
        nxt = (t.view(torch.int16) + 1).view(R.TDT[dtype])
        assert torch.equal(R.ulp(t.double(), dtype), nxt.double() - t.double())
    assert R.D_SIGMA < 2.0 ** -16
    hi, mid, lo = R.split3(torch.tensor([0.1234567, -0.087654321]), "bf16")
    assert torch.equal((hi + mid + lo).float(), torch.tensor([0.1234567, -0.087654321]))


@pytest.mark.parametrize("dtype", R.DTYPES)
def test_conditions_on_the_inputs(dtype):
    subnormal = 0.0
    for shape in sorted(set(R.FWD_SHAPES[:10] + R.TILE_FWD_SHAPES[:4])):
        for kind in R.KINDS:
            inp = R.compose_inputs(shape, dtype, 0, kind)
            got = R.simulate(inp, "stream")
            ref = R.stage_reference(inp, got, "stream")
            npix = shape[0] * shape[1] * shape[2]
            for s in R.STAGES:
                assert float(ref[s]["z"].abs().max()) <= R.FMAX[dtype] / 16, (shape, s)
                assert R.boundary_fraction(ref[s]) < 0.005 or npix < 256, (shape, kind, s, R.boundary_fraction(ref[s]))
                if dtype == "f16" and s not in ("out",):
                    z = ref[s]["ref"]
                    subnormal = max(subnormal, float(((z != 0) & (z.abs() < 2.0 ** -14)).double().mean()))
            if npix >= 256:
                for s in R.RELU_STAGES:
                    pos = float((got[s] > 0).double().mean())
                    assert 0.2 <= pos <= 0.8, (shape, kind, s, pos)
                d = (R.up2(R.pool2(inp["fine"].double())) - R.up2(inp["small"].double())).abs()
                if kind == "normal":
                    assert float((d.amax(dim=3) > 0.1).double().mean()) >= 0.5, shape
    if dtype == "f16":
        assert subnormal >= 0.01, subnormal


def test_forward_shapes_cover_the_geometry(lib):
    """At 256 compute units the streaming forward shape list has every frame width, rows-per-step, strip count, a narrow last strip, ragged
    bands, a band higher than 4 rows and two shapes whose workgroups walk more than one unit."""
    rows = {s: dict(zip(PLAN_KEYS, plan(lib, s))) for s in R.FWD_SHAPES}
    want = {(1, 2, 2): (32, 4, 1), (1, 18, 30): (32, 4, 1), (2, 10, 50): (64, 2, 1), (1, 20, 72): (96, 1, 1), (1, 22, 126): (128, 1, 1),
            (1, 8, 128): (128, 1, 1), (1, 16, 130): (96, 1, 2), (1, 6, 260): (96, 1, 3), (1, 6, 390): (128, 1, 4), (24, 22, 140): (96, 1, 2),
            (260, 4, 8): (32, 4, 1), (130, 6, 140): (96, 1, 2)}
    for s, p in rows.items():
        assert (p["FW"], p["R"], p["strips"]) == want[s], (s, p)
    assert rows[(1, 16, 130)]["SO"] == 66 and rows[(1, 6, 260)]["SO"] * 2 + 84 == 260
    assert rows[(24, 22, 140)]["BH"] == 8 and rows[(130, 6, 140)]["BH"] == 8
    assert not coverage_lost(rows, 256)
