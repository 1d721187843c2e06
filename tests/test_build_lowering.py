"""The builders decide a lowering first and record only what runs: a fused compose net allocates and packs nothing of the layer-wise net it
replaces, and what the loss evaluates (loss_desc.loss_plan) is known before anything is recorded.  Programs are built on the CPU device from
the cross-compiled library; nothing is launched.  The loss_plan tests are host only and do not need the library."""
import pytest

from deepdenoiser_amd import configs
from deepdenoiser_amd import loss_desc as LD
from deepdenoiser_amd.architecture import Architecture

B, H, W = 2, 64, 64
SMALL = dict(filters=(16, 16), convs=1)


def _program(training):
    arch = Architecture(configs.cfg2_unet_kpcn(), device="cpu", dtype="bf16", seed=2)
    prog = arch.program(B, H, W, training_json=configs.bench_training() if training else None)
    assert arch.number_of_scales() == 3
    return prog


def _flat(keep):
    if isinstance(keep, (tuple, list)):
        return [t for k in keep for t in _flat(k)]
    return [] if keep is None else [keep]


def _compose(ops):
    return [op for op in ops if getattr(op, "tag", None) == "compose_net"]


def _compose_pack_records(prog):
    return [rec[0].name for rec in prog.g._pack_records if rec[0].name.startswith("reused_compose_scales")]


def _switches(monkeypatch, **values):
    for name in ("DD_FUSE_COMPOSE", "DD_FUSE_COMPOSE_BWD", "DD_FUSE_HEAD", "DD_FUSE_LOSS_INVERT"):
        monkeypatch.delenv(name, raising=False)
    for name, v in values.items():
        monkeypatch.setenv(name, v)


def test_inference_compose_net_keeps_its_three_operands_and_packs_nothing(lib, monkeypatch):
    _switches(monkeypatch)
    prog = _program(training=False)
    launches = _compose(prog.g.fwd_ops)
    assert len(launches) == 2      # one per scale transition
    for s, op in zip((1, 0), launches):      # coarsest transition first
        bufs = _flat(op.keep)
        assert [tuple(t.shape) for t in bufs] == [(B, H >> (s + 1), W >> (s + 1), 3), (B, H >> s, W >> s, 3), (B, H >> s, W >> s, 3)]
    assert _compose_pack_records(prog) == []
    assert not prog.g.bwd_ops


def test_training_compose_net_keeps_what_the_fused_backward_reads(lib, monkeypatch):
    _switches(monkeypatch)
    prog = _program(training=True)
    launches = _compose(prog.g.fwd_ops)
    assert len(launches) == 2
    for s, op in zip((1, 0), launches):
        h, w = H >> s, W >> s
        shapes = [tuple(t.shape) for t in _flat(op.keep)]
        # small, fine, out; the blend weight (1 channel in a row of 8); the five activations.  No 8-channel packed input beside `wl`.
        assert shapes == [(B, h // 2, w // 2, 3), (B, h, w, 3), (B, h, w, 3), (B, h, w, 8)] + [(B, h, w, 24)] * 5
    assert len(_compose(prog.g.bwd_ops)) == 2      # one fused backward launch per transition
    assert _compose_pack_records(prog) == []


def test_layerwise_compose_backward_keeps_the_packed_input_and_its_weight_images(lib, monkeypatch):
    _switches(monkeypatch, DD_FUSE_COMPOSE_BWD="0")
    prog = _program(training=True)
    launches = _compose(prog.g.fwd_ops)
    assert len(launches) == 2
    for s, op in zip((1, 0), launches):
        h, w = H >> s, W >> s
        shapes = [tuple(t.shape) for t in _flat(op.keep)]
        assert shapes == [(B, h // 2, w // 2, 3), (B, h, w, 3), (B, h, w, 3), (B, h, w, 8), (B, h, w, 8)] + [(B, h, w, 24)] * 5      # netin, wl
    assert _compose(prog.g.bwd_ops) == []
    forward = ["reused_compose_scales/%s/kernel" % n for n in ("conv2d", "conv2d_1", "conv2d_2", "conv2d_3", "conv2d_4", "conv2d_5")]
    assert [n for n in _compose_pack_records(prog) if n in forward][:6] == forward      # registered once, by the first transition
    assert set(forward) <= set(_compose_pack_records(prog))


# ---------------------------------------------------------------------------------------------------------------- loss_plan (host only)
def _plan(aj, tj, dims=((16, 32), (8, 16))):
    arch = Architecture(aj, device="cpu", dtype="bf16", seed=2)
    tuples = arch.feature_prediction_tuples
    head = [t.feature_predictions[j] for j in range(arch.tuple_size) for t in tuples]      # member-major head order
    return LD.loss_plan(arch, head, tj, list(dims))


def test_loss_plan_refuses_what_the_reference_refuses(monkeypatch):
    _switches(monkeypatch)
    tj = configs.training()
    tj["features_training_settings"]["loss_weights_masked"]["ms_ssim"] = 0.5
    with pytest.raises(NotImplementedError, match="the masked ms_ssim loss term cannot run"):
        _plan(configs.architecture(**SMALL), tj)
    # the example architecture loads an Alpha pass
    with pytest.raises(Exception, match="Masking is not supported for the alpha pass, because it does not seem to make sense."):
        _plan(configs.architecture(**SMALL), configs.training(masked_mean=0.8))
    with pytest.raises(ValueError, match="the ms_ssim loss term needs tiles"):
        _plan(configs.architecture(**SMALL), configs.training(ms_ssim=(0.0, 0.0, 0.7)))


def test_loss_plan_fuses_the_inversion_when_every_term_is_pointwise(monkeypatch):
    _switches(monkeypatch)
    after, before = configs.architecture(**SMALL), configs.architecture(invert_after_multiscale=False, **SMALL)
    plan = _plan(after, configs.training())
    assert plan.fuse_invert and plan.loss_scales == 2 and not plan.ms_ssim
    assert plan.norm == 1.0 / (1.0 + 0.25) and (plan.features, plan.combined, plan.image) == ((1.0, 0.0, 0.0), (5.0, 0.0, 0.0), (10.0, 0.0, 0.0))
    assert (plan.use_image, plan.use_comb) == (True, True) and len(plan.triples) > 0
    assert not _plan(after, configs.training(feature_variation=0.7)).fuse_invert
    assert not _plan(after, configs.training(image_variation=3.0)).fuse_invert
    assert not _plan(before, configs.training()).fuse_invert
    assert _plan(after, configs.training(multiscale_loss=False)).loss_scales == 1
    monkeypatch.setenv("DD_FUSE_LOSS_INVERT", "0")
    for aj in (after, before):
        for tj in (configs.training(), configs.training(feature_variation=0.7), configs.bench_training()):
            assert not _plan(aj, tj).fuse_invert
