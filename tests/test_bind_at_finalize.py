"""Every launch is bound when Program(...) returns (engine.Graph.finalize): no list entry is an unbound maker, every launch of an MFMA family
carries its record as `info`, and a family's records say what its listed launches say -- the builders queue only what will run (a fused
compose net or a loss head that inverts the standardization itself records no layer-wise launch), and the members of a merged launch never
bind, so they leave no record.  Built on the CPU device from the cross-compiled library; nothing is launched."""
import pytest

from deepdenoiser_amd import configs, engine
from deepdenoiser_amd.architecture import Architecture

FAMILIES = (("conv_igemm", "conv_records"), ("conv_bwd", "bwd_records"), ("conv_wgrad", "wgrad_records"), ("convt", "convt_records"))
TIRAMISU = dict(filters=(16, 24, 32), convs=2)


def _check(prog, expect):
    g = prog.g
    ops = list(g.pack_ops) + list(prog.label_ops) + list(g.fwd_ops) + list(g.bwd_ops)
    assert ops and all(callable(op) for op in ops)
    assert not [op for op in ops if isinstance(op, engine._Late)], "unbound makers are left in the launch lists"
    for tag, records in FAMILIES:
        launches = [op for op in ops if getattr(op, "tag", None) == tag]
        missing = [getattr(op, "origin", op.__name__) for op in launches if not getattr(op, "info", None)]
        assert not missing, "%s launches without a record: %s" % (tag, missing)
        listed, recorded = sum(op.info["flops"] for op in launches), sum(r["flops"] for r in getattr(g, records))
        # (flops are whole numbers far below 2^53: the sums are exact in any order)
        assert listed == recorded, "%s: launches %.0f flop, %s %.0f flop" % (tag, listed, records, recorded)
        if tag in expect:
            assert launches, "no %s launch in a program that is expected to have them" % tag


@pytest.mark.parametrize("dtype", ["bf16", "f32"])
@pytest.mark.parametrize("name", ["cfg2", "tiramisu"])
def test_training_program_is_bound_and_its_records_match_its_launches(lib, name, dtype):
    aj = configs.cfg2_unet_kpcn() if name == "cfg2" else configs.cfg3_tiramisu(**TIRAMISU)
    arch = Architecture(aj, device="cpu", dtype=dtype, seed=2)
    prog = arch.program(2, 64, 64, training_json=configs.bench_training())
    expect = {"conv_igemm", "conv_wgrad"} | ({"conv_bwd", "convt"} if (name, dtype) == ("cfg2", "bf16") else set())
    _check(prog, expect)
    assert prog.g.bwd_ops


def test_inference_program_and_a_second_program_of_the_architecture_are_bound(lib):
    arch = Architecture(configs.cfg2_unet_kpcn(), device="cpu", dtype="bf16", seed=2)
    first = arch.program(1, 64, 64)
    _check(first, {"conv_igemm"})
    assert not first.g.bwd_ops and not first.g.wgrad_records and not first.g.bwd_records
    second = arch.program(2, 32, 32)      # the shared parameter store is already finalized
    assert second is not first
    _check(second, {"conv_igemm"})
