"""What the device EXR and PNG encoders share (deepdenoiser_amd/batch_encode.py), without a device: the slot layout of a batch, the one
alignment rule under its three names, the two constructors' refusal of a device that is no GPU, and that the two subclasses share no state."""
import pytest

from deepdenoiser_amd import batch_encode, openexr, png
from deepdenoiser_amd.openexr import records


class _Plan:
    def __init__(self, slot_bytes, n_records):
        self.slot_bytes, self.records = slot_bytes, [None] * n_records


def test_slot_layout_is_the_running_sums():
    plans = [_Plan(48, 3), _Plan(16, 1), _Plan(0, 0), _Plan(1600, 7)]
    bases, first, total, n = batch_encode.slot_layout(plans, lambda p: len(p.records))
    assert bases == [0, 48, 64, 64] and first == [0, 3, 4, 4] and total == 1664 and n == 11
    assert batch_encode.slot_layout([], len) == ([], [], 16, 0)                             # an empty total floors at one slot
    assert batch_encode.slot_layout([_Plan(0, 2)], lambda p: len(p.records)) == ([0], [0], 16, 2)


def test_slot_layout_is_what_both_table_layouts_start_from():
    exr_plans = [openexr.plan_write("a.exr", 37, 21, ["R", "G", "B"], ["float"] * 3), openexr.plan_write("b.exr", 1, 1, ["Y"], ["half"])]
    layout = openexr.encode._tables_layout(exr_plans)
    bases, first, total, n = batch_encode.slot_layout(exr_plans, lambda p: len(p.chunks))
    assert (layout["bases"], layout["first_chunk"], layout["total"], layout["n_chunks"]) == (bases, first, total, n)
    assert bases == [0, exr_plans[0].slot_bytes] and first == [0, len(exr_plans[0].chunks)] and n == 3 + 1       # ZIP: 16 lines per chunk
    png_plans = [png.plan_png("a.png", 37, 21, 3, segment_rows=8), png.plan_png("b.png", 1, 1, 1)]
    layout = png._tables_layout(png_plans)
    bases, first, total, n = batch_encode.slot_layout(png_plans, lambda p: len(p.segments))
    assert (layout["bases"], layout["first"], layout["total"], layout["n_segments"]) == (bases, first, total, n)
    assert bases == [0, png_plans[0].slot_bytes] and first == [0, 5] and n == 6 and total == png_plans[0].slot_bytes + 16


def test_one_alignment_rule_under_every_name():
    for n, want in ((0, 0), (1, 16), (15, 16), (16, 16), (17, 32)):
        assert batch_encode.align16(n) == records._align(n) == png._align(n) == want
    assert records._STAGE_ALIGN == batch_encode.ALIGN == 16
    assert records.timed is batch_encode.timed


def test_a_device_that_is_no_gpu_is_refused_with_the_encoders_own_message():
    with pytest.raises(ValueError) as e:
        openexr.DeviceEncoder("cpu")
    assert str(e.value) == "EXR files are encoded on a GPU: cpu is none"
    with pytest.raises(ValueError) as e:
        png.DevicePngEncoder("cpu")
    assert str(e.value) == "PNG files are encoded on a GPU: cpu is none"
    with pytest.raises(openexr.ExrError):                                                   # (the compression is looked at first, as before)
        openexr.DeviceEncoder("cpu", compression=99)


def test_the_subclasses_share_no_mutable_class_state():
    assert openexr.DeviceEncoder.time_launches is False and png.DevicePngEncoder.time_launches is False
    png.DevicePngEncoder.time_launches = True
    try:
        assert openexr.DeviceEncoder.time_launches is False and batch_encode.BatchEncoder.time_launches is False
    finally:
        del png.DevicePngEncoder.time_launches
    assert png.DevicePngEncoder.time_launches is False
    openexr.DeviceEncoder.time_launches = True
    try:
        assert png.DevicePngEncoder.time_launches is False
    finally:
        del openexr.DeviceEncoder.time_launches
    for cls in (batch_encode.BatchEncoder, openexr.DeviceEncoder, png.DevicePngEncoder):    # counters and event lists exist per instance only
        for name, value in vars(cls).items():
            assert not isinstance(value, (list, dict, set)), (cls.__name__, name)
    assert "_thresholds" in png.DevicePngEncoder._buffers and "_thresholds" not in openexr.DeviceEncoder._buffers
