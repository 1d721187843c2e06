"""frame_launch.check_frame on CPU tensors against a CPU device: the exact message of every refusal that TemporalStabilizer.stabilize and
SequenceQuality.measure raise through it (tests/test_gpu_temporal.py and tests/test_gpu_sequence_quality.py provoke them on the device),
and the motion scale the two classes share.  No GPU, no library."""
import pytest
import torch

from deepdenoiser_amd import frame_launch

CPU = torch.device("cpu")
H, W = 4, 6


def _refused(message, what, v, **k):
    with pytest.raises(ValueError) as e:
        frame_launch.check_frame(what, v, H, W, CPU, **k)
    assert str(e.value) == message


def test_check_frame_messages():
    good = torch.zeros((H, W, 3))
    for v, k in ((good, {}), (good, dict(channels=(1, 3))), (good[..., :1], dict(channels=(1, 3))), (good[..., :2], dict(least=2)),
                 (torch.zeros((H, W, 5))[..., :3], dict(channels=(1, 3), least=2))):
        assert frame_launch.check_frame("a", v, H, W, CPU, **k) is None
    head = "prediction/A must be a float32 [4,6,C] tensor on cpu, not "
    _refused(head + "torch.float64 (4, 6, 3) on cpu", "prediction/A", good.double())                       # wrong dtype
    _refused(head + "torch.float32 (4, 5, 3) on cpu", "prediction/A", torch.zeros((H, W - 1, 3)))          # wrong shape
    _refused(head + "torch.float32 (4, 6) on cpu", "prediction/A", torch.zeros((H, W)))
    _refused(head + "ndarray", "prediction/A", good.numpy())
    _refused(head + "torch.float32 (4, 6, 3) on meta", "prediction/A", torch.zeros((H, W, 3), device="meta"))      # wrong device
    dense = "motion must be a dense [H,W,ld] frame or a [..., :C] view of one"
    _refused(dense, "motion", torch.zeros((2 * H, W, 3))[::2])                                              # not dense: every other row
    _refused(dense, "motion", torch.zeros((3, H, W)).permute(1, 2, 0))                                      # channels not innermost
    _refused(dense, "motion", torch.zeros((H, W, 6))[..., ::2])
    _refused("guide Normal: 1 or 3 channels are expected, not 2", "guide Normal", good[..., :2], channels=(1, 3))
    _refused("the target of prediction/A: 1 or 3 channels are expected, not 4", "the target of prediction/A", torch.zeros((H, W, 4)), channels=(1, 3))
    _refused("motion: at least 2 channels are expected, not 1", "motion", good[..., :1], least=2)
    # the order of the checks: the tensor, then its layout, then the channel set, then the least count
    _refused(dense, "motion", torch.zeros((2 * H, W, 1))[::2], least=2)
    _refused("motion: 1 or 3 channels are expected, not 2", "motion", good[..., :2], channels=(1, 3), least=3)


def test_motion_scale():
    assert frame_launch.motion_scale() == frame_launch.MOTION_SCALE == (-1.0, 1.0)
    assert frame_launch.motion_scale(None) == (-1.0, 1.0) and frame_launch.motion_scale([1, -1]) == (1.0, -1.0)
    for bad in ((1.0,), (1.0, 2.0, 3.0), (1.0, float("nan")), (float("inf"), 1.0)):
        with pytest.raises(ValueError) as e:
            frame_launch.motion_scale(bad)
        assert str(e.value) == "motion_scale must be two finite numbers, not %r" % (bad,)
