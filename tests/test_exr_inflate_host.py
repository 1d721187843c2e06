"""The host half of the device inflate without a GPU: the options, and the upload buffer of a batch (openexr.pack_batch) followed through the
Python restatement of the inflate kernel (tests/exr_inflate_ref.py), the run copies and the numpy restatement of dd_exr_reconstruct
(tests/exr_device_ref.py): the planes must hold the bits of openexr.read_image."""
import types

import numpy as np
import pytest

import exr_device_ref as R
import exr_inflate_ref as I
from deepdenoiser_amd import openexr


@pytest.fixture(scope="module")
def files(tmp_path_factory):
    return R.fixtures(str(tmp_path_factory.mktemp("exr_inflate_host")))


def _required(parser, argv):
    """argv that the parser accepts: the positional / required arguments it names"""
    try:
        parser.parse_args(argv)
        return argv
    except SystemExit:
        return None


def test_the_three_parsers(capsys):
    from deepdenoiser_amd import predict, statistics, train
    for module in (train, statistics, predict):
        parser = module.parser()
        argv = next(a for a in (["t.json"], [], ["--input", "x"], ["x"]) if _required(module.parser(), a) is not None)
        assert parser.parse_args(argv).exr_inflate == "host"
        args = parser.parse_args(argv + ["--exr_decode", "device", "--exr_inflate", "device"])
        assert (args.exr_decode, args.exr_inflate) == ("device", "device")
        assert parser.parse_args(argv + ["--exr_decode", "device"]).exr_inflate == "host"
        capsys.readouterr()
        for extra in (["--exr_inflate", "device"], ["--exr_decode", "host", "--exr_inflate", "device"]):
            with pytest.raises(SystemExit):
                parser.parse_args(argv + extra)
            assert "--exr_inflate device needs --exr_decode device" in capsys.readouterr().err
        with pytest.raises(SystemExit):
            parser.parse_args(argv + ["--exr_decode", "device", "--exr_inflate", "gpu"])


def test_refusals_without_a_device():
    from deepdenoiser_amd.frame_bank import FrameBank
    with pytest.raises(ValueError):
        openexr.DeviceDecoder("cpu", inflate="device")
    frame_set = types.SimpleNamespace(tile=8, number_of_sources_per_example=1, source_spps=[4], scenes=[], skipped=[])
    with pytest.raises(ValueError, match="inflate='device' needs decode='device'"):
        FrameBank.for_passes(frame_set, {"Normal": 3}, {}, 4, device="cuda", decode="host", inflate="device")
    with pytest.raises(ValueError, match="inflate"):
        FrameBank.for_passes(frame_set, {"Normal": 3}, {}, 4, device="cuda", decode="device", inflate="elsewhere")
    with pytest.raises(ValueError, match="needs a device"):
        openexr.load_frame(".", None, inflate="device")


def _decode_batch(plans):
    """pack_batch -> restatement inflate of every stream -> the run copies -> reconstruct: the whole device path in numpy"""
    buffer, layout = openexr.pack_batch(plans)
    streams = buffer[layout["streams_at"]:layout["streams_at"] + layout["n_streams"] * openexr.STREAM_DTYPE.itemsize].view(openexr.STREAM_DTYPE)
    chunks = buffer[layout["chunks_at"]:layout["chunks_at"] + layout["n_chunks"] * openexr.CHUNK_DTYPE.itemsize].view(openexr.CHUNK_DTYPE)
    staged = np.full(layout["staged_bytes"], 0xA5, dtype=np.uint8)
    for s in streams:
        src, dst, n, size = int(s["src_offset"]), int(s["dst_offset"]), int(s["src_bytes"]), int(s["dst_bytes"])
        assert 0 <= src and src + n <= layout["source_bytes"] and dst % 16 == 0 and dst + (size + 15) // 16 * 16 <= layout["staged_bytes"]
        status, out = I.inflate(buffer[src:src + n].tobytes(), size)
        assert status == I.OK
        staged[dst:dst + size] = np.frombuffer(out, dtype=np.uint8)
    for src, dst, n in layout["runs"]:
        assert src % 16 == 0 and dst % 16 == 0 and src + n <= layout["source_bytes"] and dst + n <= layout["staged_bytes"]
        staged[dst:dst + n] = buffer[src:src + n]
    planes, counts = R.reconstruct(staged, chunks, [(p.height, p.width, p.channels, p.types, p.dst_masks) for p in plans])
    return planes, counts, layout


def test_batch_layout_reproduces_read_image(files):
    plans = [openexr.plan_file(path, channels) for _, path, channels in files]
    planes, counts, layout = _decode_batch(plans)
    assert layout["n_streams"] > 0 and layout["runs"]
    for (name, path, channels), plane, count in zip(files, planes, counts):
        want = openexr.read_image(path)[..., :channels]
        assert np.array_equal(R.bits(plane), R.bits(want)), name
        assert count == int(np.count_nonzero(~np.isfinite(want))), name
    # the upload is about the size of the files, not of the planes
    zips = [p for p in plans if p.compression == openexr.ZIP_COMPRESSION and p.height >= 16 and p.width >= 300]
    assert zips and all(p.source_layout()[0] < 0.8 * p.staged_bytes for p in zips)


def test_raw_chunk_in_zip_and_rle_files_alone(files):
    by_name = {name: (path, channels) for name, path, channels in files}
    for name, streams, runs in (("zip_with_raw_chunk", 2, 1), ("rle_coded_and_raw", 0, 1), ("none_37x21", 0, 1)):
        path, channels = by_name[name]
        plan = openexr.plan_file(path, channels)
        _, table, plain, places, refused = plan.source_layout()
        assert (len(table), len(plain), refused) == (streams, runs, False), name
        assert len(places) == len(plan.chunks)
        planes, _, _ = _decode_batch([plan])
        assert np.array_equal(R.bits(planes[0]), R.bits(openexr.read_image(path)[..., :channels])), name
