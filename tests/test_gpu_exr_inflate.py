"""zlib streams inflated on the device (csrc/dd_exr_inflate.hip, openexr.DeviceDecoder(inflate="device")).  Everything is bit equality: the
staged bytes against zlib.decompress, the statuses against the Python restatement (tests/exr_inflate_ref.py), the planes against
openexr.read_image and against the decoder that inflates on the host.  Only the enumerated stream lists run here; the mutation corpus stays
on the CPU, where the same decoder core runs it under sanitizers (tests/test_exr_inflate_core.py).

A file whose zlib stream is corrupt raises zlib.error out of DeviceDecoder.decode with inflate="host", whatever `errors` says (only ExrError is
kept per file); inflate="device" must do exactly the same, so "the other files of the request decode" is shown with a file whose stream is
valid but expands to the wrong size, which is an ExrError on both paths."""
import json
import os
import struct
import zlib

import numpy as np
import pytest
import torch

import exr_device_ref as R
import exr_inflate_ref as I
import frames_util as U
from deepdenoiser_amd import _lib, configs, openexr
from deepdenoiser_amd.architecture import Architecture
from deepdenoiser_amd.frame_bank import FrameBank, FrameSet

pytestmark = pytest.mark.gpu
GAP = 48                                                         # 0xA5 bytes between two streams' padded ranges


def _launch(entries):
    """entries: [(stream, dst_bytes)] -> (statuses, staged bytes, [(dst offset, dst_bytes)]); one launch"""
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    lib = _lib.load()
    table = np.zeros(len(entries), dtype=openexr.STREAM_DTYPE)
    src_at, dst_at, places = 0, GAP, []
    for k, (stream, size) in enumerate(entries):
        table[k] = (src_at, dst_at, len(stream), size)
        places.append((dst_at, size))
        src_at += len(stream)
        dst_at += (size + 15) // 16 * 16 + GAP
    source = torch.from_numpy(np.frombuffer(b"".join(s for s, _ in entries), dtype=np.uint8).copy()).cuda()
    staged = torch.full((dst_at,), I.FILL, dtype=torch.uint8, device="cuda")
    status = torch.full((len(entries),), -1, dtype=torch.int32, device="cuda")
    table_dev = torch.from_numpy(table.view(np.uint8).copy()).cuda()
    _lib.check(lib.dd_exr_inflate(table.ctypes.data, table_dev.data_ptr(), len(entries), source.data_ptr(), source.numel(), staged.data_ptr(),
                                  staged.numel(), status.data_ptr(), torch.cuda.current_stream().cuda_stream))
    return status.cpu().numpy().tolist(), staged.cpu().numpy(), places


def _outside_is_untouched(staged, places):
    mask = np.ones(staged.size, dtype=bool)
    for at, size in places:
        mask[at:at + (size + 15) // 16 * 16] = False
    return bool((staged[mask] == I.FILL).all())


def test_valid_streams_in_one_launch():
    entries = [(s, len(zlib.decompress(s))) for _, s, _ in I.valid_streams()]
    assert min(n for _, n in entries) == 1 and max(n for _, n in entries) == 491520
    statuses, staged, places = _launch(entries)
    assert statuses == [I.OK] * len(entries), [(n, _lib.INFLATE_STATUS_NAMES[s]) for (n, _, _), s in zip(I.valid_streams(), statuses) if s]
    for (name, stream, _), (at, size) in zip(I.valid_streams(), places):
        assert staged[at:at + size].tobytes() == zlib.decompress(stream), name
        assert (staged[at + size:at + (size + 15) // 16 * 16] == I.FILL).all(), name      # (an OK stream leaves its own padding too)
    assert _outside_is_untouched(staged, places)


def test_malformed_streams_between_valid_ones_in_one_launch():
    valid = [(n, s, len(zlib.decompress(s))) for n, s, _ in I.valid_streams() if len(s) <= 600]
    entries, kinds = [], []
    for k, (name, stream, size, status) in enumerate(m for m in I.malformed_streams() if len(m[1]) >= 1):      # (no bytes: refused by the host)
        entries += [(stream, size), valid[k % len(valid)][1:]]
        kinds += [(name, status), (valid[k % len(valid)][0], I.OK)]
    statuses, staged, places = _launch(entries)
    for (name, want), (stream, size), status, (at, _) in zip(kinds, entries, statuses, places):
        assert status == want == I.inflate(stream, size)[0], (name, _lib.INFLATE_STATUS_NAMES[status])
        if want == I.OK:
            assert staged[at:at + size].tobytes() == zlib.decompress(stream), name
    assert _outside_is_untouched(staged, places)


def test_a_record_that_does_not_fit_gets_its_status():
    """the device copy of the table is checked again: here it differs from the host copy"""
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    lib = _lib.load()
    stream = I.valid_streams()[0][1]
    good = np.zeros(3, dtype=openexr.STREAM_DTYPE)
    for k in range(3):
        good[k] = (0, 16 * k, len(stream), 3)
    bad = good.copy()
    bad[0]["dst_offset"], bad[2]["src_bytes"] = 8, len(stream) + 1
    source = torch.from_numpy(np.frombuffer(stream, dtype=np.uint8).copy()).cuda()
    staged = torch.full((48,), I.FILL, dtype=torch.uint8, device="cuda")
    status = torch.full((3,), -1, dtype=torch.int32, device="cuda")
    table_dev = torch.from_numpy(bad.view(np.uint8).copy()).cuda()
    _lib.check(lib.dd_exr_inflate(good.ctypes.data, table_dev.data_ptr(), 3, source.data_ptr(), source.numel(), staged.data_ptr(), 48,
                                  status.data_ptr(), torch.cuda.current_stream().cuda_stream))
    assert status.cpu().tolist() == [I.RECORD, I.OK, I.RECORD]
    want = np.full(48, I.FILL, dtype=np.uint8)
    want[16:19] = np.frombuffer(b"abc", dtype=np.uint8)
    assert np.array_equal(staged.cpu().numpy(), want)


# ---------------------------------------------------------------------------------------------------- the decoder
@pytest.fixture(scope="module")
def files(tmp_path_factory):
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    return R.fixtures(str(tmp_path_factory.mktemp("exr_inflate")))


def _want(path, channels):
    return np.ascontiguousarray(openexr.read_image(path)[..., :channels])


def _same(results, other, files):
    for (name, path, channels), (plane, count), (host_plane, host_count) in zip(files, results, other):
        want = _want(path, channels)
        assert plane.device.type == "cuda" and plane.dtype == torch.float32 and tuple(plane.shape) == want.shape, name
        assert np.array_equal(R.bits(plane.cpu().numpy()), R.bits(want)), name
        assert torch.equal(plane.view(torch.int32), host_plane.view(torch.int32)), name
        assert count == host_count == int(np.count_nonzero(~np.isfinite(want))), name


def test_every_fixture_file_in_one_call_and_in_three_batches(files):
    requests = [(path, channels) for _, path, channels in files]
    on_host = openexr.DeviceDecoder("cuda", threads=2).decode(requests)
    decoder = openexr.DeviceDecoder("cuda", threads=2, inflate="device")
    _same(decoder.decode(requests), on_host, files)
    assert decoder.host_fallbacks == 0 and decoder.launches == 1 and decoder.inflate_launches == 1
    # the upload is about the size of the files: the big ZIP file alone inflates to several times its stream bytes
    assert decoder.uploaded_bytes < sum(openexr.plan_file(*r).staged_bytes for r in requests)
    # three batches, one file above the limit
    names = ["zip_37x21", "none_5x3", "rle_16x300", "zips_1x1", "zip_20x1100_rgba"]
    by_name = {name: (name, path, channels) for name, path, channels in files}
    few = [by_name[n] for n in names]
    sizes = [openexr.plan_file(*f[1:]).staged_bytes for f in few]
    limit = 60000
    assert sizes[0] + sizes[1] <= limit < sizes[0] + sizes[1] + sizes[2] and sizes[2] + sizes[3] <= limit < sizes[4]      # {0, 1} {2, 3} {4 alone}
    small = openexr.DeviceDecoder("cuda", max_staged_bytes=limit, threads=2, inflate="device")
    small_host = openexr.DeviceDecoder("cuda", max_staged_bytes=limit, threads=2)
    for order in (few, few[::-1]):                                  # (the second call reuses the ring)
        _same(small.decode([f[1:] for f in order]), small_host.decode([f[1:] for f in order]), order)
    assert small.launches == 6 and small.host_fallbacks == 0 and small.decode([]) == []


def _outcome(decoder, requests, errors):
    try:
        return decoder.decode(requests, errors=errors)
    except Exception as e:                                          # noqa: BLE001 -- the type and the text are what is compared
        return type(e), str(e)


def test_corrupt_files_fail_as_on_the_host_path(files, tmp_path):
    by_name = {name: (path, channels) for name, path, channels in files}
    good_a, good_b = by_name["zip_5x3"], by_name["none_5x3"]
    buf = bytearray(open(by_name["zip_16x300"][0], "rb").read())
    plan = openexr.plan_file(*by_name["zip_16x300"])
    assert plan.pieces[0][1] and len(plan.pieces[0][0]) > 1000      # one coded chunk
    chunk_at = len(buf) - len(plan.pieces[0][0])
    flipped, cut, wrong_size = (str(tmp_path / n) for n in ("flipped.exr", "cut.exr", "wrong_size.exr"))
    b = bytearray(buf)
    b[chunk_at + 500] ^= 0x40
    open(flipped, "wb").write(bytes(b))
    b = bytearray(buf)
    struct.pack_into("<i", b, chunk_at - 4, len(plan.pieces[0][0]) - 7)      # the chunk's size field: its stream ends 7 bytes early
    open(cut, "wb").write(bytes(b))
    b = bytearray(open(by_name["zip_37x21"][0], "rb").read())
    last = openexr.plan_file(*by_name["zip_37x21"]).pieces[-1]
    assert last[1] and last[2] == 5 * 252
    short = zlib.compress(bytes(1000))
    at = len(b) - len(last[0])
    struct.pack_into("<i", b, at - 4, len(short))
    open(wrong_size, "wb").write(bytes(b[:at]) + short)
    host = openexr.DeviceDecoder("cuda", threads=2)
    for broken, kind in ((flipped, zlib.error), (cut, zlib.error), (wrong_size, openexr.ExrError)):
        requests = [good_a, (broken, 3), good_b]
        for errors in ("raise", "return"):
            device = openexr.DeviceDecoder("cuda", threads=2, inflate="device")
            want, have = _outcome(host, requests, errors), _outcome(device, requests, errors)
            assert device.host_fallbacks == 1, broken
            if kind is zlib.error or errors == "raise":
                assert isinstance(want, tuple) and want[0] is kind and have == want, (broken, errors, have, want)
            else:
                assert isinstance(have[1], openexr.ExrError) and str(have[1]) == str(want[1]) and "chunk expands to 1000 bytes" in str(have[1])
                for k, good in ((0, good_a), (2, good_b)):          # the other files of the request decode
                    assert np.array_equal(R.bits(have[k][0].cpu().numpy()), R.bits(_want(*good))) and have[k][1] == want[k][1] == 0
    # two broken files in one request: both are redone, the first in input order decides
    device = openexr.DeviceDecoder("cuda", threads=2, inflate="device")
    results = device.decode([(wrong_size, 3), good_a, (wrong_size, 3)], errors="return")
    assert device.host_fallbacks == 2 and isinstance(results[0], openexr.ExrError) and isinstance(results[2], openexr.ExrError)
    assert np.array_equal(R.bits(results[1][0].cpu().numpy()), R.bits(_want(*good_a)))


def test_refused_and_corrupt_files_among_several_batches(files, tmp_path, monkeypatch):
    """One call of four batches through the ring of two, then two host redos through ring slot 0: a file the device is not given at all
    (a stream above the limit, here lowered so that a 16-line chunk of 21 pixels is above it; zlib takes it, so its redo ends in a launch) and
    a file whose last stream holds the wrong number of bytes (its redo ends in the host's ExrError, without a launch)."""
    by_name = {name: (path, channels) for name, path, channels in files}
    monkeypatch.setattr(openexr.decode, "MAX_STREAM_BYTES", 4000)
    refused = by_name["zip_37x21"]
    assert openexr.plan_file(*refused).source_layout()[4] and not openexr.plan_file(*by_name["zip_5x3"]).source_layout()[4]
    b = bytearray(open(by_name["zips_37x21"][0], "rb").read())                  # (one line a chunk: none of them is above the limit)
    last = openexr.plan_file(*by_name["zips_37x21"]).pieces[-1]
    assert last[2] == 252
    short = zlib.compress(bytes(100))
    at = len(b) - len(last[0])
    struct.pack_into("<i", b, at - 4, len(short))
    wrong_size = str(tmp_path / "wrong_size.exr")
    open(wrong_size, "wb").write(bytes(b[:at]) + short)
    requests = [by_name["zip_5x3"], by_name["zips_5x3"], refused, (wrong_size, 3), by_name["none_5x3"], by_name["zip_5x3"]]
    plans = [openexr.plan_file(*r) for r in requests]
    assert [p.source_layout()[4] for p in plans] == [False, False, True, False, False, False]
    sizes = [p.staged_bytes for p in plans]
    limit = 9720
    assert sizes[0] + sizes[1] + sizes[2] > limit >= sizes[2] and sizes[2] + sizes[3] > limit                   # {0, 1} {2: refused, so empty}
    assert sizes[3] + sizes[4] <= limit < sizes[3] + sizes[4] + sizes[5]                                        # {3, 4} {5}
    device = openexr.DeviceDecoder("cuda", max_staged_bytes=limit, threads=2, inflate="device")
    results = device.decode(requests, errors="return")
    assert device.host_fallbacks == 2
    assert device.launches == 3 + 1                                 # the three batches that hold a file, and the redo of the refused file
    assert isinstance(results[3], openexr.ExrError) and "chunk expands to 100 bytes, expected 252" in str(results[3])
    for k in (0, 1, 2, 4, 5):
        plane, count = results[k]
        assert np.array_equal(R.bits(plane.cpu().numpy()), R.bits(_want(*requests[k]))) and count == 0, k


# ---------------------------------------------------------------------------------------------------- end to end
T, SPP, BEST, S = 16, 4, 16, 2


@pytest.fixture(scope="module")
def arch():
    aj = configs.architecture(filters=(16, 24), convs=1, flag_mode="NONE",
                              combined={"Diffuse": {"Color": "Diffuse Color", "Direct": "Diffuse Direct", "Indirect": "Diffuse Indirect"},
                                        "Alpha": {"Color": "Alpha", "Direct": "", "Indirect": ""}})
    return Architecture(aj, device="cpu")


@pytest.fixture(scope="module")
def tree(tmp_path_factory, arch):
    """Two scenes of different sizes and one scene with a NaN sample, as EXR renderings (the tree of tests/test_gpu_exr_decode.py)."""
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    root = str(tmp_path_factory.mktemp("exr_inflate_frames"))
    rng = np.random.default_rng(3)
    source = [f.name for f in arch.feature_predictions + arch.auxiliary_features if f.load_data]
    target = [f.name for f in arch.feature_predictions if f.load_data and f.is_target]
    U.write_scene(root, "a_good", [SPP], source, target, 32, 48, rng, sources=S, target_spp=BEST)
    U.write_scene(root, "b_nan", [SPP], source, target, 32, 32, rng, sources=S, target_spp=BEST)
    bad = U.image(rng, 32, 32, "Diffuse Color")
    bad[5, 7, 1] = np.nan
    openexr.write_image(os.path.join(root, "OpenEXR", "b_nan", U.rendering_name("b_nan", SPP, 1), "render_Diffuse Color_0001.exr"), bad)
    U.write_scene(root, "c_good", [SPP], source, target, 40, 33, rng, sources=S, target_spp=BEST)
    path = U.write_json(root, {"training": ["a_good", "b_nan", "c_good"]}, T, [SPP], S, source, target)
    return root, path


def test_frame_bank_is_the_same_bank(tree, arch):
    banks = {}
    for decode, inflate in (("host", "host"), ("device", "device")):
        lines = []
        frame_set = FrameSet.from_json(tree[1], "training", log=lines.append)
        banks[decode] = FrameBank(arch, frame_set, SPP, "cuda", threads=2, log=lines.append, decode=decode, inflate=inflate)
        banks[decode].lines = lines
    host, device = banks["host"], banks["device"]
    assert (device.decode, device.inflate, host.inflate) == ("device", "device", "host")
    assert device.decoder.inflate_launches > 0 and device.decoder.host_fallbacks == 0
    assert device.hw == host.hw and device.skipped == host.skipped and device.lines == host.lines
    assert len(host.skipped) == 1 and "b_nan" in host.skipped[0][0] and "which is not finite" in host.lines[0]
    assert [s.directory for s in device.scenes] == [s.directory for s in host.scenes]
    for name in host.planes:
        for p, (a, b) in enumerate(zip(host.planes[name], device.planes[name])):
            assert (a is None) == (b is None), (name, p)
            if a is not None:
                assert b.device.type == "cuda" and a.shape == b.shape and torch.equal(a.view(torch.int32), b.view(torch.int32)), (name, p)


def test_statistics_file_is_byte_identical(tree):
    from deepdenoiser_amd import statistics
    written = {}
    for options in ((), ("--exr_decode", "device", "--exr_inflate", "device")):
        out = os.path.join(tree[0], "statistics_inflate_" + ("device" if options else "host"))
        lines = []
        args = statistics.parser().parse_args([tree[1], "--mode", "training", "--threads", "2", "--output", out] + list(options))
        paths = statistics.main(args, log=lines.append)
        written[bool(options)] = (open(paths[0], "rb").read(), [line.replace(out, "") for line in lines])
    assert written[True] == written[False] and len(json.loads(written[False][0])) > 0


def test_load_frame_with_device_inflate(tree, arch):
    directory = os.path.join(tree[0], "OpenEXR", "a_good", U.rendering_name("a_good", SPP, 0))
    host = openexr.load_frame(directory, arch)
    device = openexr.load_frame(directory, arch, device="cuda", inflate="device")
    assert list(device) == list(host)
    for key, want in host.items():
        have = device[key]
        assert torch.is_tensor(have) and have.device.type == "cuda" and tuple(have.shape) == want.shape, key
        assert np.array_equal(R.bits(have.cpu().numpy()), R.bits(want)), key
