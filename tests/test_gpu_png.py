"""PNG output written on the device: dd_png_pack against the reference (tests/png_ref.py: byte equality of the filtered rows), dd_png_deflate
against the digests of the CPU build of the same core (tests/golden/png_segments.json), DevicePngEncoder's files read back by the reference
decoder (and Pillow where it is installed), and predict.main with --png --png_encode device."""
import io
import json
import os
import zlib

import numpy as np
import pytest
import torch

import png_ref as P
from deepdenoiser_amd import _lib, png

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
FILL = 0xA5
GAP = 32                                      # guard bytes between slots that must keep their fill


def _need_gpu():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")


def _align(n):
    return (n + 15) // 16 * 16


def _thresholds():
    return torch.from_numpy(P.THRESHOLDS.copy()).cuda()


def _plane(image, plane_channels, src_channels):
    """the fp32 plane [H, W, plane_channels] whose channels src_channels hold `image`'s; the others hold a value that must not show"""
    plane = np.full(image.shape[:2] + (plane_channels,), np.float32(0.77), dtype=np.float32)
    for c, s in enumerate(src_channels):
        plane[:, :, s] = image[:, :, c]
    return plane


def _pack(lib, image_rows, segment_rows, total, device_images=None, device_segments=None):
    """one dd_png_pack launch into a buffer of fill -> its bytes; the device copies of the tables may differ from the host's"""
    images = np.zeros(len(image_rows), dtype=png.IMAGE_DTYPE)
    for row, (plane, h, w, c, n, src_channels, exposure) in zip(images, image_rows):
        row["src"], row["H"], row["W"], row["C"], row["n_channels"], row["exposure"] = plane.data_ptr(), h, w, c, n, exposure
        row["src_channel"][:n] = src_channels
    segments = np.zeros(len(segment_rows), dtype=png.SEGMENT_DTYPE)
    segments[:] = [tuple(r) + (0,) for r in segment_rows]
    dev_images = images.copy() if device_images is None else device_images(images.copy())
    dev_segments = segments.copy() if device_segments is None else device_segments(segments.copy())
    staged = torch.full((total + GAP,), FILL, dtype=torch.uint8, device="cuda")
    dev_s, dev_i = torch.from_numpy(dev_segments.view(np.uint8).copy()).cuda(), torch.from_numpy(dev_images.view(np.uint8).copy()).cuda()
    thresholds = _thresholds()
    _lib.check(lib.dd_png_pack(segments.ctypes.data, dev_s.data_ptr(), len(segments), images.ctypes.data, dev_i.data_ptr(), len(images), thresholds.data_ptr(),
                               staged.data_ptr(), total, torch.cuda.current_stream().cuda_stream))
    return staged.cpu().numpy()


# ---------------------------------------------------------------------------------------------------- pack
LAYOUTS = [(1, 1, [0]), (3, 3, [2, 1, 0]), (3, 4, [3, 0, 2]), (1, 4, [2])]      # n, plane channels, the plane channel of every byte of a pixel


def test_pack_equals_the_reference(lib):
    """24 sizes x 4 channel layouts in ONE launch; the input (edge values, all filter types, a constant), the exposure (1, 2.5) and the segment
    rows (1, 3, 8, with a short last segment wherever H is no multiple) cycle so that every combination occurs"""
    _need_gpu()
    image_rows, segment_rows, expected, keep, at, k = [], [], [], [], 0, 0
    combos = set()
    for h in (1, 2, 9, 17):
        for w in (1, 2, 5, 16, 21, 67):
            for n, c, src_channels in LAYOUTS:
                kind, exposure, rows_per = k % 3, (1.0, 2.5)[(k // 3) % 2], (1, 3, 8)[(k // 6) % 3]
                combos.add((kind, exposure, rows_per))
                k += 1
                image = (P.edge_image(h, w, n), P.all_filters_image(h, w, n, seed=k), np.full((h, w, n), 0.18, dtype=np.float32))[kind]
                keep.append(torch.from_numpy(_plane(image, c, src_channels)).cuda())
                want = P.filtered_rows(image, exposure)
                index = len(image_rows)
                image_rows.append((keep[-1], h, w, c, n, src_channels, exposure))
                for y0 in range(0, h, rows_per):
                    count = min(rows_per, h - y0)
                    at += GAP
                    segment_rows.append((at, index, y0, count))
                    expected.append(want[y0:y0 + count].reshape(-1))
                    at += _align(expected[-1].size)
    assert len(combos) == 18
    have = _pack(lib, image_rows, segment_rows, at)
    owned = np.zeros(have.size, dtype=bool)
    for (offset, index, y0, count), want in zip(segment_rows, expected):
        got = have[offset:offset + want.size]
        assert np.array_equal(got, want), "image %d (%s) rows %d+%d" % (index, image_rows[index][1:], y0, count)
        assert (have[offset + want.size:offset + _align(want.size)] == 0).all()      # the padding is written as zero
        owned[offset:offset + _align(want.size)] = True
    assert (have[~owned] == FILL).all()                            # nothing outside a segment's own bytes, nor behind the buffer


def test_pack_wide_rows_and_full_staging(lib):
    """more than one pass of the 256 threads over a row, a segment that fills the staging buffer to within a row, and a segment below another"""
    _need_gpu()
    image = P.noisy_gradient(14, 1000, 3, seed=3)
    image[5, 7, 1] = np.nan
    plane = torch.from_numpy(image).cuda()
    want = P.filtered_rows(image, 1.0)
    rows_per = png.STAGE_BYTES // want.shape[1]                   # 12 rows of 3001 bytes
    assert rows_per == 12
    n0, n1 = rows_per * want.shape[1], (14 - rows_per) * want.shape[1]
    segment_rows = [(GAP, 0, 0, rows_per), (2 * GAP + _align(n0), 0, rows_per, 14 - rows_per)]
    total = 2 * GAP + _align(n0) + _align(n1)
    have = _pack(lib, [(plane, 14, 1000, 3, 3, [0, 1, 2], 1.0)], segment_rows, total)
    assert np.array_equal(have[GAP:GAP + n0], want[:rows_per].reshape(-1))
    assert np.array_equal(have[segment_rows[1][0]:segment_rows[1][0] + n1], want[rows_per:].reshape(-1))
    owned = np.zeros(have.size, dtype=bool)
    owned[GAP:GAP + _align(n0)] = True
    owned[segment_rows[1][0]:segment_rows[1][0] + _align(n1)] = True
    assert (have[~owned] == FILL).all()


def test_pack_trusts_no_device_record(lib):
    """the host copy is valid; the device copy names an image, rows, an offset, a channel or a width that do not fit: such a segment writes
    nothing, the others of the same launch are correct"""
    _need_gpu()
    images = [P.all_filters_image(20, 9, 3, seed=1), P.noisy_gradient(20, 9, 3, seed=2)]
    planes = [torch.from_numpy(a).cuda() for a in images]
    wants = [P.filtered_rows(a) for a in images]
    image_rows = [(planes[k], 20, 9, 3, 3, [0, 1, 2], 1.0) for k in range(2)]
    slot = 1024
    segment_rows = [(k * slot, k // 4, 4 * (k % 4), 4) for k in range(8)]      # 4 rows of 28 bytes each; segments 0 .. 3 of image 0, 4 .. 7 of image 1

    def check(have, written):
        owned = np.zeros(have.size, dtype=bool)
        for k in written:
            offset, index, y0, count = segment_rows[k]
            want = wants[index][y0:y0 + count].reshape(-1)
            assert np.array_equal(have[offset:offset + want.size], want), k
            owned[offset:offset + _align(want.size)] = True
        assert (have[~owned] == FILL).all()

    def bad_segments(table):
        table[0]["image"], table[1]["y0"], table[2]["rows"], table[3]["offset"], table[4]["offset"], table[5]["y0"], table[6]["rows"] = 2, 17, 17, 8 * slot - 16, 8, -1, 0
        return table
    check(_pack(lib, image_rows, segment_rows, 8 * slot, device_segments=bad_segments), [7])
    for field, value in (("n_channels", 2), ("src_channel", 3), ("W", 1 << 20), ("W", 4097), ("C", 33), ("H", 3), ("src", 0)):
        def bad_image(table, field=field, value=value):
            if field == "src_channel":
                table[0]["src_channel"][2] = value
            else:
                table[0][field] = value
            return table
        check(_pack(lib, image_rows, segment_rows, 8 * slot, device_images=bad_image), [4, 5, 6, 7])
    check(_pack(lib, image_rows, segment_rows, 8 * slot), range(8))


# ---------------------------------------------------------------------------------------------------- deflate
def _segment_sources():
    """[(job name, [the bytes of its segments])]: the filtered rows of the test images cut as tests/png_core_main.cpp cuts them, and the byte jobs"""
    out = []
    for name, image, exposure, rows_per in P.images():
        data, pieces, at = png.filtered_rows(image, exposure).tobytes(), [], 0
        for n in P.image_segment_lengths(image, rows_per):
            pieces.append(data[at:at + n])
            at += n
        out.append(("image " + name, pieces))
    for name, (data, lengths) in zip(P.job_names()[len(out):], P.byte_jobs()):
        pieces, at = [], 0
        for n in lengths:
            pieces.append(data[at:at + n])
            at += n
        out.append((name, pieces))
    return out


def _deflate_launch(lib, segments, bad_records=()):
    """segments: [(bytes, last)], all in one launch, every slot and the workspace with a guard of fill around it
    -> (statuses, sizes, adlers, out, records, workspace)"""
    records = np.zeros(len(segments), dtype=png.STREAM_DTYPE)
    src_at = out_at = 0
    for k, (t, last) in enumerate(segments):
        records[k] = (src_at, out_at + 16, len(t), len(t) - 1, int(last), 0)
        src_at += _align(len(t))
        out_at += 16 + _align(len(t))
    src = np.zeros(max(src_at, 16), dtype=np.uint8)
    for r, (t, _) in zip(records, segments):
        src[r["src_offset"]:r["src_offset"] + len(t)] = np.frombuffer(t, dtype=np.uint8)
    device_records = records.copy()
    for k, field, value in bad_records:
        device_records[k][field] = value
    need = lib.dd_png_deflate_workspace(len(segments))
    assert need == 4 * _lib.DEFLATE_BLOCK_TOKENS * len(segments)
    out = torch.full((out_at + 16,), FILL, dtype=torch.uint8, device="cuda")
    workspace = torch.full((need + 64,), FILL, dtype=torch.uint8, device="cuda")
    three = torch.full((3 * len(segments),), -7, dtype=torch.int32, device="cuda")
    dev_src, dev_records = torch.from_numpy(src).cuda(), torch.from_numpy(device_records.view(np.uint8).copy()).cuda()
    n = len(segments)
    _lib.check(lib.dd_png_deflate(records.ctypes.data, dev_records.data_ptr(), n, dev_src.data_ptr(), src.size, out.data_ptr(), out.numel(), workspace.data_ptr(),
                                  need, three.data_ptr(), three.data_ptr() + 4 * n, three.data_ptr() + 8 * n, torch.cuda.current_stream().cuda_stream))
    three = three.cpu().numpy()
    return three[:n], three[n:2 * n], three[2 * n:].view(np.uint32), out.cpu().numpy(), records, workspace.cpu().numpy()


@pytest.fixture(scope="module")
def deflated(lib):
    _need_gpu()
    jobs = _segment_sources()
    segments = [(t, k == len(pieces) - 1) for _, pieces in jobs for k, t in enumerate(pieces)]
    return jobs, segments, _deflate_launch(lib, segments), _deflate_launch(lib, segments)


def test_deflate_equals_the_cpu_build(deflated):
    jobs, segments, (statuses, sizes, adlers, out, records, _), _ = deflated
    golden = json.load(open(os.path.join(HERE, "golden", "png_segments.json")))
    assert sorted(golden) == sorted(name for name, _ in jobs)
    at = 0
    for name, pieces in jobs:
        have, bodies = [], []
        for k, t in enumerate(pieces):
            r = records[at]
            body = out[r["dst_offset"]:r["dst_offset"] + sizes[at]].tobytes()
            have.append((statuses[at], sizes[at], adlers[at], body))
            bodies.append(body if statuses[at] == P.OK else png.stored_blocks(t, k == len(pieces) - 1))
            at += 1
        assert P.digest(have) == golden[name], name
        assert zlib.decompress(P.stream_of(bodies, [h[2] for h in have], [len(t) for t in pieces])) == b"".join(pieces), name
    assert at == len(segments)
    assert any(s["status"] == P.RAW for s in golden["image noise_rgb_64x64"])      # what the encoder test below relies on


def test_deflate_writes_nothing_outside_its_slots(deflated):
    _, segments, (statuses, sizes, adlers, out, records, workspace), _ = deflated
    owned = np.zeros(out.size, dtype=bool)
    for r in records:
        owned[r["dst_offset"]:r["dst_offset"] + _align(int(r["dst_capacity"]))] = True
    assert (out[~owned] == FILL).all()
    assert (workspace[4 * _lib.DEFLATE_BLOCK_TOKENS * len(segments):] == FILL).all()


def test_deflate_second_launch_gives_the_same_bytes(deflated):
    _, _, first, second = deflated
    assert all(np.array_equal(first[k], second[k]) for k in range(4))


def test_deflate_trusts_no_device_record(lib):
    _need_gpu()
    segments = [(b"abcabcabc" * 40, False), (b"\x00" * 500, False), (P.filtered_rows(P.noisy_gradient(12, 30, 3)).tobytes(), True), (b"x" * 300, False),
                (b"y" * 300, True), (b"z" * 300, False)]
    bad = [(0, "src_offset", 1 << 40), (1, "dst_offset", 24), (3, "dst_capacity", 1 << 29), (4, "src_bytes", -3), (5, "last", 2)]
    statuses, sizes, adlers, out, records, _ = _deflate_launch(lib, segments, bad)
    assert list(statuses) == [P.RECORD, P.RECORD, P.OK, P.RECORD, P.RECORD, P.RECORD] and [sizes[k] for k in (0, 1, 3, 4, 5)] == [0] * 5
    r = records[2]
    body = out[r["dst_offset"]:r["dst_offset"] + sizes[2]].tobytes()
    assert zlib.decompress(body, -15) == segments[2][0] and adlers[2] == zlib.adler32(segments[2][0])
    owned = np.zeros(out.size, dtype=bool)
    owned[r["dst_offset"]:r["dst_offset"] + _align(int(r["dst_capacity"]))] = True
    assert (out[~owned] == FILL).all()                             # nothing was written through a refused record


# ---------------------------------------------------------------------------------------------------- files
def _pillow():
    try:
        from PIL import Image
        return Image
    except ImportError:
        return None


def _check_file(path, image, exposure):
    data = open(path, "rb").read()
    have = P.decode(data)
    want = P.quantise(image, exposure)
    assert have["chunks"] == [b"IHDR", b"sRGB", b"IDAT", b"IEND"] and have["srgb"] == b"\x00" and have["idat"][:2] == b"\x78\x01", path
    assert np.array_equal(have["image"], want), path
    assert np.array_equal(have["rows"], png.filtered_rows(image, exposure)), path      # the inflated IDAT is the host path's
    assert np.array_equal(P.decode(png.encode_host(image, exposure))["image"], want), path
    Image = _pillow()
    if Image is not None:
        picture = Image.open(io.BytesIO(data))
        picture.load()
        assert picture.mode == ("RGB" if want.shape[2] == 3 else "L") and np.array_equal(np.asarray(picture).reshape(want.shape), want), path


@pytest.mark.parametrize("segment_rows", [None, 16])
def test_encoder_files_decode_to_the_reference(lib, tmp_path, segment_rows):
    """67 x 53 RGB, 21 x 17 gray, 1 x 1 and 64 x 64 uniform noise in one batch; with 16 rows per segment the noise is four RAW segments"""
    _need_gpu()
    by_name = {name: (image, exposure) for name, image, exposure, _ in P.images()}
    names = ["gradient_rgb_53x67", "gradient_gray_17x21", "one_pixel", "noise_rgb_64x64", "edge_rgb", "smooth_rgb_96x128"]
    assert by_name["gradient_rgb_53x67"][0].shape == (53, 67, 3) and by_name["gradient_gray_17x21"][0].shape == (17, 21, 1)
    encoder = png.DevicePngEncoder("cuda", threads=3, segment_rows=segment_rows)
    tensors = [torch.from_numpy(by_name[name][0]).cuda() for name in names]
    tensors[1] = tensors[1][:, :, 0].contiguous()                  # [H, W] is a gray pass
    requests = [(str(tmp_path / (name + ".png")), t, by_name[name][1]) for name, t in zip(names, tensors)]
    assert encoder.encode(requests) == [path for path, _, _ in requests]
    for (path, _, exposure), name in zip(requests, names):
        _check_file(path, by_name[name][0], exposure)
    assert (encoder.pack_launches, encoder.deflate_launches) == (1, 1)
    assert encoder.raw_segments >= (5 if segment_rows else 2)     # the noise (RAW in the CPU build: tests/golden/png_segments.json) and the single pixel
    shapes = [by_name[name][0].shape for name in names]
    assert encoder.segments == sum(-(-h // (segment_rows or png.default_segment_rows(w, n))) for h, w, n in shapes)
    assert encoder.segments == (19 if segment_rows else 7)        # (96 rows of 385 bytes are two default segments)
    encoder.release()


def test_encoder_reuses_its_buffers_and_refuses_what_it_cannot_take(lib, tmp_path):
    _need_gpu()
    encoder = png.DevicePngEncoder("cuda")
    big_image, small_image = P.noisy_gradient(40, 64, 3, seed=1), P.noisy_gradient(5, 3, 1, seed=2)
    big, small = torch.from_numpy(big_image).cuda(), torch.from_numpy(small_image).cuda()
    encoder.encode([(str(tmp_path / "a.png"), big, 1.0)])
    kept = encoder._out.data_ptr(), encoder._pinned.data_ptr(), encoder._packed.data_ptr()
    encoder.encode([(str(tmp_path / "b.png"), small, 2.5)])
    assert (encoder._out.data_ptr(), encoder._pinned.data_ptr(), encoder._packed.data_ptr()) == kept
    _check_file(str(tmp_path / "a.png"), big_image, 1.0)
    _check_file(str(tmp_path / "b.png"), small_image, 2.5)
    assert encoder.encode([]) == []
    with pytest.raises(ValueError):
        encoder.encode([(str(tmp_path / "c.png"), small.cpu(), 1.0)])
    with pytest.raises(ValueError):
        encoder.encode([(str(tmp_path / "c.png"), torch.zeros(4, 4, 2, device="cuda"), 1.0)])
    with pytest.raises(ValueError):
        encoder.encode([(str(tmp_path / "c.png"), torch.zeros(2, 4097, 3, device="cuda"), 1.0)])
    encoder.release()
    assert encoder._out is None and encoder._pinned is None


# ---------------------------------------------------------------------------------------------------- command line
def test_predict_png_encode_device_writes_the_same_pictures(tmp_path):
    _need_gpu()
    from deepdenoiser_amd import configs, openexr, predict, tf_checkpoint
    from deepdenoiser_amd.architecture import Architecture
    from deepdenoiser_amd.prediction import Predictor
    FH, FW, T, O = 40, 72, 32, 4
    aj = configs.architecture(filters=(16, 24), convs=1, flag_mode="NONE")
    aj["model_directory"] = "model"
    json.dump(aj, open(tmp_path / "architecture.json", "w"))
    arch = Architecture(aj, device="cuda", dtype="f32", seed=2)
    Predictor(arch, tile_size=T, tile_overlap_size=O).prepare(FH, FW)              # (creates the parameters)
    tf_checkpoint.save_variables(arch, str(tmp_path / "model"), global_step=1)
    rng = np.random.default_rng(5)
    runs = {}
    for mode in ("plain", "host", "device"):
        runs[mode] = tmp_path / ("frame_" + mode)
        runs[mode].mkdir()
    for f in arch.feature_predictions + arch.auxiliary_features:
        if f.load_data:
            image = rng.random((FH, FW, 3)).astype(np.float32)
            for src in runs.values():
                openexr.write_image(str(src / ("render_%s_0001.exr" % f.name)), image)
    outputs = {}
    for mode, src in runs.items():
        inputs = set(os.listdir(src))
        extra = [] if mode == "plain" else ["--png", "--png_encode", mode, "--exposure", "1.5"]
        predict.main(predict.parser().parse_args([str(tmp_path / "architecture.json"), "--input", str(src), "--tile_size", str(T), "--tile_overlap_size", str(O),
                                                  "--dtype", "f32"] + extra))
        outputs[mode] = sorted(set(os.listdir(src)) - inputs)
    arrays = [n for n in outputs["plain"] if n.endswith(".npy")]
    assert arrays and outputs["plain"] == arrays
    assert outputs["host"] == outputs["device"] == sorted(arrays + [n[:-4] + ".png" for n in arrays])      # <Pass>.png for every key
    for n in arrays:
        assert open(runs["plain"] / n, "rb").read() == open(runs["host"] / n, "rb").read() == open(runs["device"] / n, "rb").read(), n
        host, device = (P.decode(open(runs[mode] / (n[:-4] + ".png"), "rb").read()) for mode in ("host", "device"))
        assert np.array_equal(host["image"], device["image"]) and np.array_equal(host["rows"], device["rows"]), n
        assert np.array_equal(device["image"], P.quantise(np.load(runs["device"] / n), 1.5)), n
