"""EXR output written on the device: dd_exr_pack against numpy (bit equality with openexr._interleave_and_predict of the bytes write_exr would
join), dd_exr_deflate against the digests of the CPU build of the same core (tests/golden/exr_deflate_streams.json), DeviceEncoder's files read
back by the host reader and by the device decoder, and predict.main with --exr_encode device."""
import json
import os
import zlib

import numpy as np
import pytest
import torch

import exr_deflate_inputs as D
import exr_device_ref as R
from deepdenoiser_amd import _lib, openexr

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
FILL = 0xA5


def _need_gpu():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")


def _align(n):
    return (n + 15) // 16 * 16


# ---------------------------------------------------------------------------------------------------- pack
HALF_SPECIALS = np.array([0.0, -0.0, 6e-8, -5.96e-8, 2.98e-8, 2.9802322e-8, 3e-8, 6.1e-5, 6.0975552e-5, 65504.0, 65519.99, 65520.0, 1e6, -1e6, np.inf, -np.inf,
                          np.nan, 1.0009765625, 1.00048828125, 1.00146484375, 0.333333], dtype=np.float32)


def _image(h, w, c, seed):
    rng = np.random.default_rng(seed)
    img = (R.smooth(h, w, c, seed=seed) * np.exp(4 * rng.standard_normal((h, w, c)))).astype(np.float32)
    flat = img.reshape(-1)
    at = rng.permutation(flat.size)[:HALF_SPECIALS.size]
    flat[at] = HALF_SPECIALS[:at.size]
    return img


def _expected_chunk(img, row0, rows, types, src_channels, coded):
    with np.errstate(over="ignore"):
        arrs = [np.ascontiguousarray(img[..., s]).astype(np.float16 if t == 1 else np.float32) for t, s in zip(types, src_channels)]
    raw = b"".join(a[r].tobytes() for r in range(row0, row0 + rows) for a in arrs)
    return np.frombuffer(openexr._interleave_and_predict(raw) if coded else raw, dtype=np.uint8)


def _same_but_nan_payload(have, want, types, coded):
    """bit equality; where HALF NaNs are involved the payload is not compared, so compare the decoded samples instead"""
    if np.array_equal(have, want):
        return True
    if not coded or 1 not in types:
        return False
    a, b = (np.frombuffer(openexr._undo_predictor_and_interleave(x.tobytes()), dtype=np.uint8) for x in (have, want))
    differ = np.flatnonzero(a != b)
    for i in differ:                                               # every differing byte lies in a HALF sample that is a NaN on both sides
        s = i & ~1
        ha, hb = int(a[s]) | int(a[s + 1]) << 8, int(b[s]) | int(b[s + 1]) << 8
        if not ((ha & 0x7C00) == 0x7C00 and (ha & 0x3FF) and (hb & 0x7C00) == 0x7C00 and (hb & 0x3FF) and (ha & 0x8000) == (hb & 0x8000)):
            return False
    return True


PACK_CASES = [(1, 1), (1, 2), (16, 1), (17, 5), (33, 70), (40, 129)]
LAYOUTS = [(1, [0]), (3, [2, 1, 0]), (4, [3, 0, 2])]              # plane channels, the plane channel of every file channel (a subset, permuted)


@pytest.mark.parametrize("kind", ["float", "half", "mixed"])
def test_pack_equals_numpy(lib, kind):
    _need_gpu()
    sources, chunk_rows, expected, planes, at = [], [], [], [], 0
    for (h, w) in PACK_CASES:
        for c, src_channels in LAYOUTS:
            img = _image(h, w, c, seed=h * 131 + w + c)
            types = [{"float": 2, "half": 1}.get(kind, 1 + (k + h) % 2) for k in range(len(src_channels))]
            planes.append(torch.from_numpy(img).cuda())
            file_index = len(sources)
            sources.append((planes[-1], h, w, c, types, src_channels))
            for lines in (16, 1):                                    # ZIP chunks, and ZIPS rows
                for coded in (1, 0):
                    for row0 in range(0, h, lines):
                        rows = min(lines, h - row0)
                        want = _expected_chunk(img, row0, rows, types, src_channels, coded)
                        at += 32                                     # a gap between slots that must keep its fill
                        chunk_rows.append((at, file_index, row0, rows, coded))
                        expected.append(want)
                        at += _align(want.size)
    total = at + 32
    chunks = np.zeros(len(chunk_rows), dtype=openexr.CHUNK_DTYPE)
    chunks[:] = chunk_rows
    table = np.zeros(len(sources), dtype=openexr.SOURCE_DTYPE)
    for row, (plane, h, w, c, types, src_channels) in zip(table, sources):
        row["src"], row["H"], row["W"], row["C"], row["n_channels"] = plane.data_ptr(), h, w, c, len(types)
        row["type"][:len(types)] = types
        row["src_channel"][:len(types)] = src_channels
    staged = torch.full((total,), FILL, dtype=torch.uint8, device="cuda")
    dev_chunks, dev_sources = torch.from_numpy(chunks.view(np.uint8)).cuda(), torch.from_numpy(table.view(np.uint8)).cuda()
    _lib.check(lib.dd_exr_pack(chunks.ctypes.data, dev_chunks.data_ptr(), len(chunks), table.ctypes.data, dev_sources.data_ptr(), len(table),
                               staged.data_ptr(), total, torch.cuda.current_stream().cuda_stream))
    have = staged.cpu().numpy()
    owned = np.zeros(total, dtype=bool)
    for (offset, file_index, row0, rows, coded), want in zip(chunk_rows, expected):
        got = have[offset:offset + want.size]
        assert _same_but_nan_payload(got, want, sources[file_index][4], coded), "file %d rows %d+%d coded %d" % (file_index, row0, rows, coded)
        owned[offset:offset + _align(want.size)] = True
    assert (have[~owned] == FILL).all()                            # nothing outside a chunk's own bytes


def test_pack_half_is_numpy_for_every_exponent(lib):
    """fp32 -> HALF over a sweep of bit patterns around every rounding border: bit-identical to astype(float16) for every non-NaN input"""
    _need_gpu()
    halves = np.arange(0, 0x7C01, dtype=np.uint32)                 # every non-negative finite half and infinity
    base = halves.astype(np.uint16).view(np.float16).astype(np.float32).view(np.uint32)
    values = np.concatenate([base + d for d in (0, 1, 0xFFF, 0x1000, 0x1001, 0x1FFF)] + [base[1:] - 1, np.array([0x33000000, 0x33000001, 0x32FFFFFF, 0x477FEFFF,
                            0x477FF000, 0x7F7FFFFF, 0x00000001, 0x007FFFFF], dtype=np.uint32)]).astype(np.uint32)
    values = values[(values & 0x7FFFFFFF) <= 0x7F800000]
    values = np.concatenate([values, values | 0x80000000]).astype(np.uint32)
    w = 4096
    h = (values.size + w - 1) // w
    img = np.zeros(h * w, dtype=np.uint32)
    img[:values.size] = values
    img = img.view(np.float32).reshape(h, w)
    plane = torch.from_numpy(img).cuda()
    chunks = np.zeros(h, dtype=openexr.CHUNK_DTYPE)
    chunks[:] = [(r * w * 2, 0, r, 1, 0) for r in range(h)]
    table = np.zeros(1, dtype=openexr.SOURCE_DTYPE)
    table[0]["src"], table[0]["H"], table[0]["W"], table[0]["C"], table[0]["n_channels"] = plane.data_ptr(), h, w, 1, 1
    table[0]["type"][0] = 1
    staged = torch.zeros(h * w * 2, dtype=torch.uint8, device="cuda")
    dev_chunks, dev_sources = torch.from_numpy(chunks.view(np.uint8)).cuda(), torch.from_numpy(table.view(np.uint8)).cuda()
    _lib.check(lib.dd_exr_pack(chunks.ctypes.data, dev_chunks.data_ptr(), h, table.ctypes.data, dev_sources.data_ptr(), 1, staged.data_ptr(), staged.numel(),
                               torch.cuda.current_stream().cuda_stream))
    have = staged.cpu().numpy().view(np.uint16)
    with np.errstate(over="ignore"):
        want = img.reshape(-1).astype(np.float16).view(np.uint16)
    assert np.array_equal(have, want)


def test_pack_trusts_no_device_record(lib):
    """the host copy is valid; the device copy names rows, a file, an offset or a channel that do not fit: nothing is written"""
    _need_gpu()
    img = _image(20, 9, 3, seed=1)
    plane = torch.from_numpy(img).cuda()
    good = np.zeros(6, dtype=openexr.CHUNK_DTYPE)
    good[:] = [(k * 1024, 0, 0, 4, 1) for k in range(6)]
    bad = good.copy()
    bad[0]["file"], bad[1]["row0"], bad[2]["rows"], bad[3]["offset"], bad[4]["offset"], bad[5]["row0"] = 1, 17, 17, 6 * 1024 - 16, 8, -1
    table = np.zeros(1, dtype=openexr.SOURCE_DTYPE)
    table[0]["src"], table[0]["H"], table[0]["W"], table[0]["C"], table[0]["n_channels"] = plane.data_ptr(), 20, 9, 3, 3
    table[0]["type"][:3] = 2
    table[0]["src_channel"][:3] = (0, 1, 2)
    for bad_table in (None, "type", "src_channel", "W"):
        dev_table = table.copy()
        chunks_dev = bad
        if bad_table == "type":
            dev_table[0]["type"][1], chunks_dev = 0, good
        elif bad_table == "src_channel":
            dev_table[0]["src_channel"][2], chunks_dev = 3, good
        elif bad_table == "W":
            dev_table[0]["W"], chunks_dev = 1 << 20, good
        staged = torch.full((6 * 1024,), FILL, dtype=torch.uint8, device="cuda")
        dev_chunks, dev_sources = torch.from_numpy(chunks_dev.view(np.uint8).copy()).cuda(), torch.from_numpy(dev_table.view(np.uint8).copy()).cuda()
        _lib.check(lib.dd_exr_pack(good.ctypes.data, dev_chunks.data_ptr(), 6, table.ctypes.data, dev_sources.data_ptr(), 1, staged.data_ptr(), 6 * 1024,
                                   torch.cuda.current_stream().cuda_stream))
        assert (staged.cpu().numpy() == FILL).all(), bad_table


# ---------------------------------------------------------------------------------------------------- deflate
def _deflate_launch(lib, inputs, bad_records=()):
    """all inputs in one launch, every slot and every workspace slice with a guard of fill around it -> (statuses, sizes, out, records, workspace)"""
    records = np.zeros(len(inputs), dtype=openexr.DEFLATE_STREAM_DTYPE)
    src_at = out_at = 0
    for k, t in enumerate(inputs):
        records[k] = (src_at, out_at + 16, len(t), len(t) - 1)
        src_at += _align(len(t))
        out_at += 16 + _align(len(t))
    src = np.zeros(max(src_at, 16), dtype=np.uint8)
    for r, t in zip(records, inputs):
        src[r["src_offset"]:r["src_offset"] + len(t)] = np.frombuffer(t, dtype=np.uint8)
    device_records = records.copy()
    for k, field, value in bad_records:
        device_records[k][field] = value
    slice_words = _lib.DEFLATE_BLOCK_TOKENS
    need = lib.dd_exr_deflate_workspace(len(inputs))
    assert need == 4 * slice_words * len(inputs)
    out = torch.full((out_at + 16,), FILL, dtype=torch.uint8, device="cuda")
    workspace = torch.full((need + 64,), FILL, dtype=torch.uint8, device="cuda")
    both = torch.full((2 * len(inputs),), -7, dtype=torch.int32, device="cuda")
    dev_src, dev_records = torch.from_numpy(src).cuda(), torch.from_numpy(device_records.view(np.uint8).copy()).cuda()
    _lib.check(lib.dd_exr_deflate(records.ctypes.data, dev_records.data_ptr(), len(inputs), dev_src.data_ptr(), src.size, out.data_ptr(), out.numel(),
                                  workspace.data_ptr(), need, both.data_ptr(), both.data_ptr() + 4 * len(inputs), torch.cuda.current_stream().cuda_stream))
    both = both.cpu().numpy()
    return both[:len(inputs)], both[len(inputs):], out.cpu().numpy(), records, workspace.cpu().numpy()


@pytest.fixture(scope="module")
def deflated(lib):
    _need_gpu()
    inputs = [t for _, t in D.enumerated()]
    return inputs, _deflate_launch(lib, inputs), _deflate_launch(lib, inputs)


def test_deflate_equals_the_cpu_build(deflated):
    inputs, (statuses, sizes, out, records, _), _ = deflated
    golden = json.load(open(os.path.join(HERE, "golden", "exr_deflate_streams.json")))
    assert list(golden) == sorted(name for name, _ in D.enumerated())
    for k, ((name, t), r) in enumerate(zip(D.enumerated(), records)):
        stream = out[r["dst_offset"]:r["dst_offset"] + sizes[k]].tobytes()
        have = D.digest(statuses[k], sizes[k], stream)
        assert have == golden[name], name
        if statuses[k] == D.OK:
            assert zlib.decompress(stream) == t, name
    status_of = {name: statuses[k] for k, (name, _) in enumerate(D.enumerated())}
    assert all(status_of[name] == D.OK for name in D.MUST_OK) and all(status_of[name] == D.RAW for name in D.MUST_RAW)


def test_deflate_writes_nothing_outside_its_slots(deflated):
    inputs, (statuses, sizes, out, records, workspace), _ = deflated
    owned = np.zeros(out.size, dtype=bool)
    for r in records:
        owned[r["dst_offset"]:r["dst_offset"] + _align(int(r["dst_capacity"]))] = True
    assert (out[~owned] == FILL).all()
    assert (workspace[4 * _lib.DEFLATE_BLOCK_TOKENS * len(inputs):] == FILL).all()
    # a slice of the workspace is written from its start: a short input leaves the rest of ITS slice, up to the next one, untouched
    words = workspace[:4 * _lib.DEFLATE_BLOCK_TOKENS * len(inputs)].reshape(len(inputs), -1)
    for k, t in enumerate(inputs):
        assert (words[k, 4 * min(len(t), _lib.DEFLATE_BLOCK_TOKENS):] == FILL).all(), D.enumerated()[k][0]


def test_deflate_second_launch_gives_the_same_bytes(deflated):
    _, first, second = deflated
    assert np.array_equal(first[0], second[0]) and np.array_equal(first[1], second[1]) and np.array_equal(first[2], second[2])


def test_deflate_trusts_no_device_record(lib):
    _need_gpu()
    inputs = [b"abcabcabc" * 40, b"\x00" * 500, D.enumerated()[-6][1], b"x" * 300, b"y" * 300]
    bad = [(0, "src_offset", 1 << 40), (1, "dst_offset", 24), (3, "dst_capacity", 1 << 29), (4, "src_bytes", -3)]
    statuses, sizes, out, records, _ = _deflate_launch(lib, inputs, bad)
    assert list(statuses) == [D.RECORD, D.RECORD, D.OK, D.RECORD, D.RECORD] and [sizes[k] for k in (0, 1, 3, 4)] == [0] * 4
    r = records[2]
    assert zlib.decompress(out[r["dst_offset"]:r["dst_offset"] + sizes[2]].tobytes()) == inputs[2]
    owned = np.zeros(out.size, dtype=bool)
    owned[r["dst_offset"]:r["dst_offset"] + _align(int(r["dst_capacity"]))] = True
    assert (out[~owned] == FILL).all()                             # nothing was written through a refused record


# ---------------------------------------------------------------------------------------------------- files
def _check_files(tmp_path, compression, kind, images):
    encoder = openexr.DeviceEncoder("cuda", compression=compression, threads=3)
    tensors = [torch.from_numpy(np.ascontiguousarray(img)).cuda() for img in images]
    requests = [(str(tmp_path / ("f%d.exr" % k)), t, kind) for k, t in enumerate(tensors)]
    written = encoder.encode(requests)
    assert written == [path for path, _, _ in requests]
    decoder = openexr.DeviceDecoder("cuda", inflate="device")
    decoded = decoder.decode([(path, 3 if img.ndim == 3 else 1) for path, img in zip(written, images)])
    assert decoder.host_fallbacks == 0                            # every device-made stream is DD_INFLATE_OK for the strict device decoder
    for path, img, (plane, _) in zip(written, images, decoded):
        with np.errstate(over="ignore"):
            want = img if kind == "float" else img.astype(np.float16).astype(np.float32)
        host = openexr.read_image(path)
        host = host if img.ndim == 3 else host[..., 0]
        assert np.array_equal(R.bits(host), R.bits(want)), path
        device = plane.cpu().numpy() if img.ndim == 3 else plane.cpu().numpy()[..., 0]
        assert np.array_equal(R.bits(device), R.bits(want)), path
        assert openexr._parse_header(open(path, "rb").read())[0]["compression"] == compression
    encoder.release()
    return encoder, written


@pytest.mark.parametrize("kind", ["float", "half"])
@pytest.mark.parametrize("compression", ["zip", "zips", "none"])
def test_encoder_files_read_back_bit_identical(lib, tmp_path, compression, kind):
    """a batch that mixes sizes, 3-channel and 1-channel planes, and one image of random floats whose chunks go RAW"""
    _need_gpu()
    images = [R.smooth(h, w, 3, seed=h + w) for h, w in R.SIZES] + [R.smooth(37, 21, 3, seed=5)[..., 0], R.raw_in_zip_image(),
                                                                      R.random_finite_bits(np.random.default_rng(8), (33, 40, 3)), R.smooth(20, 1100, 3, seed=11)]
    encoder, written = _check_files(tmp_path, R.COMPRESSIONS[compression], kind, images)
    if compression == "none":
        assert (encoder.pack_launches, encoder.deflate_launches) == (1, 0)
    else:
        assert encoder.deflate_launches == 1 and encoder.pack_launches == (2 if encoder.raw_chunks else 1)
        if kind == "float":
            assert encoder.raw_chunks > 0                          # the random floats do not shrink
            assert False in R.chunk_kinds(written[-2]) and True in R.chunk_kinds(written[-1])


def test_encoder_reuses_its_buffers_and_refuses_what_it_cannot_take(lib, tmp_path):
    _need_gpu()
    encoder = openexr.DeviceEncoder("cuda")
    big, small = torch.from_numpy(R.smooth(40, 64, 3, seed=1)).cuda(), torch.from_numpy(R.smooth(5, 3, 3, seed=2)).cuda()
    encoder.encode([(str(tmp_path / "a.exr"), big, "float")])
    kept = encoder._out.data_ptr(), encoder._pinned.data_ptr()
    encoder.encode([(str(tmp_path / "b.exr"), small, "half")])
    assert (encoder._out.data_ptr(), encoder._pinned.data_ptr()) == kept
    assert np.array_equal(R.bits(openexr.read_image(str(tmp_path / "b.exr"))), R.bits(small.cpu().numpy().astype(np.float16).astype(np.float32)))
    with pytest.raises(ValueError):
        encoder.encode([(str(tmp_path / "c.exr"), small.cpu(), "float")])
    with pytest.raises(ValueError):
        encoder.encode([(str(tmp_path / "c.exr"), small, "uint")])
    encoder.release()
    assert encoder._out is None and encoder._pinned is None
    rle = openexr.DeviceEncoder("cuda", compression=openexr.RLE_COMPRESSION)      # RLE goes through the host writer
    rle.encode([(str(tmp_path / "r.exr"), big, "float")])
    assert rle.pack_launches == 0 and np.array_equal(R.bits(openexr.read_image(str(tmp_path / "r.exr"))), R.bits(big.cpu().numpy()))


# ---------------------------------------------------------------------------------------------------- command line
def test_predict_exr_encode_device_writes_the_same_planes(tmp_path):
    _need_gpu()
    from deepdenoiser_amd import configs, predict, tf_checkpoint
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
    for encode in ("host", "device"):
        for kind in ("float", "half"):
            src = tmp_path / ("frame_%s_%s" % (encode, kind))
            src.mkdir()
            runs[encode, kind] = src
    first = runs["host", "float"]
    for f in arch.feature_predictions + arch.auxiliary_features:
        if f.load_data:
            image = rng.random((FH, FW, 3)).astype(np.float32)
            for src in runs.values():
                openexr.write_image(str(src / ("render_%s_0001.exr" % f.name)), image)
    for (encode, kind), src in runs.items():
        inputs = set(os.listdir(src))
        predict.main(predict.parser().parse_args([str(tmp_path / "architecture.json"), "--input", str(src), "--tile_size", str(T), "--tile_overlap_size", str(O),
                                                  "--dtype", "f32", "--exr", "--exr_encode", encode, "--exr_type", kind]))
        runs[encode, kind] = (src, sorted(set(os.listdir(src)) - inputs))
    names = runs["host", "float"][1]
    assert any(n.endswith(".exr") for n in names) and any(n.endswith(".npy") for n in names)
    for kind in ("float", "half"):
        (host_dir, host_names), (device_dir, device_names) = runs["host", kind], runs["device", kind]
        assert host_names == device_names == names
        for n in names:
            if n.endswith(".npy"):
                assert open(host_dir / n, "rb").read() == open(device_dir / n, "rb").read() == open(first / n, "rb").read(), n
            else:
                a, b = openexr.read_exr(str(host_dir / n))[0], openexr.read_exr(str(device_dir / n))[0]
                assert list(a) == list(b) and all(np.array_equal(R.bits(a[c]), R.bits(b[c])) for c in a), n
                if kind == "float":
                    value = np.load(host_dir / (n[:-4] + ".npy"))
                    assert np.array_equal(R.bits(openexr.read_image(str(device_dir / n))[..., :value.shape[-1]]), R.bits(value)), n
