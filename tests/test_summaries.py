"""TensorBoard event files (deepdenoiser_amd/summaries.py): round trip, the bytes of a record against one assembled by hand from
event.proto / summary.proto and the TFRecord framing, CRC failures.  (No TensorBoard is installed: parity with it is unpinned.)"""
import os
import struct

import pytest

from deepdenoiser_amd import summaries as S
from deepdenoiser_amd import tf_checkpoint, tfrecords


def test_round_trip(tmp_path):
    d = str(tmp_path / "model")
    with S.EventFileWriter(d) as w:
        w.add_scalars(100, [("loss", 1.25), ("diffuse_color_mean/1", 0.5)], wall_time=12.5)
        w.add_scalars(200, {"loss": 0.75}, wall_time=13.5)
        w.add_scalars(2 ** 40 + 3, [("combined_mean/4", -3.0)])
        path = w.path
    assert S.event_files(d) == [path]
    name = os.path.basename(path)
    assert name.startswith("events.out.tfevents.") and name.split(".")[3].isdigit() and len(name.split(".", 4)[4]) > 0
    events = S.read_events(path)
    assert events[0]["file_version"] == "brain.Event:2" and events[0]["scalars"] == [] and events[0]["wall_time"] > 0
    assert [(e["step"], e["wall_time"]) for e in events[1:3]] == [(100, 12.5), (200, 13.5)]
    assert S.read_scalars(path) == [(100, "loss", 1.25), (100, "diffuse_color_mean/1", 0.5), (200, "loss", 0.75), (2 ** 40 + 3, "combined_mean/4", -3.0)]


def test_two_writers_in_one_second_get_files_of_their_own(tmp_path):
    a, b = S.EventFileWriter(str(tmp_path)), S.EventFileWriter(str(tmp_path))
    a.add_scalars(1, [("x", 1.0)]), b.add_scalars(2, [("x", 2.0)])
    a.close(), b.close()
    assert a.path != b.path and sorted(S.event_files(str(tmp_path))) == sorted([a.path, b.path])
    assert S.read_scalars(a.path) == [(1, "x", 1.0)] and S.read_scalars(b.path) == [(2, "x", 2.0)]


def test_values_are_stored_as_float32(tmp_path):
    with S.EventFileWriter(str(tmp_path)) as w:
        w.add_scalars(1, [("x", 0.1)])
    (step, tag, value), = S.read_scalars(w.path)
    assert value == struct.unpack("<f", struct.pack("<f", 0.1))[0] and value != 0.1


def test_record_bytes_by_hand(tmp_path):
    """Event{wall_time=2.0 (field 1, 64-bit), step=300 (field 2, varint), summary (field 5) {value (field 1) {tag (field 1) = "loss",
    simple_value (field 2, 32-bit) = 1.5}}} written out byte by byte."""
    value = b"\x0a\x04loss" + b"\x15" + struct.pack("<f", 1.5)            # tag: key (1<<3)|2, length 4; simple_value: key (2<<3)|5
    summary = b"\x0a" + bytes([len(value)]) + value                          # Summary.value: key (1<<3)|2
    event = (b"\x09" + struct.pack("<d", 2.0)                                # wall_time: key (1<<3)|1
             + b"\x10" + b"\xac\x02"                                         # step: key (2<<3)|0, varint 300 = 0b10_0101100 -> ac 02
             + b"\x2a" + bytes([len(summary)]) + summary)                    # summary: key (5<<3)|2
    assert S.encode_event(2.0, step=300, scalars=[("loss", 1.5)]) == event
    head = struct.pack("<Q", len(event))
    framed = head + struct.pack("<I", tfrecords.masked_crc32c(head)) + event + struct.pack("<I", tfrecords.masked_crc32c(event))
    assert S.frame(event) == framed
    with S.EventFileWriter(str(tmp_path)) as w:
        w.add_scalars(300, [("loss", 1.5)], wall_time=2.0)
    data = open(w.path, "rb").read()
    assert data.endswith(framed)
    first = S.encode_event(S.read_events(w.path)[0]["wall_time"], file_version="brain.Event:2")
    assert first[9:] == b"\x1a\x0dbrain.Event:2"                             # file_version: key (3<<3)|2, length 13
    assert data == S.frame(first) + framed
    # the framing is the one tfrecords.write_records writes
    other = str(tmp_path / "plain.tfrecords")
    tfrecords.write_records(other, [first, event])
    assert open(other, "rb").read() == data


def test_masked_crc_known_value():
    """CRC-32C of "123456789" is 0xE3069283 (the check value of the Castagnoli polynomial); masked as TFRecord masks it."""
    c = 0xE3069283
    assert tfrecords.crc32c(b"123456789") == c
    assert tfrecords.masked_crc32c(b"123456789") == (((c >> 15) | (c << 17)) + 0xA282EAD8) & 0xFFFFFFFF


@pytest.mark.parametrize("where", ["length", "payload", "payload_crc"])
def test_flipped_byte_fails_the_crc(tmp_path, where):
    with S.EventFileWriter(str(tmp_path)) as w:
        w.add_scalars(7, [("loss", 2.0)])
    data = bytearray(open(w.path, "rb").read())
    first_len = struct.unpack("<Q", data[:8])[0]
    second = 12 + first_len + 4                      # offset of the second record
    offset = {"length": second + 8, "payload": second + 12 + 3, "payload_crc": len(data) - 1}[where]
    data[offset] ^= 0x01
    open(w.path, "wb").write(bytes(data))
    with pytest.raises(IOError):
        S.read_scalars(w.path)


def test_truncated_file_is_an_error(tmp_path):
    with S.EventFileWriter(str(tmp_path)) as w:
        w.add_scalars(7, [("loss", 2.0)])
    data = open(w.path, "rb").read()
    open(w.path, "wb").write(data[:-3])
    with pytest.raises(IOError):
        S.read_scalars(w.path)


def test_event_files_do_not_hide_the_checkpoint(tmp_path):
    """A model directory holds checkpoints AND event files (and eval_<name>/ directories): latest_checkpoint must not mind."""
    d = str(tmp_path)
    with S.EventFileWriter(d) as w:
        w.add_scalars(1, [("loss", 1.0)])
    with S.EventFileWriter(os.path.join(d, "eval_validation")) as w2:
        w2.add_scalars(1, [("loss", 1.0)])
    assert tf_checkpoint.latest_checkpoint(d) is None
    with open(os.path.join(d, "checkpoint"), "w") as f:
        f.write('model_checkpoint_path: "model.ckpt-4"\nall_model_checkpoint_paths: "model.ckpt-4"\n')
    open(os.path.join(d, "model.ckpt-4.index"), "wb").write(b"")
    got = tf_checkpoint.latest_checkpoint(d)
    assert got is not None and got.endswith("model.ckpt-4")
