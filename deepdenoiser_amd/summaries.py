"""TensorBoard event files with scalar and histogram summaries (what tf.summary.scalar / tf.summary.histogram / eval_metric_ops leave in an
Estimator's model directory, Training.py:676-698, 874-877), written and read without TensorFlow.

File: events.out.tfevents.<seconds>.<host>, a sequence of TFRecord-framed records (tfrecords.py: length, masked CRC32C, payload, masked
CRC32C; not gzipped), each a serialized `Event` message (tensorflow/core/util/event.proto):
    double wall_time = 1;  int64 step = 2;  string file_version = 3 ("brain.Event:2", the first record);
    Summary summary = 5 { repeated Value value = 1 { string tag = 1; float simple_value = 2; HistogramProto histo = 5; } }
    HistogramProto (tensorflow/core/framework/summary.proto) { double min = 1, max = 2, num = 3, sum = 4, sum_squares = 5;
                                                               repeated double bucket_limit = 6 [packed], bucket = 7 [packed]; }
The messages are encoded by hand with the varint helpers of tfrecords.py.  PARITY UNPINNED against TensorBoard itself (none is installed
here): tests check a round trip and the bytes of a record assembled by hand from the .proto, like tf_checkpoint.py and openexr.py.
"""
import os
import socket
import struct
import time

from . import tfrecords as R

FILE_VERSION = "brain.Event:2"


def _key(num, wire_type):
    return R._enc_varint((num << 3) | wire_type)


def encode_histogram(h):
    """One HistogramProto from {"min", "max", "num", "sum", "sum_squares", "bucket_limit", "bucket"} (metrics.histogram_values)."""
    out = b"".join(_key(n, 1) + struct.pack("<d", float(h[k])) for n, k in enumerate(("min", "max", "num", "sum", "sum_squares"), 1))
    for n, k in ((6, "bucket_limit"), (7, "bucket")):
        out += R._ld(n, struct.pack("<%dd" % len(h[k]), *h[k]))
    return out


def encode_event(wall_time, step=None, file_version=None, scalars=None, histograms=None, tracked=None):
    """One Event message.  summary.value[] holds, in this order, scalars: [(tag, value)] with simple_value (fp32), histograms: [(tag, dict)]
    with histo, tracked: more scalars -- the order in which Training.model_fn adds learning_rate / batch_size, the histograms and the
    tracked scalars (Training.py:676-698).  With scalars alone the bytes are what they were before histograms existed."""
    out = _key(1, 1) + struct.pack("<d", float(wall_time))
    if step is not None:
        out += _key(2, 0) + R._enc_varint(int(step) & 0xFFFFFFFFFFFFFFFF)
    if file_version is not None:
        out += R._ld(3, file_version.encode("utf-8"))
    if scalars is not None or histograms or tracked:
        def scalar(tag, value):
            return R._ld(1, R._ld(1, tag.encode("utf-8")) + _key(2, 5) + struct.pack("<f", float(value)))
        values = [scalar(tag, value) for tag, value in scalars or []]
        values += [R._ld(1, R._ld(1, tag.encode("utf-8")) + R._ld(5, encode_histogram(h))) for tag, h in histograms or []]
        values += [scalar(tag, value) for tag, value in tracked or []]
        out += R._ld(5, b"".join(values))
    return out


def frame(data):
    """TFRecord framing of one record (the bytes tfrecords.write_records writes per record)."""
    head = struct.pack("<Q", len(data))
    return head + struct.pack("<I", R.masked_crc32c(head)) + data + struct.pack("<I", R.masked_crc32c(data))


class EventFileWriter:
    """Appends scalar summaries to a new event file in `directory` (created if missing).  Every add is flushed, so a reader (TensorBoard,
    read_scalars) sees complete records while training runs."""

    def __init__(self, directory):
        os.makedirs(directory, exist_ok=True)
        now = time.time()
        self.path = os.path.join(directory, "events.out.tfevents.%010d.%s" % (int(now), socket.gethostname()))
        k = 0
        while os.path.exists(self.path):      # a second writer within the same second: a file of its own (TensorBoard's filename_suffix)
            k += 1
            self.path = os.path.join(directory, "events.out.tfevents.%010d.%s.%d" % (int(now), socket.gethostname(), k))
        self._f = open(self.path, "ab")
        self._write(encode_event(now, file_version=FILE_VERSION))

    def _write(self, event):
        self._f.write(frame(event))
        self._f.flush()

    def add_scalars(self, step, scalars, wall_time=None):
        """scalars: [(tag, value)] or {tag: value}; one Event at `step`."""
        if isinstance(scalars, dict):
            scalars = list(scalars.items())
        self._write(encode_event(time.time() if wall_time is None else wall_time, step=step, scalars=scalars))

    def add_summaries(self, step, scalars, histograms=None, tracked=None, wall_time=None):
        """ONE Event at `step` with scalars, then histograms ([(tag, dict)], metrics.histogram_values), then the scalars of `tracked`."""
        if isinstance(scalars, dict):
            scalars = list(scalars.items())
        self._write(encode_event(time.time() if wall_time is None else wall_time, step=step, scalars=scalars, histograms=histograms, tracked=tracked))

    def close(self):
        if self._f is not None:
            self._f.close()
            self._f = None

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()


def read_events(path):
    """[{'wall_time', 'step', 'file_version', 'scalars': [(tag, value)], 'histograms': [(tag, dict)], 'tags': [every value's tag, in file
    order]}] of an event file; both CRCs of every record are checked."""
    events = []
    for record in R.read_records(path):
        e = {"wall_time": None, "step": 0, "file_version": None, "scalars": [], "histograms": [], "tags": []}
        for num, wt, val in R._fields(memoryview(record)):
            if num == 1 and wt == 1:
                e["wall_time"] = struct.unpack("<d", bytes(val))[0]
            elif num == 2 and wt == 0:
                e["step"] = val - (1 << 64) if val >= (1 << 63) else val
            elif num == 3 and wt == 2:
                e["file_version"] = bytes(val).decode("utf-8")
            elif num == 5 and wt == 2:
                for vnum, vwt, value in R._fields(val):
                    if vnum != 1 or vwt != 2:
                        continue
                    tag, simple, histo = None, None, None
                    for fnum, fwt, fval in R._fields(value):
                        if fnum == 1 and fwt == 2:
                            tag = bytes(fval).decode("utf-8")
                        elif fnum == 2 and fwt == 5:
                            simple = struct.unpack("<f", bytes(fval))[0]
                        elif fnum == 5 and fwt == 2:
                            histo = _decode_histogram(fval)
                    if tag is not None and (simple is not None or histo is not None):
                        e["tags"].append(tag)
                    if tag is not None and simple is not None:
                        e["scalars"].append((tag, simple))
                    if tag is not None and histo is not None:
                        e["histograms"].append((tag, histo))
        events.append(e)
    return events


def _decode_histogram(buf):
    h = {"min": 0.0, "max": 0.0, "num": 0.0, "sum": 0.0, "sum_squares": 0.0, "bucket_limit": [], "bucket": []}
    names = {1: "min", 2: "max", 3: "num", 4: "sum", 5: "sum_squares", 6: "bucket_limit", 7: "bucket"}
    for num, wt, val in R._fields(buf):
        if num in (1, 2, 3, 4, 5) and wt == 1:
            h[names[num]] = struct.unpack("<d", bytes(val))[0]
        elif num in (6, 7) and wt == 2:      # packed
            b = bytes(val)
            h[names[num]] += list(struct.unpack("<%dd" % (len(b) // 8), b))
        elif num in (6, 7) and wt == 1:      # (a writer that does not pack)
            h[names[num]].append(struct.unpack("<d", bytes(val))[0])
    return h


def read_histograms(path):
    """[(step, tag, dict)] of every histogram in an event file, in file order."""
    return [(e["step"], tag, h) for e in read_events(path) for tag, h in e["histograms"]]


def read_scalars(path):
    """[(step, tag, value)] of every scalar in an event file, in file order."""
    return [(e["step"], tag, value) for e in read_events(path) for tag, value in e["scalars"]]


def event_files(directory):
    """The event files of a directory, oldest first."""
    return sorted(os.path.join(directory, n) for n in os.listdir(directory) if n.startswith("events.out.tfevents."))
