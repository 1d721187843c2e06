"""TensorBoard event files with scalar, histogram and image summaries (what tf.summary.scalar / tf.summary.histogram / eval_metric_ops leave in
an Estimator's model directory, Training.py:676-698, 874-877, and what tf.summary.image would: the reference writes no images), written and
read without TensorFlow.

File: events.out.tfevents.<seconds>.<host>, a sequence of TFRecord-framed records (tfrecords.py: length, masked CRC32C, payload, masked
CRC32C; not gzipped), each a serialized `Event` message (tensorflow/core/util/event.proto):
    double wall_time = 1;  int64 step = 2;  string file_version = 3 ("brain.Event:2", the first record);
    Summary summary = 5 { repeated Value value = 1 { string tag = 1; float simple_value = 2; Image image = 4; HistogramProto histo = 5; } }
    Image (tensorflow/core/framework/summary.proto) { int32 height = 1, width = 2, colorspace = 3 (1 gray, 3 RGB); bytes encoded_image_string = 4; }
    HistogramProto (tensorflow/core/framework/summary.proto) { double min = 1, max = 2, num = 3, sum = 4, sum_squares = 5;
                                                               repeated double bucket_limit = 6 [packed], bucket = 7 [packed]; }
The messages are encoded by hand with the varint helpers of tfrecords.py.  PARITY UNPINNED against TensorBoard itself (none is installed
here): tests check a round trip and the bytes of a record assembled by hand from the .proto, like tf_checkpoint.py and openexr/codec.py.

encoded_image_string is a PNG (RFC 2083) written by encode_png: 8-bit gray or RGB, not interlaced, ONE IDAT chunk, filter type 0 on every
row; decode_png reads exactly that subset.  The PNG side is pinned a little further than the event format: a hand-assembled file in the
tests, and Pillow decodes the same pixels where it is installed; what TensorBoard makes of the image value is as unpinned as the rest.
"""
import os
import socket
import struct
import time
import zlib

import numpy as np

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


PNG_SIGNATURE = b"\x89PNG\r\n\x1a\n"


def _png_chunk(kind, data):
    return struct.pack(">I", len(data)) + kind + data + struct.pack(">I", zlib.crc32(kind + data) & 0xFFFFFFFF)


def encode_png(array, level=6):
    """A PNG of a uint8 array [H, W] / [H, W, 1] (gray) or [H, W, 3] (RGB): signature, IHDR (bit depth 8, colour type 0 or 2, no interlace),
    one IDAT (every row with filter type 0, zlib.compress), IEND."""
    a = np.asarray(array)
    if a.dtype != np.uint8 or a.ndim not in (2, 3) or (a.ndim == 3 and a.shape[2] not in (1, 3)) or a.shape[0] < 1 or a.shape[1] < 1:
        raise ValueError("encode_png: a uint8 array [H, W], [H, W, 1] or [H, W, 3] is expected, not %s %s" % (a.dtype, a.shape))
    h, w = a.shape[:2]
    ch = 3 if (a.ndim == 3 and a.shape[2] == 3) else 1
    rows = np.zeros((h, 1 + w * ch), dtype=np.uint8)      # column 0: the filter type byte of the row
    rows[:, 1:] = a.reshape(h, w * ch)
    ihdr = struct.pack(">IIBBBBB", w, h, 8, 2 if ch == 3 else 0, 0, 0, 0)
    return PNG_SIGNATURE + _png_chunk(b"IHDR", ihdr) + _png_chunk(b"IDAT", zlib.compress(rows.tobytes(), level)) + _png_chunk(b"IEND", b"")


def decode_png(data):
    """The uint8 array [H, W, 3] (RGB) or [H, W] (gray) of a PNG as encode_png writes it; every chunk CRC is checked.  Anything else (another
    bit depth or colour type, interlacing, a row filter other than 0) raises ValueError."""
    data = bytes(data)
    if data[:8] != PNG_SIGNATURE:
        raise ValueError("decode_png: not a PNG")
    at, ihdr, idat, ended = 8, None, b"", False
    while at < len(data) and not ended:
        if at + 12 > len(data):
            raise ValueError("decode_png: truncated chunk")
        n, kind = struct.unpack(">I", data[at:at + 4])[0], data[at + 4:at + 8]
        body = data[at + 8:at + 8 + n]
        if len(body) != n or at + 12 + n > len(data):
            raise ValueError("decode_png: truncated chunk")
        if struct.unpack(">I", data[at + 8 + n:at + 12 + n])[0] != (zlib.crc32(kind + body) & 0xFFFFFFFF):
            raise ValueError("decode_png: bad CRC in chunk %r" % kind)
        if kind == b"IHDR":
            ihdr = struct.unpack(">IIBBBBB", body)
        elif kind == b"IDAT":
            idat += body
        elif kind == b"IEND":
            ended = True
        at += 12 + n
    if ihdr is None or not ended:
        raise ValueError("decode_png: IHDR or IEND missing")
    w, h, depth, colour, compression, filt, interlace = ihdr
    if depth != 8 or colour not in (0, 2) or compression or filt or interlace or w < 1 or h < 1:
        raise ValueError("decode_png: only 8-bit gray / RGB without interlacing is read (IHDR %r)" % (ihdr,))
    ch = 3 if colour == 2 else 1
    raw = np.frombuffer(zlib.decompress(idat), dtype=np.uint8)
    if raw.size != h * (1 + w * ch):
        raise ValueError("decode_png: %d bytes of image data, %d expected" % (raw.size, h * (1 + w * ch)))
    rows = raw.reshape(h, 1 + w * ch)
    if rows[:, 0].any():
        raise ValueError("decode_png: a row filter other than 0")
    out = rows[:, 1:].copy()
    return out.reshape(h, w, 3) if ch == 3 else out.reshape(h, w)


def image_summary(tag, array):
    """(tag, height, width, colorspace, png bytes) of a uint8 array [H, W] / [H, W, 1] / [H, W, 3]: an entry of encode_event's `images`."""
    a = np.asarray(array)
    return (tag, a.shape[0], a.shape[1], 3 if (a.ndim == 3 and a.shape[2] == 3) else 1, encode_png(a))


def _encode_image(height, width, colorspace, png):
    return (_key(1, 0) + R._enc_varint(int(height)) + _key(2, 0) + R._enc_varint(int(width)) + _key(3, 0) + R._enc_varint(int(colorspace))
            + R._ld(4, bytes(png)))


def encode_event(wall_time, step=None, file_version=None, scalars=None, histograms=None, tracked=None, images=None):
    """One Event message.  summary.value[] holds, in this order, scalars: [(tag, value)] with simple_value (fp32), histograms: [(tag, dict)]
    with histo, tracked: more scalars -- the order in which Training.model_fn adds learning_rate / batch_size, the histograms and the
    tracked scalars (Training.py:676-698) --, then images: [(tag, height, width, png bytes)] or [(tag, height, width, colorspace, png bytes)]
    (colorspace 3 = RGB when left out; image_summary) with image.  Without images the bytes are what they were before images existed, with
    scalars alone what they were before histograms existed."""
    out = _key(1, 1) + struct.pack("<d", float(wall_time))
    if step is not None:
        out += _key(2, 0) + R._enc_varint(int(step) & 0xFFFFFFFFFFFFFFFF)
    if file_version is not None:
        out += R._ld(3, file_version.encode("utf-8"))
    if scalars is not None or histograms or tracked or images:
        def scalar(tag, value):
            return R._ld(1, R._ld(1, tag.encode("utf-8")) + _key(2, 5) + struct.pack("<f", float(value)))
        values = [scalar(tag, value) for tag, value in scalars or []]
        values += [R._ld(1, R._ld(1, tag.encode("utf-8")) + R._ld(5, encode_histogram(h))) for tag, h in histograms or []]
        values += [scalar(tag, value) for tag, value in tracked or []]
        for im in images or []:
            tag, height, width, colorspace, png = im if len(im) == 5 else (im[0], im[1], im[2], 3, im[3])
            values.append(R._ld(1, R._ld(1, tag.encode("utf-8")) + R._ld(4, _encode_image(height, width, colorspace, png))))
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

    def add_images(self, step, images, wall_time=None):
        """An Event of its own at `step` that holds only images: [(tag, height, width[, colorspace], png bytes)] (image_summary)."""
        self._write(encode_event(time.time() if wall_time is None else wall_time, step=step, images=images))

    def close(self):
        if self._f is not None:
            self._f.close()
            self._f = None

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()


def read_events(path):
    """[{'wall_time', 'step', 'file_version', 'scalars': [(tag, value)], 'histograms': [(tag, dict)], 'images': [(tag, {'height', 'width',
    'colorspace', 'png'})], 'tags': [every value's tag, in file order]}] of an event file; both CRCs of every record are checked."""
    events = []
    for record in R.read_records(path):
        e = {"wall_time": None, "step": 0, "file_version": None, "scalars": [], "histograms": [], "images": [], "tags": []}
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
                    tag, simple, histo, image = None, None, None, None
                    for fnum, fwt, fval in R._fields(value):
                        if fnum == 1 and fwt == 2:
                            tag = bytes(fval).decode("utf-8")
                        elif fnum == 2 and fwt == 5:
                            simple = struct.unpack("<f", bytes(fval))[0]
                        elif fnum == 4 and fwt == 2:
                            image = _decode_image(fval)
                        elif fnum == 5 and fwt == 2:
                            histo = _decode_histogram(fval)
                    if tag is not None and (simple is not None or histo is not None or image is not None):
                        e["tags"].append(tag)
                    if tag is not None and simple is not None:
                        e["scalars"].append((tag, simple))
                    if tag is not None and histo is not None:
                        e["histograms"].append((tag, histo))
                    if tag is not None and image is not None:
                        e["images"].append((tag, image))
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


def _decode_image(buf):
    im = {"height": 0, "width": 0, "colorspace": 0, "png": b""}
    names = {1: "height", 2: "width", 3: "colorspace"}
    for num, wt, val in R._fields(buf):
        if num in names and wt == 0:
            im[names[num]] = val
        elif num == 4 and wt == 2:
            im["png"] = bytes(val)
    return im


def read_images(path):
    """[(step, tag, {'height', 'width', 'colorspace', 'png'})] of every image in an event file, in file order (decode_png reads the png)."""
    return [(e["step"], tag, im) for e in read_events(path) for tag, im in e["images"]]


def read_histograms(path):
    """[(step, tag, dict)] of every histogram in an event file, in file order."""
    return [(e["step"], tag, h) for e in read_events(path) for tag, h in e["histograms"]]


def read_scalars(path):
    """[(step, tag, value)] of every scalar in an event file, in file order."""
    return [(e["step"], tag, value) for e in read_events(path) for tag, value in e["scalars"]]


def event_files(directory):
    """The event files of a directory, oldest first."""
    return sorted(os.path.join(directory, n) for n in os.listdir(directory) if n.startswith("events.out.tfevents."))
