"""OpenEXR frames without OpenCV / the OpenEXR library: the render-pass images either side of the inference path
(TensorFlow/OpenEXRDirectory.py:54-151 loads one .exr per render pass through cv2.imdecode and hands RGB float32 to Prediction.py:223-252;
SURVEY 8f rank 4).

PARITY UNPINNED: neither OpenCV nor the OpenEXR library is installed and the reference ships no image, so nothing here has been checked
against a file written by Blender.  The container format is restated from the published "OpenEXR File Layout" document:

    int32 magic 20000630 | int32 version (low byte 2; bit 0x200 tiled, 0x800 deep, 0x1000 multi-part)
    header    = attributes (name\\0 type\\0 int32 size, value) ... \\0
                channels (chlist: name\\0 int32 type{0 uint,1 half,2 float} uint8 pLinear 3 reserved int32 xSampling int32 ySampling ... \\0),
                compression (uint8), dataWindow / displayWindow (box2i), lineOrder, pixelAspectRatio, screenWindowCenter, screenWindowWidth
    uint64 offset per chunk, chunks of 1 (none, RLE, ZIPS) or 16 (ZIP) scan lines:
    chunk     = int32 y | int32 size | data;   data = per scan line, per channel in name order, one row of that channel's samples
    ZIP / ZIPS / RLE transform the chunk bytes first: split into even and odd bytes (first half, second half), then byte deltas
    (t[i] - t[i-1] + 128), then deflate (or run-length code); a chunk that would not shrink is stored raw.

Supported: single-part scan-line files, compression NONE / RLE / ZIPS / ZIP (Blender's default), UINT / HALF / FLOAT channels without
subsampling.  Tiled, deep, multi-part files and the PIZ / PXR24 / B44 / DWA codecs raise ExrError naming what was found.

The modules, each importing only those before it: codec (the host reader and writer; numpy and zlib alone), records (the device records of
the EXR kernels), decode (DeviceDecoder and its host half), encode (DeviceEncoder and its host half), frames (frame directories,
load_frame, save_predictions, the command-line options).  torch is imported only inside the functions that need a device.
"""
from .codec import (MAGIC, NO_COMPRESSION, RLE_COMPRESSION, ZIP_COMPRESSION, ZIPS_COMPRESSION, ExrError, _decode_chunk, _interleave_and_predict,
                    _LINES, _parse_header, _rle_decode, _rle_encode, _undo_predictor_and_interleave, image_size, read_exr, read_image, write_exr,
                    write_image)
from .records import (CHUNK_DTYPE, DEFLATE_OK, DEFLATE_RAW, DEFLATE_RECORD, DEFLATE_STREAM_DTYPE, FILE_DTYPE, MAX_FILE_CHANNELS, MAX_STREAM_BYTES,
                      SOURCE_DTYPE, STREAM_DTYPE)
from .decode import DeviceDecoder, FilePlan, fill_batch_tables, pack_batch, plan_file
from .encode import FLOAT, HALF, DeviceEncoder, WritePlan, assemble, plan_write
from .frames import OpenEXRDirectory, add_encode_arguments, add_inflate_argument, load_frame, save_predictions

__all__ = [
    "MAGIC", "NO_COMPRESSION", "RLE_COMPRESSION", "ZIPS_COMPRESSION", "ZIP_COMPRESSION", "ExrError",
    "read_exr", "image_size", "read_image", "write_exr", "write_image",
    "CHUNK_DTYPE", "FILE_DTYPE", "STREAM_DTYPE", "SOURCE_DTYPE", "DEFLATE_STREAM_DTYPE", "MAX_FILE_CHANNELS", "MAX_STREAM_BYTES",
    "DEFLATE_OK", "DEFLATE_RAW", "DEFLATE_RECORD",
    "FilePlan", "plan_file", "pack_batch", "fill_batch_tables", "DeviceDecoder",
    "HALF", "FLOAT", "WritePlan", "plan_write", "assemble", "DeviceEncoder",
    "OpenEXRDirectory", "load_frame", "save_predictions", "add_encode_arguments", "add_inflate_argument",
]
