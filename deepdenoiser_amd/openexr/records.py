"""The device records of the EXR kernels as numpy dtypes, taken from the ctypes mirrors of include/dd_hip.h in _lib.py, and the two things
the decoder and the encoder do alike with them: fill a per-file row, and (batch_encode.py, under the names used here) align a chunk's offset
and run a launch between optional timing events."""
import numpy as np

from .. import _lib
from ..batch_encode import ALIGN as _STAGE_ALIGN, align16 as _align, timed  # noqa: F401

CHUNK_DTYPE = np.dtype(_lib.ExrChunk)                           # dd_exr_chunk
FILE_DTYPE = np.dtype(_lib.ExrFile)                             # dd_exr_file
STREAM_DTYPE = np.dtype(_lib.ExrStream)                         # dd_exr_stream
SOURCE_DTYPE = np.dtype(_lib.ExrSource)                         # dd_exr_source
DEFLATE_STREAM_DTYPE = np.dtype(_lib.ExrDeflateStream)          # dd_exr_deflate_stream
MAX_FILE_CHANNELS = _lib.EXR_MAX_CHANNELS
MAX_STREAM_BYTES = _lib.EXR_MAX_STREAM_BYTES
DEFLATE_OK, DEFLATE_RAW, DEFLATE_RECORD = _lib.DEFLATE_OK, _lib.DEFLATE_RAW, _lib.DEFLATE_RECORD


def fill_row(table, slot, plane, height, width, channels, types, per_channel):
    """Row `slot` of a FILE_DTYPE or SOURCE_DTYPE table (the same layout under two sets of names): the device pointer of the fp32 plane
    [height, width, channels] the file is decoded into / packed from and, per file channel, its pixel type and `per_channel` (the set of
    plane channels it is written to / the plane channel it is read from).  The rest of the row is zero."""
    pointer, last = ("dst", "dst_mask") if table.dtype == FILE_DTYPE else ("src", "src_channel")
    table[slot] = np.zeros((), dtype=table.dtype)
    row = table[slot]
    row[pointer], row["H"], row["W"], row["C"], row["n_channels"] = plane, height, width, channels, len(types)
    row["type"][:len(types)] = types
    row[last][:len(types)] = per_channel

