"""A PNG writer for the frames the runners save (`save_image_path`): 8-bit grey or RGB, filter type 0, one IDAT chunk, from zlib and
struct alone, so that saving a frame needs no imaging library on the machine that trains."""
import os
import struct
import zlib

import numpy as np

SIGNATURE = b"\x89PNG\r\n\x1a\n"


def _chunk(kind, data):
    return struct.pack(">I", len(data)) + kind + data + struct.pack(">I", zlib.crc32(kind + data) & 0xFFFFFFFF)


def write_png(path, array):
    """array: (h, w, 3) uint8 RGB or (h, w) uint8 grey, h and w > 0 (a numpy array or anything np.asarray takes; a device tensor is
    copied to the host by the caller).  The directory of `path` is created."""
    a = np.asarray(array)
    if a.dtype != np.uint8 or a.ndim not in (2, 3) or (a.ndim == 3 and a.shape[2] != 3) or a.shape[0] == 0 or a.shape[1] == 0:
        raise ValueError(f"write_png: expected a uint8 array (h, w, 3) or (h, w), got {a.dtype} {a.shape}")
    h, w = a.shape[:2]
    rows = np.zeros((h, 1 + w * (3 if a.ndim == 3 else 1)), dtype=np.uint8)                    # byte 0 of a row: filter type 0
    rows[:, 1:] = a.reshape(h, -1)
    ihdr = struct.pack(">IIBBBBB", w, h, 8, 2 if a.ndim == 3 else 0, 0, 0, 0)
    folder = os.path.dirname(os.path.abspath(path))
    os.makedirs(folder, exist_ok=True)
    with open(path, "wb") as f:
        f.write(SIGNATURE + _chunk(b"IHDR", ihdr) + _chunk(b"IDAT", zlib.compress(rows.tobytes(), 6)) + _chunk(b"IEND", b""))
