"""A PNG writer (and the reader its tests need) on the standard library: 8-bit RGB, 8-bit grey and 16-bit grey images,
non-interlaced, every scanline with filter type 0.  The rendered frames leave the package through here, so that writing
them needs no image library.
"""
import binascii
import struct
import zlib

import numpy as np

SIGNATURE = b"\x89PNG\r\n\x1a\n"
_GREY, _RGB = 0, 2      # PNG colour types


def _chunk(kind, payload):
    return struct.pack(">I", len(payload)) + kind + payload + struct.pack(">I", binascii.crc32(kind + payload) & 0xffffffff)


def encode_png(array, level=6):
    """The bytes of the PNG file of `array`: uint8 [H,W,3] (RGB), uint8 [H,W] or uint16 [H,W] (grey; a trailing axis of 1 is
    accepted).  16-bit samples are stored big-endian, as the format demands."""
    a = np.asarray(array)
    if a.ndim == 3 and a.shape[2] == 1:
        a = a[:, :, 0]
    if a.dtype == np.uint8 and a.ndim == 3 and a.shape[2] == 3:
        colour, depth = _RGB, 8
    elif a.dtype == np.uint8 and a.ndim == 2:
        colour, depth = _GREY, 8
    elif a.dtype == np.uint16 and a.ndim == 2:
        colour, depth = _GREY, 16
        a = a.astype(">u2")
    else:
        raise ValueError(f"write_png takes uint8 [H,W,3], uint8 [H,W] or uint16 [H,W], got {a.dtype} {a.shape}")
    H, W = a.shape[:2]
    if H < 1 or W < 1:
        raise ValueError("an image needs at least one pixel")
    rows = np.ascontiguousarray(a).reshape(H, -1).view(np.uint8)
    lines = np.empty((H, 1 + rows.shape[1]), dtype=np.uint8)
    lines[:, 0] = 0             # filter type 0 (None) on every scanline
    lines[:, 1:] = rows
    header = struct.pack(">IIBBBBB", W, H, depth, colour, 0, 0, 0)
    return SIGNATURE + _chunk(b"IHDR", header) + _chunk(b"IDAT", zlib.compress(lines.tobytes(), level)) + _chunk(b"IEND", b"")


def write_png(path, array, level=6):
    """Write `array` (see encode_png) to `path`."""
    data = encode_png(array, level)
    with open(path, "wb") as f:
        f.write(data)


def chunks(data):
    """[(kind, payload)] of a PNG file's bytes; raises ValueError on a bad signature, a short file or a failed CRC."""
    if data[:8] != SIGNATURE:
        raise ValueError("not a PNG file")
    out, at = [], 8
    while at < len(data):
        if at + 12 > len(data):
            raise ValueError("a chunk runs past the end of the file")
        (n,) = struct.unpack(">I", data[at:at + 4])
        kind, payload = data[at + 4:at + 8], data[at + 8:at + 8 + n]
        if at + 12 + n > len(data):
            raise ValueError("a chunk runs past the end of the file")
        (crc,) = struct.unpack(">I", data[at + 8 + n:at + 12 + n])
        if binascii.crc32(kind + payload) & 0xffffffff != crc:
            raise ValueError(f"chunk {kind!r}: CRC mismatch")
        out.append((kind, payload))
        at += 12 + n
    return out


def read_png(path):
    """The array of a file write_png wrote (uint8 [H,W,3], uint8 [H,W] or uint16 [H,W]).  Not a general decoder: filter
    type 0 only, no interlace, no palette."""
    with open(path, "rb") as f:
        parts = chunks(f.read())
    if not parts or parts[0][0] != b"IHDR" or parts[-1][0] != b"IEND":
        raise ValueError("IHDR must come first and IEND last")
    W, H, depth, colour, compression, filt, interlace = struct.unpack(">IIBBBBB", parts[0][1])
    if (colour, depth) not in ((_RGB, 8), (_GREY, 8), (_GREY, 16)) or compression or filt or interlace:
        raise ValueError("read_png reads what write_png writes: 8-bit RGB, 8- or 16-bit grey, no interlace")
    raw = zlib.decompress(b"".join(payload for kind, payload in parts if kind == b"IDAT"))
    stride = W * (3 if colour == _RGB else 1) * (depth // 8)
    lines = np.frombuffer(raw, dtype=np.uint8).reshape(H, 1 + stride)
    if lines[:, 0].any():
        raise ValueError("a scanline uses a filter other than type 0")
    body = np.ascontiguousarray(lines[:, 1:])
    if depth == 16:
        return body.view(">u2").astype(np.uint16).reshape(H, W)
    return body.reshape(H, W, 3) if colour == _RGB else body.reshape(H, W)
