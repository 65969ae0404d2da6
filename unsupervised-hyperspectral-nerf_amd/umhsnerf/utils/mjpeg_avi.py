"""Motion-JPEG in an AVI 1.0 container, in pure Python: a sequence of complete JPEG files, one per frame, which ffmpeg, VLC and
every editor open (``ffmpeg -i NAME.avi -c:v libx264 -pix_fmt yuv420p NAME.mp4`` makes an mp4 of it).

Layout: ``RIFF 'AVI '`` { ``LIST 'hdrl'`` { ``avih``; ``LIST 'strl'`` { ``strh`` (``vids`` / ``MJPG``); ``strf`` (a BITMAPINFOHEADER with
``biCompression`` ``MJPG``) } }; ``LIST 'movi'`` { one ``00dc`` chunk per frame, padded to an even size }; ``idx1`` (one 16-byte entry
per frame, offsets counted from the ``movi`` tag) }.  The frame rate is ``dwRate / dwScale`` of ``strh``, a rational.  Sizes and the
frame count are written when the file is closed.

Limits: AVI 1.0 offsets are 32-bit, and this writer keeps a file at or under ``max_bytes`` (1 GiB): when the next frame would take it
past that, the file is finished and the frames continue in ``<stem>_part002.avi``, ``_part003`` ...  (OpenDML is not written.)  No audio."""
from __future__ import annotations

import struct
from fractions import Fraction
from pathlib import Path
from typing import List, Optional

HEADER_BYTES = 224          # everything in front of the first 00dc chunk
MAX_BYTES = 1 << 30
_KEYFRAME = 0x10            # AVIIF_KEYFRAME
_HASINDEX = 0x10            # AVIF_HASINDEX


def rate_scale(fps) -> tuple:
    """fps -> (dwRate, dwScale), 32-bit: 24 -> (24, 1), 29.97 -> (2997, 100), Fraction(30000, 1001) as it is."""
    f = Fraction(fps).limit_denominator(100000) if not isinstance(fps, Fraction) else fps
    if not f > 0 or f.numerator >= 1 << 31 or f.denominator >= 1 << 31:
        raise ValueError(f"fps must be a positive rational below 2^31, got {fps!r}")
    return f.numerator, f.denominator


class MjpegAviWriter:
    """``with MjpegAviWriter(path, width, height, fps) as w: w.add_frame(jpeg_bytes)``.  Leaving the block -- also by an exception --
    closes the file valid, with the frames it has.  ``paths``: the files written so far."""

    def __init__(self, path, width: int, height: int, fps=24, max_bytes: int = MAX_BYTES):
        self.path = Path(path)
        if self.path.suffix.lower() != ".avi":
            raise ValueError(f"a Motion-JPEG file is NAME.avi, got {self.path.name!r}")
        self.width, self.height = int(width), int(height)
        if not (1 <= self.width <= 65535 and 1 <= self.height <= 65535):
            raise ValueError(f"frame size {self.width} x {self.height} outside 1..65535")
        self.rate, self.scale = rate_scale(fps)
        self.max_bytes = int(max_bytes)
        self.paths: List[Path] = []
        self.frames = 0           # in all parts
        self._file = None
        self._index: List[tuple] = []  # (offset from the movi tag, size) of the open part's frames
        self._largest = 0
        self._open()

    # -- parts --
    def _open(self) -> None:
        part = len(self.paths) + 1
        path = self.path if part == 1 else self.path.with_name(f"{self.path.stem}_part{part:03d}{self.path.suffix}")
        self._file = open(path, "wb")
        self.paths.append(path)
        self._index, self._largest = [], 0
        self._file.write(self._header(0, 0))

    def _header(self, movi_bytes: int, index_bytes: int) -> bytes:
        n = len(self._index)
        per_second = self._largest * self.rate // self.scale
        avih = struct.pack("<14I", round(1e6 * self.scale / self.rate), min(per_second, 0xFFFFFFFF), 0, _HASINDEX, n, 0, 1, self._largest,
                           self.width, self.height, 0, 0, 0, 0)
        strh = struct.pack("<4s4sIHHIIIIIIII4H", b"vids", b"MJPG", 0, 0, 0, 0, self.scale, self.rate, 0, n, self._largest, 0xFFFFFFFF, 0,
                           0, 0, self.width, self.height)
        strf = struct.pack("<IiiHH4sIiiII", 40, self.width, self.height, 1, 24, b"MJPG", self.width * self.height * 3, 0, 0, 0, 0)
        strl = b"strl" + b"strh" + struct.pack("<I", len(strh)) + strh + b"strf" + struct.pack("<I", len(strf)) + strf
        hdrl = b"hdrl" + b"avih" + struct.pack("<I", len(avih)) + avih + b"LIST" + struct.pack("<I", len(strl)) + strl
        head = b"AVI " + b"LIST" + struct.pack("<I", len(hdrl)) + hdrl + b"LIST" + struct.pack("<I", 4 + movi_bytes) + b"movi"
        riff = len(head) + movi_bytes + 8 + index_bytes  # (the idx1 chunk is written with every file, also an empty one)
        out = b"RIFF" + struct.pack("<I", riff) + head
        assert len(out) == HEADER_BYTES
        return out

    def _finish(self) -> None:
        f, self._file = self._file, None
        if f is None:
            return
        try:
            movi_bytes = f.tell() - HEADER_BYTES
            index = b"".join(struct.pack("<4sIII", b"00dc", _KEYFRAME, off, size) for off, size in self._index)
            f.write(b"idx1" + struct.pack("<I", len(index)) + index)
            f.seek(0)
            f.write(self._header(movi_bytes, len(index)))
        finally:
            f.close()

    # -- frames --
    def add_frame(self, jpeg: bytes) -> None:
        if self._file is None:
            raise ValueError("the writer is closed")
        jpeg = bytes(jpeg)
        if jpeg[:2] != b"\xff\xd8":
            raise ValueError("a frame must be one complete JPEG file (it does not start with SOI)")
        chunk = 8 + len(jpeg) + (len(jpeg) & 1)
        size_after = self._file.tell() + chunk + 8 + 16 * (len(self._index) + 1)
        if size_after > self.max_bytes and self._index:
            self._finish()
            self._open()
        self._index.append((self._file.tell() - (HEADER_BYTES - 4), len(jpeg)))
        self._largest = max(self._largest, len(jpeg))
        self._file.write(b"00dc" + struct.pack("<I", len(jpeg)) + jpeg + (b"\0" if len(jpeg) & 1 else b""))
        self.frames += 1

    def close(self) -> None:
        self._finish()

    def __enter__(self) -> "MjpegAviWriter":
        return self

    def __exit__(self, *exc) -> Optional[bool]:
        self.close()
        return None
