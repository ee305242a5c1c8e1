"""Frame-by-frame readers and a writer for 8-bit planar YUV 4:2:0 files: YUV4MPEG2 (.y4m) and
headerless I420 (.yuv). Nothing here touches the GPU, and no reader holds more than one frame.

Simplification: the chroma tags C420 (default), C420jpeg, C420mpeg2 and C420paldv differ only in
where the chroma samples sit; all four are accepted and treated as centre-sited (C420jpeg), which
is what fastvideocodec_amd.pixfmt converts. Every other chroma format, any bit depth above 8 and
interlaced material are refused with a ValueError naming the tag.
"""
from __future__ import annotations

import numpy as np

Y4M_MAGIC = b"YUV4MPEG2"
CHROMA_420 = ("420", "420jpeg", "420mpeg2", "420paldv")


def frame_bytes(w: int, h: int) -> int:
    return w * h + 2 * ((w + 1) // 2) * ((h + 1) // 2)


def _split_planes(buf: bytes, w: int, h: int):
    cw, ch = (w + 1) // 2, (h + 1) // 2
    a = np.frombuffer(buf, np.uint8)
    y = a[:w * h].reshape(h, w)
    u = a[w * h:w * h + cw * ch].reshape(ch, cw)
    v = a[w * h + cw * ch:].reshape(ch, cw)
    return y, u, v


def _open(path_or_file, mode):
    if hasattr(path_or_file, "read") or hasattr(path_or_file, "write"):
        return path_or_file, False
    return open(path_or_file, mode), True


class _Frames:
    """Shared iteration: one frame of `frame_bytes` per step, optionally after a frame header."""

    def __iter__(self):
        return self

    def close(self):
        if self._own:
            self.f.close()

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()

    def _read_frame(self, eof_ok=False):
        n = frame_bytes(self.width, self.height)
        buf = self.f.read(n)
        if eof_ok and not buf:
            raise StopIteration
        if len(buf) != n:
            raise ValueError(f"truncated frame {self.frames_read}: {len(buf)} of {n} bytes")
        self.frames_read += 1
        return _split_planes(buf, self.width, self.height)


class Y4MReader(_Frames):
    """Iterator of (y, u, v) uint8 numpy planes of a YUV4MPEG2 stream. Attributes: width, height,
    fps (num, den), chroma (the C tag's value), aspect (the A tag's value or None)."""

    def __init__(self, path_or_file):
        self.f, self._own = _open(path_or_file, "rb")
        self.frames_read = 0
        line = self._line(limit=256)
        tags = line.split(b" ")
        if tags[0] != Y4M_MAGIC:
            raise ValueError("not a YUV4MPEG2 stream")
        self.width = self.height = None
        self.fps, self.chroma, self.aspect = (25, 1), "420", None
        for t in tags[1:]:
            if not t:
                continue
            key, val = chr(t[0]), t[1:].decode("ascii", "replace")
            if key == "W":
                self.width = int(val)
            elif key == "H":
                self.height = int(val)
            elif key == "F":
                num, den = val.split(":")
                self.fps = (int(num), int(den))
            elif key == "I":
                if val != "p":
                    raise ValueError(f"unsupported Y4M interlacing tag I{val} (progressive only)")
            elif key == "A":
                self.aspect = val
            elif key == "C":
                if val not in CHROMA_420:
                    raise ValueError(f"unsupported Y4M chroma tag C{val} (8-bit 4:2:0 only)")
                self.chroma = val
            # X (comment) and unknown tags are ignored, as the format asks
        if not self.width or not self.height or self.width < 1 or self.height < 1:
            raise ValueError("Y4M header lacks a W or H tag")

    def _line(self, limit):
        out = bytearray()
        while True:
            c = self.f.read(1)
            if not c:
                if not out:
                    return None
                raise ValueError("truncated Y4M header")
            if c == b"\n":
                return bytes(out)
            out += c
            if len(out) > limit:
                raise ValueError("Y4M header line too long")

    def __next__(self):
        head = self._line(limit=256)
        if head is None:
            raise StopIteration
        if not head.startswith(b"FRAME"):
            raise ValueError(f"expected a FRAME header at frame {self.frames_read}")
        return self._read_frame()


class RawYUVReader(_Frames):
    """Iterator of (y, u, v) planes of a headerless I420 file of w x h frames."""

    def __init__(self, path_or_file, w: int, h: int, fps=(25, 1)):
        if w < 1 or h < 1:
            raise ValueError(f"bad frame size {w}x{h}")
        self.f, self._own = _open(path_or_file, "rb")
        self.width, self.height, self.fps = int(w), int(h), tuple(fps)
        self.chroma, self.aspect = "420", None
        self.frames_read = 0

    def __next__(self):
        return self._read_frame(eof_ok=True)


class Y4MWriter:
    """Writes 8-bit 4:2:0 frames as YUV4MPEG2; the header goes out with the first frame's size
    already known (w, h given here)."""

    def __init__(self, path_or_file, w: int, h: int, fps=(25, 1), chroma="420jpeg", aspect=None):
        if chroma not in CHROMA_420:
            raise ValueError(f"unsupported Y4M chroma tag C{chroma} (8-bit 4:2:0 only)")
        self.f, self._own = _open(path_or_file, "wb")
        self.width, self.height = int(w), int(h)
        head = f"YUV4MPEG2 W{w} H{h} F{int(fps[0])}:{int(fps[1])} Ip"
        if aspect:
            head += f" A{aspect}"
        self.f.write((head + f" C{chroma}\n").encode("ascii"))
        self.frames_written = 0

    def write(self, y, u, v):
        w, h = self.width, self.height
        cw, ch = (w + 1) // 2, (h + 1) // 2
        for name, p, shape in (("y", y, (h, w)), ("u", u, (ch, cw)), ("v", v, (ch, cw))):
            p = np.asarray(p)
            if p.dtype != np.uint8 or p.shape != shape:
                raise ValueError(f"{name}: expected uint8 {shape}, got {p.dtype} {p.shape}")
        self.f.write(b"FRAME\n")
        for p in (y, u, v):
            self.f.write(np.ascontiguousarray(p).tobytes())
        self.frames_written += 1

    def close(self):
        if self._own:
            self.f.close()

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()


def open_video(path, size=None):
    """Reader for a path by extension: .y4m -> Y4MReader, anything else -> RawYUVReader(size=(w, h))."""
    if str(path).lower().endswith(".y4m"):
        return Y4MReader(path)
    if size is None:
        raise ValueError("a raw YUV file needs its frame size (WxH)")
    return RawYUVReader(path, size[0], size[1])
