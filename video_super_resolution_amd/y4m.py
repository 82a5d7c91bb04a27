"""YUV4MPEG2 (`.y4m`) clips read and written frame by frame on the host: a text header in front of raw planar frames, what
`ffmpeg -i x.mp4 x.y4m` writes.  Nothing here decodes anything and nothing touches the device: `Y4MReader.read_into` fills a caller's
buffer (`ClipRunner.run_stream` hands it a pinned upload slot), `Y4MWriter.write` appends one frame.

The header is one line, `YUV4MPEG2` and space-separated tokens in any order: W<width> H<height> F<num>:<den> I<interlacing> A<num>:<den>
C<colour space> X<anything>.  Every frame is `FRAME\\n` plus the frame's bytes, the planes Y, Cb, Cr back to back: the layouts of
`frames.PIX_FORMATS`' planar names.  Colour tags and what they mean here:

    C420jpeg    yuv420p      chroma midway both ways ("center")             C420 or no C tag: the same (the format's default)
    C420mpeg2   yuv420p      co-sited horizontally ("left")
    C420paldv   yuv420p      Cb and Cr sited on alternate lines: refused unless the caller names the siting to use instead
    C420p10     yuv420p10le  "left"
    C422        yuv422p      "left"                                         C422p10   yuv422p10le   "left"
    C444        yuv444p      (no siting: "left" is reported)                C444p10   yuv444p10le

`XCOLORRANGE=FULL | LIMITED` (ffmpeg's extension) gives the range, limited when absent; other X tokens are kept and ignored.
Interlaced clips (It: top field first, Ib: bottom field first) are refused by name unless the caller passes `interlaced=True`, which
says it will deinterlace them (`ClipRunner(deinterlace=...)`); the field order is then reported as `tff`.  The frames are read as they
lie in the file either way, and the writer always writes Ip.  Out of scope, and refused by name: mixed interlacing (Im), Cmono, C411, C444alpha, depths other than 8 and 10, FRAME lines with
parameters, pipes (the frame count comes from the file's size).
"""
from __future__ import annotations

import os
from typing import Optional, Tuple

import numpy as np

from .frames import PIX_FORMATS, YUV_SITINGS, pix_chroma, pix_frame_bytes

MAGIC = b"YUV4MPEG2"
FRAME = b"FRAME\n"
# colour tag -> (pixel format, siting; None: the tag names one this project has no filter for)
TAGS = {"420jpeg": ("yuv420p", "center"), "420mpeg2": ("yuv420p", "left"), "420": ("yuv420p", "center"), "420paldv": ("yuv420p", None),
        "420p10": ("yuv420p10le", "left"), "422": ("yuv422p", "left"), "422p10": ("yuv422p10le", "left"), "444": ("yuv444p", "left"),
        "444p10": ("yuv444p10le", "left")}
PLANAR = ("yuv420p", "yuv420p10le", "yuv422p", "yuv422p10le", "yuv444p", "yuv444p10le")   # what a Y4M file can hold (no nv12 / p010le)
_MAX_HEADER = 4096


def _ratio(token: str, what: str) -> Tuple[int, int]:
    try:
        a, b = token[1:].split(":")
        a, b = int(a), int(b)
    except ValueError:
        raise ValueError(f"Y4M header: {what} token {token!r} is not <int>:<int>") from None
    if a < 0 or b < 0:
        raise ValueError(f"Y4M header: {what} token {token!r} is negative")
    return a, b


def parse_header(line: bytes, siting: Optional[str] = None, interlaced: bool = False) -> dict:
    """The header line (without its newline) -> {shape (H, W), fmt, siting, full_range, fps, aspect, extra, tff}.  `siting`: use this one
    whatever the colour tag says (the only way to read a C420paldv file).  `interlaced`: accept It / Ib; `tff` is then True / False, and
    None for Ip or no I token (Im, mixed, stays refused)."""
    try:
        tokens = line.decode("ascii").split(" ")
    except UnicodeDecodeError:
        raise ValueError("Y4M header: not ASCII") from None
    if tokens[0] != MAGIC.decode():
        raise ValueError(f"not a YUV4MPEG2 file (the header starts with {tokens[0][:16]!r})")
    if siting is not None and siting not in YUV_SITINGS:
        raise ValueError(f"unknown siting {siting!r} (known: {', '.join(YUV_SITINGS)})")
    W = H = None
    fps = None
    aspect = (0, 0)
    tag, full_range, extra, tff = "420", False, [], None
    for t in tokens[1:]:
        if not t:
            continue
        k, v = t[0], t[1:]
        if k in "WH":
            if not v.isdigit() or int(v) <= 0:
                raise ValueError(f"Y4M header: size token {t!r} is not a positive integer")
            if k == "W":
                W = int(v)
            else:
                H = int(v)
        elif k == "F":
            fps = _ratio(t, "frame rate")
        elif k == "A":
            aspect = _ratio(t, "aspect")
        elif k == "I":
            if interlaced and v in ("t", "b"):
                tff = v == "t"
            elif interlaced and v == "m":
                raise ValueError(f"Y4M header: {t!r}: mixed interlacing is out of scope (Ip, It, Ib, or no I token)")
            elif v != "p":
                raise ValueError(f"Y4M header: {t!r}: interlaced clips are out of scope (only Ip, or no I token)")
        elif k == "C":
            tag = v
        elif k == "X":
            extra.append(t)
            if v.startswith("COLORRANGE="):
                r = v[len("COLORRANGE="):]
                if r not in ("FULL", "LIMITED"):
                    raise ValueError(f"Y4M header: {t!r}: the range is FULL or LIMITED")
                full_range = r == "FULL"
        else:
            raise ValueError(f"Y4M header: unknown token {t!r}")
    if W is None or H is None:
        raise ValueError("Y4M header: no W / H token")
    if tag not in TAGS:
        base = tag.split("p")[0] if "p" in tag and tag.split("p")[0] in ("420", "422", "444") else None
        if base is not None and tag[len(base) + 1:].isdigit():
            raise ValueError(f"Y4M header: {'C' + tag!r}: {tag[len(base) + 1:]} bits per sample (only 8 and 10 are read)")
        raise ValueError(f"Y4M header: {'C' + tag!r}: colour space out of scope (known: {', '.join('C' + k for k in TAGS)})")
    fmt, tag_siting = TAGS[tag]
    if siting is None:
        if tag_siting is None:
            raise ValueError(f"Y4M header: {'C' + tag!r}: Cb and Cr are sited on alternate lines, which no filter here matches; pass "
                             f"siting='left' or 'center' to read it with that one")
        siting = tag_siting
    pix_frame_bytes(fmt, H, W)   # (raises on a shape the layout cannot hold: an odd size)
    return dict(shape=(H, W), fmt=fmt, siting=siting, full_range=full_range, fps=fps, aspect=aspect, extra=extra, tff=tff)


class Y4MReader:
    """A `.y4m` file frame by frame.  Attributes: `shape` (H, W), `fmt` (a planar name of `frames.PIX_FORMATS`), `siting`, `full_range`,
    `fps` (num, den) or None, `aspect` (num, den), `extra` (the X tokens, verbatim), `tff` (with `interlaced=True`: True for It, False for Ib, None for progressive), `frame_bytes`; `len(reader)` is the frame count, from
    the file's size.  `read_into(buf)`: the next frame into a uint8 array of `frame_bytes` elements, False at the end; `read()`: a new
    array or None; iterating yields arrays; `rewind()` starts over."""

    def __init__(self, path: str, siting: Optional[str] = None, interlaced: bool = False):
        self.path = path
        self._f = open(path, "rb")
        try:
            head = self._f.read(_MAX_HEADER)
            nl = head.find(b"\n")
            if not head.startswith(MAGIC) or nl < 0:
                raise ValueError(f"{path}: not a YUV4MPEG2 file (no header line in the first {_MAX_HEADER} bytes)")
            info = parse_header(head[:nl], siting, interlaced)
            self.shape, self.fmt, self.siting, self.full_range = info["shape"], info["fmt"], info["siting"], info["full_range"]
            self.fps, self.aspect, self.extra, self.tff = info["fps"], info["aspect"], info["extra"], info["tff"]
            self.frame_bytes = pix_frame_bytes(self.fmt, *self.shape)
            self._start = nl + 1
            self._check_marker(head[self._start:self._start + len(FRAME) + 1], 0)
            body = os.fstat(self._f.fileno()).st_size - self._start
            if body % (len(FRAME) + self.frame_bytes):
                raise ValueError(f"{path}: {body} bytes after the header is not a whole number of frames of {len(FRAME)} + "
                                 f"{self.frame_bytes} bytes ({self.fmt} {self.shape[0]}x{self.shape[1]}): truncated?")
            self._n = body // (len(FRAME) + self.frame_bytes)
            self._f.seek(self._start)
            self._i = 0
        except Exception:
            self._f.close()
            raise

    def _check_marker(self, got: bytes, i: int) -> None:
        if got[:len(FRAME)] == FRAME or not got:
            return
        if got.startswith(b"FRAME "):
            raise ValueError(f"{self.path}: frame {i}: a FRAME line with parameters ({got!r}...) is out of scope")
        raise ValueError(f"{self.path}: frame {i}: expected {FRAME!r}, found {got[:len(FRAME)]!r}")

    def __len__(self) -> int:
        return self._n

    def rewind(self) -> None:
        self._f.seek(self._start)
        self._i = 0

    def read_into(self, buf: np.ndarray) -> bool:
        if self._i >= self._n:
            return False
        if buf.dtype != np.uint8 or buf.size != self.frame_bytes or not buf.flags.c_contiguous:
            raise ValueError(f"read_into needs a contiguous uint8 array of {self.frame_bytes} elements, got {buf.dtype} {buf.shape}")
        self._check_marker(self._f.read(len(FRAME)), self._i)
        if self._f.readinto(memoryview(buf.reshape(-1))) != self.frame_bytes:
            raise ValueError(f"{self.path}: frame {self._i} is short")
        self._i += 1
        return True

    def read(self) -> Optional[np.ndarray]:
        buf = np.empty(self.frame_bytes, dtype=np.uint8)
        return buf if self.read_into(buf) else None

    def __iter__(self):
        while True:
            f = self.read()
            if f is None:
                return
            yield f

    def close(self) -> None:
        self._f.close()

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()
        return False


def header_line(shape: Tuple[int, int], fmt: str, fps: Tuple[int, int], siting: str, full_range: bool, aspect: Tuple[int, int] = (1, 1)) -> bytes:
    """The header `ffmpeg` writes for such a clip, newline included: W H F Ip A C XYSCSS XCOLORRANGE."""
    if fmt not in PLANAR:
        raise ValueError(f"a Y4M file holds planar frames ({', '.join(PLANAR)}), not {fmt!r}: write {fmt} to a headerless file")
    if siting not in YUV_SITINGS:
        raise ValueError(f"unknown siting {siting!r} (known: {', '.join(YUV_SITINGS)})")
    if fmt == "yuv420p":
        tag = "420jpeg" if siting == "center" else "420mpeg2"
    else:
        tag = [k for k, v in TAGS.items() if v[0] == fmt][0]
        if pix_chroma(fmt) != "444" and TAGS[tag][1] != siting:
            raise ValueError(f"Y4M has no colour tag for {fmt} with {siting!r} siting (C{tag} means {TAGS[tag][1]!r})")
    H, W = int(shape[0]), int(shape[1])
    pix_frame_bytes(fmt, H, W)
    return (f"YUV4MPEG2 W{W} H{H} F{int(fps[0])}:{int(fps[1])} Ip A{int(aspect[0])}:{int(aspect[1])} C{tag} XYSCSS={tag.upper()} "
            f"XCOLORRANGE={'FULL' if full_range else 'LIMITED'}\n").encode("ascii")


class _FrameWriter:
    """`write(frame)` appends one frame; `writer(j, frame)` is the same as a `ClipRunner.run_stream` sink; `frames` counts them."""

    def __init__(self, path: str, frame_bytes: Optional[int], marker: bytes):
        self.path, self.frame_bytes, self.frames, self._marker = path, frame_bytes, 0, marker
        self._f = open(path, "wb")

    def write(self, frame) -> None:
        a = np.ascontiguousarray(np.asarray(frame))
        if a.dtype != np.uint8 or (self.frame_bytes is not None and a.size != self.frame_bytes):
            raise ValueError(f"expected a uint8 frame of {self.frame_bytes} bytes, got {a.dtype} {a.shape}")
        if self._marker:
            self._f.write(self._marker)
        self._f.write(memoryview(a.reshape(-1)))
        self.frames += 1

    def __call__(self, j: int, frame) -> None:
        self.write(frame)

    def close(self) -> None:
        self._f.close()

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()
        return False


class Y4MWriter(_FrameWriter):
    """A `.y4m` file written frame by frame: the header in ffmpeg's form at once, then `write(frame)` (uint8, `frame_bytes` elements) per
    frame.  The planar formats only: nv12 and p010le go to a headerless file (`RawWriter`)."""

    def __init__(self, path: str, shape: Tuple[int, int], fmt: str, fps: Tuple[int, int], siting: str, full_range: bool,
                 aspect: Tuple[int, int] = (1, 1)):
        head = header_line(shape, fmt, fps, siting, full_range, aspect)
        super().__init__(path, pix_frame_bytes(fmt, int(shape[0]), int(shape[1])), FRAME)
        self.shape, self.fmt, self.fps, self.siting, self.full_range, self.aspect = (int(shape[0]), int(shape[1])), fmt, fps, siting, full_range, aspect
        self._f.write(head)


class RawWriter(_FrameWriter):
    """A headerless clip (`ffmpeg -f rawvideo`): the frames back to back, any format."""

    def __init__(self, path: str, frame_bytes: Optional[int] = None):
        super().__init__(path, frame_bytes, b"")


class RawReader:
    """A headerless clip of `fmt` frames of `shape` = (H, W), frame by frame: `read_into`, `len` and the attributes of `Y4MReader` that
    a header would have given (`fps` None, `aspect` (0, 0))."""

    def __init__(self, path: str, shape: Tuple[int, int], fmt: str, siting: str = "left", full_range: bool = False):
        self.path, self.shape, self.fmt, self.siting, self.full_range = path, (int(shape[0]), int(shape[1])), fmt, siting, full_range
        self.fps, self.aspect, self.extra, self.tff = None, (0, 0), [], None
        self.frame_bytes = pix_frame_bytes(fmt, *self.shape)
        size = os.path.getsize(path)
        if size == 0 or size % self.frame_bytes:
            raise ValueError(f"{path}: {size} bytes is not a whole number of {fmt} frames of {shape[0]}x{shape[1]} ({self.frame_bytes} bytes each)")
        self._n, self._i = size // self.frame_bytes, 0
        self._f = open(path, "rb")

    def __len__(self) -> int:
        return self._n

    def read_into(self, buf: np.ndarray) -> bool:
        if self._i >= self._n:
            return False
        if buf.dtype != np.uint8 or buf.size != self.frame_bytes or not buf.flags.c_contiguous:
            raise ValueError(f"read_into needs a contiguous uint8 array of {self.frame_bytes} elements, got {buf.dtype} {buf.shape}")
        if self._f.readinto(memoryview(buf.reshape(-1))) != self.frame_bytes:
            raise ValueError(f"{self.path}: frame {self._i} is short")
        self._i += 1
        return True

    def close(self) -> None:
        self._f.close()


__all__ = ["Y4MReader", "Y4MWriter", "RawReader", "RawWriter", "parse_header", "header_line", "PLANAR", "TAGS", "PIX_FORMATS"]
