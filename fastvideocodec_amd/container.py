"""On-disk container for coded video: a self-describing file of I-frame and
P-frame records with GOP / view muxing and a trailing index for random access to any GOP.

The reference has no container: its DVC path only estimates bits (DVC/net.py:57 calrealbits),
RLVC keeps compressai strings in memory (entropy_models.py:80-94) and I-frames go through BPG
files it deletes (models.py:412-429). Layout (little-endian):

  file    = "FVC1" | u16 version | u32 header_len | header (UTF-8 JSON) | record* | index
  record  = u8 kind ('I' | 'P') | u16 view | u32 gop | u16 frame | u32 payload_len | payload
  I payload = u16 h | u16 w | u8 levels | u16 q | u32 n_block_idx | block_idx (u8)
              | streams(coefficients)
  P payload = u8 precision (0 x3, 1 f32) | u8 framing (0 channel, 1 item, 2 segment)
              | u16 H/16 | u16 W/16 | u16 H/64 | u16 W/64 | streams(mv) | streams(z) | streams(feature)
  streams = u32 n | u32 len[n] (bytes) | bytes        (each stream byte-identical to compressai's
                                                      RansEncoder.encode_with_indexes output)
  index   = u32 n_records | (u8 kind, u16 view, u32 gop, u16 frame, u64 offset)* | u64 index_offset | "FVCX"

The header carries the codec name / level, frame geometry, GOP length, view and GOP counts, the
I-frame transform parameters and a CRC-32 of every entropy table, which a reader checks against
its own model before decoding. height / width are the coded (padded) size; a file coded from 8-bit
YUV (transcode.py) also carries display_height / display_width, pixfmt, fps and frames (make_header).

A file whose header has "frame_digest": "splitmix64-f32" carries, as the last 8 bytes (u64) of every
record payload, the digest (digest.py) of that frame's reconstruction at the coded size: what the
encoder held as its reference, and what a decoder must reproduce. The payload parsers read by
position and ignore trailing bytes, so a reader that knows nothing of the key decodes such a file.
"""
from __future__ import annotations

import io
import json
import struct
import zlib

import numpy as np
import torch

from . import digest as DG
from . import iframe as IF
from .entropy_models import EncodedStreams
from .net import FRAMINGS, PFrameBitstream

MAGIC = b"FVC1"
INDEX_MAGIC = b"FVCX"
VERSION = 1
_REC = struct.Struct("<cHIHI")
_IDX = struct.Struct("<cHIHQ")


def tables_crc(model) -> str:
    """CRC-32 over the model's quantised CDF tables (mv, z, feature) and scale table."""
    model.update()
    return tables_crc_of(*model._coders["tables"])


def tables_crc_of(tz, tmv, tf) -> str:
    """tables_crc of host tables (FactorizedTables z / mv, LaplaceTables feature)."""
    c = 0
    for t in (tmv, tz, tf):
        for a in (t.cdf, t.cdf_length, t.offset):
            c = zlib.crc32(np.ascontiguousarray(a, np.int32).tobytes(), c)
    c = zlib.crc32(np.ascontiguousarray(tf.scale_table, np.float32).tobytes(), c)
    return f"{c:08x}"


def _pack_streams(strings) -> bytes:
    return struct.pack(f"<I{len(strings)}I", len(strings), *[len(s) for s in strings]) + b"".join(strings)


def _unpack_streams(buf, pos):
    (n,) = struct.unpack_from("<I", buf, pos)
    pos += 4
    lens = struct.unpack_from(f"<{n}I", buf, pos)
    pos += 4 * n
    out = []
    for L in lens:
        out.append(bytes(buf[pos:pos + L]))
        pos += L
    return out, pos


def split_pframes(bs: PFrameBitstream):
    """Per-frame payloads of a batched P-frame bitstream: [(mv, z, feature) stream lists]."""
    parts = {k: getattr(bs, k).to_bytes_list() for k in ("mv", "z", "feature")}
    out = []
    for b in range(bs.batch):
        fr = []
        for k in ("mv", "z", "feature"):
            s = parts[k]
            per = len(s) // bs.batch
            fr.append(s[b * per:(b + 1) * per])
        out.append(fr)
    return out


def pframe_payload(bs: PFrameBitstream, b: int = 0, frame_streams=None) -> bytes:
    fs = frame_streams if frame_streams is not None else split_pframes(bs)[b]
    (H16, W16), (H64, W64) = bs.hw16, bs.hw64
    head = struct.pack("<BBHHHH", 1 if bs.precision == "f32" else 0, FRAMINGS.index(bs.framing), H16, W16, H64, W64)
    return head + b"".join(_pack_streams(s) for s in fs)


def pframe_from_payload(payload: bytes, device) -> PFrameBitstream:
    prec, fr, H16, W16, H64, W64 = struct.unpack_from("<BBHHHH", payload, 0)
    pos = 10
    parts = []
    for _ in range(3):
        s, pos = _unpack_streams(payload, pos)
        parts.append(EncodedStreams.from_bytes_list(s, device))
    return PFrameBitstream(parts[0], parts[1], parts[2], 1, (H16, W16), (H64, W64), FRAMINGS[fr],
                           "f32" if prec else "x3")


def iframe_payload(bs: IF.IFrameBitstream) -> bytes:
    if bs.batch != 1:
        raise ValueError("one I-frame per record")
    bidx = np.ascontiguousarray(bs.block_index, np.uint8).tobytes()
    head = struct.pack("<HHBHI", bs.h, bs.w, bs.levels, bs.q, len(bidx))
    return head + bidx + _pack_streams(bs.streams.to_bytes_list())


def iframe_from_payload(payload: bytes, device) -> IF.IFrameBitstream:
    h, w, levels, q, nb = struct.unpack_from("<HHBHI", payload, 0)
    pos = struct.calcsize("<HHBHI")
    bidx = np.frombuffer(payload, np.uint8, nb, pos).reshape(3, h // IF.BLOCK, w // IF.BLOCK).copy()
    pos += nb
    strings, pos = _unpack_streams(payload, pos)
    return IF.IFrameBitstream(1, h, w, levels, q, bidx, EncodedStreams.from_bytes_list(strings, device))


class ContainerWriter:
    def __init__(self, f, header: dict):
        self.f = f
        self.index = []
        self.digests = _has_digests(header)
        hb = json.dumps(header, sort_keys=True).encode()
        f.write(MAGIC + struct.pack("<HI", VERSION, len(hb)) + hb)

    def _record(self, kind, view, gop, frame, payload, digest=None):
        if (digest is not None) != self.digests:
            raise ValueError("every record of a file carries a digest, or none does (header key frame_digest)")
        if digest is not None:
            payload = payload + struct.pack("<Q", int(digest) & DG.MASK)
        self.index.append((kind, view, gop, frame, self.f.tell()))
        self.f.write(_REC.pack(kind, view, gop, frame, len(payload)))
        self.f.write(payload)

    def write_iframe(self, view, gop, frame, bs: IF.IFrameBitstream, digest: int | None = None):
        self._record(b"I", view, gop, frame, iframe_payload(bs), digest)

    def write_pframe(self, view, gop, frame, payload: bytes, digest: int | None = None):
        self._record(b"P", view, gop, frame, payload, digest)

    def write_payload(self, kind: bytes, view, gop, frame, payload: bytes, digest: int | None = None):
        """A record whose payload (iframe_payload / pframe_payload) was serialised earlier. digest
        (the frame's reconstruction digest, given exactly when the header has the frame_digest key)
        is appended to it."""
        if kind not in (b"I", b"P"):
            raise ValueError(f"unknown record kind {kind!r}")
        self._record(kind, view, gop, frame, payload, digest)

    def close(self):
        pos = self.f.tell()
        self.f.write(struct.pack("<I", len(self.index)))
        for e in self.index:
            self.f.write(_IDX.pack(*e))
        self.f.write(struct.pack("<Q", pos) + INDEX_MAGIC)


class ContainerReader:
    def __init__(self, data: bytes):
        self.data = memoryview(data)
        if bytes(self.data[:4]) != MAGIC:
            raise ValueError("not an FVC1 container")
        ver, hl = struct.unpack_from("<HI", self.data, 4)
        if ver != VERSION:
            raise ValueError(f"unsupported container version {ver}")
        self.header = json.loads(bytes(self.data[10:10 + hl]).decode())
        if bytes(self.data[-4:]) != INDEX_MAGIC:
            raise ValueError("missing index")
        (ipos,) = struct.unpack_from("<Q", self.data, len(self.data) - 12)
        (n,) = struct.unpack_from("<I", self.data, ipos)
        self.index = [_IDX.unpack_from(self.data, ipos + 4 + i * _IDX.size) for i in range(n)]

    def record(self, entry):
        kind, view, gop, frame, off = entry
        k2, v2, g2, f2, L = _REC.unpack_from(self.data, off)
        if (k2, v2, g2, f2) != (kind, view, gop, frame):
            raise ValueError("index does not match record")
        start = off + _REC.size
        return bytes(self.data[start:start + L])

    def gop_records(self, view, gop):
        return sorted((e for e in self.index if e[1] == view and e[2] == gop), key=lambda e: e[3])

    def gops(self):
        return sorted({(e[1], e[2]) for e in self.index})


def _has_digests(header) -> bool:
    name = header.get("frame_digest")
    if name is not None and name != DG.NAME:
        raise ValueError(f"unknown frame digest {name!r} (this reader knows {DG.NAME!r})")
    return name is not None


def record_digest(header, payload) -> int | None:
    """The reconstruction digest a record payload carries (its last 8 bytes), or None for a file
    whose header does not announce digests."""
    if not _has_digests(header):
        return None
    if len(payload) < 8:
        raise ValueError("record payload too short to carry a digest")
    return struct.unpack_from("<Q", payload, len(payload) - 8)[0]


def make_header(model, height, width, gop, gops, framing, q, display=None, pixfmt=None, fps=None, frames=None,
                frame_digest=False):
    """The container header. height / width are the coded (padded) size. Optional keys, absent
    from a file of float RGB frames at the coded size: display = (h, w) -> display_height /
    display_width (what a decoder crops to), pixfmt = {"chroma": "420", "matrix", "range"} (the
    source's 8-bit format, which a decoder converts back to), fps = (num, den), frames (total).
    frame_digest=True announces a reconstruction digest at the end of every record payload."""
    header = {"codec": model.name, "level": model.compression_level, "height": height, "width": width, "gop": gop,
              "gops": gops, "tables_crc32": tables_crc(model), "framing": framing,
              "iframe": {"transform": "rct+legall53", "levels": IF.LEVELS, "block": IF.BLOCK,
                         "band_rows": IF.BAND_ROWS, "q": q}}
    if display is not None:
        header["display_height"], header["display_width"] = int(display[0]), int(display[1])
    if pixfmt is not None:
        header["pixfmt"] = {"chroma": "420", "matrix": pixfmt["matrix"], "range": pixfmt["range"]}
    if fps is not None:
        header["fps"] = [int(fps[0]), int(fps[1])]
    if frames is not None:
        header["frames"] = int(frames)
    if frame_digest:
        header["frame_digest"] = DG.NAME
    return header


def display_size(header):
    """(display_height, display_width); the coded size for a file without display geometry."""
    H, W = header["height"], header["width"]
    h, w = header.get("display_height", H), header.get("display_width", W)
    if not (1 <= h <= H and 1 <= w <= W):
        raise ValueError(f"display size {h}x{w} does not fit the coded size {H}x{W}")
    return h, w


def info(data: bytes) -> dict:
    """What a container holds, from its header and index alone (no model, no GPU)."""
    r = ContainerReader(data)
    h, w = display_size(r.header)
    kinds = [e[0] for e in r.index]
    return {"header": r.header, "display": [h, w], "coded": [r.header["height"], r.header["width"]],
            "gops": len(r.gops()), "records": len(r.index), "iframes": kinds.count(b"I"),
            "pframes": kinds.count(b"P"), "bytes": len(r.data)}


def check_gop_digests(view, gop, expected, got):
    """Compare one GOP's stored digests [(frame, uint64)] with the decoded frames' (device int64
    [1] each): one host read, DigestMismatch at the first differing frame."""
    if not expected:
        return
    have = torch.cat(got).cpu().tolist()
    for (frame, want), g in zip(expected, have):
        if want != DG.to_uint64(g):
            raise DG.DigestMismatch(view, gop, frame, want, g)


def encode_video(model, video: torch.Tensor, f, iframe_q=None, framing="segment", views=None, digest=False):
    """Encode video [N, T, 3, H, W] (N GOPs, H and W multiples of 64) into container file f.
    GOP n is muxed as (view = views[n] if given else 0, gop = n). Frame 0 of each GOP is coded by
    the I-frame codec (step iframe_q, default from model.I_level: iframe.iframe_step), frames
    1..T-1 by the P-frame codec against the encoder's own previous reconstruction (what the
    decoder will hold). digest=True stamps every record with the digest of its reconstruction, which
    decode_video checks. Returns the encoder's reconstructions [N, T, 3, H, W]."""
    N, T, C, H, W = video.shape
    q = IF.iframe_step(model.I_level) if iframe_q is None else int(iframe_q)
    w = ContainerWriter(f, make_header(model, H, W, T, N, framing, q, frame_digest=digest))
    stamp = (lambda x: DG.to_uint64(DG.frame_digest(x).item())) if digest else (lambda x: None)
    recons = torch.empty_like(video)
    for n in range(N):
        v = 0 if views is None else int(views[n])
        ibs, x = IF.encode(video[n, 0:1].contiguous(), q)
        w.write_iframe(v, n, 0, ibs, stamp(x))
        recons[n, 0] = x[0]
        for t in range(1, T):
            bs, x = model.compress(video[n, t:t + 1].contiguous(), x, framing=framing)
            w.write_pframe(v, n, t, pframe_payload(bs), stamp(x))
            recons[n, t] = x[0]
    w.close()
    return recons


def decode_video(model, data: bytes, device=None, verify=True):
    """Decode every GOP of a container: {(view, gop): frames [T, 3, H, W]} on the device. When the
    file carries frame digests, every decoded frame's digest is computed on the device and compared
    once per GOP (one host read per GOP); DigestMismatch names the first differing frame.
    verify=False skips the check."""
    r = ContainerReader(data)
    if r.header.get("tables_crc32") != tables_crc(model):
        raise ValueError("container was coded with different entropy tables (model weights differ)")
    dev = torch.device(device) if device is not None else next(model.parameters()).device
    check = verify and _has_digests(r.header)
    out = {}
    for view, gop in r.gops():
        frames = []
        expected, got = [], []
        x = None
        for e in r.gop_records(view, gop):
            payload = r.record(e)
            if e[0] == b"I":
                x = IF.decode(iframe_from_payload(payload, dev))
            else:
                x = model.decompress(pframe_from_payload(payload, dev), x)
            frames.append(x[0])
            if check:
                expected.append((e[3], record_digest(r.header, payload)))
                got.append(DG.frame_digest(x))
        check_gop_digests(view, gop, expected, got)
        out[(view, gop)] = torch.stack(frames)
    return out


def encode_video_bytes(model, video, **kw):
    buf = io.BytesIO()
    rec = encode_video(model, video, buf, **kw)
    return buf.getvalue(), rec
