"""File-level coding: 8-bit YUV 4:2:0 frames of any size <-> an FVC1 container.

encode_file pulls frames from a reader (video_io), converts and pads them on the GPU (pixfmt),
codes GOP by GOP (I-frame codec for frame 0, P-frame chain after it) and records the display
geometry and pixel format in the header; decode_file is the inverse and writes the cropped 8-bit
planes. The quality figures are exact 8-bit per-plane PSNRs of what a decoder will deliver.

That a decoder delivers the encoder's reconstruction is checked, not assumed, when asked:
encode_file(digest=True) stamps every record with the digest (digest.py) of the reconstruction it
held, decode_file compares each decoded frame with it, and encode_file(self_check=True) decodes the
bytes it has just serialised and compares on the spot.
"""
from __future__ import annotations

import itertools

import numpy as np
import torch

from . import container as C
from . import digest as DG
from . import iframe as IF
from . import metrics as MT
from . import pixfmt as PF

DEFAULT_PIXFMT = {"chroma": "420", "matrix": "bt709", "range": "limited"}


def _upload(frames, dev):
    """[(y, u, v) numpy planes] -> three uint8 device tensors [n,h,w], [n,ch,cw], [n,ch,cw]."""
    return tuple(torch.from_numpy(np.stack([f[k] for f in frames])).to(dev) for k in range(3))


def encode_file(model, reader, f, gop=12, framing="segment", iframe_q=None, batch=1, pixfmt=None,
                recon_writer=None, digest=False, self_check=False, msssim=False):
    """Code every frame of `reader` (an iterator of (y, u, v) uint8 planes with .width, .height and
    .fps) into container file f. Frame 0 of each GOP of `gop` frames is an I-frame, the rest a
    P-frame chain on the encoder's own reconstruction; the last GOP may be short. pixfmt = {"matrix":
    "bt601" | "bt709", "range": "limited" | "full"} describes the source (default BT.709 limited). batch=G codes
    frame t of G consecutive GOPs as one [G,3,H,W] compress call; the file does not depend on it.
    recon_writer (a Y4MWriter, optional) receives the encoder's reconstruction, which is what
    decode_file delivers. digest=True stamps every record with the digest of its reconstruction at
    the coded size (header key frame_digest), which decode_file checks. self_check=True parses every
    payload back as soon as it is serialised, decodes it against the decoder-side previous frame and
    compares the digests on the device (one flag read per chunk of gop * batch frames);
    DigestMismatch names the first frame a decoder would not reproduce. The file does not depend
    on self_check. msssim=True adds "msssim_y" to the result: per frame the MS-SSIM (metrics.ms_ssim,
    data range 255) of the 8-bit source Y plane and the Y plane a decoder delivers, at the display
    size, queued beside the squared errors and read with them; the file does not depend on it, and a
    display size below five scales' minimum raises before anything is coded.
    Returns {"frames", "bytes", "bpp" (over display pixels), "psnr_y",
    "psnr_u", "psnr_v" (per frame, reconstruction against source), "height", "width",
    "coded_height", "coded_width", "gops"}."""
    if gop < 1 or batch < 1:
        raise ValueError("gop and batch must be >= 1")
    pf = dict(DEFAULT_PIXFMT, **(pixfmt or {}))
    matrix, yuv_range = pf["matrix"], pf["range"]
    dev = next(model.parameters()).device
    h, w = reader.height, reader.width
    if msssim and min(h, w) < MT.min_side(5):
        raise ValueError(f"msssim: a display size of {h}x{w} is too small for five scales: the smaller side is "
                         f"{min(h, w)}, the minimum is {MT.min_side(5)}")
    q = IF.iframe_step(model.I_level) if iframe_q is None else int(iframe_q)
    records = []   # (kind, gop, frame, payload bytes), in file order
    sse = []       # device int64 [3] per frame, in file order ([4] with msssim: the float64's bits ride along)
    nframes = ngops = 0
    Hp = Wp = None
    frames = iter(reader)
    while True:
        chunk = list(itertools.islice(frames, gop * batch))
        if not chunk:
            break
        ys, us, vs = _upload(chunk, dev)
        x, _ = PF.yuv420_to_rgb(ys, us, vs, matrix, yuv_range)
        Hp, Wp = x.shape[2:]
        n = len(chunk)
        lens = [min(gop, n - s) for s in range(0, n, gop)]  # only the last GOP may be short
        out = {}
        digs = {}   # (i, t) -> device int64 [1]: the digest of the encoder's reconstruction
        ddigs = {}  # the same of the self-check's decode
        dprev = {}  # self-check: the decoder-side previous frame of each GOP of the chunk

        def finish(i, t, rec, payload, kind):
            k = i * gop + t
            ry, ru, rv = PF.rgb_to_yuv420(rec, h, w, matrix, yuv_range)
            metric = [PF.sse_u8_device(ry, ys[k:k + 1]), PF.sse_u8_device(ru, us[k:k + 1]),
                      PF.sse_u8_device(rv, vs[k:k + 1])]
            if msssim:
                metric.append(MT.ms_ssim(ys[k:k + 1, None], ry[:, None], data_range=255).view(torch.int64))
            out[(i, t)] = (kind, payload, torch.cat(metric), (ry, ru, rv) if recon_writer is not None else None)
            if digest or self_check:
                digs[(i, t)] = DG.frame_digest(rec)
            if self_check:
                if kind == b"I":
                    dprev[i] = IF.decode(C.iframe_from_payload(payload, dev))
                else:
                    dprev[i] = model.decompress(C.pframe_from_payload(payload, dev), dprev[i])
                ddigs[(i, t)] = DG.frame_digest(dprev[i])

        prev = []
        for i in range(len(lens)):
            ibs, rec = IF.encode(x[i * gop:i * gop + 1], q)
            prev.append(rec)
            finish(i, 0, rec, C.iframe_payload(ibs), b"I")
        for t in range(1, gop):
            act = [i for i, L in enumerate(lens) if L > t]
            if not act:
                break
            if len(act) == 1:
                cur, ref = x[act[0] * gop + t:act[0] * gop + t + 1], prev[act[0]]
            else:
                cur = x[torch.tensor([i * gop + t for i in act], device=dev)]
                ref = torch.cat([prev[i] for i in act])
            bs, rec = model.compress(cur, ref, framing=framing)
            streams = C.split_pframes(bs)
            for j, i in enumerate(act):
                prev[i] = rec[j:j + 1]
                finish(i, t, prev[i], C.pframe_payload(bs, frame_streams=streams[j]), b"P")
        order = [(i, t) for i, L in enumerate(lens) for t in range(L)]
        if self_check:
            enc, dec = torch.cat([digs[k] for k in order]), torch.cat([ddigs[k] for k in order])
            if bool((enc != dec).any()):  # the chunk's one flag; the digests are read only to report
                for (i, t), want, got in zip(order, enc.tolist(), dec.tolist()):
                    if want != got:
                        raise DG.DigestMismatch(0, ngops + i, t, want, got)
        stamps = torch.cat([digs[k] for k in order]).tolist() if digest else [None] * n
        for (i, t), stamp in zip(order, stamps):  # stamps: the chunk's one read of its digests
            kind, payload, s, planes = out[(i, t)]
            records.append((kind, ngops + i, t, payload, stamp))
            sse.append(s)
            if planes is not None:
                recon_writer.write(*(p[0].cpu().numpy() for p in planes))
        nframes += n
        ngops += len(lens)
    if nframes == 0:
        raise ValueError("the source holds no frame")
    header = C.make_header(model, Hp, Wp, gop, ngops, framing, q, display=(h, w),
                           pixfmt=pf, fps=getattr(reader, "fps", None), frames=nframes, frame_digest=digest)
    start = f.tell()
    cw = C.ContainerWriter(f, header)
    for kind, g, t, payload, stamp in records:
        cw.write_payload(kind, 0, g, t, payload, stamp)
    cw.close()
    nbytes = f.tell() - start
    s = torch.stack(sse).cpu().numpy()  # the only host wait on the metric
    ch, cwid = PF.chroma_size(h, w)
    psnr = [[PF.psnr_from_sse(int(v), npx) for v in s[:, k]] for k, npx in enumerate((h * w, ch * cwid, ch * cwid))]
    res = {"frames": nframes, "gops": ngops, "bytes": nbytes, "bpp": nbytes * 8.0 / (nframes * h * w),
           "height": h, "width": w, "coded_height": Hp, "coded_width": Wp,
           "psnr_y": psnr[0], "psnr_u": psnr[1], "psnr_v": psnr[2]}
    if msssim:
        res["msssim_y"] = np.ascontiguousarray(s[:, 3]).view(np.float64).tolist()
    return res


def decode_file(model, data: bytes, writer, device=None, verify=True):
    """Decode a container and write its frames, cropped to the display size and converted to the
    header's 8-bit pixel format, to `writer` (.write(y, u, v)) in (gop, frame) order; writer=None
    decodes (and verifies) without converting or writing. A file without display geometry / pixel
    format (float RGB at the coded size) is written at the coded size as BT.709 limited-range 4:2:0.
    When the file carries frame digests, each decoded frame is checked against its record's digest
    before it is written, and DigestMismatch is raised at the first frame that differs: from there
    on the decoder no longer holds the encoder's reference frames. verify=False decodes regardless.
    Returns {"frames", "height", "width"}, and "verified" (frames checked) for a file with digests."""
    r = C.ContainerReader(data)
    if r.header.get("tables_crc32") != C.tables_crc(model):
        raise ValueError("container was coded with different entropy tables (model weights differ)")
    dev = torch.device(device) if device is not None else next(model.parameters()).device
    h, w = C.display_size(r.header)
    pf = r.header.get("pixfmt", DEFAULT_PIXFMT)
    if pf.get("chroma") != "420":
        raise ValueError(f"unsupported pixel format {pf}")
    stamped = r.header.get("frame_digest") is not None
    n = nverified = 0
    for view, gop in r.gops():
        x = None
        for e in r.gop_records(view, gop):
            payload = r.record(e)
            if e[0] == b"I":
                x = IF.decode(C.iframe_from_payload(payload, dev))
            else:
                x = model.decompress(C.pframe_from_payload(payload, dev), x)
            if stamped and verify:
                want, got = C.record_digest(r.header, payload), DG.to_uint64(DG.frame_digest(x).item())
                if want != got:
                    raise DG.DigestMismatch(view, gop, e[3], want, got)
                nverified += 1
            if writer is not None:
                y, u, v = PF.rgb_to_yuv420(x, h, w, pf["matrix"], pf["range"])
                writer.write(y[0].cpu().numpy(), u[0].cpu().numpy(), v[0].cpu().numpy())
            n += 1
    out = {"frames": n, "height": h, "width": w}
    if stamped:
        out["verified"] = nverified
    return out

