"""Frames for the encoder built by hand (test tooling, no tests in it): htj2k_frame entries whose rows are padded and
whose padding is poisoned, in host or device memory, raw calls of htj2k_encode_batch, and the CPU rebuild of a
budgeted stream from the planes the encoder reports.  m.frame_from_planes makes every plane contiguous; these do not."""
import ctypes

import numpy as np

import enc_model as em
import ffmpeg_ht_amd as m
import rc_model as rc

POISON = 0xA5


def padded_plane(a, pad, poison=POISON):
    """2-D uint8 / uint16 plane -> uint8 array of rows of `row bytes + pad` bytes, the padding filled with `poison`"""
    a = np.ascontiguousarray(a)
    rows, row = a.shape[0], a.shape[1] * a.itemsize
    buf = np.full((rows, row + pad), poison, np.uint8)
    buf[:, :row] = a.view(np.uint8).reshape(rows, row)
    return buf


def padded_frame(planes, fmt, w, h, pads):
    """(htj2k_frame, arrays it points into): plane p with pads[p] bytes of poisoned padding behind every row"""
    fr, keep = m.Frame(), []
    for p, a in enumerate(planes):
        buf = padded_plane(a, pads[p])
        keep.append(buf)
        fr.data[p] = buf.ctypes.data
        fr.linesize[p] = buf.shape[1]
    fr.width, fr.height, fr.pix_fmt = w, h, em.pix(fmt)
    return fr, keep


def device_frame(planes, fmt, w, h, pads, torch):
    """the same frame in device memory: (htj2k_frame, tensors it points into)"""
    fr, keep = m.Frame(), []
    for p, a in enumerate(planes):
        t = torch.from_numpy(padded_plane(a, pads[p])).cuda()
        keep.append(t)
        fr.data[p] = t.data_ptr()
        fr.linesize[p] = t.shape[1]
    torch.cuda.synchronize()
    fr.width, fr.height, fr.pix_fmt = w, h, em.pix(fmt)
    return fr, keep


def call_batch(enc, frames, bits, out, cap=None, in_on_device=0, out_on_device=0, n=None, **opts):
    """htj2k_encode_batch as it is: `out` a numpy uint8 array, or a device address with `cap` given -> (return code,
    offsets[0 .. n])"""
    n = len(frames) if n is None else n
    arr = (m.Frame * max(len(frames), 1))(*frames)
    o = m._enc_opts(**opts)
    offs = (ctypes.c_size_t * (max(n, 0) + 1))()
    if isinstance(out, np.ndarray):
        ptr, cap = out.ctypes.data_as(ctypes.c_void_p), out.size if cap is None else cap
    else:
        ptr = ctypes.c_void_p(out)
    r = enc.L.htj2k_encode_batch(enc.h, arr, n, bits, ctypes.byref(o), int(in_on_device), ptr, ctypes.c_size_t(cap),
                                 int(out_on_device), offs)
    return r, list(offs)


def encode_frames(enc, frames, fmt, bits, in_on_device=0, **opts):
    """hand-built frames through one call -> [codestream bytes]; raises on a refusal"""
    cap = sum(m.Encoder.bound(f.width, f.height, fmt, bits, **opts) for f in frames)
    out = np.empty(max(cap, 1), np.uint8)
    enc._logs.clear()
    r, offs = call_batch(enc, frames, bits, out, in_on_device=in_on_device, **opts)
    if r < 0:
        raise m.Htj2kError(r, "htj2k_encode_batch: " + "".join(enc._logs).strip())
    return [out[offs[i]:offs[i + 1]].tobytes() for i in range(len(frames))]


def rebuild(comps, fmt, bits, w, h, planes, guard, **opts):
    """a budgeted stream again on the CPU, from the planes the encoder reports for it: vecgen's blocks of the model's
    shifted indices, written by the host writer with the guard bits of the stream"""
    irrev = bool(opts.get("irreversible"))
    mct = em.mct_default(fmt) if opts.get("mct", -1) < 0 else bool(opts["mct"])
    idx = rc.indices(comps, fmt, bits, opts["levels"], mct, irrev, opts.get("qstep", 1.0))
    o = {k: v for k, v in opts.items() if k not in ("target_bytes", "guard_bits")}
    blocks = m.Encoder.layout(w, h, fmt, bits, **o)
    assert len(planes) == len(blocks)
    coded = [rc.code_block(rc.block_view(idx, b), p) for b, p in zip(blocks, planes)]
    return m.Encoder.assemble(w, h, fmt, bits, [c[0] for c in coded], max_u=[c[2] for c in coded], planes=planes,
                              guard_bits=guard, **o)
