"""numpy / zlib restatement of htj2k_hash_frames (include/htj2k_amd.h, csrc/cmp_kernels.hpp: k_frame_adler): the frame's
Adler-32 seeded with 0 over its packed planes, each plane's own, and the bytes hashed.  frame_hash is the definition
(zlib over the bytes); grouped_sums and combine restate how the kernel and the host get there, for the host tests."""
import zlib

import numpy as np

import cmp_model as cm

MOD = 65521


def plane_geometry(fmt, w, h):
    """[(rows, bytes of a row)] of every plane of the layout as it is hashed; pal8: the indices, then the palette"""
    if fmt == "pal8":
        return [(h, w), (1, 1024)]
    b = cm.LAYOUTS[fmt][5]
    return [(rows, cols * b) for rows, cols in cm.plane_shapes(fmt, w, h)]


def info_geometry(info):
    return [(info.plane_height[p], info.plane_width[p] * info.plane_bytes_per_sample[p]) for p in range(info.nplanes)]


def packed(plane, rows, rowbytes):
    """the bytes of a plane that are hashed: `rows` rows of `rowbytes` bytes of a 2-D array that may be wider"""
    a = np.ascontiguousarray(plane)
    a = a.view(np.uint8).reshape(a.shape[0], -1)
    assert a.shape[0] >= rows and a.shape[1] >= rowbytes, (a.shape, rows, rowbytes)
    return np.ascontiguousarray(a[:rows, :rowbytes]).tobytes()


def frame_hash(planes, info=None, geometry=None):
    """{"adler32", "plane_adler32", "nbytes"} as FrameHash.as_dict(): planes are 2-D arrays; with an Info (or a geometry
    from plane_geometry) only plane_height rows of plane_width * plane_bytes_per_sample bytes count, else all of them"""
    if info is not None:
        geometry = info_geometry(info)
    if geometry is None:
        geometry = [(np.asarray(p).shape[0], np.ascontiguousarray(p).view(np.uint8).reshape(np.asarray(p).shape[0], -1).shape[1])
                    for p in planes]
    assert len(geometry) == len(planes)
    parts = [packed(p, rows, rb) for p, (rows, rb) in zip(planes, geometry)]
    v = 0
    for b in parts:
        v = zlib.adler32(b, v)
    return {"adler32": v & 0xFFFFFFFF, "plane_adler32": [zlib.adler32(b, 0) & 0xFFFFFFFF for b in parts] + [0] * (4 - len(parts)),
            "nbytes": sum(len(b) for b in parts)}


def grouped_sums(data, rowbytes=None):
    """(A, B) before the final mod, as k_frame_adler accumulates them in 64 bits: the plane `data` (bytes, rows of
    `rowbytes`, default one row) cut into 16-byte groups of a row; a group at offset o of the L bytes adds A_g = sum d_k
    and (w + 65521) A_g - sum k d_k with w = (L - o) mod 65521, the weight in 32-bit steps as the kernel takes them"""
    d = np.frombuffer(data, np.uint8)
    L = d.size
    rowbytes = L if rowbytes is None else rowbytes
    rows = L // rowbytes
    assert rows * rowbytes == L
    gpr = -(-rowbytes // 16)
    padded = np.zeros((rows, gpr * 16), np.uint64)
    padded[:, :rowbytes] = d.reshape(rows, rowbytes)
    g = padded.reshape(rows, gpr, 16)
    ag = g.sum(2)                                                   # at most 4080
    kg = (g * np.arange(16, dtype=np.uint64)).sum(2)
    y = np.arange(rows, dtype=np.uint64)[:, None]
    off = (np.arange(gpr, dtype=np.uint64) * np.uint64(16))[None, :]
    left = ((np.uint64(rows) - y) % np.uint64(MOD)) * np.uint64(rowbytes % MOD)
    assert int(left.max()) < 1 << 32                                # the kernel's 32-bit product
    wgt = (left % np.uint64(MOD) + np.uint64(MOD) - off % np.uint64(MOD)) % np.uint64(MOD)
    bg = (wgt + np.uint64(MOD)) * ag - kg
    assert int(bg.max()) < 1 << 29                                  # the bound the 2^38-byte limit rests on
    A, B = int(ag.sum(dtype=np.uint64)), int(bg.sum(dtype=np.uint64))
    assert B < 1 << 64 and (L >> 4) * ((1 << 29) - 1) < 1 << 64      # no wrap of the 64-bit accumulator at this length
    return A, B


def adler_of(A, B):
    return ((B % MOD) << 16 | (A % MOD)) & 0xFFFFFFFF


def combine(parts):
    """the frame's value from [(A_p, B_p, L_p)] of its planes in order: A = sum A_p,
    B = sum (B_p + A_p * bytes after plane p), mod 65521"""
    A = B = after = 0
    for a, b, n in reversed(parts):
        a, b = a % MOD, b % MOD
        A += a
        B += b + a * (after % MOD)
        after += n
    return adler_of(A, B)
