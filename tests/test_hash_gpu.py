"""htj2k_hash_frames / htj2k_job_hash / htj2k_pipe_receive_hash on the GPU against the zlib model (hash_model): every
figure -- the frame's Adler-32, each plane's, the bytes hashed -- for equality.

Every layout family at 8 and 16 bits on host and on device operands, rows at the tails of the 16-byte groups, linesizes
equal to the row, row + 1, row + 13 and rounded to 64, base pointers off by 0, 1, 2 and 15 bytes, 0xAB dirt in the
padding, weights that wrap and sums at their largest, batches of unlike frames, more planes than grid.z takes, jobs,
pipes and the C example.  Run as a program, the module runs all of it on its own contexts:
test_everything_on_poisoned_buffers does that in a child process under HTJ2K_POISON=1."""
import ctypes
import json
import os
import subprocess
import sys
import time
import zlib

import numpy as np
import pytest
import torch  # noqa: F401  (before the library: device operands are made through it)

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
if __name__ == "__main__":
    sys.path[:0] = [HERE, ROOT]

import ffmpeg_ht_amd as m
import hash_model as hm
import oracle
import streams

KATS = json.load(open(os.path.join(HERE, "golden", "kats.json")))
# one, three and four interleaved components, planar 4:4:4 / 4:2:2 / 4:2:0, two components, XYZ12, PAL8: 8 and 16 bits
LAYOUTS = ["gray", "gray16le", "rgb24", "rgb48le", "rgba", "rgba64le", "yuv444p", "yuv444p16le", "yuv422p", "yuv422p10le",
           "yuv420p", "yuv420p16le", "yuva420p", "ya8", "ya16le", "xyz12le", "pal8"]
SIZES = [(17, 5), (49, 3), (1, 1), (257, 7)]
LS_MODES = ["row", "row+1", "row+13", "to64"]
OFFSETS = [0, 1, 2, 15]
ROWBYTES = [1, 15, 16, 17, 47, 48, 49]
EINVAL = -22


class HFrame:
    """one frame in host memory with a linesize and a base offset of its own: every byte of its buffers that is not
    hashed is 0xAB"""

    def __init__(self, fmt, w, h, rng, ls_mode="row", off=0, value=None):
        self.fmt, self.w, self.h, self.off = fmt, w, h, off
        self.geo = hm.plane_geometry(fmt, w, h)
        self.bufs, self.ls = [], []
        for rows, rb in self.geo:
            ls = {"row": rb, "row+1": rb + 1, "row+13": rb + 13, "to64": -(-rb // 64) * 64}[ls_mode]
            buf = np.full(off + ls * rows + 16, 0xAB, np.uint8)
            data = rng.integers(0, 256, size=(rows, rb), dtype=np.uint8) if value is None else np.full((rows, rb), value, np.uint8)
            for y in range(rows):
                buf[off + y * ls: off + y * ls + rb] = data[y]
            self.bufs.append(buf)
            self.ls.append(ls)

    def planes(self):
        """the bytes that are hashed, as tight 2-D arrays"""
        return [np.stack([b[self.off + y * ls: self.off + y * ls + rb] for y in range(rows)])
                for b, ls, (rows, rb) in zip(self.bufs, self.ls, self.geo)]

    def arrays(self):
        """planes() as the binding takes numpy planes: 16-bit layouts as rows of uint16"""
        two = self.fmt != "pal8" and hm.cm.LAYOUTS[self.fmt][5] == 2
        return [p.view("<u2") if two else p for p in self.planes()]

    def want(self):
        return hm.frame_hash(self.planes())

    def padding(self, p):
        """indices into bufs[p] of the bytes that are not hashed"""
        rows, rb = self.geo[p]
        mask = np.ones(self.bufs[p].size, bool)
        for y in range(rows):
            mask[self.off + y * self.ls[p]: self.off + y * self.ls[p] + rb] = False
        return np.flatnonzero(mask)

    def frame(self, bases=None):
        fr = m.Frame()
        for p in range(len(self.geo)):
            fr.data[p] = (self.bufs[p].ctypes.data if bases is None else bases[p]) + self.off
            fr.linesize[p] = self.ls[p]
        fr.width, fr.height, fr.pix_fmt = self.w, self.h, m.PIX_NAMES.index(self.fmt)
        return fr

    def on_device(self):
        """(frame of device addresses, tensors to keep): the same bytes, dirt and offset on the device"""
        ts = [torch.from_numpy(b).cuda() for b in self.bufs]
        torch.cuda.synchronize()
        return self.frame([t.data_ptr() for t in ts]), ts


def both(dec, f):
    """the frame hashed as a host and as a device operand"""
    host = dec.framecrc([f.frame()], f.fmt)[0]
    fd, keep = f.on_device()
    dev = dec.framecrc([fd], f.fmt, on_device=True)[0]
    return host, dev


def check_layout(dec, fmt, i):
    for k, (w, h) in enumerate(SIZES):
        f = HFrame(fmt, w, h, np.random.default_rng(100 * i + k), LS_MODES[(i + k) % 4], OFFSETS[(i // 4 + k) % 4])
        want = f.want()
        host, dev = both(dec, f)
        assert host == want and dev == want, (fmt, w, h, host, dev, want)
        assert want["nbytes"] == sum(r * b for r, b in f.geo) and want["plane_adler32"][len(f.geo):] == [0] * (4 - len(f.geo))


def check_tails(dec, rowbytes):
    """rows of 1 .. 49 bytes, 1 to 5 of them, on every linesize and offset: short groups alone, after full ones, on both paths"""
    k = ROWBYTES.index(rowbytes)
    for rows in range(1, 6):
        for j, ls_mode in enumerate(LS_MODES):
            f = HFrame("gray", rowbytes, rows, np.random.default_rng(rowbytes * 8 + rows), ls_mode, OFFSETS[(j + k + rows) % 4])
            want = f.want()
            assert want["adler32"] == zlib.adler32(f.planes()[0].tobytes(), 0)
            host, dev = both(dec, f)
            assert host == want and dev == want, (rowbytes, rows, ls_mode, f.off, host, dev, want)


def check_dirt(dec):
    """padding is never read: any dirt gives the same value, one changed padding byte too; one changed sample byte does not"""
    for i, fmt in enumerate(("rgb24", "yuv420p16le", "pal8")):
        for ls_mode, off in (("row+13", 1), ("to64", 0)):
            f = HFrame(fmt, 37, 5, np.random.default_rng(50 + i), ls_mode, off)
            want = f.want()
            assert both(dec, f) == (want, want)
            for p in range(len(f.geo)):
                pad = f.padding(p)
                f.bufs[p][pad[len(pad) // 2]] ^= 0x5A                     # one padding byte
                assert both(dec, f) == (want, want), (fmt, ls_mode, p)
                f.bufs[p][pad] = np.random.default_rng(p).integers(0, 256, size=pad.size, dtype=np.uint8)   # all of them
                assert both(dec, f) == (want, want), (fmt, ls_mode, p)
            for p in range(len(f.geo)):
                rows, rb = f.geo[p]
                at = f.off + (rows - 1) * f.ls[p] + rb - 1                  # the plane's last hashed byte
                f.bufs[p][at] ^= 1
                now = f.want()
                assert now["adler32"] != want["adler32"] and now["plane_adler32"][p] != want["plane_adler32"][p]
                assert both(dec, f) == (now, now), (fmt, ls_mode, p)
                want = now


def check_extremes(dec):
    """weights that wrap (a plane just past 65521 bytes) and sums at their largest"""
    f = HFrame("rgb24", 300, 73, np.random.default_rng(7), "row+1", 2)
    assert f.want()["nbytes"] == 65700 and both(dec, f) == (f.want(), f.want())
    f = HFrame("rgb24", 300, 73, None, "row", 0, value=0xFF)
    assert both(dec, f) == (f.want(), f.want())
    ones = np.full((1024, 1024), 0xFF, np.uint8)
    want = hm.frame_hash([ones])
    assert want["adler32"] == zlib.adler32(b"\xff" * (1 << 20), 0)
    assert dec.framecrc([[ones]], "gray")[0] == want
    t = torch.from_numpy(ones).cuda()
    torch.cuda.synchronize()
    fr, keep = m.frame_from_planes([ones], "gray")
    fr.data[0] = t.data_ptr()
    assert dec.framecrc([fr], "gray", on_device=True)[0] == want
    big = np.full((1024, 2048 * 3), 0xFFFF, np.uint16)                         # 12 MiB of 0xFF: many workgroups a plane
    want = hm.frame_hash([big])
    assert want["nbytes"] == 2048 * 1024 * 6
    assert dec.framecrc([[big]], "rgb48le")[0] == want
    t = torch.from_numpy(big.view(np.int16)).cuda()
    torch.cuda.synchronize()
    fr, keep = m.frame_from_planes([big], "rgb48le")
    fr.data[0] = t.data_ptr()
    assert dec.framecrc([fr], "rgb48le", on_device=True)[0] == want
    assert dec.compare_ms() > 0


def check_batches(dec):
    """frames of different layouts and sizes in one call, as host and as device operands"""
    rng = np.random.default_rng(21)
    fs = [HFrame(fmt, w, h, rng, LS_MODES[i % 4], OFFSETS[(i + 1) % 4])
          for i, (fmt, w, h) in enumerate([("rgb24", 65, 5), ("yuv422p10le", 17, 2), ("pal8", 33, 9), ("gray16le", 257, 3),
                                           ("yuva420p", 19, 7), ("xyz12le", 48, 1), ("rgba64le", 5, 5)])]
    want = [f.want() for f in fs]
    assert dec.framecrc([f.frame() for f in fs], None) == want
    devs = [f.on_device() for f in fs]
    assert dec.framecrc([d for d, _ in devs], None, on_device=True) == want
    assert dec.framecrc([f.arrays() for f in fs], [f.fmt for f in fs]) == want         # numpy planes, a layout each
    assert len({w["adler32"] for w in want}) == len(want)
    bad = fs[1].frame()
    bad.linesize[2] -= 14                                                              # below the row
    with pytest.raises(m.Htj2kError) as e:
        dec.framecrc([fs[0].frame(), bad], None)
    assert e.value.code == EINVAL


def check_many_frames(dec, n=70000):
    """more planes than grid.z takes in one launch: 9 x 7 rgba frames out of one buffer"""
    size = 9 * 4 * 7
    a = np.random.default_rng(9).integers(0, 256, size=(n, size), dtype=np.uint8)
    rec = np.dtype({"names": ["data", "linesize", "width", "height", "pix_fmt"], "formats": [("<u8", 4), ("<i4", 4), "<i4", "<i4", "<i4"],
                    "offsets": [0, 32, 48, 52, 56], "itemsize": ctypes.sizeof(m.Frame)})
    t = np.zeros(n, rec)
    t["data"][:, 0] = a.ctypes.data + size * np.arange(n, dtype=np.uint64)
    t["linesize"][:, 0] = 36
    t["width"], t["height"], t["pix_fmt"] = 9, 7, m.PIX_NAMES.index("rgba")
    out = (m.FrameHash * n)()
    assert dec.L.htj2k_hash_frames(dec.h, t.ctypes.data_as(ctypes.c_void_p), 0, n, out) == 0
    got = np.frombuffer(out, np.dtype({"names": ["adler32", "plane_adler32", "nbytes"], "formats": ["<u4", ("<u4", 4), "<u8"],
                                       "offsets": [0, 4, 24], "itemsize": ctypes.sizeof(m.FrameHash)}))
    want = np.array([zlib.adler32(a[i].tobytes(), 0) for i in range(n)], np.uint32)
    assert np.array_equal(got["adler32"], want) and np.array_equal(got["plane_adler32"][:, 0], want)
    assert not got["plane_adler32"][:, 1:].any() and (got["nbytes"] == size).all()


def damaged_copy(data, seed=0):
    """headers intact, 64 random bytes in the code-block bodies: it parses, and some of its blocks are rejected"""
    rng = np.random.default_rng(seed)
    b = bytearray(data)
    start = data.index(b"\xff\x93") + 2
    for _ in range(64):
        b[int(rng.integers(start, len(b) - 2))] = int(rng.integers(0, 256))
    return bytes(b)


def check_jobs(dec, orc):
    for kat in KATS:                                                    # the known answers, and nothing downloaded
        job = dec.job().parse(bytes.fromhex(kat["hex"])).upload().run()
        got = job.framecrc()
        assert len(got) == 1 and got[0]["adler32"] == int(kat["framecrc"], 16), (kat["name"], got)
        assert got[0]["nbytes"] == kat["width"] * kat["height"] * (3 if kat["pix_fmt"] == "rgb24" else 1)
        job.free()
    names = ["rgb_mct", "pal8_jp2", "yuv420p8", "gray16", "yuv422p12_97", "rgb10_mct", "gray_l5_cb64"]
    datas = [streams.get(n)[0] for n in names]
    job = dec.job().parse_batch(datas)
    out = (m.FrameHash * len(names))()
    assert dec.L.htj2k_job_hash(dec.h, job.h, out) == EINVAL            # before the upload
    job.upload()
    assert dec.L.htj2k_job_hash(dec.h, job.h, out) == EINVAL            # before the first run
    job.run()
    got = job.framecrc()
    for f, (name, data) in enumerate(zip(names, datas)):
        info, planes = job.download_frame(f)
        assert got[f] == hm.frame_hash(planes, info), name
        assert got[f]["adler32"] == oracle.framecrc(planes) == oracle.framecrc(orc.decode(data)[1]), name
    assert got[1]["plane_adler32"][1] != 0 and got[1]["nbytes"] == 56 * 40 + 1024     # the palette is part of a pal8 frame
    job.run(stages=3)                                                   # a run that did not write the frames
    with pytest.raises(m.Htj2kError) as e:
        job.framecrc()
    assert e.value.code == EINVAL
    job.run()
    assert job.framecrc() == got
    # a packet whose blocks the decoder rejects is still a frame (the blocks stay zero): the call answers for all of them
    bad = damaged_copy(datas[6])
    info_o, planes_o, _ = orc.decode(bad)
    assert orc.block_errors() > 0 and orc.underrun_blocks() == 0
    job.parse_batch([datas[0], bad, datas[3]]).upload().run()
    got3 = job.framecrc()
    assert job.block_errors() == orc.block_errors()
    assert [g["adler32"] for g in got3] == [got[0]["adler32"], oracle.framecrc(planes_o), got[3]["adler32"]]
    assert got3[1] == hm.frame_hash(job.download_frame(1)[1]) and got3[1]["adler32"] != got[6]["adler32"]
    # a packet that does not parse fails the whole batch (htj2k_job_parse_batch): there is no job to ask
    with pytest.raises(m.Htj2kError):
        job.parse_batch([datas[0], b"\x00\x01garbage" * 9])
    assert dec.L.htj2k_job_hash(dec.h, job.h, out) == EINVAL
    job.free()


def drain(pipe, pkts, receive):
    """all packets through the pipe -> what `receive` gave per packet, None where the packet failed"""
    got, sent = [], 0
    while len(got) < len(pkts):
        while sent < len(pkts) and pipe.send(pkts[sent]):
            sent += 1
        if sent == len(pkts):
            pipe.flush()
        try:
            r = receive(pipe)
            assert r is not None
            got.append(r)
        except m.Htj2kError as e:
            got.append(("error", e.code))
    return got


def check_pipes(dec, orc):
    names = ["rgb_mct", "pal8_jp2", "yuv420p8", "gray16", "gray_l5_cb64", "p1_gray_cb32", "gray_97_q2", "rgb10_mct"]
    pkts = [streams.get(names[i % len(names)])[0] for i in range(16)]
    pkts[7] = pkts[7][:40]                                              # fails to parse: its batch is retried packet by packet
    pipe = dec.pipe(batch=4, depth=2)
    try:
        crcs = drain(pipe, pkts, lambda p: p.receive_crc())
        assert pipe.receive_crc() is None and pipe.receive() is None    # drained
        frames = drain(pipe, pkts, lambda p: p.receive())
        assert pipe.receive_crc() is None
    finally:
        pipe.close()
    for i, (c, f) in enumerate(zip(crcs, frames)):
        if i == 7:
            assert c[0] == "error" and f[0] == "error" and c[1] < 0 and c[1] != m.EAGAIN, (c, f)
            continue
        (info_c, h), (info_f, planes) = c, f
        assert all(getattr(info_c, k) == getattr(info_f, k) for k in ("width", "height", "pix_fmt", "nplanes", "bits_per_raw_sample")), i
        assert h == hm.frame_hash(planes, info_f), (i, h)
        assert h["adler32"] == oracle.framecrc(orc.decode(pkts[i])[1]), i
    # receive_crc between receive_device calls: a hashed frame is no hand-out, the frames handed out keep their promise
    # (valid until all frames of depth - 1 further batches are out), and the pipe neither stalls nor frees early
    batch, depth = 4, 3
    pkts = [streams.get(names[i % len(names)])[0] for i in range(30)]
    want = [orc.decode(d)[1] for d in pkts]
    pipe = dec.pipe(batch=batch, depth=depth)
    held = []
    try:
        sent = got = 0
        while got < len(pkts):
            while sent < len(pkts) and pipe.send(pkts[sent]):
                sent += 1
            if sent == len(pkts):
                pipe.flush()
            if got % 2 or got // batch == 2:                            # a batch of hashes only among the mixed ones
                info, h = pipe.receive_crc()
                assert h["adler32"] == oracle.framecrc(want[got]), got
            else:
                info = m.Info()
                assert dec.L.htj2k_pipe_info(pipe.h, ctypes.byref(info)) == 0
                held.append((got, info, pipe.receive_device()))
            got += 1
            while held and (got - 1) // batch - held[0][0] // batch >= depth - 1:
                i, inf, f = held.pop(0)
                assert all(np.array_equal(a, b) for a, b in zip(dec.fetch_device_frame(inf, f), want[i])), i
        for i, inf, f in held:
            assert all(np.array_equal(a, b) for a, b in zip(dec.fetch_device_frame(inf, f), want[i])), i
        assert pipe.receive_crc() is None
    finally:
        pipe.close()


def framecrc_text(version, planes_of):
    """what examples/htj2k_framecrc writes for frames whose oracle planes are planes_of[i] = (info, planes)"""
    info0 = planes_of[0][0]
    lines = ["#software: %s" % version, "#tb 0: 1/25", "#media_type 0: video", "#codec_id 0: rawvideo",
             "#dimensions 0: %dx%d" % (info0.width, info0.height), "#sar 0: %d/%d" % (info0.sar_num, info0.sar_den or 1)]
    for i, (info, planes) in enumerate(planes_of):
        size = sum(np.ascontiguousarray(p).nbytes for p in planes)
        lines.append("0, %10d, %10d, %8d, %8d, 0x%08x" % (i, i, 1, size, oracle.framecrc(planes)))
    return "\n".join(lines) + "\n"


def check_c_example(orc, tmp):
    r = subprocess.run(["make", "-C", ROOT, "examples"], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-2000:]
    names = ["rgb_mct", "yuv422p12_97", "rgb_tiles"]
    seq = os.path.join(tmp, "three.j2k")
    with open(seq, "wb") as f:
        f.write(b"".join(streams.get(n)[0] for n in names))
    decoded = [orc.decode(streams.get(n)[0], **streams.get(n)[1])[:2] for n in names]
    r = subprocess.run([os.path.join(ROOT, "examples", "htj2k_framecrc"), seq], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, (r.stdout, r.stderr)
    assert r.stdout == framecrc_text(m.load_library().htj2k_version().decode(), decoded), r.stdout


@pytest.fixture(scope="module")
def dec():
    d = m.Decoder(device_id=0)
    yield d
    d.close()


@pytest.mark.gpu
@pytest.mark.parametrize("fmt", LAYOUTS)
def test_layouts_on_host_and_device_operands(dec, fmt):
    check_layout(dec, fmt, LAYOUTS.index(fmt))


@pytest.mark.gpu
@pytest.mark.parametrize("rowbytes", ROWBYTES)
def test_group_tails(dec, rowbytes):
    check_tails(dec, rowbytes)


@pytest.mark.gpu
def test_padding_is_never_read(dec):
    check_dirt(dec)


@pytest.mark.gpu
def test_weights_that_wrap_and_largest_sums(dec):
    check_extremes(dec)


@pytest.mark.gpu
def test_batches_of_unlike_frames(dec):
    check_batches(dec)


@pytest.mark.gpu
def test_more_planes_than_one_launch_takes(dec):
    check_many_frames(dec)


@pytest.mark.gpu
def test_jobs(dec, orc):
    check_jobs(dec, orc)


@pytest.mark.gpu
def test_pipes(dec, orc):
    check_pipes(dec, orc)


@pytest.mark.gpu
def test_c_example_program(orc, tmp_path):
    check_c_example(orc, str(tmp_path))


def run_everything(dec, orc, tmp):
    for i, fmt in enumerate(LAYOUTS):
        check_layout(dec, fmt, i)
    for rowbytes in ROWBYTES:
        check_tails(dec, rowbytes)
    check_dirt(dec)
    check_extremes(dec)
    check_batches(dec)
    check_many_frames(dec)
    check_jobs(dec, orc)
    check_pipes(dec, orc)
    check_c_example(orc, tmp)


POISON_TIMEOUT = 180


@pytest.mark.gpu
def test_everything_on_poisoned_buffers(tmp_path):
    """HTJ2K_POISON=1 (read once per process, so a fresh child, and the C example as its child inherits it): every new
    device buffer starts as 0xA5 bytes, and all of the above must still give the model's results"""
    r = subprocess.run([sys.executable, os.path.abspath(__file__), str(tmp_path)], capture_output=True, text=True,
                       timeout=POISON_TIMEOUT, env=dict(os.environ, HTJ2K_POISON="1"))
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-3000:]
    assert "poisoned buffers: ok" in r.stdout, r.stdout[-3000:]


if __name__ == "__main__":
    import tempfile
    t0 = time.time()
    _dec, _orc = m.Decoder(device_id=0), oracle.OracleDecoder()
    with tempfile.TemporaryDirectory() as _tmp:
        run_everything(_dec, _orc, sys.argv[1] if len(sys.argv) > 1 else _tmp)
    _dec.close()
    _orc.close()
    print("%s buffers: ok, %.1f s" % ("poisoned" if os.environ.get("HTJ2K_POISON") == "1" else "plain", time.time() - t0))
