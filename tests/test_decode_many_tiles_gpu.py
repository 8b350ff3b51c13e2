"""The product decoder on jobs of more than 65535 tile-components or tiles.  The IDWT kernels k_idwt_h / k_idwt_v and
k_idwt_tile and the unfused pack k_mct_pack index their table with blockIdx.z, and their launches put a job's whole
count into grid.z: more than the 65535 that CUDA takes there and than the 65536 the device properties state.  The HIP
runtime on gfx950 launches such grids all the same, and these tests pin that every entry is
computed; the streaming kernels take the count in a 1-D grid.  Every case is the smallest stream that crosses the
count (tiles of one or four samples, one or two levels) and is compared with the CPU oracle plane by plane, bit for
bit; each case also asserts that it still is over the count: by the tiles its SIZ segments state, by the
tile-components of the job, and by the tile-components with a coded block, which are the ones the IDWT launches carry.

The unit entry Decoder.idwt (htj2k_idwt_plane) takes a single plane, so no caller can hand it more than 65535 planes:
there is no test of it here.  (htj2k_idwt_bench is the one caller of the same launches with a plane count; it fills its
planes itself and returns a time only.)"""
import functools
import struct

import numpy as np
import pytest

import ffmpeg_ht_amd as m
import vecgen

pytestmark = pytest.mark.gpu

Z = 65535                                                   # the count the jobs here cross
YUV = dict(dx=[1, 2, 2], dy=[1, 2, 2])


def content(shapes, seed):
    """seeded samples that leave no tile-component without a coded block, whatever the tiles (one without takes no part
    in the IDWT launches, and the job would fall short of the count it is here for): every sample is above mid-grey, so
    no sample and no LL band is zero after the level shift, and of three components of one size (the RCT's) no two are
    equal anywhere"""
    rng = np.random.default_rng(seed)
    comps = [rng.integers(140, 240, (h, w)) for w, h in shapes]
    if len(shapes) == 3 and shapes[0] == shapes[1] == shapes[2]:
        for c in (0, 2):
            comps[c] = comps[1] + rng.integers(1, 12, comps[1].shape) * rng.choice([-1, 1], comps[1].shape)
    return comps


def _rgb(w, h, seed, tile):
    return vecgen.encode(content([(w, h)] * 3, seed), tile=tile, nlevels=1, mct=1)


def _gray(w, h, seed, tile, **kw):
    return vecgen.encode(content([(w, h)], seed), tile=tile, nlevels=1, **kw)


def _yuv420(w, h, seed, tile):
    return vecgen.encode(content([(w, h), (w // 2, h // 2), (w // 2, h // 2)], seed), tile=tile, nlevels=2, width=w, height=h, **YUV)


# name -> (packets of the job from a seed, tiles, tile-components, decoder options)
CASES = {
    "A_rgb_2x2":       (lambda s: [_rgb(296, 296, s, (2, 2))], 21904, 65712, {}),
    "B_rgb_1x1":       (lambda s: [_rgb(148, 148, s, (1, 1))], 21904, 65712, {}),
    "C_rgb_1x1_x3":    (lambda s: [_rgb(148, 148, s + k, (1, 1)) for k in range(3)], 65712, 197136, {}),
    "D_gray_65535":    (lambda s: [_gray(255, 257, s, (1, 1))], 65535, 65535, {}),
    "D_gray_65536":    (lambda s: [_gray(255, 257, s, (1, 1)), _gray(1, 1, s + 1, (1, 1))], 65536, 65536, {}),
    "E_gray97_float":  (lambda s: [_gray(364, 362, s + k, (2, 2), transform=0, qstep=1.0) for k in range(2)], 65884, 65884, {}),
    "E_gray97_fixed":  (lambda s: [_gray(364, 362, s + k, (2, 2), transform=0, qstep=1.0) for k in range(2)], 65884, 65884, {"bitexact": 1}),
    "F_yuv420_2x2":    (lambda s: [_yuv420(210, 210, s + k, (2, 2)) for k in range(2)], 22050, 66150, {}),
}
LAST_THAT_FITS = "D_gray_65535"                             # every other case is over the limit

MODES = {"idwt_generic": (0, 1), "idwt_tile": (1, 1), "idwt_stream_fused": (3, 1), "idwt_stream_unfused": (3, 0)}
RUNS = [("A_rgb_2x2", mode) for mode in MODES] + \
       [(name, mode) for name in list(CASES)[1:] for mode in ("idwt_stream_fused", "idwt_generic")]
RUNS = [r + ("job",) for r in RUNS] + [r + ("decode",) for r in RUNS if r[0] in ("A_rgb_2x2", "B_rgb_1x1", "D_gray_65535")]
PIPE = ("C_rgb_1x1_x3", "idwt_stream_fused", "pipe")


@functools.lru_cache(maxsize=None)
def packets(name, mode="idwt_generic", path="job"):
    """the streams of a case.  Every run of a case (a mode, and the job, the one-call or the pipe path) has pictures of its
    own: a job's device buffers are not cleared, and memory that an earlier run of the same pictures has left behind
    holds the right answer, so a launch that skipped table entries would pass on it (seen with a library built to do
    just that)"""
    return CASES[name][0](1000 * list(CASES).index(name) + 10 * list(MODES).index(mode) + 3 * ["job", "decode", "pipe"].index(path))


def siz_tiles(cs):
    """the number of tiles the SIZ marker segment of a codestream states"""
    assert cs[:4] == b"\xff\x4f\xff\x51"
    xs, ys, xo, yo, xt, yt, xto, yto = struct.unpack(">8I", cs[8:40])
    return (-(-(xs - xto) // xt)) * (-(-(ys - yto) // yt))


@pytest.fixture(scope="module")
def dec():
    d = m.Decoder(device_id=0)
    yield d
    d.close()


@pytest.fixture(scope="module")
def references(orc):
    """the oracle's frames of a case and mode, decoded once: -> [(info, planes, bytes consumed)]; and, from the oracle
    parser's block table, that every tile-component of the case has a coded block (a plane starts at a multiple of 64
    samples and none here has more than four, so plane_off // 64 numbers the tile-components of a frame)"""
    cache = {}

    def get(*run):
        if run not in cache:
            name, kw = run[0], CASES[run[0]][3]
            coded = 0
            for p in packets(*run):
                blocks = orc.plan_blocks(p, **kw)
                coded += np.unique(blocks["plane_off"][blocks["npasses"] > 0] // 64).size
            assert coded == CASES[name][2], run
            cache[run] = [orc.decode(p, **kw) for p in packets(*run)]
            assert orc.block_errors() == 0
        return cache[run]
    return get


def same_frame(got, want, what):
    (info, planes), (info_o, planes_o) = got, want[:2]
    assert (info.width, info.height, info.pix_fmt, info.bits_per_raw_sample) == \
           (info_o.width, info_o.height, info_o.pix_fmt, info_o.bits_per_raw_sample), what
    assert len(planes) == len(planes_o), what
    for p, (a, b) in enumerate(zip(planes, planes_o)):
        assert a.shape == b.shape and np.array_equal(a, b), what + (p,)


@pytest.mark.parametrize("name,mode,path", RUNS, ids=["%s-%s-%s" % r for r in RUNS])
def test_jobs_beyond_one_grid_z(dec, references, name, mode, path):
    _, ntiles, ntc, kw = CASES[name]
    pkts, want = packets(name, mode, path), references(name, mode, path)
    assert sum(siz_tiles(p) for p in pkts) == ntiles
    if name == LAST_THAT_FITS:
        assert ntiles == ntc == Z
    else:
        assert ntc > Z
    idwt_mode, fuse = MODES[mode]
    dec.set_int("idwt_mode", idwt_mode)
    dec.set_int("fuse_pack", fuse)
    dec.set_int("bitexact", kw.get("bitexact", 0))
    try:
        if path == "decode":                                # the one-call path
            info, planes, consumed, st = dec.decode(pkts[0])
            assert consumed == want[0][2] and st.n_block_errors == 0
            same_frame((info, planes), want[0], (name, mode, path))
            return
        job = dec.job().parse_batch(pkts).upload().run().wait()
        try:
            assert job.num_tilecomps() == ntc and job.num_frames() == len(pkts)
            assert job.block_errors() == 0
            for f in range(len(pkts)):
                same_frame(job.download_frame(f), want[f], (name, mode, path, f))
        finally:
            job.free()
    finally:
        dec.set_int("bitexact", 0)
        dec.set_int("idwt_mode", 3)
        dec.set_int("fuse_pack", 1)


def test_pipe_batch_beyond_one_grid_z(dec, references):
    """the three frames of case C as one batch of a pipe: 65712 pack tiles, 197136 tile-components"""
    pkts, want = packets(*PIPE), references(*PIPE)
    assert sum(siz_tiles(p) for p in pkts) == CASES[PIPE[0]][1] > Z
    pipe = dec.pipe(batch=3)
    try:
        for p in pkts:
            assert pipe.send(p)
        pipe.flush()
        got = [pipe.receive() for _ in pkts]
        assert pipe.receive() is None
    finally:
        pipe.close()
    for f, g in enumerate(got):
        assert g is not None
        same_frame(g, want[f], PIPE + (f,))
