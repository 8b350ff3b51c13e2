"""The HT block kernels of every route a job can take, on unit tables (tests/ht_route_cases.py; knob "unit_ht" of
htj2k_ht_blocks, Decoder.ht_blocks(route=...)) against the CPU oracle: oracle.ht_decode_block + roi_cases.dequant,
compared as bit patterns over the whole sample buffer, so that every window, every sample between the windows and the
status of every block is checked.  The blocks of one wavefront differ in shape, content, M_b, zbp and pass count, which
the frames of a job never make them do.  tests/test_ht_route_cases.py pins the tables on the CPU.

Which table reaches which kernel (route -> HtChoice: ht_blocks() in csrc/htj2k_device.hip):
  column_wide    route 1: k_ht_unstuff_g<32>, k_ht_vlc (a block wider than 64 columns), k_ht_refine, k_ht_decode<true>
                 route 0: k_ht_unstuff, k_ht_vlc, k_ht_refine, k_ht_decode<true> (the unit entry's fixed choice)
  column_mid     route 1: k_ht_unstuff_g<32>, k_ht_vlc2, k_ht_refine, k_ht_decode<true>
  column_narrow  route 1: k_ht_unstuff_g<16>, k_ht_vlc2, k_ht_refine, k_ht_decode<true>
  multi_nb4_cleanup_br0..3   k_ht_unstuff_g<16>, k_ht_vlc2, k_ht_decode_multi<4, T, false>, T = 5/3 (step 1, another step),
                             9/7 float, 9/7 integer
  multi_nb4_refine_br0..3    ... k_ht_refine<uint32_t, false>, k_ht_decode_multi<4, T, true>
  multi_nb2_cleanup_br0..3   k_ht_unstuff_g<32>, k_ht_vlc2, k_ht_decode_multi<2, T, false>
  multi_nb2_refine_br0..3    ... k_ht_refine<uint64_t, false>, k_ht_decode_multi<2, T, true>
  multi_one_block            k_ht_decode_multi<4, 9/7 float, false>, a wave with one block
  raw table (test_transcode_ht_gpu.raw_table), route 2: k_ht_decode_multi<4 | 2, RAW, false | true>; route 1:
                 k_ht_vlc | k_ht_vlc2 and k_ht_decode_raw<true>
  c16_route3     k_ht_unstuff_g<32>, k_ht_vlc2, k_ht_decode_pair
  c16_route4     k_ht_unstuff_g<32>, k_ht_vlc2, k_ht_decode<true> with 16-bit stores
  broken_route2_nb4 / _nb2, broken_route3_nb2, broken_route4_nb1: the same kernels with rejected blocks in their waves

No kernel is given a block of more than 4096 samples (ht_route_cases.OVERSIZE): the entry refuses them on every route."""
import numpy as np
import pytest

import ht_route_cases as rc
import roi_cases

pytestmark = pytest.mark.gpu

EINVAL, EXTERNAL = -22, -0x20545845


@pytest.fixture(scope="module")
def dec():
    import ffmpeg_ht_amd as m
    d = m.Decoder()
    assert d.device_name().startswith("gfx950"), d.device_name()
    yield d
    d.close()


@pytest.fixture
def t(request):
    """the table of that name (built, and its blocks decoded by the oracle, when the first test asks)"""
    return {t.name: t for t in rc.all_tables()}[request.param]


def _desc(block, branch, data_off=0, plane_off=0, stride=None, flags=None, **over):
    import ffmpeg_ht_amd as m
    d = m.BlockDesc()
    d.data_off, d.plane_off, d.lcup, d.lref, d.w, d.h = data_off, plane_off, block.lcup, block.lref, block.w, block.h
    d.stride = block.w if stride is None else stride
    d.npasses, d.zbp, d.M_b, d.roi_shift = block.npasses, block.zbp, block.M_b, 0
    d.flags = ((8 if block.causal else 0) | branch[0]) if flags is None else flags
    d.f_step, d.i_step = branch[1], branch[2]
    for k, v in over.items():
        setattr(d, k, v)
    return d


def _ht_blocks(dec, *a, **kw):
    """Decoder.ht_blocks; a failure of the HIP runtime ends the session: nothing more is started on a device that has faulted"""
    import ffmpeg_ht_amd as m
    try:
        return dec.ht_blocks(*a, **kw)
    except m.Htj2kError as e:
        if e.code == EXTERNAL:
            pytest.exit("HIP runtime failure in htj2k_ht_blocks: %s %r" % (a[2:], kw.get("route")), returncode=3)
        raise


def _descs(t):
    return [_desc(e.block, e.branch, e.data_off, e.plane_off, e.stride) for e in t.entries]


def _run_and_check(dec, t, route):
    out = t.fill.copy()
    got, status = _ht_blocks(dec, _descs(t), t.pool, t.nsamples, route=route, out=out)
    want = t.expected()
    got = got if t.sixteen else got.view(np.uint32)
    assert got.shape == want.shape
    # status: non-zero for exactly the blocks the oracle rejects
    assert np.array_equal(status != 0, t.bad_status()), (t.name, route, np.flatnonzero((status != 0) != t.bad_status()))
    if np.array_equal(got, want):
        return
    wrong = [(k, e.block.shape, e.block.cls, e.block.npasses, e.block.M_b, e.block.zbp, e.branch, int((t.window(got, e) != t.window(want, e)).sum()))
             for k, e in enumerate(t.entries) if not np.array_equal(t.window(got, e), t.window(want, e))]
    covered = np.zeros(want.shape, dtype=bool)
    for e in t.entries:
        b = e.block
        covered[(e.plane_off + np.arange(b.h)[:, None] * e.stride + np.arange(b.w)[None, :]).ravel()] = True
    stray = np.flatnonzero((got != want) & ~covered)
    raise AssertionError("%s, route %d: %d blocks differ from the oracle (index, shape, class, npasses, M_b, zbp, dequantiser, samples): %r; "
                         "%d samples outside every window changed, first at %r"
                         % (t.name, route, len(wrong), wrong[:12], stray.size, stray[:8].tolist()))


@pytest.mark.parametrize("route", [1, 0])
@pytest.mark.parametrize("t", rc.NAMES_ROUTE1, indirect=True)
def test_column_route(dec, t, route):
    """every shape, class, pass count and dequantiser through the route of the jobs without a faster one, with each of
    its front ends (k_ht_vlc / k_ht_vlc2, two and four blocks per wave in the un-stuffing kernel), and through the unit
    entry's fixed choice"""
    _run_and_check(dec, t, route)


@pytest.mark.parametrize("t", rc.NAMES_ROUTE2, indirect=True)
def test_multi_route(dec, t):
    """k_ht_decode_multi, four and two blocks per wave, each dequantiser, without and with blocks that carry SigProp /
    MagRef passes: blocks of every admissible shape and class side by side in a wave, taller than the 64-row register
    window beside shorter ones, without passes beside coded ones, a last wave that is not full"""
    _run_and_check(dec, t, 2)


@pytest.mark.parametrize("t", rc.NAMES_ROUTE34, indirect=True)
def test_sixteen_bit_routes(dec, t):
    """k_ht_decode_pair and k_ht_decode<true> with 16-bit stores: the int32 plane of the oracle cast to int16 (exact:
    M_b <= 15), +-16383 at M_b = 15 among them; the int16 samples between the windows untouched"""
    _run_and_check(dec, t, t.route)


@pytest.mark.parametrize("t", rc.NAMES_BROKEN, indirect=True)
def test_rejected_blocks_beside_good_ones(dec, t):
    """Lcup < 2, a bad Scup, an exponent bound above maxbp in waves with blocks that decode: status non-zero for exactly
    the blocks the oracle rejects, their windows zero, their wave-mates as the oracle has them, the padding untouched"""
    assert t.bad_status().sum() == 6
    _run_and_check(dec, t, t.route)


# ---------------------------------------------------------------- raw stores
@pytest.fixture(scope="module")
def raw():
    from test_transcode_ht_gpu import raw_table
    return raw_table()


def _pcup(d, pool):
    if d.npasses == 0 or d.lcup < 2:
        return 0
    scup = (pool[d.data_off + d.lcup - 1] << 4) + (pool[d.data_off + d.lcup - 2] & 15)
    return d.lcup - scup if 2 <= scup <= d.lcup and scup <= 4079 else 0


def _coded(d):
    return d.npasses - (d.npasses - d.npasses % 3 if d.npasses % 3 else d.npasses - 3)


@pytest.mark.parametrize("route,maxw,refine", [(1, 1024, True), (1, 64, True), (2, 64, False), (2, 64, True), (2, 32, False), (2, 32, True)])
def test_raw_stores_on_the_job_routes(dec, raw, route, maxw, refine):
    """the transcoder's raw stores (the expectation of test_ht_blocks_raw: xc_ht_model.raw_index of the oracle's words)
    through k_ht_decode_raw<true> behind k_ht_vlc and k_ht_vlc2, and through k_ht_decode_multi<NB, RAW, REFINE>"""
    descs, pool, expect, soff = raw
    keep = [k for k, d in enumerate(descs) if d.w <= maxw and (refine or _coded(d) == 1)]
    assert len(keep) > 8
    assert refine == any(_coded(descs[k]) > 1 for k in keep)
    if route == 2:                                           # what the route asks, computed: the MagSgn bits of a wave in LDS
        nb = 4 if maxw <= 32 else 2
        assert rc.multi_lds(nb, max(_pcup(descs[k], pool) for k in keep)) <= rc.MULTI_LDS_MAX
    got, status = _ht_blocks(dec, [descs[k] for k in keep], pool, soff, raw=True, route=route)
    assert not status.any()
    want = np.full(soff, 0x7FFFFFFF, dtype=np.int32)
    for k in keep:
        o, w = expect[k]
        want[o:o + w.size] = w.ravel()
    bad = [k for k in keep if not np.array_equal(got[expect[k][0]:expect[k][0] + expect[k][1].size], expect[k][1].ravel())]
    assert not bad, [(k, descs[k].w, descs[k].h, descs[k].npasses) for k in bad]
    assert np.array_equal(got, want)                         # the windows of the blocks left out: as they went in


# ---------------------------------------------------------------- refusals
def _refused(dec, descs, pool, route, raw=False, nsamples=8192):
    import ffmpeg_ht_amd as m
    rng = np.random.default_rng(route)
    out = rng.integers(0, 1 << 32, nsamples, dtype=np.uint64).astype(np.uint32)
    before = out.copy()
    with pytest.raises(m.Htj2kError) as err:
        _ht_blocks(dec, descs, pool, nsamples, raw=raw, route=route, out=out)
    assert err.value.code == EINVAL
    assert np.array_equal(out, before)


def _accepted(dec, descs, pool, route, nsamples=8192):
    got, status = _ht_blocks(dec, descs, pool, nsamples, route=route)
    assert not status.any()


def _pool(*blks):
    pool, offs = b"", []
    for b in blks:
        offs.append(len(pool))
        pool += b.data + b"\0" * ((-len(b.data)) % 16)
    return pool, offs


def test_tables_a_route_excludes_are_refused(dec, raw):
    """HTJ2K_ERR_EINVAL before anything is uploaded, the buffer as it went in; the same block is taken where the one
    condition it misses is not asked"""
    import ffmpeg_ht_amd as m
    B, BR = rc.blocks(), roi_cases.BRANCHES
    rng = np.random.default_rng(99)
    good = B[(32, 32), "dense", "c"]
    pool, _ = _pool(good)
    _accepted(dec, [_desc(good, BR[0])], pool, 3)
    # route 3: an odd width (even stride and offset); route 4 takes it
    odd = B[(31, 33), "dense", "c"]
    pool, _ = _pool(odd)
    _refused(dec, [_desc(odd, BR[0], stride=32)], pool, 3)
    _accepted(dec, [_desc(odd, BR[0], stride=32)], pool, 4)
    # ... an odd stride, an odd offset
    pool, _ = _pool(good)
    _refused(dec, [_desc(good, BR[0], stride=33)], pool, 3)
    _refused(dec, [_desc(good, BR[0], plane_off=1)], pool, 3)
    # routes 3 and 4: M_b = 16 (+-32767), a two-pass block, another step; routes 1 and 2 take them
    v = rng.integers(-32767, 32768, (32, 32))
    v[0, 0] = 32767
    wide16 = rc.Block((32, 32), "top", v, 1)
    assert wide16.M_b == 16 and wide16.ret == 1
    two = rc.Block((32, 32), "dense", rng.integers(-200, 201, (32, 32)), 2)
    assert two.ret == 1 and two.M_b <= 15
    for blk, br in ((wide16, BR[0]), (two, BR[0]), (good, BR[1])):
        pool, _ = _pool(blk)
        for route in (3, 4):
            _refused(dec, [_desc(blk, br)], pool, route)
        for route in (1, 2):
            _accepted(dec, [_desc(blk, br)], pool, route)
    # ... and one such block among good ones
    pool, offs = _pool(good, two)
    for route in (3, 4):
        _refused(dec, [_desc(good, BR[0]), _desc(two, BR[0], data_off=offs[1], plane_off=1024)], pool, route)
    # route 2: two transforms, a block of 65 columns, a ROI shift, a refining block of 65 rows; route 1 takes them
    w65 = B[(65, 7), "dense", "c"]
    tall = rc.Block((32, 65), "dense", rng.integers(-200, 201, (65, 32)), 2)
    assert tall.ret == 1
    pool, offs = _pool(good, w65, tall)
    cases = [[_desc(good, BR[0]), _desc(good, BR[2], plane_off=1024)],
             [_desc(good, BR[0]), _desc(w65, BR[0], data_off=offs[1], plane_off=1024)],
             [_desc(good, BR[0]), _desc(good, BR[0], plane_off=1024, roi_shift=3)],
             [_desc(good, BR[0]), _desc(tall, BR[0], data_off=offs[2], plane_off=1024)]]
    for descs in cases:
        _refused(dec, descs, pool, 2)
        _ht_blocks(dec, descs, pool, 8192, route=1)            # (a shifted block decodes to whatever it does: not compared here)
    # a cleanup-only block of 65 rows beside a refining one of 64: taken
    low = rc.Block((32, 64), "dense", rng.integers(-200, 201, (64, 32)), 3)
    t65 = B[(32, 65), "dense", "c"]
    pool, offs = _pool(low, t65)
    _accepted(dec, [_desc(low, BR[0]), _desc(t65, BR[0], data_off=offs[1], plane_off=2048)], pool, 2)
    # the raw entry on the 16-bit routes
    descs, rpool, _, soff = raw
    for route in (3, 4):
        _refused(dec, [descs[0]], rpool, route, raw=True, nsamples=soff)
    # more than 4096 samples: every route
    for shape in rc.OVERSIZE:
        big = B[shape, "dense", "1"]
        pool, _ = _pool(big)
        for route in range(5):
            _refused(dec, [_desc(big, BR[0])], pool, route, nsamples=16384)
    # the knob itself
    with pytest.raises(m.Htj2kError) as err:
        dec.set_int("unit_ht", 5)
    assert err.value.code == EINVAL
    _accepted(dec, [_desc(good, BR[0])], _pool(good)[0], 0)
