"""The IDWT launch plan of a job (build_descriptors and pk16_eligibility in htj2k_device.hip: the plain level tables, the
fusable groups, the fused launches per (components, store kind), the three-level and two-level launches, the packed
arithmetic) pinned launch for launch.  The other tests assert counts and inequalities of a job's launches; here every
case has the exact list: the algorithmic and the least-HBM bytes of every launch of the run, with coef16, ll16 and
idwt_packed, at the default knobs, with the pack stage not fused and with the two-level launch taken wherever the job allows
it -- and the frames are the oracle's.

Every case is the smallest shape at which its branch of the planner exists; test_case_geometry asserts on the CPU, from the
oracle's tile-component table, that it reaches that branch.

tests/golden/idwt_plan.json was written by write_golden() below, run on the commit BEFORE the planner was rewritten into
its named steps: it is what that code launched, never the output of the code under test.  To pin a deliberate change of the
plan, run write_golden() on the commit before it, look at the difference, and say in the commit what moved."""
import json
import os

import numpy as np
import pytest

import vecgen
from test_depths_gpu import store_kinds
from test_hetero_streams import _oracle_tilecomps

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "idwt_plan.json")
YUV420 = dict(dx=[1, 2, 2], dy=[1, 2, 2])

# name: (width, height, components, depth, frames of its job, encoder keywords, decoder knobs)
CASES = {
    "rgb_x3_x2": (256, 72, 3, 8, 2, dict(mct=1, nlevels=5), {}),             # x3 and x2 together, packed arithmetic
    "rgb_x2_level0": (16, 5, 3, 8, 3, dict(mct=1, nlevels=2), {}),            # x2 with the plain level at level 0
    "gray8": (64, 40, 1, 8, 2, dict(nlevels=3), {}),                          # one-component group, 8-bit plane store
    "gray16": (64, 40, 1, 16, 2, dict(nlevels=2), {}),                        # 16-bit plane store
    "rgb48_12": (64, 40, 3, 12, 2, dict(mct=1, nlevels=2), {}),               # rgb48 store
    "yuv420": (64, 48, 3, 8, 2, dict(nlevels=3, width=64, height=48, **YUV420), {}),   # three groups of two sizes in one launch
    "four": (32, 16, 4, 8, 2, dict(nlevels=2), {}),                           # four-component group, general store
    "rgb_w30": (30, 9, 3, 8, 2, dict(mct=1, nlevels=2), {}),                  # width no multiple of 4: general kernels
    "rgb97_float": (64, 40, 3, 8, 2, dict(mct=1, nlevels=3, transform=0, qstep=1.0), dict(bitexact=0)),
    "rgb97_fixed": (64, 40, 3, 8, 2, dict(mct=1, nlevels=3, transform=0, qstep=1.0), dict(bitexact=1)),
    "rgb_tiles": (128, 64, 3, 8, 2, dict(mct=1, nlevels=2, tile=(64, 32)), {}),   # several pack tiles per frame
    "line": (16, 1, 1, 8, 2, dict(nlevels=1), {}),                            # one-sample lines: not fusable, k_idwt_tile
    "empty_level": (2, 2, 1, 8, 2, dict(nlevels=3, offset=(1, 1)), {}),   # tile_ok false: generic path
}
# one frame of every case that decodes with bitexact 0, in the order of CASES: the empty level of the last one sends the whole
# job down the generic path; without it the job is every fused launch at once, several (components, store kind) per level
_BITEXACT0 = [n for n in CASES if not CASES[n][6].get("bitexact")]
MIXED = {"mixed": _BITEXACT0, "mixed_fusable": [n for n in _BITEXACT0 if n != "empty_level"]}
# (at its default the knob idwt_x2 leaves jobs this small their two launches: the third setting runs the two-level launch)
SETTINGS = {"default": {}, "unfused": dict(fuse_pack=0), "x2_always": dict(idwt_x2=1)}
DEFAULTS = dict(coef16=1, ll16=1, idwt_x3=1, idwt_x2=2, idwt_pk=1, fuse_pack=1, idwt_mode=3, bitexact=0)


def _encode(name, k):
    w, h, nc, depth, _, ekw, _ = CASES[name]
    sub = {key: ekw[key] for key in ("dx", "dy") if key in ekw}
    img = vecgen.synth_image(w, h, nc, depth=depth, seed=7 * sorted(CASES).index(name) + k + 1, noise=1 << (depth - 5), **sub)
    return vecgen.encode(img, depth=depth, **ekw)


_made = {}


def job_of(orc, name):
    """(codestreams, the oracle's planes of each, decoder knobs) of a case's job, made once"""
    if name not in _made:
        if name in MIXED:
            parts = [job_of(orc, n) for n in MIXED[name]]
            _made[name] = ([p[0][0] for p in parts], [p[1][0] for p in parts], {})
        else:
            pkts = [_encode(name, k) for k in range(CASES[name][4])]
            knobs = CASES[name][6]
            _made[name] = (pkts, [orc.decode(p, **knobs)[1] for p in pkts], knobs)
    return _made[name]


# ---------------------------------------------------------------- what the shapes are there for (CPU)
def _tilecomps(orc, name):
    data = job_of(orc, name)[0][0]
    r, tcs, info = _oracle_tilecomps(orc, data, want_info=True, **CASES[name][6])
    assert r >= 0, name
    return tcs, info


def _levels(tc):
    return [(int(tc["linelen"][lev][0]), int(tc["linelen"][lev][1]), int(tc["mod"][lev][0]), int(tc["mod"][lev][1]))
            for lev in range(int(tc["ndeclevels"]))]


def _fast(lh, lv, mh, mv):
    return not mh & 1 and lh % 4 == 0 and lh >= 8 and lv >= 2


def test_case_geometry(orc):
    fast, kinds, tcs_of = {}, {}, {}
    for name in CASES:
        tcs, info = _tilecomps(orc, name)
        tcs_of[name] = tcs
        assert all(t["coded"] for t in tcs), name
        fast[name] = all(_fast(*g) for t in tcs for g in _levels(t))
        kinds[name] = store_kinds(tcs, info, 8 if CASES[name][3] == 8 else 16)      # (gray16 and rgb48 frames are full-range)
    at_origin = lambda name: all(g[2:] == (0, 0) for t in tcs_of[name] for g in _levels(t))
    # x3: five levels, levels 0-2 plain for every plane; x2: one rgb24 launch over a plain level of fast geometry at the origin
    assert fast["rgb_x3_x2"] and at_origin("rgb_x3_x2") and kinds["rgb_x3_x2"] == {0} and len(_levels(tcs_of["rgb_x3_x2"][0])) == 5
    assert fast["rgb_x2_level0"] and at_origin("rgb_x2_level0") and kinds["rgb_x2_level0"] == {0}
    assert [g[:2] for g in _levels(tcs_of["rgb_x2_level0"][0])] == [(8, 3), (16, 5)]       # the plain level is level 0
    assert fast["gray8"] and kinds["gray8"] == {2} and len(tcs_of["gray8"]) == 1
    assert fast["gray16"] and kinds["gray16"] == {3}
    assert fast["rgb48_12"] and kinds["rgb48_12"] == {1}
    assert fast["yuv420"] and kinds["yuv420"] == {2}
    assert [(int(t["w"]), int(t["h"])) for t in tcs_of["yuv420"]] == [(64, 48), (32, 24), (32, 24)]
    assert fast["four"] and kinds["four"] == {-1} and len(tcs_of["four"]) == 4 and int(tcs_of["four"][0]["pix_step"]) == 4
    assert not fast["rgb_w30"] and kinds["rgb_w30"] == {-1} and 30 % 4                      # general kernels, no 16-bit sub-bands
    assert fast["rgb97_float"] and {int(t["transform"]) for t in tcs_of["rgb97_float"]} == {0} and kinds["rgb97_float"] == {0}
    assert fast["rgb97_fixed"] and {int(t["transform"]) for t in tcs_of["rgb97_fixed"]} == {2} and kinds["rgb97_fixed"] == {0}
    assert len(tcs_of["rgb_tiles"]) == 4 * 3 and fast["rgb_tiles"] and kinds["rgb_tiles"] == {0}
    assert _levels(tcs_of["line"][0]) == [(16, 1, 0, 0)] and kinds["line"] == {None}         # one-sample columns: not fusable
    # [1, 3) halves to [1, 2) and to [1, 1): the lowest level is empty, the planes of a tile launch would fall out of step
    assert [g[:2] for g in _levels(tcs_of["empty_level"][0])] == [(0, 0), (1, 1), (2, 2)]


# ---------------------------------------------------------------- the launches of a run
def run_job(dec, pkts):
    """-> (frames, signature, the figures step by step that only the comparison against another build reads)"""
    job = dec.job().parse_batch(pkts).upload().run().wait()
    frames = [job.download_frame(f)[1] for f in range(len(pkts))]
    sig = dict(alg_bytes=[by for ms, by in job.idwt_launches()], hbm_bytes=job.idwt_hbm_bytes(),
               coef16=int(job.coef16()), ll16=job.ll16(), idwt_packed=job.idwt_packed())
    extra = dict(framecrc=[d for d in job.framecrc()], ht_blocks_per_wave=job.ht_blocks_per_wave(), block_errors=job.block_errors())
    job.free()
    return frames, sig, extra


def set_knobs(dec, knobs):
    for knob, value in DEFAULTS.items():
        dec.set_int(knob, knobs.get(knob, value))


def plan_report(dec, orc, settings, log=None):
    """{case: {setting: (signature, extra)}} of every case and the mixed jobs under every one of `settings` (name: knobs); every
    frame is compared with the oracle's on the way"""
    out = {}
    try:
        for name in list(CASES) + list(MIXED):
            pkts, want, knobs = job_of(orc, name)
            out[name] = {}
            for sname, s in settings.items():
                set_knobs(dec, dict(knobs, **s))
                frames, sig, extra = run_job(dec, pkts)
                for f, (planes, planes_o) in enumerate(zip(frames, want)):
                    assert len(planes) == len(planes_o) and all(np.array_equal(a, b) for a, b in zip(planes, planes_o)), (name, sname, f)
                assert extra["block_errors"] == 0, (name, sname)
                out[name][sname] = (sig, extra)
                if log:
                    log("%s %s %s %s" % (name, sname, json.dumps(sig, sort_keys=True), json.dumps(extra, sort_keys=True)))
    finally:
        set_knobs(dec, {})
    return out


def write_golden(dec, orc, path=GOLDEN):
    """the file this module tests against; see the module's docstring for the commit it is to be run on"""
    rep = plan_report(dec, orc, SETTINGS)
    with open(path, "w") as f:
        json.dump({name: {s: sig for s, (sig, extra) in by.items()} for name, by in rep.items()}, f, indent=1, sort_keys=True)
        f.write("\n")


@pytest.fixture(scope="module")
def dec():
    import ffmpeg_ht_amd as m
    d = m.Decoder()
    assert d.device_name().startswith("gfx950"), d.device_name()
    yield d
    d.close()


@pytest.mark.gpu
@pytest.mark.parametrize("name", list(CASES) + list(MIXED))
def test_launches_are_the_pinned_ones(dec, orc, name):
    """the frames are the oracle's, and the run launched what the golden file lists: the byte figures are sums of integers far
    below 2^53, so equality is exact"""
    with open(GOLDEN) as f:
        golden = json.load(f)[name]
    pkts, want, knobs = job_of(orc, name)
    try:
        for sname, s in SETTINGS.items():
            set_knobs(dec, dict(knobs, **s))
            frames, sig, extra = run_job(dec, pkts)
            print(name, sname, sig)
            assert extra["block_errors"] == 0, (name, sname)
            for f, (planes, planes_o) in enumerate(zip(frames, want)):
                assert len(planes) == len(planes_o) and all(np.array_equal(a, b) for a, b in zip(planes, planes_o)), (name, sname, f)
            assert sig == golden[sname], (name, sname)
    finally:
        set_knobs(dec, {})
