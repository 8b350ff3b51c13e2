"""The unit tables of tests/ht_route_cases.py on the CPU: every block against the oracle, every table against the
conditions of the route it was built for (restated in ht_route_cases.admits from the knob's description in
include/htj2k_amd.h), so that a table built wrong fails here and not as a refusal on the GPU."""
import numpy as np

import ht_route_cases as rc
import oracle
import roi_cases


def test_every_block_decodes_and_the_lossless_ones_give_the_source_back():
    B = rc.blocks()
    for shape in rc.NARROW + rc.MID + rc.WIDE:
        for cls in rc.classes_of(shape):
            assert (shape, cls, "c") in B and ((shape, cls, "r") in B) == (cls != "top16"), (shape, cls)
    for shape in rc.OVERSIZE:                               # the oracle takes them; no kernel is given one
        assert shape[0] * shape[1] > 4096 and all((shape, "dense", k) in B for k in "123")
    for key, b in B.items():
        assert b.ret == 1, key
        p = 1 if b.passes > 1 else 0
        assert b.M_b >= max(b.max_U + p, 1) == b.least and b.M_b <= 30, key
        assert b.zbp >= 0 and b.P0 + b.zbp == b.M_b - 1 - p and b.npasses == b.passes + 3 * b.P0, key
        if b.vals is not None:                              # one or three passes and step 1: lossless
            got = roi_cases.dequant(b.t1, b.M_b, rc.BR53).view(np.int32)
            assert np.array_equal(got, b.vals), key
        # a placeholder set moves nothing: the same words as the block without it
        if b.P0:
            ret, t1 = oracle.ht_decode_block(b.data, b.lcup, b.lref, b.passes, b.zbp + b.P0, b.w, b.h, b.M_b, vsc=b.causal)
            assert ret == 1 and np.array_equal(t1, b.t1), key


def test_the_pool_holds_what_the_tables_are_meant_to_mix():
    B = [b for k, b in rc.blocks().items() if k[0] not in rc.OVERSIZE]
    for passes in (1, 2, 3):
        assert {0, 1, 2} <= {b.P0 for b in B if b.passes == passes}, passes
        assert {0, 1, 2, 3} <= {b.M_b - b.least for b in B if b.passes == passes and b.cls in ("ones", "threes", "dense")}, passes
    assert any(b.zbp == 0 for b in B) and any(b.causal for b in B)
    top16 = [b for b in B if b.cls == "top16"]
    assert top16 and all(b.max_U == 15 and b.M_b == 15 and b.passes == 1 for b in top16)
    top32 = [b for b in B if b.cls == "top32"]
    # (with SigProp / MagRef passes the cleanup pass codes one plane less: max_U = 28, and p = 1 makes M_b 29 again)
    assert {b.M_b for b in top32 if b.passes == 1} == {29, 30} == {b.M_b for b in top32 if b.passes > 1}
    assert all(b.max_U == (29 if b.passes == 1 else 28) for b in top32)


def test_the_rejected_blocks_are_the_three_constructions():
    E = rc.broken_blocks()
    assert [b.bad for b in E] == ["lcup", "scup", "maxbp"]
    assert all(b.ret < 0 for b in E)
    assert E[0].lcup < 2 and E[1].pcup == 0 and E[2].P0 + E[2].zbp + 1 < E[2].max_U


def _check_layout(t):
    """windows inside the buffer, disjoint, and room around them that must come back untouched"""
    n = 2 * t.nsamples if t.sixteen else t.nsamples
    used = np.zeros(n, dtype=np.int32)
    for e in t.entries:
        b = e.block
        assert e.stride >= b.w and e.plane_off + (b.h - 1) * e.stride + b.w <= t.nsamples, t.name
        idx = (e.plane_off + np.arange(b.h)[:, None] * e.stride + np.arange(b.w)[None, :]).ravel()
        used[idx] += 1
    assert used.max() == 1 and (used == 0).sum() >= 8, t.name
    exp = t.expected()
    fill = t.fill.view(np.int16) if t.sixteen else t.fill
    assert exp.shape == fill.shape and np.array_equal(exp[used == 0], fill[used == 0]), t.name


def test_every_table_meets_the_conditions_of_its_route():
    tables = rc.all_tables()
    assert len({t.name for t in tables}) == len(tables)
    for names, fn in ((rc.NAMES_ROUTE1, rc.route1_tables), (rc.NAMES_ROUTE2, rc.route2_tables), (rc.NAMES_ROUTE34, rc.route34_tables),
                      (rc.NAMES_BROKEN, rc.broken_tables)):
        assert names == [t.name for t in fn()]
    for t in tables:
        ok, nb = rc.admits(t.route, t.entries)
        assert ok, t.name
        if t.route == 2:
            assert nb == t.nb, t.name
            assert t.refine == any(e.block.passes > 1 for e in t.entries), t.name
        if t.route in (2, 3, 4):
            assert all(e.block.w <= 64 for e in t.entries), t.name
        _check_layout(t)
        if len(t.entries) > 20:                              # M_b at both ends of what the route takes, zbp 0 beside larger ones
            coded = [e.block for e in t.entries if e.block.npasses]
            assert (min(b.M_b for b in coded), max(b.M_b for b in coded)) == (1, 15 if t.sixteen else 30), t.name
            assert {0, 1, 2} <= {b.zbp for b in coded} and max(b.zbp for b in coded) >= 13, t.name
        strides = [e.stride - e.block.w for e in t.entries]
        if len(t.entries) > 1:
            assert any(strides) and not all(strides), t.name
            assert t.route == 3 or any(e.plane_off % 2 for e in t.entries), t.name
            assert any(e.block.npasses == 0 for e in t.entries) or "broken" in t.name, t.name


def test_the_tables_cover_what_they_are_for():
    r1, r2, r34, br = rc.route1_tables(), rc.route2_tables(), rc.route34_tables(), rc.broken_tables()
    # route 1: every shape in every class, cleanup-only and refined; a table for each front end
    keys = {(e.block.shape, e.block.cls, "r" if e.block.passes > 1 else "c") for e in r1[0].entries if e.block.npasses}
    assert keys == {k for k in rc.blocks() if k[0] not in rc.OVERSIZE}
    assert max(e.block.w for e in r1[0].entries) > 64 >= max(e.block.w for e in r1[1].entries) > 32 >= max(e.block.w for e in r1[2].entries)
    # route 2: each dequantiser x REFINE x blocks per wave; every shape of at most 64 columns in the three plain classes
    # in the tables of two per wave, the largest values in tables of small blocks
    combos = {(t.entries[0].branch, t.refine, t.nb) for t in r2 if len(t.entries) > 1}
    assert combos == {(br_, rf, nb) for br_ in roi_cases.BRANCHES for rf in (False, True) for nb in (4, 2)}
    for t in r2:
        if len(t.entries) == 1:
            continue
        have = {(e.block.shape, e.block.cls) for e in t.entries if e.block.passes == 1}
        if t.nb == 2:
            assert have >= {(s, c) for s in rc.NARROW + rc.MID for c in rc.classes_of(s) if c in ("ones", "threes", "dense")}, t.name
            assert any(32 < e.block.w <= 64 for e in t.entries), t.name
        assert {c for _, c in have} == set(rc.C32), t.name
        hs = {e.block.h for e in t.entries if e.block.npasses}
        assert hs >= {65, 129, 130, 1024}, t.name                        # past the 64-row window, beside blocks inside it
        if t.refine:
            assert {2, 3} <= {e.block.passes for e in t.entries}, t.name
            assert 32 < max(e.block.h for e in t.entries if e.block.passes > 1) <= 64, t.name
    assert {len(t.entries) % 4 for t in r2 if len(t.entries) > 1} == {0, 1, 2, 3}
    assert any(len(t.entries) == 1 for t in r2)
    # routes 3 and 4: every admissible shape in every class, the largest 16-bit value among them
    for t in r34:
        if len(t.entries) == 1:
            continue
        shapes = [s for s in rc.NARROW + rc.MID if t.route == 4 or s[0] % 2 == 0]
        have = {(e.block.shape, e.block.cls) for e in t.entries if e.block.npasses}
        assert have == {(s, c) for s in shapes for c in rc.classes_of(s) if c in rc.C16}, t.name
        assert max(e.block.M_b for e in t.entries if e.block.npasses) == 15, t.name
        assert len(t.entries) % 4 in (1, 3) and len(t.entries) % 2 == 1, t.name
    assert sorted(len(t.entries) == 1 for t in r34) == [False, False, True, True]
    # rejected blocks: every construction on every route, in waves with blocks that decode
    assert {(t.route, t.nb) for t in br} == {(2, 4), (2, 2), (3, 2), (4, 1)}
    for t in br:
        bad = t.bad_status()
        assert {e.block.bad for e in t.entries if e.block.bad} == {"lcup", "scup", "maxbp"}, t.name
        assert [e.block.bad is not None for e in t.entries] == list(bad), t.name
        if t.nb > 1:                                                     # per construction a wave that also holds a good block
            waves = [t.entries[g:g + t.nb] for g in range(0, len(bad), t.nb)]
            for how in ("lcup", "scup", "maxbp"):
                assert any(any(e.block.bad == how for e in wv) and any(e.block.bad is None for e in wv) for wv in waves), (t.name, how)


def test_the_lds_cap_is_computed():
    """four resp. two blocks with the table's longest MagSgn segment stay within the default of HTJ2K_MULTI_LDS, and the
    largest values are there all the same"""
    assert rc.multi_lds(4, rc.max_pcup_that_fits(4)) <= rc.MULTI_LDS_MAX < rc.multi_lds(4, rc.max_pcup_that_fits(4) + 4)
    for t in rc.route2_tables() + [t for t in rc.broken_tables() if t.route == 2]:
        longest = max(e.block.pcup for e in t.entries)
        assert rc.multi_lds(t.nb, longest) <= rc.MULTI_LDS_MAX, t.name
        # ... and the table is not far below the cap either: its longest segment takes more than half of it
        if len(t.entries) > 20:
            assert rc.multi_lds(t.nb, longest) > rc.MULTI_LDS_MAX // 2, t.name
