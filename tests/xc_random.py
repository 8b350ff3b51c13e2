"""Seeded random sources for the transcoder (tests/test_transcode_random_host.py on the CPU,
tools/gpu_transcode_random.py on the GPU): draw(rng) gives the vector factory's keywords of a source, its kind and its
content; make(d) the codestream; predicted(d, ...) the verdict htj2k_transcode_check must give it.  numpy and the vector
factory only, no GPU.  Test tooling only.

A draw: a layout of tests/test_encode_gpu.py's FORMATS; 1 .. 300 by 1 .. 200, in one draw of ten 1 .. 3 one way; Part-1, HT
or MIXED 2 : 1 : 1; 0 .. 6 levels; every legal block shape; 5/3, or 9/7 at a log-uniform step; the Part-1 mode switches,
HT passes, placeholder sets and VSC; dropped passes; every progression; precincts no smaller than the blocks; layers;
SOP + EPH; tiles; guard bits; noise or a synthetic picture per component; for Part-1 in one of two a container variant of
tests/cs_rewrite.py (the draw then carries SOP + EPH, which the rewriter needs); in one of three a budget share.  One
draw in eight is put out of scope on purpose (OUT_CLASSES)."""
import numpy as np

import cs_rewrite
import enc_model as em
import enc_tiles_model as tm
import ffmpeg_ht_amd as m
import vecgen
from test_encode_gpu import FORMATS
from xc_source import Source, block_rects, enc_opts

PATCHWELCOME = -0x45574150
STYLES = [0, 0, 1, 2, 4, 8, 0x20, 5, 0x0A, 0x2F]
IN_VARIANTS = ["same", "plt", "tp3_tlm_plt", "tp_each_packet", "tp3_interleaved", "ppm", "ppt", "ppt_tp3", "coc_qcc_main",
               "poc_split", "poc_layers"]
OUT_VARIANTS = ["coc_qcc_tile", "rgn_main", "rgn_tile"]
# (ppm_tp3 is left out: the reference's parser, and so the oracle, reads a PPM stream cut into several tile-parts as
# another picture -- DESIGN.md section 5, "Random sources through the transcoder")
OUT_CLASSES = ["origin", "rgn", "signed", "comp_levels", "comp_guard", "depths", "precincts", "no_opt_in", "reduce", "variant"]
WORDS = {"origin": "origin", "rgn": "region of interest", "signed": "is signed", "comp_levels": "differs in levels",
         "comp_guard": "differs in depth or guard bits", "depths": "differs in depth or guard bits",
         "precincts": "precincts cut", "no_opt_in": "HT code-blocks already", "reduce": "reduction factor",
         "coc_qcc_tile": "coding parameters of its own", "rgn_main": "region of interest",
         "rgn_tile": "tile 0 has "}            # (an RGN in a tile-part header: "coding parameters of its own" or "a region of interest")
MAX_TILES = 400                                            # the CPU rebuild takes its time per tile


def _tile(rng, fmt, w, h):
    """8 .. 300 each way, log-uniform, drawn again where the encoder refuses the grid (an empty tile-component) or the
    picture would have more than MAX_TILES tiles"""
    while True:
        tile = (int(2.0 ** rng.uniform(3, np.log2(300))), int(2.0 ** rng.uniform(3, np.log2(300))))
        if not tm.refused(fmt, w, h, tile) and len(tm.grid(w, h, tile)) <= MAX_TILES:
            return tile


def _content(rng, dims, depths, signed):
    out = []
    for (cw, ch), depth in zip(dims, depths):
        if rng.random() < 0.3:
            c = rng.integers(0, 1 << depth, size=(ch, cw)).astype(np.int32)
        else:
            c = vecgen.synth_image(cw, ch, 1, depth=depth, seed=int(rng.integers(0, 1000)))[0]
        out.append(c - (1 << (depth - 1)) if signed else c)
    return out


def draw(rng):
    """-> dict: fmt, bits, w, h, kind ("p1" | "ht" | "mixed"), kw (vecgen.encode's keywords), comps (the content),
    variant (a name of cs_rewrite.variants or None), share (a budget share or None), out (None or one of OUT_CLASSES)"""
    fmt, bits = FORMATS[int(rng.integers(0, len(FORMATS)))]
    nc = em.layout(fmt)[0]
    w, h = int(rng.integers(1, 301)), int(rng.integers(1, 201))
    if rng.random() < 0.1:
        if rng.random() < 0.5:
            w = int(rng.integers(1, 4))
        else:
            h = int(rng.integers(1, 4))
    kind = ["p1", "p1", "ht", "mixed"][int(rng.integers(0, 4))]
    levels = int(rng.integers(0, 7))
    cbw = int(rng.integers(2, 11))
    cb = (cbw, int(rng.integers(2, min(10, 12 - cbw) + 1)))
    irrev = bool(rng.random() < 0.5)
    qstep = float(2.0 ** rng.uniform(-5, 2))
    mct = int(fmt in em.RGB and rng.random() < 0.6)
    style = STYLES[int(rng.integers(0, len(STYLES)))]
    passes, vsc = int(rng.integers(1, 4)), bool(rng.random() < 0.3)
    plhd = int(rng.integers(1, 3)) if rng.random() < 0.2 else 0
    drop = int(rng.integers(1, 6)) if rng.random() < 0.4 else 0
    prog = int(rng.integers(0, 5))
    prec = None
    if rng.random() < 0.3:
        prec = [(int(rng.integers(cb[0] + 1, 16)), int(rng.integers(cb[1] + 1, 16))) for _ in range(int(rng.integers(1, 3)))]
    layers, layer_seed = (int(rng.integers(2, 7)), int(rng.integers(0, 1000))) if rng.random() < 0.4 else (1, 0)
    marks = bool(rng.random() < 0.5)
    tile = _tile(rng, fmt, w, h) if rng.random() < 0.3 else (0, 0)
    guard = int(rng.integers(1, 6)) if rng.random() < 0.3 else 0
    variant = IN_VARIANTS[int(rng.integers(0, len(IN_VARIANTS)))] if rng.random() < 0.5 else None
    share = float(rng.uniform(0.1, 0.9)) if rng.random() < 1 / 3 else None
    out = OUT_CLASSES[int(rng.integers(0, len(OUT_CLASSES)))] if rng.random() < 1 / 8 else None

    args = em.vecgen_args(fmt, w, h, bits, levels, cb, mct, guard)
    kw = dict(depth=bits, dx=args["dx"], dy=args["dy"], width=w, height=h, nlevels=levels, cb=cb, transform=0 if irrev else 1,
              mct=mct, prog=prog, tile=tile, guard_bits=guard)
    if irrev:
        kw["qstep"] = qstep
    depths, signed = [bits] * nc, False

    # ---- out of scope on purpose: the class may change the draw's kind, and falls on another where it cannot apply
    if out in ("comp_levels", "comp_guard", "depths") and nc == 1:
        out = "signed"
    if out == "rgn" and bits > 8:                          # the factory's Maxshift needs M_b + shift <= 30
        out = "variant"
    if out == "variant":
        kind, variant = "p1", OUT_VARIANTS[int(rng.integers(0, len(OUT_VARIANTS)))]
        if variant == "coc_qcc_tile" and nc == 1:
            variant = "rgn_tile"
    elif out is not None:
        variant = None
    if out == "no_opt_in" and kind == "p1":
        kind = "ht" if rng.random() < 0.5 else "mixed"
    if out == "origin":
        off = (4 * int(rng.integers(0, 4)), 4 * int(rng.integers(0, 4)))           # multiples of every sub-sampling factor
        off = off if any(off) else (4, 0)
        kw["offset"] = off
        kw["tile_offset"] = off if tile != (0, 0) or rng.random() < 0.5 else (0, 0)
    elif out == "rgn":
        kind, irrev = "p1", False
        kw.update(transform=1, guard_bits=0)
        kw.pop("qstep", None)
        # (on component 0: the reference counts every component's bit-planes with component 0's shift, DESIGN.md section 5
        # "Region of interest", so a shift on another component alone gives a stream no decoder here reads)
        kw["roi_shift"] = [12] + [0] * (nc - 1)
    elif out == "signed":
        signed = True
        kw["sgnd"] = True
    elif out in ("comp_levels", "comp_guard"):
        # (an override equal to the common value leaves the draw in scope: predicted() looks at the values)
        c = int(rng.integers(1, nc))
        kw["mct"] = 0
        if out == "comp_guard":
            kw["guard_bits"] = guard or int(rng.integers(1, 6))
        kw["comp"] = [None] * c + [{"nlevels": int(rng.integers(0, 7))} if out == "comp_levels" else {"guard_bits": int(rng.integers(1, 6))}]
    elif out == "depths":
        c = int(rng.integers(1, nc))
        depths[c] = bits - 1 if bits > 5 else bits + 1
        kw.update(mct=0, depth=depths)
    elif out == "precincts":
        prec = [(int(rng.integers(1, cb[0] + 1)), int(rng.integers(1, cb[1] + 1)))]

    # ---- what the kind and the variant ask of the rest
    if kind == "p1":
        kw.update(part1=True, cblk_style=style, drop_passes=drop)
        if variant is not None:
            marks = True                                   # the rewriter finds the packets by their SOP and EPH markers
            if variant == "coc_qcc_main" and nc == 1:
                variant = "same"
            if variant == "poc_split":                     # two volumes in the COD's own order: LRCP or RLCP, one layer, two levels
                prog, layers, layer_seed = prog % 2, 1, 0
                kw.update(prog=prog, nlevels=max(levels, 2))
            if variant == "poc_layers":                    # LRCP with layers
                layers = max(layers, 2)
                kw.update(prog=0)
    else:
        variant = None
        if kind == "ht":
            kw.update(passes=passes, vsc=vsc)
            if passes == 1 and plhd:
                kw["placeholder_sets"] = plhd
        else:
            kw.update(mixed=True, vsc=vsc, drop_passes=drop)
    if prec:
        kw["prec"] = prec
    if layers > 1:
        kw.update(layers=layers, layer_seed=layer_seed)
    if marks:
        kw.update(sop=True, eph=True)
    comps = _content(rng, em.comp_dims(fmt, w, h), depths, signed)
    return dict(fmt=fmt, bits=bits, w=w, h=h, kind=kind, kw=kw, comps=comps, variant=variant, share=share, out=out)


def describe(d):
    """the draw without its content, for a log line"""
    return {k: v for k, v in d.items() if k != "comps"}


def make(d, rewritten=True):
    """-> the draw's codestream (RuntimeError where the vector factory refuses the configuration); rewritten=False: a
    draw with a variant as the factory wrote it"""
    cs = vecgen.encode(d["comps"], **d["kw"])
    if d["variant"] is None or not rewritten:
        return cs
    return dict(cs_rewrite.variants(cs, False))[d["variant"]]


def cuts_blocks(orc, d, src):
    """do the precincts of src cut its code-blocks?  The oracle's block rectangles against the encoder's layout"""
    opts = enc_opts(d["kw"])
    layout = m.Encoder.layout(d["w"], d["h"], d["fmt"], d["bits"], **opts)
    tiles = m.Encoder.tiles(d["w"], d["h"], d["fmt"], d["bits"], **opts)
    if len(orc.plan_blocks(src)) != len(layout):
        return True
    got = sorted((comp, x, y, int(e["w"]), int(e["h"])) for e, _, _, _, comp, x, y in block_rects(orc, src, tiles, em.layout(d["fmt"])[0]))
    return got != sorted((b["comp"], b["x"], b["y"], b["w"], b["h"]) for b in layout)


def predicted(d, ht_sources=True, reduced=False, orc=None, src=None):
    """-> (code, word of the log line) htj2k_transcode_check and the transcoder must answer the draw with, (0, None) for
    a draw in scope: from the effective parameters, in the order the product looks at them.  reduced: the decoder was
    opened with a reduction factor.  A draw of the class "precincts" needs the oracle and the stream"""
    kw, out = d["kw"], d["out"]
    if d["kind"] != "p1" and not ht_sources:
        return PATCHWELCOME, WORDS["no_opt_in"]
    if reduced:
        return PATCHWELCOME, WORDS["reduce"]
    if any(kw.get("offset", (0, 0))) or any(kw.get("tile_offset", (0, 0))):
        return PATCHWELCOME, WORDS["origin"]
    if kw.get("sgnd"):
        return PATCHWELCOME, WORDS["signed"]
    if any(kw.get("roi_shift", [0])) or d["variant"] == "rgn_main":
        return PATCHWELCOME, WORDS["rgn"]
    depth = kw["depth"] if isinstance(kw["depth"], list) else [kw["depth"]]
    if any(v != depth[0] for v in depth):
        return PATCHWELCOME, WORDS["depths"]
    for c in kw.get("comp") or []:
        if c and c.get("guard_bits", kw["guard_bits"]) != kw["guard_bits"]:
            return PATCHWELCOME, WORDS["comp_guard"]
        if c and c.get("nlevels", kw["nlevels"]) != kw["nlevels"]:
            return PATCHWELCOME, WORDS["comp_levels"]
    if d["variant"] in ("coc_qcc_tile", "rgn_tile"):
        return PATCHWELCOME, WORDS[d["variant"]]
    if out == "precincts" and cuts_blocks(orc, d, src):
        return PATCHWELCOME, WORDS["precincts"]
    return 0, None


def headroom(tab):
    """a Part-1 block with passes that fills every magnitude bit of its band: the rule has no HT block for it"""
    return any(e["flags"] & 4 and e["npasses"] and e["zbp"] >= e["M_b"] for e in tab)


def prepare(orc, d):
    """a draw as far as the reference goes -> dict: status "factory" (the vector factory refuses the configuration),
    "refused" (out of scope: code, word), "headroom" (left out: no HT block for one of its Part-1 blocks) or "ok"
    (in scope: s, the Source)"""
    try:
        src = make(d)
    except RuntimeError as e:
        return dict(status="factory", why=str(e))
    code, word = predicted(d, orc=orc, src=src)
    if code:
        return dict(status="refused", src=src, code=code, word=word)
    if headroom(orc.plan_blocks(src)):
        return dict(status="headroom", src=src)
    return dict(status="ok", src=src, s=Source(orc, src, d["kw"]))
