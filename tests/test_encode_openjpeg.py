"""The host writer's streams decoded by OpenJPEG 2.5.4 (through Pillow): a decoder that was not written here reads what
htj2k_enc_assemble_planes writes -- blocks at plane 0, blocks coded from a higher bit-plane and signalled through their
zero-bit-plane count alone, blocks shifted to all zero, blocks left out by the allocation model -- and returns the
oracle's pixels: exactly for 5/3, within one LSB of the coded depth for 9/7 (the project's rule for two float
syntheses, tests/test_oracle_random_openjpeg.py).  A 5/3 stream with every plane 0 also returns the source.  What the
pixels of a stream with shifted blocks must be comes from the allocation model's reconstruction (rc_model.recon: the
kept planes and the half bit below them): OpenJPEG's 5/3 pixels equal it through the inverse transform exactly, and
the oracle's dequantised 9/7 coefficients, which OpenJPEG's pixels were just compared with, equal it within the 1 ULP
of the float path -- so a zero-bit-plane count that two decoders merely read alike is not enough.  CPU only.

Layouts: those Pillow hands back sample for sample (tests/enc_opj.py).  Subsampled layouts and multi-component layouts
deeper than 8 bits are left out: Pillow upsamples the former and narrows the latter to 8 bits."""
import numpy as np
import pytest

import enc97_model as e97
import enc_model as em
import enc_opj
import oracle
import ffmpeg_ht_amd as m
import rc_model as rc
import vecgen

SIZES = [((17, 9), 5, (4, 4)), ((1, 1), 0, (6, 6)), ((1, 255), 5, (2, 10)), ((255, 1), 3, (10, 2)),
         ((200, 136), 5, (6, 6)), ((64, 40), 0, (5, 5)), ((512, 384), 5, (6, 6))]
TRANSFORMS = [(False, 1.0), (True, 1 / 32), (True, 0.25), (True, 2.0)]
CASES = [(fmt, bits, i) for fmt, bits in enc_opj.LAYOUTS for i in range(len(SIZES))]


def synth(fmt, w, h, bits, seed=3):
    return [vecgen.synth_image(cw, ch, 1, depth=bits, seed=seed + c)[0] for c, (cw, ch) in enumerate(em.comp_dims(fmt, w, h))]


def plane_vectors(idx, blocks, wts, free, smallest, rng):
    """[(name, planes)]: all 0; seeded 0 .. k per block (k the bit length of its largest magnitude: some blocks become
    all zero); what the allocation model chooses for 50 % and 10 % of the free size (block bytes: the share of the
    whole stream less the smallest stream's headers and empty packets)"""
    out = [("zero", [0] * len(blocks))]
    ks = [int(np.abs(rc.block_view(idx, b).astype(np.int64)).max()).bit_length() for b in blocks]
    out.append(("random", [int(rng.integers(0, k + 1)) for k in ks]))
    lens, dists = rc.tables(idx, blocks, wts)
    for share in (0.5, 0.1):
        room = max(0, int(free * share) - smallest)
        out.append(("model %d%%" % round(share * 100), rc.planes_of(rc.allocate(lens, dists, room), lens)))
    return out


def ulp_diff(a, b):
    """largest distance of two float32 arrays in units in the last place (as tests/test_gpu_parity.py counts them)"""
    ai, bi = (x.view(np.int32).astype(np.int64) for x in (np.ascontiguousarray(a, np.float32), np.ascontiguousarray(b, np.float32)))
    ai = np.where(ai < 0, -(ai & 0x7FFFFFFF), ai)
    bi = np.where(bi < 0, -(bi & 0x7FFFFFFF), bi)
    return int(np.abs(ai - bi).max()) if ai.size else 0


def model_pixels_53(idx, blocks, planes, fmt, bits, levels, mct, w, h):
    """5/3: the model's reconstruction of every block through the inverse transform, inverse RCT, level shift and clip"""
    rec = [np.zeros(x.shape, np.int64) for x in idx]
    for b, p in zip(blocks, planes):
        if p >= 0:
            rec[b["comp"]][b["y"]:b["y"] + b["h"], b["x"]:b["x"] + b["w"]] = rc.recon(rc.block_view(idx, b), p)
    out = [oracle.idwt(r.astype(np.int32), ((0, r.shape[1]), (0, r.shape[0])), levels, 1) for r in rec]
    if mct:
        out[:3] = oracle.mct(1, *out[:3])
    px = [np.clip(x.astype(np.int64) + (1 << (bits - 1)), 0, (1 << bits) - 1) for x in out]
    return enc_opj.arrange(em.to_planes(px, fmt, bits), fmt, w, h)


def model_coefficients_97(idx, blocks, planes, coded, guard, qstep, bits, levels):
    """9/7: what the dequantiser must hand to the inverse transform: twice the reconstruction (the kept planes and the
    half bit below them) aligned to bit 31 - M_b, times step / 2^(31 - M_b) in float32 (tests/test_encode_rc_host.py)"""
    st = e97.steps(qstep, bits, levels)
    rec = [np.zeros(x.shape, np.float32) for x in idx]
    for b, p, c in zip(blocks, planes, coded):
        if not c[0]:
            continue
        Mb = b["expn"] + guard - 1
        v = rc.block_view(idx, b).astype(np.int64)
        mag = (np.abs(v) >> p) << p
        val = np.sign(v) * np.where(mag > 0, (2 * mag + (1 << p)) << (30 - Mb), 0)
        scale = np.float32(st[rc.band_entry(b)][2]) / np.float32(1 << (31 - Mb))
        rec[b["comp"]][b["y"]:b["y"] + b["h"], b["x"]:b["x"] + b["w"]] = val.astype(np.float32) * scale
    return rec


@pytest.mark.skipif(not enc_opj.HAVE_OPJ, reason="Pillow/OpenJPEG not importable")
@pytest.mark.parametrize("fmt,bits,size", CASES, ids=["%s-%d-%dx%d" % (f, b, *SIZES[i][0]) for f, b, i in CASES])
def test_openjpeg_decodes_the_host_writers_streams(orc, fmt, bits, size):
    (w, h), levels, cb = SIZES[size]
    rng = np.random.default_rng(1000 * size + bits)
    mct = em.mct_default(fmt)
    comps = synth(fmt, w, h, bits)
    source = em.to_planes(comps, fmt, bits)
    shifted = 0
    for irreversible, qstep in TRANSFORMS:
        opts = dict(levels=levels, cb=cb, irreversible=irreversible, qstep=qstep)
        blocks = m.Encoder.layout(w, h, fmt, bits, **opts)
        idx = rc.indices(comps, fmt, bits, levels, mct, irreversible, qstep)
        wts = rc.weights(fmt, w, h, bits, levels, mct, irreversible, qstep)
        full = [rc.code_block(rc.block_view(idx, b), 0) for b in blocks]
        free = len(m.Encoder.assemble(w, h, fmt, bits, [c[0] for c in full], max_u=[c[2] for c in full], **opts))
        smallest = len(m.Encoder.assemble(w, h, fmt, bits, [b""] * len(blocks), **opts))
        for name, planes in plane_vectors(idx, blocks, wts, free, smallest, rng):
            coded = [rc.code_block(rc.block_view(idx, b), p) for b, p in zip(blocks, planes)]
            cs = m.Encoder.assemble(w, h, fmt, bits, [c[0] for c in coded], max_u=[c[2] for c in coded], planes=planes, **opts)
            what = (fmt, bits, w, h, "9/7 %g" % qstep if irreversible else "5/3", name)
            _, want, _ = orc.decode(cs, req_pix_fmt=em.pix(fmt))
            assert orc.block_errors() == 0, what
            lossless = not irreversible and name == "zero"
            bad = enc_opj.compare(cs, fmt, bits, w, h, want, irreversible, source if lossless else None)
            assert bad is None, (what, bad)
            if irreversible:
                orc.decode_blocks(cs, req_pix_fmt=em.pix(fmt))
                model = model_coefficients_97(idx, blocks, planes, coded, em.qcd_guard_bits(cs), qstep, bits, levels)
                for tc, r in enumerate(model):
                    assert ulp_diff(orc.plane(tc), r) <= 1, (what, tc)
            else:
                model = model_pixels_53(idx, blocks, planes, fmt, bits, levels, mct, w, h)
                assert np.array_equal(enc_opj.pixels(cs, fmt), model), what
            shifted += sum(1 for c, p in zip(coded, planes) if c[0] and p > 0)
    # the case means something: blocks that are coded from a higher plane went through OpenJPEG (a 1 x 1 frame of one
    # sample per component may have none)
    assert shifted > 0 or w * h == 1, (fmt, bits, w, h)
