"""Catalogue of generated HTJ2K test streams shared by the CPU and GPU suites.
Each entry: name -> (callable returning the codestream bytes, decode kwargs)."""
import functools

import numpy as np

import vecgen


@functools.lru_cache(maxsize=None)
def _img(w, h, nc, depth=8, seed=1, noise=8, dx=None, dy=None):
    return vecgen.synth_image(w, h, nc, depth=depth, seed=seed, noise=noise,
                              dx=list(dx) if dx else None, dy=list(dy) if dy else None)


def _enc(img_args, **kw):
    return vecgen.encode(_img(*img_args), **kw)


CASES = {
    # --- reversible 5/3 ---
    "gray_l5_cb64":      (lambda: _enc((200, 150, 1, 8, 3)), {}),
    "gray_l5_cb32":      (lambda: _enc((200, 150, 1, 8, 3), cb=(5, 5)), {}),
    "gray_l3_cb16x64":   (lambda: _enc((200, 150, 1, 8, 3), cb=(4, 6), nlevels=3), {}),
    "gray_l3_cb256x16":  (lambda: _enc((300, 90, 1, 8, 13), cb=(8, 4), nlevels=3), {}),
    "gray_l2_cb4x1024":  (lambda: _enc((40, 1100, 1, 8, 14), cb=(2, 10), nlevels=2), {}),
    "gray_l0":           (lambda: _enc((200, 150, 1, 8, 3), nlevels=0), {}),
    "gray_offset":       (lambda: _enc((201, 149, 1, 8, 4), nlevels=2, offset=(3, 5)), {}),
    "gray_deep_levels":  (lambda: _enc((37, 23, 1, 8, 15), nlevels=8), {}),
    "rgb_mct":           (lambda: _enc((190, 131, 3, 8, 5), mct=1), {}),
    "rgb_nomct_rlcp":    (lambda: _enc((190, 131, 3, 8, 5), prog=1, nlevels=4), {}),
    "rgb_rpcl_prec":     (lambda: _enc((190, 131, 3, 8, 5), mct=1, prog=2, prec=[(7, 7), (6, 6)], nlevels=3), {}),
    "rgb_pcrl_prec":     (lambda: _enc((190, 131, 3, 8, 5), mct=1, prog=3, prec=[(7, 7), (6, 6)], nlevels=3), {}),
    "rgb_cprl_prec":     (lambda: _enc((190, 131, 3, 8, 5), mct=1, prog=4, prec=[(7, 7), (6, 6)], nlevels=3), {}),
    "rgb_tiles":         (lambda: _enc((190, 131, 3, 8, 5), mct=1, tile=(64, 64), nlevels=3), {}),
    "rgb_tiles_offsets": (lambda: _enc((190, 131, 3, 8, 6), mct=1, tile=(100, 70), nlevels=3, offset=(7, 9), tile_offset=(2, 3)), {}),
    "gray_sop_eph":      (lambda: _enc((200, 150, 1, 8, 3), sop=True, eph=True), {}),
    "gray12":            (lambda: _enc((160, 120, 1, 12, 7, 40), depth=12, nlevels=4), {}),
    "gray16":            (lambda: _enc((160, 120, 1, 16, 8, 400), depth=16, nlevels=4), {}),
    "rgb10_mct":         (lambda: _enc((160, 120, 3, 10, 8, 20), depth=10, nlevels=4, mct=1), {}),
    "rgba8":             (lambda: _enc((96, 80, 4, 8, 16), nlevels=3), {}),
    "yuv420p8":          (lambda: _enc((190, 130, 3, 8, 12, 8, (1, 2, 2), (1, 2, 2)), dx=[1, 2, 2], dy=[1, 2, 2], width=190, height=130), {}),
    "tiny_7x5":          (lambda: _enc((7, 5, 1, 8, 9), nlevels=1), {}),
    "tiny_1x1":          (lambda: vecgen.encode([np.array([[77]])], nlevels=0), {}),
    "tiny_3x1_l2":       (lambda: vecgen.encode([np.array([[77, 3, 250]])], nlevels=2), {}),
    "tiny_1x9_l3":       (lambda: vecgen.encode([np.arange(9).reshape(9, 1) * 20], nlevels=3), {}),
    "noise_max":         (lambda: vecgen.encode([np.random.default_rng(2).integers(0, 256, (130, 130))], nlevels=3), {}),
    "all_zero":          (lambda: vecgen.encode([np.full((100, 100), 128)], nlevels=3), {}),
    "one_sample_blocks": (lambda: vecgen.encode([np.where(np.add.outer(np.arange(128) % 64, np.arange(128) % 64) == 0, 200, 128)], nlevels=1), {}),
    "force_include":     (lambda: _enc((100, 100, 1, 8, 17), nlevels=3, force_include=True), {}),
    "psot_zero":         (lambda: _enc((100, 100, 1, 8, 17), nlevels=3, psot_zero=True), {}),
    "placeholder_1":     (lambda: _enc((200, 150, 1, 8, 3), placeholder_sets=1), {}),
    "placeholder_2_3p":  (lambda: _enc((200, 150, 1, 8, 3), placeholder_sets=2, passes=3), {}),
    "lowres_1":          (lambda: _enc((200, 150, 1, 8, 3)), {"reduction_factor": 1}),
    "lowres_3_rgb":      (lambda: _enc((190, 131, 3, 8, 5), mct=1), {"reduction_factor": 3}),
    # --- refinement passes ---
    "gray_3passes":      (lambda: _enc((200, 150, 1, 8, 3), passes=3), {}),
    "gray_2passes":      (lambda: _enc((200, 150, 1, 8, 3), passes=2), {}),
    "gray_3passes_vsc":  (lambda: _enc((200, 150, 1, 8, 3), passes=3, vsc=True), {}),
    "rgb_3passes_cb32":  (lambda: _enc((190, 131, 3, 8, 5), mct=1, passes=3, cb=(5, 5)), {}),
    # --- irreversible 9/7 (float path; bitexact=1 selects the fixed-point path) ---
    "gray_97_q2":        (lambda: _enc((200, 150, 1, 8, 3), transform=0, qstep=2), {}),
    "gray_97_fine":      (lambda: _enc((200, 150, 1, 8, 3), transform=0, qstep=1 / 32), {}),
    "rgb_97_ict":        (lambda: _enc((190, 131, 3, 8, 5), transform=0, mct=1, qstep=1), {}),
    "gray_97_3passes":   (lambda: _enc((200, 150, 1, 8, 3), passes=3, transform=0, qstep=2), {}),
    "yuv422p12_97":      (lambda: _enc((192, 128, 3, 12, 11, 30, (1, 2, 2), (1, 1, 1)), depth=12, dx=[1, 2, 2], dy=[1, 1, 1],
                                       transform=0, qstep=1, cb=(5, 5), width=192, height=128), {}),
    "gray_97_offset":    (lambda: _enc((201, 149, 1, 8, 4), nlevels=3, offset=(3, 5), transform=0, qstep=1), {}),
    "gray_97_bitexact":  (lambda: _enc((200, 150, 1, 8, 3), transform=0, qstep=2), {"bitexact": 1}),
    "rgb_97_bitexact":   (lambda: _enc((190, 131, 3, 8, 5), transform=0, mct=1, qstep=1), {"bitexact": 1}),
    # --- regressions found by tools/gpu_random_configs.py ---
    # 9/7 fixed point through the general path of the fused final level, last quadruple of a row partly outside the
    # line (width = 3 mod 4): a lane without output used to leave the lifting of its neighbour short of a DPP source
    "rgb_97_bitexact_w87": (lambda: _enc((87, 96, 3, 8, 365, 4), transform=0, qstep=4.0, mct=1, nlevels=2, cb=(6, 2)), {"bitexact": 1}),
    "rgb12_97_bitexact_w91": (lambda: _enc((91, 40, 3, 12, 366, 4), depth=12, transform=0, qstep=4.0, mct=1, nlevels=5, cb=(6, 2)), {"bitexact": 1}),
    # image offset + 4:2:0: the last chroma row of the picture is covered by no tile-component (jpeg2000dec.c:2312-2358)
    "yuv420_offset_uncovered_row": (lambda: _enc((377, 15, 3, 8, 169, 4, (1, 2, 2), (1, 2, 2)), nlevels=4, cb=(2, 6), offset=(2, 5), dx=[1, 2, 2], dy=[1, 2, 2], width=377, height=15), {}),
    # 42 tiles x 3 components = 126 tile-components per frame (a batch of three used to exceed a 250 limit)
    "yuv420_42_tiles":   (lambda: _enc((212, 168, 3, 8, 337, 4, (1, 2, 2), (1, 2, 2)), nlevels=2, cb=(6, 5), tile=(32, 32), prog=4, dx=[1, 2, 2], dy=[1, 2, 2], width=212, height=168), {}),
    # --- palettised JP2 (pclr + cmap boxes): pal8, the palette is AVFrame.data[1] (jpeg2000dec.c:2900-2901) ---
    "pal8_jp2":           (lambda: vecgen.jp2_wrap(vecgen.encode([(np.add.outer(np.arange(40), np.arange(56)) * 3 % 200).astype(np.int32)], nlevels=2),
                                                   56, 40, 1, 8, colourspace=16,
                                                   palette=[((i * 7) & 255, (255 - i) & 255, (i * 3 + 1) & 255) for i in range(200)]), {}),
    # --- Part-1 (MQ-coded) blocks: decode_cblk() instead of the HT decoder; style bits BYPASS 1, RESET 2,
    #     TERMALL 4, VSC 8, SEGSYM 0x20 ---
    "p1_gray":            (lambda: _enc((200, 150, 1, 8, 3), part1=True), {}),
    "p1_gray_cb32":       (lambda: _enc((200, 150, 1, 8, 3), part1=True, cb=(5, 5)), {}),
    "p1_gray_cb16x64":    (lambda: _enc((200, 150, 1, 8, 3), part1=True, cb=(4, 6), nlevels=3), {}),
    "p1_gray_cb64x4":     (lambda: _enc((200, 150, 1, 8, 3), part1=True, cb=(6, 2), nlevels=2), {}),
    "p1_gray_cb4x1024":   (lambda: _enc((40, 1100, 1, 8, 14), part1=True, cb=(2, 10), nlevels=2), {}),
    "p1_gray_cb128x32":   (lambda: _enc((300, 90, 1, 8, 13), part1=True, cb=(7, 5), nlevels=2), {}),
    "p1_cb256x16_modes":  (lambda: _enc((600, 70, 1, 12, 13, 60), depth=12, part1=True, cb=(8, 4), nlevels=1, cblk_style=0x29), {}),
    "p1_gray_cb1024x4":   (lambda: _enc((1100, 40, 1, 8, 14), part1=True, cb=(10, 2), nlevels=1), {}),
    "p1_bypass":          (lambda: _enc((200, 150, 1, 12, 3, 60), depth=12, part1=True, cblk_style=0x01), {}),
    "p1_reset":           (lambda: _enc((200, 150, 1, 8, 3), part1=True, cblk_style=0x02), {}),
    "p1_termall":         (lambda: _enc((200, 150, 1, 8, 3), part1=True, cblk_style=0x04), {}),
    "p1_vsc":             (lambda: _enc((200, 150, 1, 8, 3), part1=True, cblk_style=0x08), {}),
    "p1_segsym":          (lambda: _enc((200, 150, 1, 8, 3), part1=True, cblk_style=0x20), {}),
    "p1_bypass_termall":  (lambda: _enc((200, 150, 1, 12, 3, 60), depth=12, part1=True, cblk_style=0x05), {}),
    "p1_all_switches":    (lambda: _enc((160, 120, 1, 16, 8, 400), depth=16, nlevels=4, part1=True, cblk_style=0x2F), {}),
    "p1_rgb_mct":         (lambda: _enc((190, 131, 3, 8, 5), mct=1, part1=True), {}),
    "p1_rgb_tiles":       (lambda: _enc((190, 131, 3, 8, 6), mct=1, tile=(100, 70), nlevels=3, offset=(7, 9), tile_offset=(2, 3), part1=True), {}),
    "p1_yuv420":          (lambda: _enc((190, 130, 3, 8, 12, 8, (1, 2, 2), (1, 2, 2)), dx=[1, 2, 2], dy=[1, 2, 2], width=190, height=130, part1=True), {}),
    "p1_truncated_1":     (lambda: _enc((200, 150, 1, 8, 3), part1=True, drop_passes=1), {}),
    "p1_truncated_2":     (lambda: _enc((200, 150, 1, 8, 3), part1=True, drop_passes=2, cblk_style=0x04), {}),
    "p1_truncated_5":     (lambda: _enc((200, 150, 1, 8, 3), part1=True, drop_passes=5), {}),
    "p1_97":              (lambda: _enc((200, 150, 1, 8, 3), part1=True, transform=0, qstep=1), {}),
    "p1_97_rgb_bitexact": (lambda: _enc((190, 131, 3, 8, 5), part1=True, transform=0, mct=1, qstep=1), {"bitexact": 1}),
    "p1_lowres_2":        (lambda: _enc((190, 131, 3, 8, 5), mct=1, part1=True), {"reduction_factor": 2}),
    "p1_noise_max":       (lambda: vecgen.encode([np.random.default_rng(2).integers(0, 256, (130, 130))], nlevels=3, part1=True), {}),
    "p1_all_zero":        (lambda: vecgen.encode([np.full((100, 100), 128)], nlevels=3, part1=True), {}),
    "p1_tiny_3x1":        (lambda: vecgen.encode([np.array([[77, 3, 250]])], nlevels=2, part1=True), {}),
    # --- MIXED (SPcod bits 6-7 = 3): HT and Part-1 blocks in one stream, told apart in the packet header
    #     (jpeg2000dec.c:1256-1340).  OpenJPEG does not read MIXED streams: restatement + own round trip only ---
    "mixed_gray":         (lambda: _enc((200, 150, 1, 8, 3), mixed=True), {}),
    "mixed_rgb_cb32":     (lambda: _enc((190, 131, 3, 8, 5), mct=1, mixed=True, cb=(5, 5), nlevels=3), {}),
    "mixed_3passes_vsc":  (lambda: _enc((200, 150, 1, 8, 3), mixed=True, passes=3, vsc=True), {}),
    "mixed_gray16_tiles": (lambda: _enc((160, 120, 1, 16, 8, 400), depth=16, nlevels=3, mixed=True, tile=(96, 64)), {}),
    # --- Maxshift region of interest (RGN segments, T.800 Annex H): the bands are coded in M_b + s planes, the decoder
    #     shifts the samples below 2^s up (jpeg2000htdec.c:1326-1328, jpeg2000dec.c:2071-2086).  tests/test_roi_streams.py
    #     has the round trips.  "roi" in a name = the stream carries RGN ---
    "roi_gray":           (lambda: _enc((200, 150, 1, 8, 3), roi_shift=12), {}),
    "roi_gray_3passes":   (lambda: _enc((200, 150, 1, 8, 3), roi_shift=12, passes=3), {}),
    "roi_gray_2passes":   (lambda: _enc((200, 150, 1, 8, 3), roi_shift=12, passes=2), {}),
    "roi_gray_l3_cb256x16": (lambda: _enc((300, 90, 1, 8, 13), roi_shift=12, cb=(8, 4), nlevels=3), {}),
    "roi_rgb_mct_cb32":   (lambda: _enc((190, 131, 3, 8, 5), roi_shift=12, mct=1, cb=(5, 5)), {}),
    "roi_rgb_tiles":      (lambda: _enc((190, 131, 3, 8, 5), roi_shift=12, mct=1, tile=(64, 64), nlevels=3, sop=True, eph=True), {}),
    "roi_gray12":         (lambda: _enc((160, 120, 1, 12, 7, 40), depth=12, nlevels=4, roi_shift=12), {}),
    "p1_roi_gray":        (lambda: _enc((200, 150, 1, 8, 3), roi_shift=12, part1=True), {}),
    "p1_roi_rgb_mct":     (lambda: _enc((190, 131, 3, 8, 5), roi_shift=12, mct=1, part1=True), {}),
    "roi_mixed_gray":     (lambda: _enc((200, 150, 1, 8, 3), roi_shift=12, mixed=True), {}),
    # one component with a shift: its blocks take the ROI path, the others' the fast path, in the same launches.  The
    # reference computes every component's nonzerobits with component 0's shift (jpeg2000dec.c:1194), so only component 0
    # can be the one (test_roi_streams.py: [0, 12, 0] is refused by both parsers)
    "roi_rgb_nomct_comp0": (lambda: _enc((190, 131, 3, 8, 5), roi_shift=[12, 0, 0], prog=1, nlevels=4), {}),
    # SPrgn larger than the shift the blocks were coded with: the up-shift carries magnitude bits into and past bit 31
    "roi_gray_bias1":     (lambda: _enc((200, 150, 1, 8, 3), roi_shift=12, rgn_value_bias=1), {}),
    "roi_gray_bias3":     (lambda: _enc((200, 150, 1, 8, 3), roi_shift=10, rgn_value_bias=3, cb=(5, 5)), {}),
    "p1_roi_gray_bias1":  (lambda: _enc((200, 150, 1, 8, 3), roi_shift=12, rgn_value_bias=1, part1=True), {}),
    "p1_roi_gray_bias3":  (lambda: _enc((200, 150, 1, 8, 3), roi_shift=10, rgn_value_bias=3, part1=True, cb=(5, 5)), {}),
    "roi_gray_97":        (lambda: _enc((200, 150, 1, 8, 3), roi_shift=12, transform=0, qstep=1), {}),
    "roi_gray_97_bitexact": (lambda: _enc((200, 150, 1, 8, 3), roi_shift=12, transform=0, qstep=2), {"bitexact": 1}),
}

# --- components of one tile coded differently (COC / QCC).  comp=[dict | None, ...]: a dict overrides the common values for
#     that component (vecgen.COMP_KEYS).  COD / QCD carry component 0's values.  tests/test_hetero_streams.py has the round
#     trips and the OpenJPEG comparison of the Part-1 twins, tests/test_hetero_gpu.py the device paths ---
_RGB = (190, 131, 3, 8, 5)
_YUV420 = (190, 130, 3, 8, 12, 8, (1, 2, 2), (1, 2, 2))
_PREC_A, _PREC_B, _PREC_C = [(7, 7), (6, 6)], [(6, 5), (5, 6)], [(8, 6), (5, 5), (6, 7)]


def _nl(*levels):
    return [dict(nlevels=n) for n in levels]


# name -> (_img arguments, encode keywords, decode keywords); HET_PART1 in test_hetero_streams.py names the ones whose
# Part-1 twin OpenJPEG is asked about
HET = {
    # levels
    "het_rgb_levels_530":       (_RGB, dict(comp=_nl(5, 3, 0)), {}),
    "het_rgb_mct_levels_424":   (_RGB, dict(mct=1, comp=_nl(4, 2, 4)), {}),
    "het_rgb_ict_levels_424":   (_RGB, dict(mct=1, transform=0, qstep=1, comp=_nl(4, 2, 4)), {}),
    "het_rgb_ict_levels_424_bitexact": (_RGB, dict(mct=1, transform=0, qstep=1, comp=_nl(4, 2, 4)), {"bitexact": 1}),
    "het_yuv420_levels_250":    (_YUV420, dict(dx=[1, 2, 2], dy=[1, 2, 2], width=190, height=130, comp=_nl(2, 5, 0)), {}),
    "het_rgba_levels_3331":     ((96, 80, 4, 8, 16), dict(comp=_nl(3, 3, 3, 1)), {}),
    "het_gray_alpha":           ((96, 80, 2, 8, 18), dict(comp=_nl(4, 1)), {}),
    "het_rgb_deep_vs_none":     ((37, 23, 3, 8, 15), dict(comp=_nl(8, 0, 1)), {}),
    # wavelets
    "het_rgb_53_97_97":         (_RGB, dict(comp=[None, dict(transform=0, qstep=1), dict(transform=0, qstep=2)]), {}),
    "het_rgb_53_97_97_bitexact": (_RGB, dict(comp=[None, dict(transform=0, qstep=1), dict(transform=0, qstep=2)]), {"bitexact": 1}),
    "het_rgb_mct_flag_wavelets_differ": (_RGB, dict(mct=1, comp=[None, dict(transform=0, qstep=1), None]), {}),
    # blocks
    "het_rgb_cb_64x64_256x16_4x1024": ((300, 140, 3, 8, 13), dict(nlevels=2, comp=[None, dict(cb=(8, 4)), dict(cb=(2, 10))]), {}),
    "het_rgb_cb_32_64_16":      (_RGB, dict(nlevels=3, comp=[dict(cb=(5, 5)), dict(cb=(6, 6)), dict(cb=(4, 4))]), {}),
    "het_rgb_passes_132":       (_RGB, dict(comp=[dict(passes=1), dict(passes=3, vsc=True), dict(passes=2)]), {}),
    # quantisation
    # (component 2: M_b = 8 + 2 (HH) + 2 (bias) + 5 - 1 = 16, above what 16-bit sub-bands take)
    "het_rgb_guard_125":        (_RGB, dict(comp=[dict(guard_bits=1), dict(guard_bits=2), dict(guard_bits=5, expn_bias=2)]), {}),
    "het_rgb_97_qsteps":        (_RGB, dict(transform=0, comp=[dict(qstep=2), dict(qstep=1 / 32), dict(qstep=8)]), {}),
    "het_rgb10_expn_bias":      ((160, 120, 3, 10, 8, 20), dict(depth=10, nlevels=4, comp=[None, dict(expn_bias=3), dict(expn_bias=1)]), {}),
    # packet order: resolutions that exist for some components only, precinct grids of their own
    "het_rgb_lrcp_levels_prec": (_RGB, dict(prog=0, comp=[dict(nlevels=4, prec=_PREC_A), dict(nlevels=2, prec=_PREC_B), dict(nlevels=3, prec=_PREC_C)]), {}),
    "het_rgb_rlcp_levels_prec": (_RGB, dict(prog=1, comp=[dict(nlevels=4, prec=_PREC_A), dict(nlevels=2, prec=_PREC_B), dict(nlevels=3, prec=_PREC_C)]), {}),
    "het_rgb_rpcl_levels_prec": (_RGB, dict(prog=2, comp=[dict(nlevels=4, prec=_PREC_A), dict(nlevels=2, prec=_PREC_B), dict(nlevels=3, prec=_PREC_C)]), {}),
    "het_rgb_pcrl_levels_prec": (_RGB, dict(prog=3, comp=[dict(nlevels=4, prec=_PREC_A), dict(nlevels=2, prec=_PREC_B), dict(nlevels=3, prec=_PREC_C)]), {}),
    "het_rgb_cprl_levels_prec": (_RGB, dict(prog=4, comp=[dict(nlevels=4, prec=_PREC_A), dict(nlevels=2, prec=_PREC_B), dict(nlevels=3, prec=_PREC_C)]), {}),
    "het_rgb_rpcl_levels_prec_tiles": ((190, 131, 3, 8, 6), dict(prog=2, tile=(100, 70), offset=(7, 9), tile_offset=(2, 3),
                                        comp=[dict(nlevels=4, prec=_PREC_A), dict(nlevels=2, prec=_PREC_B), dict(nlevels=3, prec=_PREC_C)]), {}),
    "het_rgb_cprl_levels_prec_tiles": ((190, 131, 3, 8, 6), dict(prog=4, tile=(100, 70), offset=(7, 9), tile_offset=(2, 3),
                                        comp=[dict(nlevels=4, prec=_PREC_A), dict(nlevels=2, prec=_PREC_B), dict(nlevels=3, prec=_PREC_C)]), {}),
    # header location: COC / QCC in the first tile-part header of every tile
    "het_rgb_tiles_coc_in_tile_hdr": (_RGB, dict(tile=(64, 64), nlevels=3, coc_in_tile_hdr=True, comp=[None, dict(nlevels=1, guard_bits=3), dict(cb=(5, 5))]), {}),
    # region of interest and MIXED
    "het_roi_comp0_levels":     (_RGB, dict(roi_shift=[12, 0, 0], prog=1, comp=_nl(4, 2, 3)), {}),
    "het_mixed_levels":         (_RGB, dict(mixed=True, cb=(5, 5), comp=_nl(3, 1, 4)), {}),
    # reduced resolution
    "het_lowres_2":             (_RGB, dict(comp=_nl(5, 3, 3)), {"reduction_factor": 2}),
}


def het_encode(name, **more):
    """the stream of HET[name], with further encode keywords (part1=True: its Part-1 twin)"""
    args, kw, _ = HET[name]
    return _enc(args, **dict(kw, **more))


for _n in HET:
    CASES[_n] = (functools.partial(het_encode, _n), HET[_n][2])


# --- components of unequal bit depth.  Every frame goes through a conversion per component (add 1 << (cbps - 1), clip to
#     [0, 2^cbps - 1], shift left by precision - cbps; jpeg2000dec.c:2301-2364), whose constants the pack kernel, the fast
#     stores of the fused final level and the host's choice of kernels each read per component.  tests/test_depths_streams.py
#     pins the streams on the CPU, tests/test_depths_gpu.py has the device routes.
#     name -> (picture (width, height, seed, kind), depths, encode keywords, decode keywords); kind "synth": the seeded
#     picture of vecgen.synth_image per component at its own depth, "checker": the clipping picture of depths_image.
#     Two shapes: DEPTHS_FAST with three levels (every level of even origin and a width that is a multiple of 4: the fast
#     stores) and DEPTHS_ODD with two (width 1 mod 4, odd height: the general path).  Every kind of packed three-component
#     case (layout, shape, component transform) has an entry whose three depths are pairwise different, so that any two
#     components' constants exchanged change the frame; 8/7/8 and 8/12/8 are there because such pictures are common ---
DEPTHS_FAST, DEPTHS_ODD = (256, 96), (53, 37)
_F, _O = dict(nlevels=3), dict(nlevels=2)
_S422, _S420 = dict(dx=[1, 2, 2], dy=[1, 1, 1]), dict(dx=[1, 2, 2], dy=[1, 2, 2])
_Q = dict(transform=0)                                  # 9/7; the clip cases: qstep 0.5 for 8-bit layouts, 1 to 2 for 16-bit ones


def _f(seed, kind="synth"):
    return DEPTHS_FAST + (seed, kind)


def _o(seed, kind="synth"):
    return DEPTHS_ODD + (seed, kind)


DEPTHS = {
    # ---- fast geometry, lossless: every fast store of the fused final level
    "dep_rgb24_583":              (_f(1), [5, 8, 3], dict(_F), {}),                                     # rgb24 store
    "dep_rgb24_878_rct":          (_f(2), [8, 7, 8], dict(_F, mct=1), {}),                              # rgb24 store behind the RCT
    "dep_rgb24_876_rct":          (_f(22), [8, 7, 6], dict(_F, mct=1), {}),
    "dep_rgb48_8_12_8":           (_f(3), [8, 12, 8], dict(_F), {}),                                    # rgb48 store, 12 bits
    "dep_rgb48_8_12_8_rct":       (_f(4), [8, 12, 8], dict(_F, mct=1, guard_bits=5), {}),
    "dep_rgb48_12_10_16":         (_f(5), [12, 10, 16], dict(_F), {}),                                  # rgb48 store, 16 bits (M_b > 15)
    "dep_rgb48_12_10_16_rct":     (_f(6), [12, 10, 16], dict(_F, mct=1, guard_bits=7), {}),
    "dep_rgb48_8_12_8_rct_qcc":   (_f(7), [8, 12, 8], dict(_F, mct=1, comp=[dict(guard_bits=7), None, dict(guard_bits=7)]), {}),
    "dep_yuv422p12_10_12_9":      (_f(8), [10, 12, 9], dict(_F, **_S422), {}),                          # 16-bit plane store
    "dep_yuv420p_866":            (_f(9), [8, 6, 6], dict(_F, **_S420), {}),                            # 8-bit plane store
    "dep_yuv420p_866_levels_322": (_f(10), [8, 6, 6], dict(_F, comp=_nl(3, 2, 2), **_S420), {}),        # luma's final level a launch of its own
    "dep_yuv444p_878":            (_f(11), [8, 7, 8], dict(_F), {"req_pix_fmt": "yuv444p"}),            # 8-bit plane store, comp0 0, 1, 2
    "dep_yuv444p16_8_12_8":       (_f(12), [8, 12, 8], dict(_F), {"req_pix_fmt": "yuv444p16le"}),       # 16-bit plane store, 16 bits
    "dep_ya16_12_8":              (_f(13), [12, 8], dict(_F), {}),                                      # general path from here on
    "dep_ya8_8_1":                (_f(14), [8, 1], dict(_F), {}),
    "dep_rgba_8881":              (_f(15), [8, 8, 8, 1], dict(_F), {}),
    "dep_rgba64_10_10_10_16":     (_f(16), [10, 10, 10, 16], dict(_F), {}),
    # 50 x 40 tiles: the packed stores of a tile start at any byte
    "dep_rgb24_583_tiles50":      (_f(17), [5, 8, 3], dict(nlevels=2, tile=(50, 40)), {}),
    "dep_rgb48_8_12_8_tiles50":   (_f(18), [8, 12, 8], dict(nlevels=2, tile=(50, 40)), {}),
    # ---- fast geometry, 9/7
    "dep_rgb48_10_12_9_ict":      (_f(19), [10, 12, 9], dict(_F, mct=1, guard_bits=5, qstep=1, **_Q), {}),
    "dep_rgb48_10_12_9_ict_bitexact": (_f(19), [10, 12, 9], dict(_F, mct=1, guard_bits=5, qstep=1, **_Q), {"bitexact": 1}),
    "dep_rgb24_876_ict":          (_f(20), [8, 7, 6], dict(_F, mct=1, qstep=1, **_Q), {}),
    # ---- Part-1 twin, reduced resolution, signed components (the reference ignores the sign bit: jpeg2000dec.c:2301-2364
    #      add the DC shift all the same, the frame is the picture moved up by half the range)
    "p1_dep_rgb24_876_rct":       (_f(22), [8, 7, 6], dict(_F, mct=1, part1=True), {}),
    "dep_rgb24_583_lowres_1":     (_f(1), [5, 8, 3], dict(_F), {"reduction_factor": 1}),
    "dep_rgb48_8_12_8_sgnd":      (_f(21, "signed"), [8, 12, 8], dict(_F, sgnd=True), {}),
    # ---- 53 x 37, lossless: the general path of the fused final level and k_mct_pack
    "dep_odd_rgb24_583":          (_o(31), [5, 8, 3], dict(_O), {}),
    "dep_odd_rgb24_876_rct":      (_o(32), [8, 7, 6], dict(_O, mct=1), {}),
    "dep_odd_rgb48_8_12_8":       (_o(33), [8, 12, 8], dict(_O), {}),
    "dep_odd_rgb48_12_10_16":     (_o(34), [12, 10, 16], dict(_O), {}),
    "dep_odd_yuv422p12_10_12_9":  (_o(35), [10, 12, 9], dict(_O, **_S422), {}),
    "dep_odd_yuv420p_866":        (_o(36), [8, 6, 6], dict(_O, **_S420), {}),
    "dep_odd_ya16_12_8":          (_o(37), [12, 8], dict(_O), {}),
    "dep_odd_ya8_8_1":            (_o(38), [8, 1], dict(_O), {}),
    "dep_odd_rgba_8881":          (_o(39), [8, 8, 8, 1], dict(_O), {}),
    "dep_odd_rgba64_10_10_10_16": (_o(40), [10, 10, 10, 16], dict(_O), {}),
    "dep_odd_rgb48_10_12_9_ict":  (_o(41), [10, 12, 9], dict(_O, mct=1, guard_bits=5, qstep=1, **_Q), {}),
    "dep_odd_rgb48_10_12_9_ict_bitexact": (_o(41), [10, 12, 9], dict(_O, mct=1, guard_bits=5, qstep=1, **_Q), {"bitexact": 1}),
    # ---- clipping: a checkerboard between 0 and 2^d - 1 coded 9/7 rings past both ends of every component's range
    #      (tests/test_depths_streams.py counts the samples), so the upper bound and the zero bound of every component count
    "dep_clip_rgb24_583":         (_f(51, "checker"), [5, 8, 3], dict(_F, qstep=0.5, **_Q), {}),
    "dep_clip_rgb48_10_12_9":     (_f(52, "checker"), [10, 12, 9], dict(_F, qstep=1.5, **_Q), {}),
    "dep_clip_rgba_8881":         (_f(61, "checker"), [8, 8, 8, 1], dict(_F, qstep=0.5, **_Q), {}),
    "dep_clip_yuv420p_866":       (_f(53, "checker"), [8, 6, 6], dict(_F, qstep=0.5, **dict(_Q, **_S420)), {}),
    "dep_clip_yuv422p12_10_12_9": (_f(54, "checker"), [10, 12, 9], dict(_F, qstep=1.0, **dict(_Q, **_S422)), {}),
    "dep_clip_odd_rgb24_583":     (_o(55, "checker"), [5, 8, 3], dict(_O, qstep=0.5, **_Q), {}),
    "dep_clip_odd_rgb48_10_12_9": (_o(56, "checker"), [10, 12, 9], dict(_O, qstep=1.5, **_Q), {}),
    # (a 1-bit plane of 53 x 37 has about 17 samples past each end on average: these two seeds give it more than 20)
    "dep_clip_odd_rgba_8881":     (_o(116, "checker"), [8, 8, 8, 1], dict(_O, qstep=0.5, **_Q), {}),
    "dep_clip_odd_ya8_8_1":       (_o(72, "checker"), [8, 1], dict(_O, qstep=0.5, **_Q), {}),
    "dep_clip_odd_ya16_12_8":     (_o(59, "checker"), [12, 8], dict(_O, qstep=2.0, **_Q), {}),
    "dep_clip_odd_rgba64_10_10_10_16": (_o(60, "checker"), [10, 10, 10, 16], dict(_O, qstep=1.0, **_Q), {}),
}


@functools.lru_cache(maxsize=None)
def _depths_image(w, h, seed, kind, depths, dx, dy):
    out = []
    for c, d in enumerate(depths):
        cw, ch = -(-w // dx[c]), -(-h // dy[c])
        if kind == "checker":
            # ((x // 5 + y // 3) & 1) * (2^d - 1), seeded noise of -1 or +1, clipped to the component's range
            y, x = np.mgrid[0:ch, 0:cw]
            noise = np.random.default_rng([seed, c]).integers(0, 2, (ch, cw)) * 2 - 1
            out.append(np.clip(((x // 5 + y // 3) & 1) * ((1 << d) - 1) + noise, 0, (1 << d) - 1).astype(np.int32))
        else:
            noise = min(max((1 << d) >> 5, 1), 400)
            out.append(vecgen.synth_image(w, h, len(depths), depth=d, seed=seed, noise=noise, dx=list(dx), dy=list(dy),
                                          signed=kind == "signed")[c])
    return out


def depths_image(name, seed=None):
    """the picture of DEPTHS[name] (or the same kind of picture from another seed): one array per component, each at its
    own depth and size"""
    (w, h, s, kind), depths, kw, _ = DEPTHS[name]
    nc = len(depths)
    return _depths_image(w, h, s if seed is None else seed, kind, tuple(depths), tuple(kw.get("dx") or [1] * nc), tuple(kw.get("dy") or [1] * nc))


def depths_encode(name, seed=None, **more):
    """the stream of DEPTHS[name], over another seed's picture and with further encode keywords if given"""
    (w, h, _, _), depths, kw, _ = DEPTHS[name]
    kw = dict(kw, **more)
    if kw.get("dx"):
        kw.update(width=w, height=h)
    return vecgen.encode(depths_image(name, seed), depth=list(depths), **kw)


def depths_decode_kw(name, pix_names):
    """DEPTHS[name]'s decode keywords as the decoders take them: req_pix_fmt as an index into pix_names"""
    kw = dict(DEPTHS[name][3])
    if "req_pix_fmt" in kw:
        kw["req_pix_fmt"] = pix_names.index(kw["req_pix_fmt"])
    return kw


# (a case with req_pix_fmt needs a decoder opened with it: test_depths_gpu.py opens one, the catalogue's shared tests cannot)
for _n in DEPTHS:
    if "req_pix_fmt" not in DEPTHS[_n][3]:
        CASES[_n] = (functools.partial(depths_encode, _n), DEPTHS[_n][3])


# --- quality layers.  The factory deals the coding passes of every block out over the layers (vecgen.encode layers=,
#     layer_seed=): blocks first included in a later layer, blocks that skip a layer, empty packets, HT cleanup and refinement
#     bytes from different packets, Part-1 codeword segments cut at any byte.  The coefficients do not change, so every case
#     decodes to the frame of its one-layer twin (layers_twin).  tests/test_layers_streams.py pins the streams and what is in
#     them on the CPU, tests/test_layers_gpu.py takes them through the device routes.
#     name -> (_img arguments or a DEPTHS name, encode keywords, decode keywords) ---
_G, _G12, _G16 = (200, 150, 1, 8, 3), (200, 150, 1, 12, 3, 60), (160, 120, 1, 16, 8, 400)
_HETP = [dict(nlevels=4, prec=_PREC_A), dict(nlevels=2, prec=_PREC_B), dict(nlevels=3, prec=_PREC_C)]
_ORD = dict(mct=1, prec=[(7, 7), (6, 6)], nlevels=3, layers=3, passes=3)

LAYERS = {
    # HT, one pass
    "lay2_gray":             (_G, dict(layers=2, layer_seed=1), {}),
    "lay3_gray_cb32":        (_G, dict(layers=3, layer_seed=2, cb=(5, 5)), {}),
    "lay7_rgb_mct":          (_RGB, dict(layers=7, layer_seed=3, mct=1), {}),
    "lay40_gray":            (_G, dict(layers=40, layer_seed=4), {}),          # mostly empty packets
    # HT, refinement
    "lay2_gray_3passes":     (_G, dict(layers=2, layer_seed=205, passes=3), {}),
    "lay3_gray_3passes":     (_G, dict(layers=3, layer_seed=6, passes=3), {}),
    "lay3_gray_2passes":     (_G, dict(layers=3, layer_seed=7, passes=2), {}),
    "lay4_placeholder_2_3p": (_G, dict(layers=4, layer_seed=208, placeholder_sets=2, passes=3), {}),
    "lay3_rgb_3passes_cb32_vsc": (_RGB, dict(layers=3, layer_seed=9, mct=1, passes=3, cb=(5, 5), vsc=True), {}),
    # Part-1 styles
    "p1_lay3_gray":          (_G, dict(layers=3, layer_seed=10, part1=True), {}),
    "p1_lay3_bypass":        (_G12, dict(layers=3, layer_seed=211, depth=12, part1=True, cblk_style=0x01), {}),
    "p1_lay4_termall":       (_G, dict(layers=4, layer_seed=12, part1=True, cblk_style=0x04), {}),
    "p1_lay3_reset":         (_G, dict(layers=3, layer_seed=13, part1=True, cblk_style=0x02), {}),
    "p1_lay3_segsym":        (_G, dict(layers=3, layer_seed=14, part1=True, cblk_style=0x20), {}),
    "p1_lay5_bypass_termall": (_G12, dict(layers=5, layer_seed=15, depth=12, part1=True, cblk_style=0x05), {}),
    "p1_lay6_all_switches":  (_G16, dict(layers=6, layer_seed=16, depth=16, nlevels=4, part1=True, cblk_style=0x2F), {}),
    "p1_lay3_cb4x1024":      ((40, 150, 1, 8, 14), dict(layers=3, layer_seed=17, part1=True, cb=(2, 10), nlevels=2), {}),
    "p1_lay3_cb1024x4":      ((300, 40, 1, 8, 14), dict(layers=3, layer_seed=25, part1=True, cb=(10, 2), nlevels=3), {}),
    # MIXED
    "mixed_lay3_gray":       (_G, dict(layers=3, layer_seed=19, mixed=True), {}),
    "mixed_lay3_3passes_vsc": (_G, dict(layers=3, layer_seed=20, mixed=True, passes=3, vsc=True), {}),
    # the five packet orders, precincts; per-component levels and precinct grids; tiles with offsets
    "lay3_rgb_lrcp_prec":    (_RGB, dict(_ORD, layer_seed=21, prog=0), {}),
    "lay3_rgb_rlcp_prec":    (_RGB, dict(_ORD, layer_seed=22, prog=1), {}),
    "lay3_rgb_rpcl_prec":    (_RGB, dict(_ORD, layer_seed=23, prog=2), {}),
    "lay3_rgb_pcrl_prec":    (_RGB, dict(_ORD, layer_seed=24, prog=3), {}),
    "lay3_rgb_cprl_prec":    (_RGB, dict(_ORD, layer_seed=25, prog=4), {}),
    "lay2_het_pcrl_levels_prec": (_RGB, dict(layers=2, layer_seed=26, prog=3, passes=3, comp=_HETP), {}),
    "lay2_het_cprl_levels_prec": (_RGB, dict(layers=2, layer_seed=27, prog=4, passes=3, comp=_HETP), {}),
    "lay3_rgb_tiles_offsets": ((190, 131, 3, 8, 6), dict(layers=3, layer_seed=28, mct=1, tile=(64, 64), nlevels=3, offset=(7, 9), tile_offset=(2, 3), passes=3), {}),
    # other axes
    "lay3_gray_97":          (_G, dict(layers=3, layer_seed=129, transform=0, qstep=2, passes=3), {}),
    "lay3_rgb_97_bitexact":  (_RGB, dict(layers=3, layer_seed=30, transform=0, mct=1, qstep=1, passes=3), {"bitexact": 1}),
    "lay2_roi_gray":         (_G, dict(layers=2, layer_seed=131, roi_shift=12, passes=3), {}),
    "p1_lay3_roi_gray":      (_G, dict(layers=3, layer_seed=32, roi_shift=12, part1=True), {}),
    "lay3_yuv420p8":         (_YUV420, dict(layers=3, layer_seed=33, dx=[1, 2, 2], dy=[1, 2, 2], width=190, height=130, passes=2), {}),
    "lay3_gray16":           (_G16, dict(layers=3, layer_seed=34, depth=16, nlevels=4, passes=3), {}),
    "lay2_sop_eph":          (_G, dict(layers=2, layer_seed=135, sop=True, eph=True, passes=3), {}),
    "lay3_lowres_2":         (_RGB, dict(layers=3, layer_seed=36, mct=1, passes=3), {"reduction_factor": 2}),
    "lay2_tiny_7x5":         ((7, 5, 1, 8, 9), dict(layers=2, layer_seed=1937, nlevels=1, passes=3), {}),
    "lay2_all_zero":         ("all_zero", dict(layers=2, layer_seed=38, nlevels=3), {}),
    "lay3_dep_rgb48_8_12_8_rct": ("dep_rgb48_8_12_8_rct", dict(layers=3, layer_seed=39, passes=3), {}),
}


def layers_image(name):
    """the picture of LAYERS[name], one array per component"""
    src = LAYERS[name][0]
    if src == "all_zero":
        return [np.full((100, 100), 128)]
    return depths_image(src) if isinstance(src, str) else _img(*src)


def layers_encode(name, stats=None, **more):
    """the stream of LAYERS[name], with further encode keywords if given"""
    src, kw, _ = LAYERS[name]
    if isinstance(src, str) and src in DEPTHS:
        kw = dict(DEPTHS[src][2], depth=list(DEPTHS[src][1]), **kw)
    return vecgen.encode(layers_image(name), stats=stats, **dict(kw, **more))


def layers_twin(name, **more):
    """the one-layer twin of LAYERS[name]: same keywords, layers=1"""
    return layers_encode(name, layers=1, **more)


for _n in LAYERS:
    CASES[_n] = (functools.partial(layers_encode, _n), LAYERS[_n][2])


# the reference keeps the 16-bit layer count of SGcod in 8 bits (j2k_host.h: layers), and so do both parsers: 256 layers
# count as 0, 257 as 1.  What such a stream decodes to is whatever that makes of it; tests/test_layers_streams.py asks
# only that the two parsers agree on it.  CPU only, outside CASES
LAYERS_WRAP = {
    "lay256_gray": ((64, 48, 1, 8, 3), dict(layers=256, layer_seed=40, nlevels=2, passes=3)),
    "lay257_gray": ((64, 48, 1, 8, 3), dict(layers=257, layer_seed=41, nlevels=2, passes=3)),
}


@functools.lru_cache(maxsize=None)
def get(name):
    fn, kw = CASES[name]
    return fn(), kw
