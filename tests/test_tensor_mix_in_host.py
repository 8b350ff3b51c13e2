"""Tensors as frames through a colour matrix, without a device: the symbols and the struct, the image size, every refusal
of htj2k_encode_tensor_mix and htj2k_tensor_to_frames_mix in its order with a NULL context, htj2k_tensor_mix_in_rgb against
its float64 restatement, and the numpy model (tensor_mix_in_model) against a torch chain on the CPU written in the
definition's order, against tensor_in_model under the identity mix, and as the inverse of mix_model's Y'CbCr mix."""
import ctypes
import itertools
import math

import numpy as np
import pytest
import torch

import cmp_model as cm
import ffmpeg_ht_amd as m
import mix_model as mm
import tensor_in_model as tim
import tensor_mix_in_model as tmi
import tensor_model as tm
from test_tensor_host import frame

EINVAL, ENOSYS, PATCHWELCOME = -22, -38, -0x45574150
TORCH = {"float32": torch.float32, "float16": torch.float16, "bfloat16": torch.bfloat16}
NEW = ("htj2k_tensor_mix_in_rgb", "htj2k_tensor_image_size_mix_in", "htj2k_tensor_to_frames_mix", "htj2k_encode_tensor_mix")


@pytest.fixture(scope="module")
def L():
    return m.load_library()


def test_symbols_and_struct():
    L = m.load_library()
    for name in NEW:
        assert hasattr(L, name) and name in m.EXPORTS
    assert ctypes.sizeof(m.TensorMixIn) == 88
    assert m.TensorMixIn.m.offset == 8 and m.TensorMixIn.b.offset == 72
    mix = m.tensor_mix_in([[1, 2, 3], [4, 5, -0.0]], [0.5, -1], "box")
    assert (mix.nin, mix.chroma) == (3, 1) and [mix.m[1][k] for k in range(4)] == [4.0, 5.0, 0.0, 0.0] and mix.b[1] == -1.0
    assert math.copysign(1.0, mix.m[1][2]) == -1.0           # signed zeros are kept
    with pytest.raises(ValueError):
        m.tensor_mix_in(np.zeros((5, 3)))
    with pytest.raises(ValueError):
        m.tensor_mix_in(np.zeros((3, 3)), chroma="left")
    assert callable(m.Decoder.rgb_mix_in)


def size_call(L, fmt, w, h, bits, spec, mix):
    e, b = ctypes.c_size_t(), ctypes.c_size_t()
    r = L.htj2k_tensor_image_size_mix_in(m.PIX_NAMES.index(fmt), w, h, bits, None if spec is None else ctypes.byref(spec),
                                         None if mix is None else ctypes.byref(mix), ctypes.byref(e), ctypes.byref(b))
    return r, e.value, b.value


def test_image_size_counts_the_tensors_channels(L):
    for fmt, bits in (("yuv420p", 8), ("yuv422p10le", 10), ("rgb24", 8), ("gray", 8), ("rgba", 8)):
        nc = cm.LAYOUTS[fmt][0]
        for K in (1, 2, 3, 4):
            for dtype, esize in (("float32", 4), ("float16", 2), ("bfloat16", 2)):
                mix = m.tensor_mix_in(np.ones((nc, K)))
                assert size_call(L, fmt, 21, 11, bits, m.tensor_spec(dtype), mix) == (0, K * 21 * 11, K * 21 * 11 * esize)
        e, b = ctypes.c_size_t(), ctypes.c_size_t()
        spec = m.tensor_spec("float16")
        assert L.htj2k_tensor_image_size(m.PIX_NAMES.index(fmt), 21, 11, bits, ctypes.byref(spec), ctypes.byref(e), ctypes.byref(b)) == 0
        assert size_call(L, fmt, 21, 11, bits, spec, None) == (0, e.value, b.value) and e.value == nc * 21 * 11
    ok = m.tensor_mix_in(np.ones((3, 3)))
    assert size_call(L, "yuv420p", 21, 11, 8, None, ok)[0] == EINVAL
    assert size_call(L, "pal8", 21, 11, 8, m.tensor_spec("float16"), ok)[0] == PATCHWELCOME
    assert size_call(L, "yuv420p", 21, 11, 9, m.tensor_spec("float16"), ok)[0] == EINVAL
    assert size_call(L, "yuv420p", 0, 11, 8, m.tensor_spec("float16"), ok)[0] == EINVAL
    bad = m.tensor_mix_in(np.ones((3, 3)))
    bad.nin = 5
    assert size_call(L, "yuv420p", 21, 11, 8, m.tensor_spec("float16"), bad)[0] == EINVAL


def enc_call(L, spec, mix, fmt="yuv420p", w=20, h=10, bits=8, n=1, src=0x1000, src_bytes=1 << 40, out=0x1000, offsets=True, ctx=None,
             plain=False):
    """htj2k_encode_tensor_mix on memory that is never touched; plain: htj2k_encode_tensor, which has no mix"""
    offs = (ctypes.c_size_t * (abs(n) + 2))()
    pix = m.PIX_NAMES.index(fmt) if isinstance(fmt, str) else fmt
    head = (ctx, ctypes.c_void_p(src), ctypes.c_size_t(src_bytes), n, w, h, pix, bits, None if spec is None else ctypes.byref(spec))
    tail = (None, ctypes.c_void_p(out), ctypes.c_size_t(1 << 20), 0, offs if offsets else None)
    if plain:
        return L.htj2k_encode_tensor(*head, *tail)
    return L.htj2k_encode_tensor_mix(*head, None if mix is None else ctypes.byref(mix), *tail)


def frames_call(L, spec, mix, frames, bits=8, n=None, src=0x1000, src_bytes=1 << 40, ctx=None, plain=False):
    arr = (m.Frame * len(frames))(*frames) if frames is not None else None
    head = (ctx, ctypes.c_void_p(src), ctypes.c_size_t(src_bytes), (len(frames) if n is None else n), bits,
            None if spec is None else ctypes.byref(spec))
    if plain:
        return L.htj2k_tensor_to_frames(*head, arr)
    return L.htj2k_tensor_to_frames_mix(*head, None if mix is None else ctypes.byref(mix), arr)


def _spec(**kw):
    s = m.tensor_spec("float16")
    for k, v in kw.items():
        setattr(s, k, v)
    return s


def _mix(nc=3, K=3, **kw):
    """a valid mix of K channels for nc components, then fields overwritten: nin, chroma, m=(c, k, v), b=(c, v)"""
    x = m.tensor_mix_in(np.ones((nc, K)))
    for k, v in kw.items():
        if k == "m":
            x.m[v[0]][v[1]] = v[2]
        elif k == "b":
            x.b[v[0]] = v[1]
        else:
            setattr(x, k, v)
    return x


BAD = (math.nan, math.inf, -math.inf)


def test_encode_tensor_mix_refuses_in_its_order_with_a_null_context(L):
    ok, mix = m.tensor_spec("float16"), _mix()
    bad_spec = _spec(dtype=7, layout=9, out_w=-1)
    assert enc_call(L, ok, mix) == ENOSYS
    assert enc_call(L, m.tensor_spec("float32", "NHWC"), _mix(3, 4, chroma=1), "rgb48le", 7, 3, 12, n=5) == ENOSYS
    assert enc_call(L, ok, _mix(1, 3), "gray") == ENOSYS and enc_call(L, ok, _mix(4, 1), "rgba") == ENOSYS
    # scale and bias are not read with a mix
    s = m.tensor_spec("float16")
    s.scale[0], s.bias[1] = math.nan, math.inf
    assert enc_call(L, s, mix) == ENOSYS and enc_call(L, s, None) == EINVAL
    # 1 .. 3: missing arguments, n, the size, before the layout
    assert enc_call(L, ok, mix, "pal8", src=0) == EINVAL and enc_call(L, None, mix, "pal8") == EINVAL
    assert enc_call(L, ok, mix, "pal8", out=0) == EINVAL and enc_call(L, ok, mix, "pal8", offsets=False) == EINVAL
    assert enc_call(L, ok, mix, "pal8", n=0) == EINVAL and enc_call(L, ok, mix, "pal8", w=0) == EINVAL and enc_call(L, ok, mix, "pal8", h=-1) == EINVAL
    # 4: the layout before everything of the spec and the mix
    assert enc_call(L, bad_spec, _mix(nin=9, chroma=7), "pal8", bits=99, src_bytes=0, src=0x1001) == PATCHWELCOME
    for bad_fmt in (-1, len(m.PIX_NAMES)):
        assert enc_call(L, ok, mix, bad_fmt) == EINVAL
    # 5: bits, before dtype
    assert enc_call(L, bad_spec, mix, bits=9) == EINVAL and enc_call(L, ok, mix, bits=0) == EINVAL
    assert enc_call(L, ok, mix, "yuv422p10le", bits=11) == EINVAL and enc_call(L, ok, mix, "yuv422p10le", bits=10) == ENOSYS
    # 6: dtype and layout, before the mix
    for kw in (dict(dtype=-1), dict(dtype=3), dict(layout=-1), dict(layout=2)):
        assert enc_call(L, _spec(**kw), mix) == EINVAL
    # 7: the mix in the place of scale and bias: nin, chroma, then the entries that are read
    for nin in (0, -1, 5):
        assert enc_call(L, ok, _mix(nin=nin)) == EINVAL
    for chroma in (-1, 2):
        assert enc_call(L, ok, _mix(chroma=chroma)) == EINVAL
    for v in BAD:
        for c, k in itertools.product(range(3), range(3)):
            assert enc_call(L, ok, _mix(m=(c, k, v))) == EINVAL
        for c in range(3):
            assert enc_call(L, ok, _mix(b=(c, v))) == EINVAL
        # entries that are not read: row 3 of a layout of three components, column 3 of a tensor of three channels
        assert enc_call(L, ok, _mix(m=(3, 0, v))) == ENOSYS and enc_call(L, ok, _mix(m=(0, 3, v))) == ENOSYS
        assert enc_call(L, ok, _mix(b=(3, v))) == ENOSYS
        assert enc_call(L, ok, _mix(1, 2, m=(1, 0, v)), "gray") == ENOSYS and enc_call(L, ok, _mix(1, 2, m=(0, 1, v)), "gray") == EINVAL
    # 8: no window, and it comes behind the mix
    for ow, oh in ((0, 1), (1, 0), (-1, -1), (20, 10), (4, 4)):
        assert enc_call(L, _spec(out_w=ow, out_h=oh), mix) == EINVAL
    # 9: src_bytes counts K channels
    for K in (1, 2, 3, 4):
        need = K * 20 * 10 * 2
        assert enc_call(L, ok, _mix(3, K), src_bytes=need) == ENOSYS and enc_call(L, ok, _mix(3, K), src_bytes=need - 1) == EINVAL
        assert enc_call(L, ok, _mix(3, K), n=3, src_bytes=3 * need - 1) == EINVAL
    assert enc_call(L, m.tensor_spec("float32"), mix, src_bytes=3 * 20 * 10 * 4 - 1) == EINVAL
    # 10
    assert enc_call(L, ok, mix, src=0x1001) == EINVAL and enc_call(L, ok, mix, src=0x1002) == ENOSYS
    assert enc_call(L, m.tensor_spec("float32"), mix, src=0x1002) == EINVAL


def test_tensor_to_frames_mix_refuses_in_its_order_with_a_null_context(L):
    ok, mix = m.tensor_spec("float16"), _mix()
    f, pal = frame("yuv420p", 20, 10), frame("pal8", 20, 10)
    assert frames_call(L, ok, mix, [f]) == ENOSYS
    assert frames_call(L, m.tensor_spec("float32", "NHWC"), _mix(3, 1, chroma=1), [frame("xyz12le", 7, 3)] * 4, bits=12) == ENOSYS
    assert frames_call(L, ok, mix, [pal], src=0) == EINVAL and frames_call(L, None, mix, [pal]) == EINVAL
    assert frames_call(L, ok, mix, None, n=1) == EINVAL and frames_call(L, ok, mix, [pal], n=0) == EINVAL
    assert frames_call(L, _spec(dtype=7, layout=9, out_w=-1), _mix(nin=0, chroma=9), [pal], bits=99, src_bytes=0) == PATCHWELCOME
    assert frames_call(L, _spec(dtype=7), mix, [f], bits=9) == EINVAL and frames_call(L, ok, mix, [f], bits=0) == EINVAL
    for kw in (dict(dtype=-1), dict(dtype=3), dict(layout=-1), dict(layout=2)):
        assert frames_call(L, _spec(**kw), mix, [f]) == EINVAL
    for bad in (_mix(nin=0), _mix(nin=5), _mix(chroma=-1), _mix(chroma=2)):
        assert frames_call(L, ok, bad, [f]) == EINVAL
    for v in BAD:
        for c, k in itertools.product(range(3), range(3)):
            assert frames_call(L, ok, _mix(m=(c, k, v)), [f]) == EINVAL
        assert frames_call(L, ok, _mix(b=(2, v)), [f]) == EINVAL
        assert frames_call(L, ok, _mix(m=(3, 1, v)), [f]) == ENOSYS and frames_call(L, ok, _mix(m=(1, 3, v)), [f]) == ENOSYS
        assert frames_call(L, ok, _mix(b=(3, v)), [f]) == ENOSYS
    for ow, oh in ((0, 1), (1, 0), (-1, -1), (20, 10)):
        assert frames_call(L, _spec(out_w=ow, out_h=oh), mix, [f]) == EINVAL
    assert frames_call(L, ok, mix, [f, frame("yuv422p", 20, 10)]) == EINVAL and frames_call(L, ok, mix, [f, frame("yuv420p", 21, 10)]) == EINVAL
    g = frame("yuv420p", 20, 10)
    g.data[2] = None
    assert frames_call(L, ok, mix, [f, g]) == EINVAL
    g = frame("yuv420p", 20, 10)
    g.linesize[1] = 9
    assert frames_call(L, ok, mix, [g]) == EINVAL
    for K in (1, 2, 3, 4):
        need = K * 20 * 10 * 2
        assert frames_call(L, ok, _mix(3, K), [f], src_bytes=need) == ENOSYS and frames_call(L, ok, _mix(3, K), [f], src_bytes=need - 1) == EINVAL
        assert frames_call(L, ok, _mix(3, K), [f, f], src_bytes=2 * need - 1) == EINVAL
    assert frames_call(L, ok, mix, [f], src=0x1001) == EINVAL and frames_call(L, ok, mix, [f], src=0x1002) == ENOSYS
    assert frames_call(L, m.tensor_spec("float32"), mix, [f], src=0x1002) == EINVAL


def test_a_null_mix_refuses_exactly_as_the_plain_twin(L):
    ok = m.tensor_spec("float16")
    nan_scale, inf_bias = m.tensor_spec("float16"), m.tensor_spec("float16")
    nan_scale.scale[2], inf_bias.bias[0] = math.nan, math.inf
    f = frame("yuv420p", 20, 10)
    short = frame("yuv420p", 20, 10)
    short.linesize[0] = 19
    need = 3 * 20 * 10 * 2
    enc_cases = [dict(), dict(fmt="pal8"), dict(src=0), dict(n=0), dict(w=0), dict(bits=9), dict(spec=_spec(dtype=3)), dict(spec=nan_scale),
                 dict(spec=inf_bias), dict(spec=_spec(out_w=20, out_h=10)), dict(src_bytes=need - 1), dict(src_bytes=need), dict(src=0x1001),
                 dict(fmt="gray", spec=nan_scale), dict(fmt="xyz12le", bits=12), dict(offsets=False), dict(out=0)]
    codes = set()
    for kw in enc_cases:
        kw = dict(kw)
        spec = kw.pop("spec", ok)
        a, b = enc_call(L, spec, None, **kw), enc_call(L, spec, None, plain=True, **kw)
        assert a == b, kw
        codes.add(a)
    assert codes == {ENOSYS, EINVAL, PATCHWELCOME}
    frame_cases = [dict(frames=[f]), dict(frames=[frame("pal8", 20, 10)]), dict(frames=[f], src=0), dict(frames=[f], n=0), dict(frames=[f], bits=9),
                   dict(frames=[f], spec=_spec(layout=2)), dict(frames=[f], spec=nan_scale), dict(frames=[f], spec=_spec(out_w=1, out_h=1)),
                   dict(frames=[f, frame("yuv420p", 21, 10)]), dict(frames=[short]), dict(frames=[f], src_bytes=need - 1),
                   dict(frames=[f], src_bytes=need), dict(frames=[f], src=0x1001), dict(frames=None, n=1)]
    for kw in frame_cases:
        kw = dict(kw)
        spec, frames = kw.pop("spec", ok), kw.pop("frames")
        assert frames_call(L, spec, None, frames, **kw) == frames_call(L, spec, None, frames, plain=True, **kw), kw


# ------------------------------------------------------------------ htj2k_tensor_mix_in_rgb

def _ulps(a, b):
    """distance of float32 a from float64 b in units of a's last place"""
    a = np.float32(a)
    if a == np.float32(b):
        return 0.0
    return abs(float(a) - b) / float(np.spacing(np.abs(np.float32(b))))


GAINS = [(None, None), ((255.0, 255.0, 255.0), None), ((2.0, 0.5, -1.5), (-1.0, 0.25, 3.0)), ((1 / 0.229, 1 / 0.224, 1 / 0.225), (-2.1, -2.0, -1.8))]


def test_rgb_helper_is_within_one_ulp_of_its_float64_restatement():
    for standard, full, bits, alpha, (gain, offset), chroma in itertools.product((601, 709, 2020), (False, True), (8, 10, 12, 16), (False, True),
                                                                                 GAINS, ("cosited", "box")):
        mix = m.Decoder.rgb_mix_in(standard, bits, full, alpha, gain, offset, chroma)
        want_m, want_b = tmi.rgb(standard, full, bits, alpha, gain, offset)
        nc = 4 if alpha else 3
        assert (mix.nin, mix.chroma) == (nc, tmi.CHROMA[chroma])
        for c in range(4):
            for k in range(4):
                want = want_m[c, k] if c < nc and k < nc else 0.0
                assert _ulps(mix.m[c][k], want) <= 1.0, (standard, full, bits, alpha, gain, c, k, mix.m[c][k], want)
            want = want_b[c] if c < nc else 0.0
            assert _ulps(mix.b[c], want) <= 1.0, (standard, full, bits, gain, offset, c, mix.b[c], want)
        if gain is None:                                       # without gain and offset b is the constant itself
            assert [mix.b[c] for c in range(3)] == [0.0 if full else 16.0 * (1 << (bits - 8)), float(1 << (bits - 1)), float(1 << (bits - 1))]
    # the luma row at 8 bits, limited range, BT.601: 219 times Kr, Kg, Kb
    mix = m.Decoder.rgb_mix_in(601, 8)
    assert [mix.m[0][k] for k in range(3)] == [np.float32(219 * 0.299), np.float32(219 * (1.0 - 0.299 - 0.114)), np.float32(219 * 0.114)]


def test_rgb_helper_refusals(L):
    mix = m.TensorMixIn()
    g3 = ctypes.c_float * 3

    def call(mixp=ctypes.byref(mix), standard=709, full=0, bits=10, alpha=0, gain=None, offset=None, chroma=0):
        return L.htj2k_tensor_mix_in_rgb(mixp, standard, full, bits, alpha, None if gain is None else g3(*gain),
                                         None if offset is None else g3(*offset), chroma)

    assert call() == 0 and call(gain=(1, 2, 3), offset=(0, -1, 1), chroma=1, alpha=1) == 0
    assert call(mixp=None) == EINVAL
    for standard in (0, 600, 2100):
        assert call(standard=standard) == EINVAL
    for bits in (7, 17, 0):
        assert call(bits=bits) == EINVAL
    for v in (0.0, -0.0, math.nan, math.inf, -math.inf):
        for k in range(3):
            gain = [1.0, 1.0, 1.0]
            gain[k] = v
            assert call(gain=gain) == EINVAL
    for v in BAD:
        for k in range(3):
            offset = [0.0, 0.0, 0.0]
            offset[k] = v
            assert call(offset=offset) == EINVAL
    for chroma in (-1, 2):
        assert call(chroma=chroma) == EINVAL
    with pytest.raises(m.Htj2kError):
        m.Decoder.rgb_mix_in(709, 7)


# ------------------------------------------------------------------ the model against a torch chain

def torch_frames(t, fmt, bits, mix, layout="NCHW"):
    """the definition as a torch eager chain on t's device: elementwise operations and strided slices only, every
    operation on float32 tensors in the definition's order -> per image the list of component arrays (int64 samples)"""
    nc, _, cw, ch, _, _ = cm.LAYOUTS[fmt]
    nin, chroma, m4, b4 = tmi.unpack(mix)
    x = t.float()
    chw = x if layout == "NCHW" else x.permute(0, 3, 1, 2)
    assert chw.shape[1] == nin
    peak = float((1 << bits) - 1)
    dev = t.device
    comps = []
    for c in range(nc):
        sw, sh = (cw, ch) if c in (1, 2) else (0, 0)
        fw, fh = 1 << sw, 1 << sh
        g = []
        for k in range(nin):
            f = chw[:, k]
            gk = f[:, ::fh, ::fw].clone()
            if chroma == tmi.BOX and (fw > 1 or fh > 1):
                cnt = torch.zeros(gk.shape[1:], dtype=torch.float64, device=dev)
                for fy in range(fh):
                    for fx in range(fw):
                        part = f[:, fy::fh, fx::fw]
                        rows, cols = part.shape[1:]
                        if fy or fx:
                            gk[:, :rows, :cols] = gk[:, :rows, :cols] + part
                        cnt[:rows, :cols] += 1
                rcp = (1.0 / cnt).float()                      # the float32 nearest to 1 / N
                gk = torch.where(cnt > 1, gk * rcp, gk)
            g.append(gk)
        w = [torch.tensor(float(m4[c][k]), dtype=torch.float32, device=dev) for k in range(nin)]
        a = g[0] * w[0]
        for k in range(1, nin):
            a = a + g[k] * w[k]
        u = a + torch.tensor(float(b4[c]), dtype=torch.float32, device=dev)
        r = torch.round(u)                                     # half to even
        s = torch.where(r > 0, torch.clamp(r, max=peak), torch.zeros_like(r))      # NaN compares false: 0
        comps.append(s.to(torch.int64))
    return comps


def check_against_torch(got_planes, comps, fmt, bits, what):
    """model (or device) planes of n frames against torch_frames' components"""
    for i, planes in enumerate(got_planes):
        have = cm.components(planes, fmt, bits)
        for c, want in enumerate(comps):
            assert np.array_equal(have[c], want[i].cpu().numpy()), (what, i, c)


def random_bits(shape, dtype, rng, lo=-0.2, hi=1.3):
    """values in [lo, hi) of the element type, with a sprinkle of the corners of the format -> (torch tensor, bit patterns)"""
    v = rng.uniform(lo, hi, size=shape).astype(np.float32)
    flat = v.reshape(-1)
    special = np.array([np.nan, np.inf, -np.inf, -0.0, 0.0, 6e-8, 1e-40, 3e38, -3e38, 65504.0], np.float32)
    at = rng.choice(flat.size, size=min(flat.size // 7, 40), replace=False)
    flat[at] = special[np.arange(at.size) % special.size]
    t = torch.from_numpy(v).to(TORCH[dtype]).contiguous()
    bits = t.view(torch.int32 if dtype == "float32" else torch.int16).numpy().view(tm.BITS_DTYPE[dtype])
    return t, bits


def random_mix(nc, K, chroma, rng, peak):
    mat = rng.uniform(-1.0, 1.0, size=(nc, K)) * peak
    mat[rng.random((nc, K)) < 0.15] = -0.0
    return mat.astype(np.float32), rng.uniform(-4.0, peak / 2, size=nc).astype(np.float32), chroma


# sizes whose last footprints are clipped: N = 3 (4:1:1 at w = 4 k + 3), 6 (4:1:0, 3 columns x 2 rows), 12 (4:1:0, 4 x 3 and 3 x 4);
# test_the_chain_cases_have_the_clipped_footprints counts them
CHAIN = [("yuv420p", 8, 5, 3), ("yuv420p", 8, 6, 4), ("yuv422p10le", 10, 9, 5), ("yuv411p", 8, 7, 2), ("yuv411p", 8, 11, 3), ("yuv410p", 8, 7, 6),
         ("yuv410p", 8, 11, 7), ("yuv410p", 8, 8, 8), ("yuv444p12le", 12, 5, 3), ("yuva420p", 8, 3, 3), ("rgb24", 8, 5, 3), ("rgba", 8, 4, 2),
         ("gray", 8, 3, 2), ("ya8", 8, 3, 3), ("rgb48le", 16, 3, 2), ("xyz12le", 12, 2, 5), ("gray16le", 16, 1, 1)]


def footprint_sizes(fmt, w, h):
    _, _, cw, ch, _, _ = cm.LAYOUTS[fmt]
    xs = {min(1 << cw, w - x) for x in range(0, w, 1 << cw)}
    ys = {min(1 << ch, h - y) for y in range(0, h, 1 << ch)}
    return {a * b for a in xs for b in ys}


def test_the_chain_cases_have_the_clipped_footprints():
    seen = set()
    for fmt, _, w, h in CHAIN:
        seen |= footprint_sizes(fmt, w, h)
    assert {1, 2, 3, 4, 6, 8, 12, 16} <= seen, seen


@pytest.mark.parametrize("case", CHAIN, ids=lambda c: "%s-%d-%dx%d" % c)
def test_model_agrees_with_a_torch_chain_in_the_definitions_order(case):
    fmt, bits, w, h = case
    nc = cm.LAYOUTS[fmt][0]
    rng = np.random.default_rng(CHAIN.index(case))
    for dtype in tm.DTYPES:
        for K in (1, 2, 3, 4):
            for chroma in (tmi.COSITED, tmi.BOX):
                layout = "NCHW" if (K + chroma) % 2 else "NHWC"
                shape = (2, K, h, w) if layout == "NCHW" else (2, h, w, K)
                t, tbits = random_bits(shape, dtype, rng)
                mix = random_mix(nc, K, chroma, rng, (1 << bits) - 1)
                got = tmi.frames(tbits, fmt, bits, mix, dtype, layout)
                assert [p.shape for p in got[0]] == [tuple(s) for s in cm.plane_shapes(fmt, w, h)]
                check_against_torch(got, torch_frames(t, fmt, bits, mix, layout), fmt, bits, (case, dtype, K, chroma, layout))
                # a TensorMixIn struct says what the triple says
                struct = m.tensor_mix_in(mix[0], mix[1], chroma)
                again = tmi.frames(tbits, fmt, bits, struct, dtype, layout)
                assert all(np.array_equal(a, b) for fa, fb in zip(got, again) for a, b in zip(fa, fb))


def test_model_at_the_corners():
    f32 = np.float32
    one = lambda vals, m_, b_, bits=8: [int(v) for v in tmi.frame(np.array(vals, f32).reshape(len(m_[0]), 1, 1).view(np.uint32), "gray", bits,
                                                                   (np.array(m_, f32), np.array(b_, f32), tmi.COSITED))[0].ravel()]
    assert one([np.inf, 1.0], [[0.0, 1.0]], [0.0]) == [0]                 # inf * 0 is NaN: sample 0
    assert one([np.inf, 1.0], [[1.0, 1.0]], [0.0]) == [255]
    assert one([3e38, 3e38], [[1.0, 1.0]], [0.0]) == [255]                # the sum overflows to +inf: the peak
    assert one([-3e38, -3e38], [[1.0, 1.0]], [9.0]) == [0]                # to -inf: 0
    assert one([np.inf, np.inf], [[1.0, -1.0]], [0.0]) == [0]             # inf - inf
    assert one([np.nan], [[1.0]], [5.0]) == [0] and one([-0.0], [[1.0]], [0.0]) == [0]
    assert one([2.5], [[1.0]], [0.0]) == [2] and one([3.5], [[1.0]], [0.0]) == [4] and one([0.5], [[1.0]], [0.0]) == [0]
    assert one([1.0, 7.0], [[2.0, -0.0]], [0.5]) == [2]                   # a weight of -0.0 adds -0: 2.5 ties to 2
    assert one([254.5], [[1.0]], [0.0]) == [254] and one([254.51], [[1.0]], [0.0]) == [255]
    # box: the exact mean of four, a clipped pair, a clipped single; 1 / 3 is the rounded reciprocal, not a division
    img = np.array([[[1.0, 2.0, 10.0], [3.0, 4.0, 20.0], [7.0, 8.0, 30.0]]], f32)
    u = tmi.component_u(img, "yuv420p", (np.ones((3, 1), f32), None, tmi.BOX), 1)
    assert u.tolist() == [[2.5, 15.0], [7.5, 30.0]]
    three = np.array([[[1.0, 1.0, 1.0, 1.0, 5.0, 5.0, 5.0]]], f32)
    u = tmi.component_u(three, "yuv411p", (np.ones((3, 1), f32), None, tmi.BOX), 2)
    assert u.tolist() == [[1.0, float(f32(15.0) * f32(1.0 / 3.0))]] and f32(1.0 / 3.0).view(np.uint32) == 0x3EAAAAAB
    # binary16 subnormals are values
    sub = np.array([0x0001, 0x03FF], np.uint16).reshape(1, 1, 2)
    assert tmi.frame(sub, "gray16le", 16, (np.array([[2.0 ** 24]], f32), None, tmi.COSITED), "float16")[0].tolist() == [[1, 1023]]


@pytest.mark.parametrize("fmt", ["gray", "ya8", "rgb24", "rgba", "rgb48le", "yuv444p12le", "yuv422p10le", "yuv420p", "yuv411p", "yuv410p",
                                 "yuva420p", "xyz12le"])
def test_identity_mix_is_tensor_in_model(fmt):
    nc, depth = cm.LAYOUTS[fmt][0], cm.LAYOUTS[fmt][4]
    rng = np.random.default_rng(len(fmt))
    for (w, h), dtype, layout in itertools.product(((5, 3), (8, 4), (1, 1)), tm.DTYPES, ("NCHW", "NHWC")):
        shape = (2, nc, h, w) if layout == "NCHW" else (2, h, w, nc)
        v = rng.uniform(-3.0, (1 << depth) + 3.0, size=shape).astype(np.float32)      # finite elements
        t = torch.from_numpy(v).to(TORCH[dtype]).contiguous()
        tbits = t.view(torch.int32 if dtype == "float32" else torch.int16).numpy().view(tm.BITS_DTYPE[dtype])
        want = tim.frames(tbits, fmt, depth, dtype, layout)
        got = tmi.frames(tbits, fmt, depth, tmi.identity(nc), dtype, layout)
        assert all(np.array_equal(a, b) and a.dtype == b.dtype for fa, fb in zip(got, want) for a, b in zip(fa, fb)), (fmt, w, h, dtype, layout)


def test_box_is_cosited_on_the_averaged_tensor():
    rng = np.random.default_rng(2)
    for fmt, bits, w, h in (("yuv420p", 8, 7, 5), ("yuv422p10le", 10, 9, 2), ("yuv411p", 8, 11, 3), ("yuv410p", 8, 11, 7)):
        for dtype, layout in (("float32", "NCHW"), ("float16", "NHWC"), ("bfloat16", "NCHW")):
            shape = (1, 3, h, w) if layout == "NCHW" else (1, h, w, 3)
            t, tbits = random_bits(shape, dtype, rng)
            mat, off, _ = random_mix(3, 3, tmi.BOX, rng, (1 << bits) - 1)
            box = tmi.frame(tbits[0], fmt, bits, (mat, off, tmi.BOX), dtype, layout)
            pre = tmi.averaged(tbits[0], fmt, (mat, off, tmi.BOX), dtype, layout)
            cos = tmi.frame(pre, fmt, bits, (mat, off, tmi.COSITED), "float32", layout)
            assert np.array_equal(box[1], cos[1]) and np.array_equal(box[2], cos[2]), (fmt, dtype, layout)


# ------------------------------------------------------------------ the round trip in the model

ROUND_TRIP_LAYOUTS = {8: ["yuv444p", "yuv422p", "yuv420p", "yuv411p", "yuv410p"], 10: ["yuv444p10le", "yuv422p10le", "yuv420p10le"],
                      12: ["yuv444p12le", "yuv422p12le", "yuv420p12le"], 16: ["yuv444p16le", "yuv422p16le", "yuv420p16le"]}


def round_trip_planes(fmt, bits, rng):
    """random samples of the whole cube, and its eight corners as whole footprints in the first rows"""
    _, _, cw, ch, _, nbytes = cm.LAYOUTS[fmt]
    w, h = (256, 80) if (cw, ch) == (0, 0) else (64, 16)
    peak = (1 << bits) - 1
    comps = [rng.integers(0, peak + 1, size=s, dtype=np.int64) for s in cm.plane_shapes(fmt, w, h)]
    for j, corner in enumerate(itertools.product((0, peak), repeat=3)):
        comps[0][0:1 << ch, j << cw:(j + 1) << cw] = corner[0]
        comps[1][0, j], comps[2][0, j] = corner[1], corner[2]
    return [(c << cm.shift(fmt, bits)).astype(np.uint8 if nbytes == 1 else np.uint16) for c in comps], w, h


@pytest.mark.parametrize("bits", [8, 10, 12, 16])
@pytest.mark.parametrize("standard", [601, 709, 2020])
def test_round_trip_through_float32_is_the_identity(standard, bits):
    """samples -> mix_model with ycbcr(...) -> float32 -> this model with rgb(...) and the same arguments -> the same samples"""
    rng = np.random.default_rng(standard + bits)
    worst = 0.0
    for fmt in ROUND_TRIP_LAYOUTS[bits]:
        planes, w, h = round_trip_planes(fmt, bits, rng)
        for full in (False, True):
            out = mm.image(planes, fmt, bits, mm.ycbcr(standard, full, bits), "float32", "NCHW")
            mat, off = tmi.rgb(standard, full, bits)
            for chroma in (tmi.COSITED, tmi.BOX):
                back = tmi.frame(out, fmt, bits, (mat, off, chroma), "float32", "NCHW")
                for c, (a, b) in enumerate(zip(back, planes)):
                    assert a.dtype == b.dtype and np.array_equal(a, b), (standard, bits, fmt, full, chroma, c, int(np.count_nonzero(a != b)))
                chw = tim.element_values(out, "float32")
                for c in range(3):
                    u = tmi.component_u(chw, fmt, (mat, off, chroma), c).astype(np.float64)
                    worst = max(worst, float(np.abs(u - np.rint(u)).max()))
    assert worst < 0.25, worst          # far from the ties at .5: the identity does not hang on a rounding
