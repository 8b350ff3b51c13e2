"""numpy restatement of tensors as frames with transfer curves (include/htj2k_amd.h "tensors as frames, with curves",
csrc/curve_in_kernels.hpp): the frames that htj2k_tensor_to_frames_curves writes for a tensor of K channels, and that
htj2k_encode_tensor_curves encodes.  It is tensor_mix_in_model with three steps added, each a separate np.float32
operation: the in-curve on every element before the gather, the out-curve on the mix's result, then gain and offset.
R(x; curve) is the root (np.fmax against 0, then np.sqrt `root` times: IEEE square roots, correctly rounded) followed by
curve_model.curve_eval, the E of the other direction.  torch_chain() is the chain of eager torch operations a caller runs
today for a layout without chroma shifts; mix_in_xyz() and fill_root() are the float64 restatements of
htj2k_tensor_mix_in_xyz and htj2k_tensor_curve_fill_root."""
import numpy as np

import cmp_model as cm
import curve_model as cvm
import tensor_in_model as tim
import tensor_mix_in_model as tmi


def root_eval(x, table, x0=0.0, inv_dx=1.0, root=0):
    """R(x; curve): p = x when root is 0; else fmaxf(x, 0) (a NaN becomes 0) square-rooted `root` times; then E(p)"""
    p = np.asarray(x, np.float32)
    if root:
        with np.errstate(invalid="ignore"):
            p = np.fmax(p, np.float32(0.0)).astype(np.float32)
            for _ in range(root):
                p = np.sqrt(p).astype(np.float32)
    return cvm.curve_eval(p, table, x0, inv_dx)


def unpack(curves):
    """a TensorCurvesIn struct, or a dict of the same keys, as a dict: in / out are None or (table, x0, inv_dx, root)"""
    if isinstance(curves, dict):
        q = dict(curves)
        q.setdefault("in", None)
        q.setdefault("out", None)
        q.setdefault("in_mask", 7)
        q.setdefault("out_mask", 7)
        for key, d in (("gain", 1.0), ("offset", 0.0)):
            v = np.full(4, d, np.float32)
            given = np.atleast_1d(np.asarray(q.get(key, d), np.float32))
            v[:given.shape[0] if given.shape[0] > 1 else 4] = given
            q[key] = v
        return q

    def one(cv, table):
        return None if cv.n == 0 else (np.array(table[:cv.n], np.float32), float(cv.x0), float(cv.inv_dx), int(cv.root))
    return {"in": one(curves.in_, curves.tables[0]), "out": one(curves.out, curves.tables[1]), "in_mask": int(curves.in_mask),
            "out_mask": int(curves.out_mask), "gain": np.array(list(curves.gain), np.float32), "offset": np.array(list(curves.offset), np.float32)}


def curved_in(chw_values, curves):
    """h: every element of every channel the in-mask names through the in-curve"""
    q = unpack(curves)
    return [root_eval(v, *q["in"]) if (q["in"] is not None and (q["in_mask"] >> k) & 1) else np.asarray(v, np.float32)
            for k, v in enumerate(chw_values)]


def component_w(chw_values, fmt, mix, curves, c):
    """w of every sample of component c, float32, from the image's float32 values (K, H, W)"""
    _, _, cw, ch, _, _ = cm.LAYOUTS[fmt]
    nin, chroma, m, b = tmi.unpack(mix)
    q = unpack(curves)
    assert len(chw_values) == nin
    sw, sh = (cw, ch) if c in (1, 2) else (0, 0)
    g = [tmi.gather(h, sw, sh, chroma) for h in curved_in(chw_values, q)]
    u = tmi.mix_rows(g, m[c], b[c], nin)
    v = root_eval(u, *q["out"]) if (q["out"] is not None and (q["out_mask"] >> c) & 1) else u
    with np.errstate(over="ignore", under="ignore", invalid="ignore"):
        return ((v * q["gain"][c]).astype(np.float32) + q["offset"][c]).astype(np.float32)


def component_samples(chw_values, fmt, bits, mix, curves, c):
    """the integer samples of component c: tensor_in_model's end (rint, 0 unless > 0, the peak where reached)"""
    return tim.samples(component_w(chw_values, fmt, mix, curves, c), 1.0, -0.0, bits)


def frame(img_bits, fmt, bits, mix, curves, dtype="float32", layout="NCHW"):
    """one image's bit patterns, (K, H, W) or (H, W, K) -> the planes of its frame"""
    nc, planar, _, _, _, nbytes = cm.LAYOUTS[fmt]
    img = np.asarray(img_bits)
    chw = tim.element_values(img if layout == "NCHW" else img.transpose(2, 0, 1), dtype)
    word = np.uint8 if nbytes == 1 else np.uint16
    q = unpack(curves)
    comps = [(component_samples(chw, fmt, bits, mix, q, c) << cm.shift(fmt, bits)).astype(word) for c in range(nc)]
    if planar:
        return comps
    return [np.ascontiguousarray(np.stack(comps, -1).reshape(chw.shape[1], chw.shape[2] * nc))]


def frames(tensor_bits, fmt, bits, mix, curves, dtype="float32", layout="NCHW"):
    """(n, ...) bit patterns -> n frames (lists of planes)"""
    q = unpack(curves)
    return [frame(img, fmt, bits, mix, q, dtype, layout) for img in np.asarray(tensor_bits)]


def fill_root(kind, n, lo=0.0, hi=1.0, param=0.0, root=0):
    """htj2k_tensor_curve_fill_root in float64, not rounded: F(y_j ^ (2 ^ root)), y_j = lo + j (hi - lo) / (n - 1)"""
    y = lo + np.arange(n, dtype=np.float64) * (hi - lo) / float(n - 1)
    for _ in range(root):
        y = y * y
    return cvm.function(kind, y, param)


def mix_in_xyz(primaries, scale=1.0):
    """htj2k_tensor_mix_in_xyz in float64: the normalised primary matrix, linear RGB -> linear XYZ, times scale"""
    a = np.array([[x / y, 1.0, (1.0 - x - y) / y] for x, y in cvm.PRIMARIES[primaries]], np.float64).T
    w = np.array([cvm.D65[0] / cvm.D65[1], 1.0, (1.0 - cvm.D65[0] - cvm.D65[1]) / cvm.D65[1]], np.float64)
    return a * np.linalg.solve(a, w)[None, :] * scale


def _torch_curve(x, curve):
    """R in eager torch operations: a clamp and square roots, then the subtraction, the product, a clamp, an index and a
    lerp written out"""
    import torch
    table, x0, inv_dx, root = curve
    t = torch.as_tensor(np.append(table, table[-1]).astype(np.float32), device=x.device)
    n = len(table)
    p = x
    if root:
        p = torch.where(torch.isnan(p), torch.zeros_like(p), torch.clamp(p, min=0.0))
        for _ in range(root):
            p = torch.sqrt(p)
    u = torch.mul(torch.sub(p, x0), inv_dx)
    u = torch.where(torch.isnan(u), torch.zeros_like(u), torch.clamp(u, 0.0, float(n - 1)))
    i = u.to(torch.int64)
    r = torch.sub(u, i.float())
    lo, hi = t[i], t[i + 1]
    return torch.add(lo, torch.mul(r, torch.sub(hi, lo)))


def torch_chain(t, mix, curves, bits, nc, shift=0):
    """the eager chain a caller runs today, for layouts without a chroma shift: t (n, K, H, W) of any float dtype ->
    (n, nc, H, W) int32 sample words: a widening, a curve, the products and sums of the matrix in the definition's order, a
    second curve, a scale and an offset, a round, a clamp and a shift"""
    import torch
    nin, _, m, b = tmi.unpack(mix)
    q = unpack(curves)
    peak = float((1 << bits) - 1)
    f = t.float()
    h = [_torch_curve(f[:, k], q["in"]) if (q["in"] is not None and (q["in_mask"] >> k) & 1) else f[:, k] for k in range(nin)]
    out = []
    for c in range(nc):
        a = torch.mul(h[0], float(m[c][0]))
        for k in range(1, nin):
            a = torch.add(a, torch.mul(h[k], float(m[c][k])))
        u = torch.add(a, float(b[c]))
        v = _torch_curve(u, q["out"]) if (q["out"] is not None and (q["out_mask"] >> c) & 1) else u
        w = torch.add(torch.mul(v, float(q["gain"][c])), float(q["offset"][c]))
        r = torch.round(w)
        s = torch.where(r > 0, torch.clamp(r, max=peak), torch.zeros_like(r))      # NaN fails r > 0
        out.append(s.to(torch.int32) << shift)
    return torch.stack(out, 1)
