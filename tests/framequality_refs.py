"""Float64 yardstick of the frame-quality operator (sin_inn_amd.flowsynth.quality), its test inputs and its error budget.

    reference(pred, target)      the definition restated in numpy float64: every window summed directly under the 2-D weights
                                 w[i] w[j], nothing separable, nothing shared with `flowsynth.quality_composed`
    budget(pred, target)         per window, a bound on |fp32 result - float64 result| derived from the roundings of the operations
    inputs(kind, b, c, h, w)     the input families of the tests;  SHAPES: the shapes, from the kernel's tile
    defect(name, pred, target)   the definition with one seeded mistake, for the tests that show the budget tells them apart

The budget.  u = 2^-24.  A filtered moment is two 11-term dot products with weights rounded to fp32; a dot product of n terms in any
order, fused or not, is within gamma_n sum |g_k x_k| of the exact one (gamma_n = n u / (1 - n u)), and the weight's own rounding adds
one u: each pass is within gamma_12, both within gamma_24 of the filtered |x| (the second pass also filters the first one's error:
(1 + gamma_12)^2 - 1 <= gamma_24).  The second moments filter a product that was itself rounded: gamma_25.  From there every
operation of the formula is followed with `Err`: a value known to within e, through +, -, *, / with the result's own rounding
u (|v| + e) added each time.  The subtraction E[pp] - mu_p^2 keeps the ABSOLUTE errors of both terms while the difference may be
small against them -- that is the cancellation -- and the sum s_p + s_t + C2 it feeds is at least of the size of C2 = 9e-4, which is what
keeps the quotient bounded where the variance vanishes.  Nothing here is fitted to what any implementation returns.
"""
import functools
import os
import re
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

U = 2.0 ** -24
WIN, SIGMA = 11, 1.5
C1, C2 = 0.01 ** 2, 0.03 ** 2
KINDS = ('texture', 'noise', 'constant', 'self', 'one pixel')


def tile():
    """(TY, TX): the kernel's window tile, read from the source"""
    src = open(os.path.join(ROOT, 'sin-inn_amd', 'csrc', 'framequality.hip')).read()
    m = re.search(r'constexpr int FQ_TY = (\d+), FQ_TX = (\d+);', src)
    return int(m.group(1)), int(m.group(2))


def shapes():
    """[(B, C, H, W)]: one window and one more each way; an exact tile and a one-window sliver each way; 2 x 2 ragged tiles"""
    ty, tx = tile()
    return [(1, 3, 11, 11), (3, 1, 11, 12), (1, 1, 12, 11),
            (1, 1, ty + 10, tx + 10), (3, 3, ty + 11, tx + 10), (1, 3, ty + 10, tx + 11), (1, 1, ty + 11, tx + 11),
            (3, 3, 2 * ty + 10 - 3, 2 * tx + 10 - 5)]


def window(sigma=SIGMA, normalise=True):
    g = np.exp(-(np.arange(WIN, dtype=np.float64) - WIN // 2) ** 2 / (2 * sigma * sigma))
    return g / g.sum() if normalise else g


def to_bytes32(x):
    """the u8 rule in fp32, as the kernel evaluates it: clamp(round-half-even(fl32(255 x)), 0, 255), as a float32 array of bytes"""
    x = np.asarray(x, dtype=np.float32)
    return np.clip(np.rint(x * np.float32(255)), 0, 255).astype(np.float32)


def _moments(x, w2):
    """sum over the 11 x 11 window of w2 * x at every valid position: (..., H, W) -> (..., H - 10, W - 10), summed directly"""
    v = np.lib.stride_tricks.sliding_window_view(x, (WIN, WIN), axis=(-2, -1))
    return np.einsum('...ij,ij->...', v, w2, optimize=False)


def ssim_map64(p, t, w2=None, c1=C1, c2=C2):
    w2 = np.outer(window(), window()) if w2 is None else w2
    mp, mt = _moments(p, w2), _moments(t, w2)
    s_p, s_t, s_pt = _moments(p * p, w2) - mp * mp, _moments(t * t, w2) - mt * mt, _moments(p * t, w2) - mp * mt
    return ((2 * mp * mt + c1) * (2 * s_pt + c2)) / ((mp * mp + mt * mt + c1) * (s_p + s_t + c2))


def reference(pred, target, quantize=False):
    """dict(sqerr, mse, psnr, ssim: (B,) float64; map: (B, C, H - 10, W - 10) float64) of fp32 frames (B, C, H, W).  Float mode: the
    float64 value of the definition on the given fp32 numbers.  Quantised mode: on the bytes of the fp32 rule; sqerr is their integer
    sum, SSIM is taken on fl32(byte / 255) as the definition says."""
    p32, t32 = (np.asarray(a.detach().cpu().numpy() if torch.is_tensor(a) else a, dtype=np.float32) for a in (pred, target))
    b = p32.shape[0]
    n = p32[0].size
    if quantize:
        bp, bt = to_bytes32(p32), to_bytes32(t32)
        sq = ((bp.astype(np.int64) - bt.astype(np.int64)) ** 2).reshape(b, -1).sum(1)
        sqerr = sq.astype(np.float64)
        mse = sqerr / (65025.0 * n)
        p, t = (bp / np.float32(255)).astype(np.float64), (bt / np.float32(255)).astype(np.float64)
    else:
        p, t = p32.astype(np.float64), t32.astype(np.float64)
        sqerr = ((p - t) ** 2).reshape(b, -1).sum(1)
        mse = sqerr / n
    with np.errstate(divide='ignore'):
        psnr = np.where(mse == 0, np.inf, 10 * np.log10(1 / np.where(mse == 0, 1.0, mse)))
    smap = ssim_map64(p, t)
    return dict(sqerr=sqerr, mse=mse, psnr=psnr, ssim=smap.reshape(b, -1).mean(1), map=smap, p=p, t=t)


# ---- the budget ----

def gamma(n):
    return n * U / (1 - n * U)


class Err:
    """a float64 value v that an fp32 computation knows to within e"""

    def __init__(self, v, e):
        self.v, self.e = v, e

    @staticmethod
    def _rounded(v, e0):
        return Err(v, e0 + U * (np.abs(v) + e0))

    def __add__(self, o):
        return Err._rounded(self.v + o.v, self.e + o.e)

    def __sub__(self, o):
        return Err._rounded(self.v - o.v, self.e + o.e)

    def __mul__(self, o):
        return Err._rounded(self.v * o.v, np.abs(self.v) * o.e + np.abs(o.v) * self.e + self.e * o.e)

    def __truediv__(self, o):
        assert np.all(np.abs(o.v) > o.e), 'the divisor may vanish within its error'
        q = self.v / o.v
        return Err._rounded(q, (self.e + np.abs(q) * o.e) / (np.abs(o.v) - o.e))

    def twice(self):
        return Err(2 * self.v, 2 * self.e)          # exact in binary


def budget(p, t):
    """(B, C, H - 10, W - 10): the bound on |ssim_map in fp32 - ssim_map in float64| for float64 frames p, t (the values the fp32
    computation starts from, exactly)"""
    w2 = np.outer(window(), window())
    ap, at = np.abs(p), np.abs(t)
    mp, mt = Err(_moments(p, w2), gamma(24) * _moments(ap, w2)), Err(_moments(t, w2), gamma(24) * _moments(at, w2))
    epp = Err(_moments(p * p, w2), gamma(25) * _moments(p * p, w2))
    ett = Err(_moments(t * t, w2), gamma(25) * _moments(t * t, w2))
    ept = Err(_moments(p * t, w2), gamma(25) * _moments(ap * at, w2))
    c1, c2 = Err(C1, U * C1), Err(C2, U * C2)
    mpp, mtt, mpt = mp * mp, mt * mt, mp * mt
    s_p, s_t, s_pt = epp - mpp, ett - mtt, ept - mpt
    s = ((mpt.twice() + c1) * (s_pt.twice() + c2)) / ((mpp + mtt + c1) * (s_p + s_t + c2))
    return s.e


# ---- inputs ----

def inputs(kind, b, c, h, w, seed=0):
    """(pred, target): fp32 (B, C, H, W) on the host"""
    from sin_inn_amd import flowdata
    g = torch.Generator().manual_seed(1000 * seed + 17 * h + w + 7 * b + c)
    noise = torch.rand(b, c, h, w, generator=g)
    if kind == 'texture':
        yy, xx = torch.meshgrid(torch.arange(h, dtype=torch.float64), torch.arange(w, dtype=torch.float64), indexing='ij')
        target = torch.stack([flowdata.texture(xx, yy, seed + n)[:c] for n in range(b)])
        pred = torch.stack([flowdata.texture(xx + 0.3, yy - 0.2, seed + n)[:c] for n in range(b)])
        return pred.float(), target.float()
    if kind == 'noise':
        return torch.rand(b, c, h, w, generator=g), noise
    if kind == 'constant':
        return torch.full((b, c, h, w), 0.5), noise
    if kind == 'self':
        return noise.clone(), noise
    if kind == 'one pixel':
        pred = noise.clone()
        pred[b - 1, c - 1, h // 2, w - 6] += 0.25
        return pred, noise
    raise KeyError(kind)


@functools.lru_cache(maxsize=None)
def case(kind, shape, quantize=False):
    """(pred, target, reference dict, budget map) of one input family at one shape: computed once, shared, not to be modified"""
    pred, target = inputs(kind, *shape)
    ref = reference(pred, target, quantize)
    return pred, target, ref, budget(ref['p'], ref['t'])


# ---- seeded defects: the definition with one mistake, in float64 ----

DEFECTS = ('shifted window', 'sigma 1.4', 'unnormalised window', 'C2 swapped for C1', 'halo counted twice', 'dropped last row')


def defect(name, pred, target):
    """dict(sqerr, ssim, map) of the float-mode definition with the named mistake; `map` keeps the reference's shape where it can"""
    ref = reference(pred, target)
    p, t = ref['p'], ref['t']
    out = dict(sqerr=ref['sqerr'], map=ref['map'])
    if name == 'shifted window':                       # every window starts one pixel to the right (the last column wraps)
        out['map'] = ssim_map64(np.roll(p, -1, axis=-1), np.roll(t, -1, axis=-1))
    elif name == 'sigma 1.4':
        out['map'] = ssim_map64(p, t, np.outer(window(1.4), window(1.4)))
    elif name == 'unnormalised window':
        out['map'] = ssim_map64(p, t, np.outer(window(normalise=False), window(normalise=False)))
    elif name == 'C2 swapped for C1':
        out['map'] = ssim_map64(p, t, c1=C2, c2=C1)
    elif name == 'halo counted twice':                 # every tile also counts its 10-pixel halo: the strips between tiles twice
        ty, tx = tile()
        h, w = p.shape[-2:]
        d2 = (p - t) ** 2
        extra = np.zeros(p.shape[0])
        for y0 in range(ty, h - 10, ty):
            extra += d2[..., y0:y0 + 10, :].reshape(p.shape[0], -1).sum(1)
        for x0 in range(tx, w - 10, tx):
            extra += d2[..., :, x0:x0 + 10].reshape(p.shape[0], -1).sum(1)
        out['sqerr'] = ref['sqerr'] + extra
    elif name == 'dropped last row':
        out['map'] = ref['map'][..., :-1, :]
    else:
        raise KeyError(name)
    out['ssim'] = out['map'].reshape(p.shape[0], -1).mean(1)
    return out
