"""TEST INFRASTRUCTURE: float64 references, cases and the exclusion rule of the frame-synthesis tests (tests/test_flowsynth_host.py,
tests/test_gpu_flowsynth.py).

    composed64     `sin_inn_amd.flowsynth.compose_from` (the definition `flowsynth.composed` evaluates) on float64 CPU tensors, with the
                   warp of oracle/sininn_oracle.py and the summation splat of oracle/flow_oracle.py
    stepwise64     the same frames written out step by step from `oracle.flow_oracle.function_softsplat(.., 'softmax')`, the oracle's
                   warp and torch arithmetic: what the host test holds composed64 against
    CASES          the shapes and flows of the GPU test;  `case(name)` builds one
    excluded       output pixels whose hole decision may differ between fp32 and float64 (see there)
"""
import os
import re

import torch

from oracle import flow_oracle as FO
from oracle import sininn_oracle as SO

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
F64 = torch.float64
ZONE = 1e-4                   # a landing coordinate this close to an integer may fall on the other side of it in fp32
MAX_EXCLUDED = 0.005          # share of a case's output pixels the rule may leave out


def warp64(img, flow):
    """Resample2d; on an axis of length 1 the sample lies outside the frame (sin_inn_amd/flowsynth.py)"""
    if img.shape[-2] < 2 or img.shape[-1] < 2:
        return torch.zeros_like(img)
    return SO.flow_warp(img, flow)


def metric64(target, img, flow):
    return SO.photometric_l1(target, warp64(img, flow))


def taus32(taus):
    """the times as the kernel sees them: rounded to fp32, then exact in float64"""
    return torch.tensor([float(t) for t in taus], dtype=torch.float32).to(F64).tolist()


def composed64(frame1, frame2, flow12, flow21, taus):
    from sin_inn_amd import flowsynth
    a = [t.detach().cpu().to(F64) for t in (frame1, frame2, flow12, flow21)]
    return flowsynth.compose_from(*a, taus32(taus), metric64, FO.softsplat_sum)


def stepwise64(frame1, frame2, flow12, flow21, taus):
    i0, i1, f01, f10 = (t.detach().cpu().to(F64) for t in (frame1, frame2, flow12, flow21))
    z0 = -20 * (i0 - warp64(i1, f01)).abs().mean(1, keepdim=True)
    z1 = -20 * (i1 - warp64(i0, f10)).abs().mean(1, keepdim=True)
    frames = []
    for tau in taus32(taus):
        s0 = FO.function_softsplat(i0, tau * f01, z0, 'softmax')
        s1 = FO.function_softsplat(i1, (1 - tau) * f10, z1, 'softmax')
        n0 = FO.softsplat_sum(z0.exp(), tau * f01)
        n1 = FO.softsplat_sum(z1.exp(), (1 - tau) * f10)
        a0, a1 = (1 - tau) * (n0 != 0), tau * (n1 != 0)
        out = (1 - tau) * i0 + tau * i1
        both = (a0 + a1) != 0
        blend = (a0 * s0 + a1 * s1) / torch.where(both, a0 + a1, torch.ones_like(a0))
        frames.append(torch.where(both, blend, out))
    return torch.stack(frames, 1)


def hole_maps(frame1, frame2, flow12, flow21, taus):
    """(N0 == 0, N1 == 0), each (B, K, H, W) bool, in float64"""
    i0, i1, f01, f10 = (t.detach().cpu().to(F64) for t in (frame1, frame2, flow12, flow21))
    e0 = (-20 * metric64(i0, i1, f01)).exp()
    e1 = (-20 * metric64(i1, i0, f10)).exp()
    h0 = torch.stack([FO.softsplat_sum(e0, t * f01)[:, 0] == 0 for t in taus32(taus)], 1)
    h1 = torch.stack([FO.softsplat_sum(e1, (1 - t) * f10)[:, 0] == 0 for t in taus32(taus)], 1)
    return h0, h1


def excluded(flow12, flow21, taus):
    """(B, K, H, W) bool.  A hole decision is discontinuous: a tap whose bilinear weight is exactly zero in float64 may be non-zero in
    fp32 once tau * F has been rounded.  Left out are the output pixels that get such a marginal tap: for a source whose float64 landing
    coordinate x + tau F lies within ZONE of an integer n on an axis -- and is not the same number in fp32, where nothing can differ --
    the pixels at n - 1 and n + 1 on that axis (its taps of weight below ZONE in either precision), on the rows / columns of its taps on
    the other axis; if both axes are marginal, the 3 x 3 block round the landing point."""
    b, _, h, w = flow12.shape
    ts = taus32(taus)
    out = torch.zeros(b, len(ts), h, w, dtype=torch.bool)
    ys, xs = torch.meshgrid(torch.arange(h, dtype=F64), torch.arange(w, dtype=F64), indexing='ij')
    for k, tau in enumerate(ts):
        for flow, t in ((flow12, tau), (flow21, 1 - tau)):
            flow = flow.detach().cpu().to(torch.float32)
            t32 = torch.tensor(t, dtype=torch.float32)                       # 1 - tau is rounded to fp32 as the kernel rounds it
            o64 = [xs + float(t32) * flow[:, 0].to(F64), ys + float(t32) * flow[:, 1].to(F64)]
            o32 = [xs.float() + t32 * flow[:, 0], ys.float() + t32 * flow[:, 1]]
            near = [((o - o.round()).abs() < ZONE) & (o != p.to(F64)) for o, p in zip(o64, o32)]
            for bb, yy, xx in (near[0] | near[1]).nonzero().tolist():
                cols, rows = [], []
                for axis, lst in ((0, cols), (1, rows)):
                    o = float(o64[axis][bb, yy, xx])
                    if near[axis][bb, yy, xx]:
                        n = round(o)
                        lst += [n - 1, n + 1] + ([n] if near[1 - axis][bb, yy, xx] else [])
                    else:
                        n = int(torch.floor(torch.tensor(o)))
                        lst += [n, n + 1]
                for r in rows:
                    for c in cols:
                        if 0 <= r < h and 0 <= c < w:
                            out[bb, k, r, c] = True
    return out


def scatter_block_cap():
    """FS_SCATTER_MAX_BLOCKS of csrc/flowsynth.hip, read from the source with the line that applies it"""
    src = open(os.path.join(ROOT, 'sin-inn_amd', 'csrc', 'flowsynth.hip')).read()
    m = re.search(r'constexpr int FS_SCATTER_MAX_BLOCKS = (\d+);', src)
    assert m and 'ntiles < FS_SCATTER_MAX_BLOCKS ? ntiles : FS_SCATTER_MAX_BLOCKS' in src
    tile = re.search(r'constexpr int FS_TX = (\d+), FS_TY = (\d+);', src)
    return int(m.group(1)), int(tile.group(1)), int(tile.group(2))


def smooth_field(g, b, c, h, w, grid=(3, 4)):
    """(b, c, h, w) in [0, 1): uniform noise on a coarse grid, enlarged bilinearly"""
    coarse = torch.rand(b, c, *grid, generator=g)
    if h == 1 and w == 1:
        return coarse[:, :, :1, :1].contiguous()
    return torch.nn.functional.interpolate(coarse, size=(h, w), mode='bilinear', align_corners=True).contiguous()


def random_inputs(seed, b, c, h, w, amplitude=6.0):
    """frames in [0, 1] and smooth flows of up to `amplitude` pixels, fp32, from Generator(seed)"""
    g = torch.Generator().manual_seed(seed)
    frames = [smooth_field(g, b, c, h, w, grid=(5, 7)) for _ in range(2)]
    flows = [(smooth_field(g, b, 2, h, w) * 2 - 1) * amplitude for _ in range(2)]
    return frames + flows


def _quarter(t):
    return (t * 4).round() / 4


def constructed(kind, h=12, w=16, c=3, seed=1):
    """Flows that are exact multiples of 1/4, for tau in {0, 1/2, 1}: every landing coordinate is exact in fp32 and float64.
    converge: the columns contract onto the middle, four sources per target column at tau = 1/2 (the softmax weights decide).
    diverge:  frame1's columns spread apart (holes in its splat only), frame2 does not move.
    band:     the sources of rows 4..7 of both frames leave the frame, the others stay: nothing lands on the band at tau = 1/2."""
    g = torch.Generator().manual_seed(seed)
    i0, i1 = smooth_field(g, 1, c, h, w, grid=(5, 7)), smooth_field(g, 1, c, h, w, grid=(5, 7))
    ys, xs = torch.meshgrid(torch.arange(h, dtype=torch.float32), torch.arange(w, dtype=torch.float32), indexing='ij')
    f01, f10 = torch.zeros(1, 2, h, w), torch.zeros(1, 2, h, w)
    mid = w // 2
    if kind == 'converge':
        f01[0, 0], f10[0, 0] = (mid - xs) * 1.5, (mid - xs) * 0.5
        f01[0, 1] = _quarter((ys - h // 2) * 0.25)
    elif kind == 'diverge':
        f01[0, 0] = (xs - mid) * 2.0
    elif kind == 'band':
        f01[0, 1, 4:8], f10[0, 1, 4:8] = 8.0 * h, 8.0 * h
        f01[0, 0, :4], f10[0, 0, 8:] = 0.25, -0.5
    else:
        raise KeyError(kind)
    assert bool(((f01 * 4) == (f01 * 4).round()).all()) and bool(((f10 * 4) == (f10 * 4).round()).all())
    return [i0, i1, f01.contiguous(), f10.contiguous()]


def past_cap_shape():
    """(h, w) of one sample whose 2 * tiles exceed the scatter kernel's block cap, ragged in both directions"""
    cap, tx, ty = scatter_block_cap()
    tiles_x = 32
    tiles_y = cap // (2 * tiles_x) + 1
    return tiles_y * ty - 7, tiles_x * tx - 24


# name -> (seed, b, c, h, w, taus); h = w = None: past_cap_shape().  The seeds are those under which `excluded` stays below
# MAX_EXCLUDED (tests/test_flowsynth_host.py checks it on the CPU).
CASES = {
    '1x1': (0, 1, 3, 1, 1, (0.5,)),
    '13x37': (0, 2, 3, 13, 37, (0.0, 0.3, 1.0)),
    '5x1031': (0, 1, 3, 5, 1031, (0.25, 0.875)),
    'past cap': (0, 1, 3, None, None, (0.4,)),
    '13x37 grey': (0, 2, 1, 13, 37, (0.0, 0.7, 1.0)),
}
CONSTRUCTED = ('converge', 'diverge', 'band')
CONSTRUCTED_TAUS = (0.0, 0.5, 1.0)


def case(name):
    """(frame1, frame2, flow12, flow21, taus), fp32 on the CPU"""
    if name in CONSTRUCTED:
        return constructed(name) + [CONSTRUCTED_TAUS]
    seed, b, c, h, w, taus = CASES[name]
    if h is None:
        h, w = past_cap_shape()
    if name == '1x1':
        g = torch.Generator().manual_seed(seed)
        i0, i1 = torch.rand(1, c, 1, 1, generator=g), torch.rand(1, c, 1, 1, generator=g)
        # frame1 lands at (0.3, -0.2): the taps above the frame are dropped, the others clamp to the one pixel; frame2 leaves the frame
        return [i0, i1, torch.tensor([0.6, -0.4]).reshape(1, 2, 1, 1), torch.tensor([5.0, 5.0]).reshape(1, 2, 1, 1), taus]
    return random_inputs(seed, b, c, h, w) + [taus]
