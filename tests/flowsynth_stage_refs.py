"""TEST INFRASTRUCTURE: the frame synthesis (csrc/flowsynth.hip) checked stage by stage from the accumulator a call leaves
in its workspace (tests/test_flowsynth_stages_host.py, tests/test_gpu_flowsynth_stages.py).  Plain numpy; nothing here calls the
package's operators.

    case(name), CASES, EXACT_FLOWS   the inputs: (i0, i1, f01, f10, taus) as fp32 numpy arrays
    stage1(case, acc)      the tau = 0 / tau = 1 planes: w = exp(Z) against float64 under a derived relative budget, I * w == fl32(I * w)
    stage2(case, acc)      every accumulator element against the exact sum of fl32(I * w_k) * tap32, budget (n + C_SUM) 2^-24 A
    stage3(case, acc, out, u8)   the blend restated in numpy fp32 on the accumulator of the call: bitwise; the bytes on the host
    exact_check(case, acc)       zero frames, quarter-pixel flows and times: the N planes equal float64 exactly
    model(case, ...)       the kernel's arithmetic one rounding at a time in numpy fp32, with the lane merges of a 64-lane wave, three
                           orders of summation, the contractible steps fused or not, and one seeded defect at a time (DEFECTS)

u = 2^-24.  Stage 1 (per source pixel, relative to w; all bounds first order with u replaced by U1 = u (1 + 2^-10), which covers the
products of errors: fewer than 2^10 roundings meet in one value).  With s = x + fx, p = 2 s / (W - 1), g = p - 1 the kernel forms
fl(s), / (W - 1), * 2 (exact), - 1, + 1, * W, - 1, * 0.5 (exact):

    err(fl s) = u |s|;  err(/) = err / (W - 1) + u |s| / (W - 1): together u |p| after the doubling 2 u |p|;  err(g) = 2 u |p| + u |g|
    err(g + 1) = 3 u |p| + u |g|;   err(* W) = W u (4 |p| + |g|);   err(- 1) adds u |p W - 1|  (none if the two are contracted)
    d_ix = u / 2 (W (4 |p| + |g|) + |p W - 1|),   d_iy likewise with H

The divisions are IEEE (v_div_scale / v_div_fixup in the code object, hipcc's default).  ix - floor(ix) is exact; 1 - that is one
rounding of a value in [0, 1].  The zero-padded bilinear surface is continuous and piecewise bilinear, so a coordinate error d moves the
sample by at most d times the largest difference of neighbouring taps in the cells it may cross: Sx, Sy are taken over the 4 x 4 taps
round the float64 cell (the local |t01 - t00|, |t11 - t10|, .. and those of the adjoining cells, d being far below one pixel).

    e_c = d_ix Sx_c + d_iy Sy_c                                                   the coordinate
        + 5 u sum |t_ij| wy_i wx_j + 2 u max |t_ij|                               two products and up to three adds per term; 1 - wx1, 1 - wy1
        + u |v_c - warped_c|                                                      the subtraction
    E(l1) = sum_c e_c + (C - 1) u l1;   E(mean) = E(l1) / C + u mean;   E(z) = 20 E(mean) + u |z|      (z = -20 mean <= 0)
    |w - w64| / w64 <= E(z) + EXPF_ULPS * 2^-23

Stage 2 (per accumulator element).  The terms v * tap are exact in float64 (24 x 24 bits); n of them are non-zero, A = sum |term|.
Each product is rounded once (u |term|, or not at all where it is fused into the add that follows); the n terms are then added in
n - 1 adds, in any order, merged in lanes or in the atomics, each within u of a partial sum that is at most A (1 + n u): n u A to first
order, the second-order part (n - 1) n u^2 A is below u A for n <= 4096.  C_SUM = 1.
"""
import math
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import flowsynth_refs as R  # noqa: E402  (smooth_field, scatter_block_cap: no operator of the package)

F32, F64 = np.float32, np.float64
U = 2.0 ** -24
U1 = U * (1 + 2.0 ** -10)
C_SUM = 1
# expf: no bound for it in the documentation or headers shipped with the toolchain, so it is measured (tools/expf_ulp.hip on the
# arguments `expf_arguments()` collects from CASES): worst 0.81 ulp on an MI355X -> allowance ceil(2 * 0.81) = 2 ulp
EXPF_ULPS = 2
H9, W33 = 9, 33
QUARTER_TAUS = (0.0, 0.25, 0.5, 0.75, 1.0)


# ---- cases ------------------------------------------------------------------------------------------------------------------------

def _frames(seed, b, c, h, w):
    """two frames in [0.05, 0.95]: smooth, every value and every product with w >= e^-20 normal"""
    g = torch.Generator().manual_seed(seed)
    return [(0.05 + 0.9 * R.smooth_field(g, b, c, h, w, grid=(5, 7))).numpy().astype(F32) for _ in range(2)]


def _smooth_flows(seed, b, h, w, amplitude=6.0):
    g = torch.Generator().manual_seed(seed + 1000)
    return [((R.smooth_field(g, b, 2, h, w) * 2 - 1) * amplitude).numpy().astype(F32) for _ in range(2)]


def _grid(h=H9, w=W33):
    ys, xs = np.meshgrid(np.arange(h, dtype=F32), np.arange(w, dtype=F32), indexing='ij')
    return ys, xs


NONFINITE_SOURCES = (
    # (flow, y, x, fx, fy): at the tile seam x = 31 | 32, the block seam y = 7 | 8, the wave-pair seam y = 1 | 2, beside live neighbours
    (0, 1, 31, math.nan, None), (0, 2, 32, None, math.inf), (0, 7, 0, -math.inf, -math.inf), (0, 8, 5, 3e9, None),
    (0, 0, 0, None, -3e9), (0, 4, 16, math.nan, math.nan), (0, 1, 5, None, math.nan), (0, 8, 32, math.inf, None),
    (1, 2, 31, math.inf, None), (1, 7, 32, None, math.nan), (1, 8, 31, -3e9, 3e9), (1, 0, 32, math.nan, -math.inf),
    (1, 5, 7, 3e9, None), (1, 3, 0, None, -math.inf),
    # a live source landing at (-0.5, 0.25) at tau = 1/2 with a NaN source on its right: nwx = -1, nwy = 0 against the zeroed taps of
    # a lane that has none; and one landing at (0.25, -0.75) with an Inf source below it: nwx = 0, nwy = -1
    (0, 3, 10, -21.0, -5.5), (0, 3, 11, math.nan, None), (0, 4, 20, -39.5, -9.5), (0, 5, 20, None, math.inf),
)


def quarter_flows(kind):
    """(f01, f10), (B, 2, 9, 33): every component a multiple of 1/4"""
    ys, xs = _grid()
    b = 4 if kind == 'out of frame' else 1
    f01, f10 = np.zeros((b, 2, H9, W33), F32), np.zeros((b, 2, H9, W33), F32)
    if kind in ('shift', 'non-finite'):                       # every lane merges
        f01[:, 0], f01[:, 1], f10[:, 0], f10[:, 1] = 1.25, -0.75, -2.5, 0.25
    elif kind == 'random':                    # merges by coincidence only; neighbours often differ in exactly one of nwx, nwy
        rng = np.random.default_rng(5)
        f01[:] = rng.integers(-24, 25, f01.shape) / 4
        f10[:] = rng.integers(-24, 25, f10.shape) / 4
        # lane 31 of a wave and its lane 32 (the first pixel of the next row) land side by side at t = 1: (21.5, 2.25), (22.5, 2.25)
        f01[0, :, 0, 31], f01[0, :, 1, 0] = (-9.5, 2.25), (22.5, 1.25)
        f10[0, :, 4, 31], f10[0, :, 5, 0] = (-9.5, -1.75), (22.5, -2.75)
    elif kind == 'fold':                      # at t = 1/2 every source of a row lands on column 16
        f01[0, 0], f01[0, 1] = 2 * (16 - xs), 0.25
        f10[0, 0], f10[0, 1] = 16 - xs, -0.5
    elif kind == 'shear':                     # nwy steps inside a row while nwx_r == nwx + 1: give_h must refuse there
        f01[0, 0], f01[0, 1] = 0.5, 0.25 * xs
        f10[0, 0], f10[0, 1] = 0.25 * ys, -0.5 * xs
    elif kind == 'out of frame':              # one sample per side: a row / column leaves whole, the next two straddle the border
        for f in (f01, f10):
            f[0, 1, 0], f[0, 1, 1:3] = -8.0, -2.5
            f[1, 1, 8], f[1, 1, 6:8] = 8.0, 2.5
            f[2, 0, :, 0], f[2, 0, :, 1:3] = -8.0, -2.5
            f[3, 0, :, 32], f[3, 0, :, 30:32] = 8.0, 2.5
    else:
        raise KeyError(kind)
    if kind == 'non-finite':
        for which, y, x, fx, fy in NONFINITE_SOURCES:
            f = (f01, f10)[which]
            if fx is not None:
                f[0, 0, y, x] = fx
            if fy is not None:
                f[0, 1, y, x] = fy
    return f01, f10


EXACT_FLOWS = ('shift', 'random', 'fold', 'shear', 'out of frame', 'non-finite')

# name -> (seed, B, C, H, W, taus, flows);  flows: 'smooth' or a kind of quarter_flows
CASES = {
    '9x33': (1, 2, 3, H9, W33, (0.0, 0.1, 0.3, 0.7, 1.0), 'smooth'),
    '9x33 grey': (2, 2, 1, H9, W33, (0.0, 0.1, 0.3, 0.7, 1.0), 'smooth'),
    '1x1': (3, 1, 3, 1, 1, (0.0, 0.4, 1.0), 'smooth'),
    '1x40': (4, 1, 3, 1, 40, (0.0, 0.4, 1.0), 'smooth'),
    '12x1': (5, 1, 3, 12, 1, (0.0, 0.4, 1.0), 'smooth'),
    'past cap': (6, 257, 3, H9, W33, (0.0, 0.4, 1.0), 'smooth'),
    'K=64': (7, 1, 3, H9, W33, tuple(j / 63 for j in range(64)), 'smooth'),
    'shift': (8, 1, 3, H9, W33, QUARTER_TAUS, 'shift'),
    'random': (9, 1, 3, H9, W33, QUARTER_TAUS, 'random'),
    'fold': (10, 1, 3, H9, W33, QUARTER_TAUS, 'fold'),
    'shear': (11, 1, 3, H9, W33, QUARTER_TAUS, 'shear'),
    'out of frame': (12, 4, 3, H9, W33, QUARTER_TAUS, 'out of frame'),
    'non-finite': (13, 1, 3, H9, W33, QUARTER_TAUS, 'non-finite'),
}


def case(name, zero_frames=False):
    """(i0, i1, f01, f10, taus): fp32 arrays and the times as a tuple"""
    seed, b, c, h, w, taus, flows = CASES[name]
    i0, i1 = _frames(seed, b, c, h, w)
    if zero_frames:
        i0, i1 = np.zeros_like(i0), np.zeros_like(i1)
    f01, f10 = _smooth_flows(seed, b, h, w, amplitude=min(6.0, max(h, w) / 2)) if flows == 'smooth' else quarter_flows(flows)
    assert f01.shape == (b, 2, h, w)
    return i0, i1, f01, f10, taus


def tau32(taus):
    return np.asarray([float(t) for t in taus], dtype=F32)


def end_times(taus):
    t = tau32(taus)
    k0, k1 = np.flatnonzero(t == 0), np.flatnonzero(t == 1)
    assert len(k0) and len(k1), 'every case has the times 0 and 1'
    return int(k0[0]), int(k1[0])


def tile_counts(b, h, w):
    cap, tx, ty = R.scatter_block_cap()
    return (w + tx - 1) // tx, (h + ty - 1) // ty, 2 * b * ((w + tx - 1) // tx) * ((h + ty - 1) // ty), cap


# ---- the reproducible part: landing coordinates and tap weights in fp32 -----------------------------------------------------------

def landing32(t, fx, fy, fused=False):
    """ox = x + fl(t * fx), oy = y + fl(t * fy) in fp32; `fused`: the seeded defect of one rounding for both steps"""
    h, w = fx.shape[-2:]
    ys, xs = _grid(h, w)
    with np.errstate(all='ignore'):
        if fused:
            return (F64(t) * fx.astype(F64) + xs).astype(F32), (F64(t) * fy.astype(F64) + ys).astype(F32)
        return xs + F32(t) * fx, ys + F32(t) * fy


def taps32(ox, oy, h, w):
    """splat_taps behind the kernel's guard: (any, nwx, nwy, [nw, ne, sw, se] fp32, [vnw, vne, vsw, vse]); all zero where not `any`"""
    with np.errstate(all='ignore'):
        ok = np.isfinite(ox) & np.isfinite(oy) & (np.abs(ox) < F32(1e9)) & (np.abs(oy) < F32(1e9))
        ox, oy = np.where(ok, ox, F32(0)), np.where(ok, oy, F32(0))
        flx, fly = np.floor(ox), np.floor(oy)
        nwx, nwy = flx.astype(np.int64), fly.astype(np.int64)
        sex, sey = (nwx + 1).astype(F32), (nwy + 1).astype(F32)
        wts = [(sex - ox) * (sey - oy), (ox - flx) * (sey - oy), (sex - ox) * (oy - fly), (ox - flx) * (oy - fly)]
    x0, x1 = (nwx >= 0) & (nwx < w), (nwx + 1 >= 0) & (nwx + 1 < w)
    y0, y1 = (nwy >= 0) & (nwy < h), (nwy + 1 >= 0) & (nwy + 1 < h)
    val = [x0 & y0, x1 & y0, x0 & y1, x1 & y1]
    assert all(t.dtype == F32 for t in wts)
    return ok, np.where(ok, nwx, 0), np.where(ok, nwy, 0), [np.where(ok, t, F32(0)) for t in wts], [v & ok for v in val]


TAP_OFFSETS = ((0, 0), (0, 1), (1, 0), (1, 1))           # (dy, dx) of nw, ne, sw, se


def side_time(taus, k, side):
    t = tau32(taus)[k]
    return F32(1) - t if side else t


# ---- stage 1 ------------------------------------------------------------------------------------------------------------------------

def w_reference(src, oth, flow):
    """float64 w = exp(-20 mean_c |src - warp(oth, flow)|) per source pixel and its relative budget (module text): (B, H, W) each"""
    b, c, h, w = src.shape
    v = src.astype(F64)
    if h < 2 or w < 2:
        warped, e_c = np.zeros_like(v), np.zeros_like(v)
    else:
        ys, xs = np.meshgrid(np.arange(h, dtype=F64), np.arange(w, dtype=F64), indexing='ij')
        with np.errstate(all='ignore'):
            fx, fy = flow[:, 0].astype(F64), flow[:, 1].astype(F64)
            px, py = 2 * (xs + fx) / (w - 1), 2 * (ys + fy) / (h - 1)
            ix, iy = (px * w - 1) / 2, (py * h - 1) / 2
            bad = ~(np.abs(ix) < 1e9) | ~(np.abs(iy) < 1e9)            # NaN, Inf and the kernel's guard: the sample is 0
            assert not bool(((np.abs(np.abs(ix) - 1e9) < 1e3) | (np.abs(np.abs(iy) - 1e9) < 1e3)).any()), 'a coordinate at the guard'
            d_ix = U1 / 2 * (w * (4 * np.abs(px) + np.abs(px - 1)) + np.abs(px * w - 1))
            d_iy = U1 / 2 * (h * (4 * np.abs(py) + np.abs(py - 1)) + np.abs(py * h - 1))
        ix, iy, d_ix, d_iy = (np.where(bad, 0.0, a) for a in (ix, iy, d_ix, d_iy))
        assert float(d_ix.max()) < 0.01 and float(d_iy.max()) < 0.01
        x0 = np.clip(np.floor(ix), -2, w).astype(np.int64)
        y0 = np.clip(np.floor(iy), -2, h).astype(np.int64)
        wx1, wy1 = np.clip(ix - x0, 0, 1), np.clip(iy - y0, 0, 1)      # clipped cells hold zeros only
        pad = np.pad(oth.astype(F64), ((0, 0), (0, 0), (3, 3), (3, 3)))
        bi = np.arange(b)[:, None, None, None]
        ci = np.arange(c)[None, :, None, None]
        patch = np.stack([np.stack([pad[bi, ci, (y0 + 3 + dy)[:, None], (x0 + 3 + dx)[:, None]] for dx in (-1, 0, 1, 2)], -1)
                          for dy in (-1, 0, 1, 2)], -2)                # (B, C, H, W, 4 rows, 4 columns)
        sx = np.abs(np.diff(patch, axis=-1)).max((-1, -2))
        sy = np.abs(np.diff(patch, axis=-2)).max((-1, -2))
        t = patch[..., 1:3, 1:3]
        wy = np.stack([1 - wy1, wy1], -1)[:, None, :, :, :, None]
        wx = np.stack([1 - wx1, wx1], -1)[:, None, :, :, None, :]
        warped = (t * wy * wx).sum((-1, -2))
        e_c = (d_ix[:, None] * sx + d_iy[:, None] * sy + 5 * U1 * (np.abs(t) * wy * wx).sum((-1, -2)) + 2 * U1 * np.abs(t).max((-1, -2)))
        warped, e_c = np.where(bad[:, None], 0.0, warped), np.where(bad[:, None], 0.0, e_c)
    d = np.abs(v - warped)
    l1 = d.sum(1)
    e_l1 = (e_c + U1 * d).sum(1) + (c - 1) * U1 * l1
    mean = l1 / c
    z = -20 * mean
    e_z = 20 * (e_l1 / c + U1 * mean) + U1 * np.abs(z)
    return np.exp(z), e_z + EXPF_ULPS * 2.0 ** -23


def unreadable(flow):
    """(B, H, W): sources whose landing coordinate at their own end time is 0 * Inf or 0 * NaN: they write nothing, w cannot be read"""
    return ~np.isfinite(flow[:, 0]) | ~np.isfinite(flow[:, 1])


def own_w(case_, acc):
    """the kernel's own w, (B, 2, H, W) fp32, read from the channel-C planes of tau = 0 (side 0) and tau = 1 (side 1)"""
    c = case_[0].shape[1]
    k0, k1 = end_times(case_[4])
    return np.stack([acc[:, k0, 0, c], acc[:, k1, 1, c]], 1)


def _ratio(err, budget):
    """max err / budget; where the budget is 0 the error must be 0"""
    with np.errstate(all='ignore'):
        r = np.where(budget > 0, err / np.where(budget > 0, budget, 1), np.where(err == 0, 0.0, np.inf))
    r = np.where(np.isfinite(err), r, np.inf)
    return float(r.max()) if r.size else 0.0


def stage1(case_, acc):
    """(worst |w - w64| / budget, number of I * w elements that are not fl32(I * w_k))"""
    i0, i1, f01, f10, taus = case_
    c = i0.shape[1]
    ks = end_times(taus)
    wk = own_w(case_, acc)
    worst, wrong = 0.0, 0
    for side, (src, oth, flow) in enumerate(((i0, i1, f01), (i1, i0, f10))):
        w64, rel = w_reference(src, oth, flow)
        dead = unreadable(flow)
        got = wk[:, side].astype(F64)
        worst = max(worst, _ratio(np.where(dead, np.abs(got), np.abs(got - w64)), np.where(dead, 0.0, rel * w64)))
        want = src * wk[:, side][:, None]                                   # numpy fp32: one rounding
        assert want.dtype == F32
        with np.errstate(all='ignore'):
            wrong += int((~(acc[:, ks[side], side, :c] == want)).sum())
    return worst, wrong


# ---- stage 2 ------------------------------------------------------------------------------------------------------------------------

def stage2_reference(case_, wk):
    """(S, A, n), each (B, K, 2, C + 1, H, W): the exact sum of the terms fl32(I * w_k) * tap32 landing on an element (float64; the
    24 x 24 bit products are exact, the float64 adds lose below n 2^-53 A, 2^-29 of the budget), the sum of their magnitudes and the
    number of non-zero ones"""
    i0, i1, f01, f10, taus = case_
    b, c, h, w = i0.shape
    k_n, hw = len(taus), h * w
    s = np.zeros((b, k_n, 2, c + 1, hw), F64)
    a = np.zeros_like(s)
    n = np.zeros(s.shape, np.int64)
    lead = (np.arange(b)[:, None, None, None] * (c + 1) + np.arange(c + 1)[None, :, None, None]) * hw
    for side, (src, flow) in enumerate(((i0, f01), (i1, f10))):
        with np.errstate(all='ignore'):
            vals = np.concatenate([src * wk[:, side][:, None], wk[:, side][:, None]], 1)
        assert vals.dtype == F32
        vals = np.where(np.isfinite(vals), vals, F32(0)).astype(F64)
        for k in range(k_n):
            ox, oy = landing32(side_time(taus, k, side), flow[:, 0], flow[:, 1])
            ok, nwx, nwy, wts, val = taps32(ox, oy, h, w)
            for (dy, dx), wt, vl in zip(TAP_OFFSETS, wts, val):
                m = np.broadcast_to(vl[:, None], vals.shape)
                idx = (lead + ((nwy + dy) * w + nwx + dx)[:, None])[m]
                term = (vals * wt.astype(F64)[:, None])[m]
                size = b * (c + 1) * hw
                s[:, k, side] += np.bincount(idx, weights=term, minlength=size).reshape(b, c + 1, hw)
                a[:, k, side] += np.bincount(idx, weights=np.abs(term), minlength=size).reshape(b, c + 1, hw)
                n[:, k, side] += np.bincount(idx, weights=(term != 0), minlength=size).astype(np.int64).reshape(b, c + 1, hw)
    shape = (b, k_n, 2, c + 1, h, w)
    return s.reshape(shape), a.reshape(shape), n.reshape(shape)


def stage2(case_, acc, ref=None):
    """worst |acc - S| / ((n + C_SUM) u A) over every element; an element no term lands on must be an exact 0"""
    s, a, n = ref if ref is not None else stage2_reference(case_, own_w(case_, acc))
    return _ratio(np.abs(acc.astype(F64) - s), np.where(n > 0, (n + C_SUM) * U * a, 0.0))


def exact_check(case_, acc):
    """zero frames, quarter-pixel flows and times: the number of elements that differ from float64 (N planes), or are not +0 / 0
    (colour planes)"""
    c = case_[0].shape[1]
    b, _, h, w = case_[0].shape
    ones = np.ones((b, 2, h, w), F32)
    for side, flow in enumerate((case_[2], case_[3])):
        ones[:, side][unreadable(flow)] = 0                   # what own_w reads there; such a source lands nowhere at any time
    wk = own_w(case_, acc)
    s, a, n = stage2_reference(case_, ones)
    assert bool((s == s.astype(F32).astype(F64)).all()) and bool((s * 256 == np.rint(s * 256)).all())       # exact in fp32
    with np.errstate(all='ignore'):
        return int((~(wk == ones)).sum()) + int((~(acc.astype(F64) == s)).sum())


# ---- stage 3 ------------------------------------------------------------------------------------------------------------------------

def blend32(case_, acc, defect=None):
    """flowsynth_blend_kernel in numpy fp32, one rounding per operation: (out (B, K, C, H, W) fp32, bytes uint8)"""
    i0, i1, _, _, taus = case_
    c = i0.shape[1]
    acc = np.asarray(acc, dtype=F32)
    tk = tau32(taus).reshape(1, -1, 1, 1, 1)
    sk = F32(1) - tk
    n0, n1 = acc[:, :, 0, c:], acc[:, :, 1, c:]
    if defect == 'negative zero not a hole':
        full0, full1 = n0.view(np.uint32) != 0, n1.view(np.uint32) != 0
    else:
        full0, full1 = n0 != 0, n1 != 0
    w0, w1 = sk * full0.astype(F32), tk * full1.astype(F32)
    den = w0 + w1
    d0, d1 = np.where(n0 == 0, F32(1), n0), np.where(n1 == 0, F32(1), n1)
    with np.errstate(all='ignore'):
        blend = (w0 * (acc[:, :, 0, :c] / d0) + w1 * (acc[:, :, 1, :c] / d1)) / den
    first = tk if defect == 'fallback tau for both' else sk
    fallback = first * i0[:, None] + tk * i1[:, None]
    out = np.where(den != 0, blend, fallback)
    assert out.dtype == F32
    with np.errstate(all='ignore'):
        u8 = np.clip(np.rint(out * F32(255)), 0, 255)
    return out, np.where(np.isfinite(u8), u8, 0).astype(np.uint8)


def stage3(case_, acc, out, u8):
    """(number of outputs whose bits differ from the restatement on `acc`, number of bytes that differ from the host rule on `out`)"""
    want, _ = blend32(case_, acc)
    out = np.ascontiguousarray(out, dtype=F32)
    with np.errstate(all='ignore'):
        host = np.clip(np.rint(out * F32(255)), 0, 255)
    host = np.where(np.isfinite(host), host, 0).astype(np.uint8)
    return int((out.view(np.uint32) != want.view(np.uint32)).sum()), int((np.asarray(u8) != host).sum())


# ---- the kernel model -----------------------------------------------------------------------------------------------------------------

DEFECTS = ('south hand-over dropped', 'east give across lanes 31-32', 'east hand-over across lanes 31-32', 'give_h without nwy', 'merged value one element off',
           'dead neighbour takes', 'side 1 uses tau', 't * F fused into the add', 'tiles past the cap skipped', 'plane stride C',
           'metric summed over channels', 'negative zero not a hole', 'fallback tau for both')
ORDERS = ('source', 'reversed', 'merged')


def _fma(a, b, c):
    """fl32(a * b + c): the product exact in float64, the sum rounded there first (a double rounding in rare ties; it is a model of
    `a contraction happened`, not of a particular instruction)"""
    return (a.astype(F64) * b.astype(F64) + c.astype(F64)).astype(F32)


def model_w(src, oth, flow, contract, defect):
    """(w, v, z): fp32 (B, H, W), (B, C + 1, H, W) and expf's argument, the scatter kernel's per-source part one rounding at a time"""
    b, c, h, w = src.shape
    ys, xs = _grid(h, w)
    one = F32(1)
    warped = np.zeros_like(src)
    with np.errstate(all='ignore'):
        if h >= 2 and w >= 2:
            fx, fy = flow[:, 0], flow[:, 1]
            gxn = (xs + fx) / F32(w - 1) * F32(2) - one
            gyn = (ys + fy) / F32(h - 1) * F32(2) - one
            if contract:
                ix = _fma(gxn + one, np.full_like(gxn, w), np.full_like(gxn, -1)) * F32(0.5)
                iy = _fma(gyn + one, np.full_like(gyn, h), np.full_like(gyn, -1)) * F32(0.5)
            else:
                ix, iy = ((gxn + one) * F32(w) - one) * F32(0.5), ((gyn + one) * F32(h) - one) * F32(0.5)
            ok = (np.abs(ix) < F32(1e9)) & (np.abs(iy) < F32(1e9))
            ix, iy = np.where(ok, ix, F32(0)), np.where(ok, iy, F32(0))
            flx, fly = np.floor(ix), np.floor(iy)
            wx1, wy1 = ix - flx, iy - fly
            wx0, wy0 = one - wx1, one - wy1
            x0, y0 = np.clip(flx, -2, w).astype(np.int64), np.clip(fly, -2, h).astype(np.int64)
            pad = np.pad(oth, ((0, 0), (0, 0), (2, 2), (2, 2)))
            bi, ci = np.arange(b)[:, None, None, None], np.arange(c)[None, :, None, None]
            t00, t01 = pad[bi, ci, (y0 + 2)[:, None], (x0 + 2)[:, None]], pad[bi, ci, (y0 + 2)[:, None], (x0 + 3)[:, None]]
            t10, t11 = pad[bi, ci, (y0 + 3)[:, None], (x0 + 2)[:, None]], pad[bi, ci, (y0 + 3)[:, None], (x0 + 3)[:, None]]
            wx0, wx1, wy0, wy1 = (a[:, None] for a in (wx0, wx1, wy0, wy1))
            if contract:
                z = np.broadcast_to
                warped = _fma(t11 * wy1, z(wx1, t11.shape), _fma(t10 * wy1, z(wx0, t11.shape),
                                                                 _fma(t01 * wy0, z(wx1, t11.shape), t00 * wy0 * wx0)))
            else:
                warped = t00 * wy0 * wx0 + t01 * wy0 * wx1 + t10 * wy1 * wx0 + t11 * wy1 * wx1
            warped = np.where(ok[:, None], warped, F32(0)).astype(F32)
        l1 = np.zeros((b, h, w), F32)
        for ch in range(c):
            l1 = l1 + np.abs(src[:, ch] - warped[:, ch])
        mean = l1 if defect == 'metric summed over channels' else l1 / F32(c)
        z = F32(-20) * mean
        wgt = np.exp(z.astype(F64)).astype(F32)              # a correctly rounded expf
        v = np.concatenate([src * wgt[:, None], wgt[:, None]], 1)
    assert v.dtype == F32
    return wgt, v, z


def _pad_lanes(a, fill=0):
    """(..., H, W) -> (..., H' / 2, W' / 32, 64): the waves of the 32 x 8 tiles (a wave is two rows of 32 pixels), dead lanes = fill"""
    h, w = a.shape[-2:]
    hp, wp = -(-h // 8) * 8, -(-w // 32) * 32
    a = np.pad(a, [(0, 0)] * (a.ndim - 2) + [(0, hp - h), (0, wp - w)], constant_values=fill)
    a = a.reshape(a.shape[:-2] + (hp // 2, 2, wp // 32, 32))
    return np.moveaxis(a, -3, -2).reshape(a.shape[:-4] + (hp // 2, wp // 32, 64))


def _down(a, d):
    """__shfl_down over the last axis (64 lanes): a lane past the end keeps its own value"""
    o = a.copy()
    o[..., :64 - d] = a[..., d:]
    return o


def _up(a, d):
    o = a.copy()
    o[..., d:] = a[..., :64 - d]
    return o


def model(case_, contract=False, order='source', defect=None, stats=None):
    """(acc (B, K, 2, C + 1, H, W), out, u8): both kernels in numpy fp32"""
    i0, i1, f01, f10, taus = case_
    b, c, h, w = i0.shape
    k_n, hw = len(taus), h * w
    stride = c if defect == 'plane stride C' else c + 1
    acc = np.zeros(b * k_n * 2 * (c + 1) * hw, F32)
    tiles_x, tiles_y, _, cap = tile_counts(b, h, w)
    lane = np.arange(64)
    for side, (src, oth, flow) in enumerate(((i0, i1, f01), (i1, i0, f10))):
        _, v, _ = model_w(src, oth, flow, contract, defect)
        alive = np.ones((b, h, w), bool)
        if defect == 'tiles past the cap skipped':
            ys, xs = np.meshgrid(np.arange(h), np.arange(w), indexing='ij')
            tile = ((side * b + np.arange(b)[:, None, None]) * tiles_y + ys // 8) * tiles_x + xs // 32
            alive = tile < cap
        for k in range(k_n):
            t = tau32(taus)[k] if defect == 'side 1 uses tau' else side_time(taus, k, side)
            ox, oy = landing32(t, flow[:, 0], flow[:, 1], fused=(defect == 't * F fused into the add'))
            ok, nwx, nwy, wts, val = taps32(ox, oy, h, w)
            ok = ok & alive
            base = ((np.arange(b) * k_n + k) * 2 + side) * stride * hw
            o_nw = nwy * w + nwx
            if order != 'merged':
                # one add per valid non-zero tap, in the order of the sources or against it
                idx = np.stack([(base[:, None, None, None] + np.arange(c + 1)[None, :, None, None] * hw + (o_nw + dy * w + dx)[:, None])
                                for dy, dx in TAP_OFFSETS], -1)
                con = np.stack([np.where((vl & ok)[:, None], v * wt[:, None], F32(0)) for wt, vl in zip(wts, val)], -1)
                m = con != 0
                idx, con = idx[m], con[m]
                if order == 'reversed':
                    idx, con = idx[::-1], con[::-1]
                np.add.at(acc, idx, con)
                continue
            any_ = _pad_lanes(ok, False)
            lx, ly = _pad_lanes(nwx), _pad_lanes(nwy)
            any_r, nwx_r, nwy_r = _down(any_, 1), _down(lx, 1), _down(ly, 1)
            any_d, nwx_d, nwy_d = _down(any_, 32), _down(lx, 32), _down(ly, 32)
            if defect == 'dead neighbour takes':
                any_r, any_d = np.ones_like(any_r), np.ones_like(any_d)
            # lane 31 -> 32 is the last pixel of a row and the first of the next.  'give': the giver's test is gone, the taker's is not,
            # so what is handed over is lost.  'hand-over': both are gone -- the coordinates are still compared, so the value lands on
            # its own address from another lane: not a defect of the result
            not31 = (lane & 31) != 31
            if defect in ('east give across lanes 31-32', 'east hand-over across lanes 31-32'):
                not31 = np.ones(64, bool)
            not0 = np.ones(64, bool) if defect == 'east hand-over across lanes 31-32' else (lane & 31) != 0
            same_row = np.ones_like(any_) if defect == 'give_h without nwy' else nwy_r == ly
            give_h = any_ & not31 & any_r & (nwx_r == lx + 1) & same_row
            give_v = any_ & (lane < 32) & any_d & (nwx_d == lx) & (nwy_d == ly + 1)
            take_h = not0 & _up(give_h, 1) & (lane != 0)
            take_v = (lane >= 32) & _up(give_v, 32)
            take_v_kept = take_v
            if defect == 'south hand-over dropped':                     # the second wave of each block (tile rows 2 and 3)
                wave = (np.arange(any_.shape[-3]) % 4)[:, None, None]
                take_v_kept = take_v & (wave != 1)
            if stats is not None:
                both = any_ & any_r & ((lane & 31) != 31) & (nwx_r == lx + 1)
                stats['give_h'] = stats.get('give_h', 0) + int(give_h.sum())
                stats['give_v'] = stats.get('give_v', 0) + int(give_v.sum())
                stats['refused_h_by_row'] = stats.get('refused_h_by_row', 0) + int((both & (nwy_r != ly)).sum())
                stats['seam_31_32'] = stats.get('seam_31_32', 0) + int((any_ & any_r & (lane == 31) & (nwx_r == lx + 1)
                                                                        & (nwy_r == ly)).sum())
                some, every = val[0] | val[1] | val[2] | val[3], val[0] & val[1] & val[2] & val[3]
                stats['split_validity'] = stats.get('split_validity', 0) + int((some & ~every & ok).sum())
            vl_l = [_pad_lanes(x & ok, False) for x in val]
            onw = _pad_lanes(o_nw)
            pb = base.reshape(b, 1, 1, 1)
            for ch in range(c + 1):
                vc = _pad_lanes(v[:, ch])
                tw = [_pad_lanes(x) for x in wts]
                cnw, cne, csw, cse = (np.where(m, vc * x, F32(0)) for x, m in zip(tw, vl_l))
                rsw, rse = _up(csw, 32), _up(cse, 32)
                if contract:                                            # the product fused into the add of what was handed over
                    cnw = np.where(take_v_kept, np.where(vl_l[0], _fma(vc, tw[0], rsw), rsw), cnw)
                    cne = np.where(take_v_kept, np.where(vl_l[1], _fma(vc, tw[1], rse), rse), cne)
                else:
                    cnw, cne = np.where(take_v_kept, cnw + rsw, cnw), np.where(take_v_kept, cne + rse, cne)
                csw, cse = np.where(give_v, F32(0), csw), np.where(give_v, F32(0), cse)
                sne, sse = _up(cne, 1), _up(cse, 1)
                if defect == 'merged value one element off':
                    cne, cse = np.where(take_h, cne + sne, cne), np.where(take_h, cse + sse, cse)
                else:
                    cnw, csw = np.where(take_h, cnw + sne, cnw), np.where(take_h, csw + sse, csw)
                cne, cse = np.where(give_h, F32(0), cne), np.where(give_h, F32(0), cse)
                for (dy, dx), con, vl in zip(TAP_OFFSETS, (cnw, cne, csw, cse), vl_l):
                    m = any_ & vl & (con != 0)
                    idx = pb + ch * hw + onw + dy * w + dx
                    np.add.at(acc, idx[m], con[m].astype(F32))
    acc = acc.reshape(b, k_n, 2, c + 1, h, w)
    out, u8 = blend32(case_, acc, defect)
    return acc, out, u8


def expf_arguments():
    """the arguments z = fl32(-20 mean) the committed cases hand to expf, from the model: a sorted fp32 array"""
    zs = []
    for name in CASES:
        i0, i1, f01, f10, _ = case(name)
        for src, oth, flow in ((i0, i1, f01), (i1, i0, f10)):
            for contract in (False, True):
                zs.append(model_w(src, oth, flow, contract, None)[2].ravel())
    return np.unique(np.concatenate(zs))


if __name__ == '__main__':
    expf_arguments().tofile(sys.argv[1])
