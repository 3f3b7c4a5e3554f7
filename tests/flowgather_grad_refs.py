"""TEST INFRASTRUCTURE: the float64 reference, the per-element budget and the cases of the tests of the gather operator's gradient
(tests/test_flowgather_grad_host.py, tests/test_gpu_flowgather_grad.py).

    gather_grad64(i0, i1, flows, slots, taus, g)   d loss / d flows in float64 for g = d loss / d out, by numpy index arithmetic, one
                                                   (b, k) at a time.  It shares no code with `flowsynth.gather_from` (only the tap
                                                   lookup and the sample budget of tests/flowgather_refs.py).  Returns
                                                   (dflows, budget), both (T', 4, H, W) float64.
    cells_agree(flows, slots, h, w)                every sample takes the same cell in fp32 and in float64 (and is refused by both or
                                                   by neither): the condition under which the budget holds on EVERY element
    CASES, case(name), table(...)                  shapes, tables and flows built from target coordinates

The gradient, per row (b, k), sample s in {0, 1}, pixel p, with out_c, D of the forward pass:

    dG_s = k_s S_s,   k_s = c_s a_s / D,   S_s = sum_c g_c (grad_q W_s,c - out_c grad_q n_s)                (x and y components)
    grad_q W: d/dqx = wy0 (t01 - t00) + wy1 (t11 - t10),  d/dqy = wx0 (t10 - t00) + wx1 (t11 - t01)   in the cell floor(q)

The budget bounds |fp32 - float64| to first order with u = 2^-24, for the fused kernel's order of operations and for the chain-rule
order autograd takes through `gather_from` alike (the latter multiplies every tap by the upstream factor before the taps are
combined, so its rounding scales with the taps, not with their differences).  Inputs are exact; both precisions take the same cell.

  coordinate   dq <= u (|c G| + |q|) per axis, as in the forward budget.  Inside a cell the slope along x is linear in qy with
               derivative t11 - t10 - t01 + t00 =: X (the mixed difference), and the slope along y is linear in qx with the same X:
               the coordinate error moves the x slope by dqy |X| and the y slope by dqx |X|.
  weights      q - floor(q) is exact, 1 - w one rounding, a product of two another: at most 3u each, as in DESIGN 19.4.
  slope        four taps, each with a weight error (3u |t|) and a product (u |t|), three sums of partials of at most 2 M, M the
               largest |tap| of the cell: (12 + 4 + 6) u M = 22 u M.  The slopes of n: the same with the taps of the all-ones image.
  term         T_c = slope(W_c) - out_c slope(n): the forward pass's own error d out_c enters times |slope(n)|, the slope error of n
               times |out_c|, the product and the difference one rounding each:
               dT_c <= dslope(W_c) + d out_c |slope n| + |out_c| dslope(n) + 2 u |out_c slope n| + u |T_c|.
  sum over c   dS <= sum_c |g_c| dT_c + C u sum_c |g_c| (2 M_c + |out_c|): each product g_c T_c one rounding and C - 1 sums (in the
               chain-rule order the sum over c runs per tap, over terms of size |g_c| M_c).
  factor       k = c a / D: a0 = fl(1 - tau) carries u, the product c a, the quotient and the product k S one each: 4 u; D carries the
               forward pass's dD, and D - dD >= e / 2 bounds 1 / D by 2 / e:   d(k S) <= |k| dS + |k S| (4 u + dD / (D - dD)).
  rows         the m contributions v_1 .. v_m of one element are summed in a fixed order: sum_i dv_i + (m - 1) u sum_i |v_i|.

A sample whose coordinate is not finite, or 1e9 or more in size, contributes exactly 0 in both precisions.  Second-order terms are
covered by the factor 1 + 2^-10 of the forward budget.
"""
import importlib.util
import os

import numpy as np
import torch

from flowgather_refs import EPS, SECOND_ORDER, U, _cell, _padded, _sample, smooth

SLOPE_ROUNDINGS = 22


def _coords(c, gx, gy, xs, ys):
    with np.errstate(invalid='ignore', over='ignore'):
        sx, sy = c * gx, c * gy
        qx, qy = xs + sx, ys + sy
    ok = np.isfinite(qx) & np.isfinite(qy) & (np.abs(qx) < 1e9) & (np.abs(qy) < 1e9)
    qx, qy, sx, sy = (np.where(ok, a, 0.0) for a in (qx, qy, sx, sy))
    return ok, qx, qy, U * (np.abs(sx) + np.abs(qx)), U * (np.abs(sy) + np.abs(qy))


def _slopes(plane, ok, qx, qy, dqx, dqy):
    """(d/dqx, d/dqy, their budgets) of the bilinear interpolant of the zero-padded plane in the cell floor(q)"""
    fx, fy = np.floor(qx), np.floor(qy)
    ax, ay = qx - fx, qy - fy
    t00, t01, t10, t11 = _cell(_padded(plane), fx.astype(np.int64), fy.astype(np.int64))
    sx = (1 - ay) * (t01 - t00) + ay * (t11 - t10)
    sy = (1 - ax) * (t10 - t00) + ax * (t11 - t01)
    mixed = np.abs(t11 - t10 - t01 + t00)
    big = np.max(np.abs(np.stack([t00, t01, t10, t11])), 0)
    ex, ey = dqy * mixed + SLOPE_ROUNDINGS * U * big, dqx * mixed + SLOPE_ROUNDINGS * U * big
    return tuple(np.where(ok, a, 0.0) for a in (sx, sy, ex, ey)) + (np.where(ok, big, 0.0),)


def gather_grad64(frame1, frame2, flows, slots, taus, grad_out):
    """(dflows, budget) for g = grad_out (B, K, C, H, W): see the module text.  taus as the kernel sees them, rounded to fp32."""
    i0, i1, fl, g = (t.detach().cpu().to(torch.float64).numpy() for t in (frame1, frame2, flows, grad_out))
    tab = slots.numpy()
    coef = tab[..., 4:].copy().view(np.float32).astype(np.float64)
    tau = np.asarray([float(t) for t in taus], dtype=np.float32).astype(np.float64)
    b, c, h, w = i0.shape
    k = len(tau)
    ys, xs = np.meshgrid(np.arange(h, dtype=np.float64), np.arange(w, dtype=np.float64), indexing='ij')
    ones = np.ones((h, w))
    grad, err = np.zeros(fl.shape), np.zeros(fl.shape)
    mag, count = np.zeros(fl.shape), np.zeros(fl.shape[:2], dtype=np.int64)
    for bb in range(b):
        for kk in range(k):
            idx = [int(v) for v in tab[bb, kk, :2]]
            ch = [int(v) for v in tab[bb, kk, 2:4]]
            imgs, a = (i0[bb], i1[bb]), (1 - tau[kk], tau[kk])
            geo, smp = [], []
            for s in range(2):
                gx, gy = fl[idx[s], ch[s]], fl[idx[s], ch[s] + 1]
                geo.append(_coords(coef[bb, kk, s], gx, gy, xs, ys))
                smp.append(_sample(imgs[s], ones, coef[bb, kk, s], gx, gy, xs, ys))
            (w0, n0, dw0, dn0), (w1, n1, dw1, dn1) = smp
            a0, a1 = a
            # the forward pass and its budget, as tests/flowgather_refs.gather64 derives it
            lin = a0 * i0[bb] + a1 * i1[bb]
            num, den = a0 * w0 + a1 * w1, a0 * n0 + a1 * n1
            top, bottom = num + EPS * lin, den + EPS
            out = top / bottom
            d_lin = U * (np.abs(i0[bb]) + np.abs(a0 * i0[bb]) + np.abs(a1 * i1[bb]) + np.abs(lin))
            d_num = a0 * dw0 + a1 * dw1 + U * (np.abs(w0) + np.abs(a0 * w0) + np.abs(a1 * w1) + np.abs(num))
            d_den = a0 * dn0 + a1 * dn1 + U * (np.abs(n0) + np.abs(a0 * n0) + np.abs(a1 * n1) + np.abs(den))
            d_top, d_bottom = d_num + EPS * d_lin + U * np.abs(top), d_den + U * np.abs(bottom)
            assert float((bottom - d_bottom).min()) > 0.5 * EPS
            d_out = (d_top + np.abs(out) * d_bottom) / (bottom - d_bottom) + U * np.abs(out)
            for s in range(2):
                ok, qx, qy, dqx, dqy = geo[s]
                nx, ny, enx, eny, _ = _slopes(ones, ok, qx, qy, dqx, dqy)
                sums, errs, sizes = [0.0, 0.0], [0.0, 0.0], 0.0
                for cc in range(c):
                    wx, wy, ewx, ewy, big = _slopes(imgs[s][cc], ok, qx, qy, dqx, dqy)
                    gc = g[bb, kk, cc]
                    for axis, (sw, sn, ew, en) in enumerate(((wx, nx, ewx, enx), (wy, ny, ewy, eny))):
                        term = sw - out[cc] * sn
                        d_term = ew + d_out[cc] * np.abs(sn) + np.abs(out[cc]) * en + 2 * U * np.abs(out[cc] * sn) + U * np.abs(term)
                        sums[axis] = sums[axis] + gc * term
                        errs[axis] = errs[axis] + np.abs(gc) * d_term
                    sizes = sizes + np.abs(gc) * (2 * big + np.abs(out[cc]))
                factor = coef[bb, kk, s] * a[s] / bottom
                rel = 4 * U + d_bottom / (bottom - d_bottom)
                for axis in range(2):
                    val = factor * sums[axis]
                    d_val = np.abs(factor) * (errs[axis] + c * U * sizes) + np.abs(val) * rel
                    val, d_val = np.where(ok, val, 0.0), np.where(ok, d_val, 0.0)
                    grad[idx[s], ch[s] + axis] += val
                    err[idx[s], ch[s] + axis] += d_val
                    mag[idx[s], ch[s] + axis] += np.abs(val)
                    count[idx[s], ch[s] + axis] += 1
    err = err + U * np.maximum(count - 1, 0)[:, :, None, None] * mag
    return torch.from_numpy(grad), torch.from_numpy(SECOND_ORDER * err)


def cells_agree(flows, slots, h, w):
    """True where, for every row, sample and pixel, the fp32 coordinate (the product rounded, then the sum, as the kernel) and the
    float64 one are accepted or refused alike and fall into the same cell"""
    fl32 = flows.detach().cpu().numpy().astype(np.float32)
    tab = slots.numpy()
    coef = tab[..., 4:].copy().view(np.float32)
    ys, xs = np.meshgrid(np.arange(h, dtype=np.float32), np.arange(w, dtype=np.float32), indexing='ij')
    same = True
    with np.errstate(invalid='ignore', over='ignore'):
        for row, cf in zip(tab.reshape(-1, 6), coef.reshape(-1, 2)):
            for s in range(2):
                for g, p in ((fl32[row[s], row[2 + s]], xs), (fl32[row[s], row[2 + s] + 1], ys)):
                    q32 = p + cf[s] * g                                             # float32 throughout: two roundings
                    q64 = p.astype(np.float64) + np.float64(cf[s]) * g.astype(np.float64)
                    ok32, ok64 = np.abs(q32) < np.float32(1e9), np.abs(q64) < 1e9
                    same = same and bool((ok32 == ok64).all())
                    both = ok32 & ok64
                    same = same and bool((np.floor(q32[both]).astype(np.float64) == np.floor(q64[both])).all())
    return same


# ---- inputs ----

def _bits(v):
    return int(np.float32(v).view(np.int32))


def table(b, k, reverse_first=False, shared=()):
    """A (b, k, 6) slot table over 2 b k + 1 slices (the last one unnamed).  Row r = b K + k: G1 = channels 0-1 of slice r with c1 =
    COEF[r], G0 = channels 2-3 of slice b k + r with c0 = COEF[r + 1].  `reverse_first`: the rows of pair 0 are reverse rows, G0 =
    channels 0-1 of G1's slice with c0 = -c1.  `shared`: (r, r2) pairs, row r2 reads the G1 of row r (same slice, same c1)."""
    coefs = (0.625, 0.375, 0.8125, 0.25, 0.5, 0.6875)
    rows = []
    for r in range(b * k):
        c1, c0 = coefs[r % len(coefs)], coefs[(r + 1) % len(coefs)]
        row = [b * k + r, r, 2, 0, _bits(c0), _bits(c1)]
        if reverse_first and r < k:
            row = [r, r, 0, 0, _bits(-c1), _bits(c1)]
        rows.append(row)
    for r, r2 in shared:
        rows[r2][1], rows[r2][3], rows[r2][5] = rows[r][1], rows[r][3], rows[r][5]
    return torch.tensor(rows, dtype=torch.int32).reshape(b, k, 6), 2 * b * k + 1


def snapped(q):
    """q with its fractional part mapped from [0, 1) into [1/16, 15/16]: fp32 and float64 then take the same cell"""
    f = np.floor(q)
    return f + 1 / 16 + (q - f) * (14 / 16)


def target_flows(seed, slots, slices, h, w):
    """(slices, 4, h, w) fp32 flows built from target coordinates, G = (q - p) / c, for the owner of every named channel pair (the
    first row that names it; a later row names it with c or -c, which keeps the fractional parts in range).  q = p + a smooth
    displacement of a few pixels, with bands that cross each of the four borders and a patch far outside, snapped."""
    g = torch.Generator().manual_seed(seed)
    ys, xs = np.meshgrid(np.arange(h, dtype=np.float64), np.arange(w, dtype=np.float64), indexing='ij')
    fl = np.zeros((slices, 4, h, w))
    done = set()
    tab = slots.reshape(-1, 6).numpy()
    coef = tab[:, 4:].copy().view(np.float32).astype(np.float64)
    for row, cf in zip(tab, coef):
        for s in range(2):
            key = (int(row[s]), int(row[2 + s]))
            if key in done:
                continue
            done.add(key)
            disp = ((smooth(g, 1, 2, h, w) * 2 - 1) * 3.0)[0].to(torch.float64).numpy()
            by, bx = max(1, h // 6), max(1, w // 8)
            if w > 1:
                disp[0, :, :bx] -= bx + 0.4
                disp[0, :, w - bx:] += bx + 0.3
            if h > 1:
                disp[1, :by, :] -= by + 0.2
                disp[1, h - by:, :] += by + 0.6
            if h >= 5 and w >= 16:
                disp[:, h // 2, w // 2:w // 2 + 3] = np.array([3.0 * w, -2.0 * h]).reshape(2, 1)
            if h == 1 and w == 1:
                disp[:] = np.array([0.3, -0.45]).reshape(2, 1, 1)
            qx, qy = snapped(xs + disp[0]), snapped(ys + disp[1])
            fl[key[0], key[1]], fl[key[0], key[1] + 1] = (qx - xs) / cf[s], (qy - ys) / cf[s]
    return torch.from_numpy(fl).to(torch.float32).contiguous()


def frames(seed, b, c, h, w):
    g = torch.Generator().manual_seed(seed)
    return smooth(g, b, c, h, w, grid=(5, 7)), smooth(g, b, c, h, w, grid=(5, 7))


def grad_out(seed, b, k, c, h, w):
    g = torch.Generator().manual_seed(seed + 1000)
    return (torch.rand(b, k, c, h, w, generator=g) * 2 - 1).contiguous()


# name -> (seed, b, c, h, w, taus, reverse_first, shared)
CASES = {
    '1x1': (1, 1, 3, 1, 1, (0.5,), False, ()),
    '13x37': (2, 2, 3, 13, 37, (0.3, 0.5, 0.9), True, ((3, 5),)),
    '5x1031': (3, 1, 1, 5, 1031, (0.0, 1.0), False, ()),
    '24x40': (4, 3, 3, 24, 40, (0.25, 0.7), False, ()),
    '17x300': (5, 2, 1, 17, 300, tuple((i + 0.5) / 64 for i in range(64)), False, ((0, 64),)),
}
HOST_CASES = ('1x1', '13x37', '5x1031')


def case(name):
    """(frame1, frame2, flows, slots, taus, grad_out), fp32 / int32 on the CPU"""
    seed, b, c, h, w, taus, reverse_first, shared = CASES[name]
    i0, i1 = frames(seed, b, c, h, w)
    slots, slices = table(b, len(taus), reverse_first, shared)
    return i0, i1, target_flows(seed, slots, slices, h, w), slots, taus, grad_out(seed, b, len(taus), c, h, w)


# ---- the trainer ----

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def flow_main():
    """video-interpolation/main.py as a module, loaded from its file (the repository's root holds a main.py of its own)"""
    spec = importlib.util.spec_from_file_location('flow_main_between', os.path.join(ROOT, 'video-interpolation', 'main.py'))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def trainer_args(net='RBF', argv=(), **kw):
    """the namespace of `main.py train --synthetic 4 24 40 --batch 3 --net <net> <argv>` with its network built, seeded"""
    m = flow_main()
    args = m.get_args(['train', '--synthetic', '4', '24', '40', '--batch', '3', '--net', net, *argv])
    torch.manual_seed(0)
    args.net = m.build_net(args)
    for name, v in kw.items():
        setattr(args, name, v)
    return args


def trainer_batch():
    """SyntheticClip(4, 24, 40), batch 3: [frame1, frame2, times, scale, gt] as the trainer's loader collates them; dt = 2 / 3"""
    from sin_inn_amd import flowdata
    clip = flowdata.SyntheticClip(4, 24, 40, seed=0)
    return [clip.video[0:3], clip.video[1:4], clip.T[0:3], torch.tensor([clip.flow_scale] * 3, dtype=torch.float64), clip.flow[0:3]]
