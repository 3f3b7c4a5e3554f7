"""TEST INFRASTRUCTURE: the float64 reference, the per-element budget and the cases of the gather-synthesis tests
(tests/test_flowgather_host.py, tests/test_gpu_flowgather.py).

    gather64(i0, i1, flows, slots, taus)   the definition in float64 with numpy index arithmetic, one (b, k) at a time.  It shares no
                                           code with `flowsynth.gather_composed` nor with the oracle's warp (which has quirk C-18).
                                           Returns (out, budget), both (B, K, C, H, W) float64.
    CASES, case(name)                      the shapes and flows of the GPU test

The budget is derived from the roundings of the fp32 evaluation (fused or composed), to first order, with u = 2^-24 the bound of one
rounding relative to its result.  Inputs are taken as exact (they are the same fp32 numbers in both precisions).

  coordinate   q = p + fl(c G): the product carries u |c G|, the sum u |q|:  dq <= u (|c G| + |q|) per axis.
  sample       W(q) = sum of w_i t_i over the four taps (t_i = 0 outside the frame) is continuous and piecewise bilinear.  Inside one
               cell |dW / dqx| <= max(|t01 - t00|, |t11 - t10|) =: Dx and |dW / dqy| <= max(|t10 - t00|, |t11 - t01|) =: Dy, so the
               coordinate error moves W by at most dqx Dx + dqy Dy.  Where q lies within dq of a cell border the fp32 coordinate may
               fall into the neighbouring cell: Dx, Dy are then the larger of the two cells' (of the four at a corner).  The same with
               the taps of the all-ones image (1 inside, 0 outside) for n.
               In-cell arithmetic: q - floor(q) is exact; 1 - w one rounding; a weight product one more: each of the four weights
               carries at most 3u (weights <= 1).  W: four weight errors times |t| (12 u M), four products and three sums, each at most u M
               with M the largest |tap| of the cell: 19 u M.  n is given the same bound with M = 1 (its products by 1 are exact).
  blend        a0 = fl(1 - tau) carries u, a1 = tau is exact.
               L   = a0 I0 + a1 I1:   dL   <= u |I0| + u (|a0 I0| + |a1 I1|) + u |L|
               num = a0 W0 + a1 W1:   dnum <= a0 dW0 + a1 dW1 + u |W0| + u (|a0 W0| + |a1 W1|) + u |num|
               den likewise from n0, n1.
               N = num + e L (e L is exact, e = 2^-10):  dN <= dnum + e dL + u |N|;   D = den + e:  dD <= dden + u |D|
  quotient     out = N / D with D >= e:   dout <= (dN + |out| dD) / (D - dD) + u |out|

Second-order terms are smaller than the first-order ones by a factor of the order of u / e = 2^-14; the budget is multiplied by
1 + 2^-10 to cover them.  The budget is a few tens of u in the interior, grows with the distance of q from the origin, and is loose (by
about 1 / e = 2^10) only where both samples have left the frame and D is e itself.
"""
import numpy as np
import torch

U = 2.0 ** -24
EPS = 2.0 ** -10
SECOND_ORDER = 1 + 2.0 ** -10


def _padded(img):
    """(H + 4, W + 4) with two zeros on every side: cell (x0, y0) with x0 in [-2, W] reads without a bounds check"""
    return np.pad(img, 2)


def _cell(pad, x0, y0):
    """the four taps of the cells whose north-west tap is (x0, y0) (arrays), from a padded plane; cells further out are all zero"""
    h, w = pad.shape[0] - 4, pad.shape[1] - 4
    far = (x0 < -2) | (x0 > w) | (y0 < -2) | (y0 > h)
    xs, ys = np.clip(x0, -2, w) + 2, np.clip(y0, -2, h) + 2
    taps = [np.where(far, 0.0, pad[ys + dy, xs + dx]) for dy, dx in ((0, 0), (0, 1), (1, 0), (1, 1))]
    return taps


def _sample(planes, ones, c, gx, gy, xs, ys):
    """sample(I, p + c G) for the planes (C, H, W) of one frame: (W (C, H, W), n, dW (C, H, W), dn), the d's the budget of the sample"""
    h, w = ones.shape
    with np.errstate(invalid='ignore', over='ignore'):
        sx, sy = c * gx, c * gy
        qx, qy = xs + sx, ys + sy
    ok = np.isfinite(qx) & np.isfinite(qy) & (np.abs(qx) < 1e9) & (np.abs(qy) < 1e9)
    qx, qy, sx, sy = (np.where(ok, a, 0.0) for a in (qx, qy, sx, sy))
    fx, fy = np.floor(qx), np.floor(qy)
    x0, y0 = fx.astype(np.int64), fy.astype(np.int64)
    ax, ay = qx - fx, qy - fy
    dqx, dqy = U * (np.abs(sx) + np.abs(qx)), U * (np.abs(sy) + np.abs(qy))
    # the cells the fp32 coordinate may fall into
    shifts = []
    for dy in (-1, 0, 1):
        for dx in (-1, 0, 1):
            reach_x = (dx == 0) | ((ax <= dqx) if dx < 0 else (1 - ax <= dqx))
            reach_y = (dy == 0) | ((ay <= dqy) if dy < 0 else (1 - ay <= dqy))
            shifts.append((dx, dy, reach_x & reach_y))

    def one(plane):
        pad = _padded(plane)
        t00, t01, t10, t11 = _cell(pad, x0, y0)
        val = (1 - ay) * ((1 - ax) * t00 + ax * t01) + ay * ((1 - ax) * t10 + ax * t11)
        slope_x, slope_y, big = np.zeros_like(qx), np.zeros_like(qx), np.zeros_like(qx)
        for dx, dy, reach in shifts:
            a, b, cc, d = _cell(pad, x0 + dx, y0 + dy)
            slope_x = np.maximum(slope_x, np.where(reach, np.maximum(np.abs(b - a), np.abs(d - cc)), 0.0))
            slope_y = np.maximum(slope_y, np.where(reach, np.maximum(np.abs(cc - a), np.abs(d - b)), 0.0))
            big = np.maximum(big, np.where(reach, np.max(np.abs(np.stack([a, b, cc, d])), 0), 0.0))
        return np.where(ok, val, 0.0), np.where(ok, dqx * slope_x + dqy * slope_y + 19 * U * big, 0.0)

    vals, errs = zip(*(one(p) for p in planes))
    n, dn = one(ones)
    return np.stack(vals), n, np.stack(errs), dn


def gather64(frame1, frame2, flows, slots, taus):
    """(out, budget): the definition in float64 and the bound on |fp32 - out| derived above.  frames (B, C, H, W), flows (T', 4, H, W),
    slots the host table (B, K, 6) int32, taus K values: the times as the kernel sees them, rounded to fp32."""
    i0, i1, fl = (t.detach().cpu().to(torch.float64).numpy() for t in (frame1, frame2, flows))
    table = slots.numpy()
    coef = table[..., 4:].copy().view(np.float32).astype(np.float64)
    tau = np.asarray([float(t) for t in taus], dtype=np.float32).astype(np.float64)
    b, c, h, w = i0.shape
    k = len(tau)
    ys, xs = np.meshgrid(np.arange(h, dtype=np.float64), np.arange(w, dtype=np.float64), indexing='ij')
    ones = np.ones((h, w))
    out, budget = np.zeros((b, k, c, h, w)), np.zeros((b, k, c, h, w))
    for bb in range(b):
        for kk in range(k):
            idx0, idx1, ch0, ch1 = (int(v) for v in table[bb, kk, :4])
            w0, n0, dw0, dn0 = _sample(i0[bb], ones, coef[bb, kk, 0], fl[idx0, ch0], fl[idx0, ch0 + 1], xs, ys)
            w1, n1, dw1, dn1 = _sample(i1[bb], ones, coef[bb, kk, 1], fl[idx1, ch1], fl[idx1, ch1 + 1], xs, ys)
            a1 = tau[kk]
            a0 = 1 - a1
            lin = a0 * i0[bb] + a1 * i1[bb]
            num = a0 * w0 + a1 * w1
            den = a0 * n0 + a1 * n1
            top, bottom = num + EPS * lin, den + EPS
            res = top / bottom
            d_lin = U * (np.abs(i0[bb]) + np.abs(a0 * i0[bb]) + np.abs(a1 * i1[bb]) + np.abs(lin))
            d_num = a0 * dw0 + a1 * dw1 + U * (np.abs(w0) + np.abs(a0 * w0) + np.abs(a1 * w1) + np.abs(num))
            d_den = a0 * dn0 + a1 * dn1 + U * (np.abs(n0) + np.abs(a0 * n0) + np.abs(a1 * n1) + np.abs(den))
            d_top = d_num + EPS * d_lin + U * np.abs(top)
            d_bottom = d_den + U * np.abs(bottom)
            assert float((bottom - d_bottom).min()) > 0.5 * EPS
            out[bb, kk] = res
            budget[bb, kk] = SECOND_ORDER * ((d_top + np.abs(res) * d_bottom) / (bottom - d_bottom) + U * np.abs(res))
    return torch.from_numpy(out), torch.from_numpy(budget)


# ---- inputs ----

def smooth(g, n, c, h, w, grid=(3, 4)):
    """(n, c, h, w) in [0, 1): uniform noise on a coarse grid, enlarged bilinearly"""
    coarse = torch.rand(n, c, *grid, generator=g)
    if h == 1 and w == 1:
        return coarse[:, :, :1, :1].contiguous()
    return torch.nn.functional.interpolate(coarse, size=(h, w), mode='bilinear', align_corners=True).contiguous()


def frames(seed, b, c, h, w):
    g = torch.Generator().manual_seed(seed)
    return smooth(g, b, c, h, w, grid=(5, 7)), smooth(g, b, c, h, w, grid=(5, 7))


def border_flows(seed, t, h, w):
    """(t, 4, h, w) fp32: smooth flows of a few pixels; near each of the four borders a band that carries the sample across it by a
    fractional amount; a block of integer flows (half of them to outside the frame, when scaled by 1/2 .. 1), and a patch sent far
    outside the frame on both axes"""
    g = torch.Generator().manual_seed(seed)
    fl = (smooth(g, t, 4, h, w) * 2 - 1) * 3.0
    by, bx = max(1, h // 6), max(1, w // 8)
    fl[:, 0::2, :, :bx] -= 2.0 * bx + 0.37           # x flows: across the left border (forward and backward channels alike)
    fl[:, 0::2, :, w - bx:] += 2.0 * bx + 0.61
    fl[:, 1::2, :by, :] -= 2.0 * by + 0.29
    fl[:, 1::2, h - by:, :] += 2.0 * by + 0.73
    if h >= 5 and w >= 16:
        cy, cx = h // 2, w // 2
        fl[:, :, cy - 1:cy + 1, cx - 4:cx] = torch.tensor([4.0, -2.0, -6.0, 2.0]).view(1, 4, 1, 1)
        fl[:, :, cy - 1:cy + 1, cx:cx + 4] = torch.tensor([4.0 * w, 2.0 * h, -4.0 * w, -2.0 * h]).view(1, 4, 1, 1)
    return fl.contiguous()


def mixed_slots(b, k, slices, taus, seed=0):
    """a (b, k, 6) table over `slices` time slices that mixes regular entries (G0 = channels 2-3 of another slice, c0 = tau) and reverse
    ones (G0 = channels 0-1 of G1's slice, c0 = -tau), in the bit layout of `flowsynth.gather_slots`"""
    g = torch.Generator().manual_seed(seed)
    rows = []
    for bb in range(b):
        for kk in range(k):
            tau = np.float32(taus[kk])
            idx1 = int(torch.randint(slices, (1,), generator=g))
            if (bb * k + kk) % 2 == 0:
                idx0, ch0, c0 = int(torch.randint(slices, (1,), generator=g)), 2, tau
            else:
                idx0, ch0, c0 = idx1, 0, -tau
            c1 = np.float32(1) - tau
            rows.append([idx0, idx1, ch0, 0, int(np.float32(c0).view(np.int32)), int(np.float32(c1).view(np.int32))])
    return torch.tensor(rows, dtype=torch.int32).reshape(b, k, 6)


# name -> (seed, b, c, h, w, taus, time slices): the slices outnumber b k everywhere (T' > B K)
CASES = {
    '1x1': (1, 1, 3, 1, 1, (0.5,), 3),
    '13x37': (2, 2, 3, 13, 37, (0.0, 0.3, 1.0), 9),
    '5x1031': (3, 1, 1, 5, 1031, (0.25, 0.875), 4),
}


def case(name):
    """(frame1, frame2, flows, slots, taus), fp32 / int32 on the CPU"""
    seed, b, c, h, w, taus, slices = CASES[name]
    i0, i1 = frames(seed, b, c, h, w)
    if name == '1x1':
        # slice 0: I1 is sampled at (0.3, -0.2) * (1 - tau) -- two taps inside, two above the frame; slice 1: I0 leaves the frame
        fl = torch.tensor([[0.6, -0.4, 9.0, 9.0], [1.0, 1.0, 5.0, 5.0], [0.0, 0.0, 0.0, 0.0]]).reshape(3, 4, 1, 1)
        half = int(np.float32(0.5).view(np.int32))
        return i0, i1, fl, torch.tensor([[[1, 0, 2, 0, half, half]]], dtype=torch.int32), taus
    return i0, i1, border_flows(seed, slices, h, w), mixed_slots(b, len(taus), slices, taus, seed), taus
