"""TEST INFRASTRUCTURE: the float64 reference, the per-element budget and the cases of the tests of the gather rule at a list of points
(tests/test_flowgather_points_host.py, tests/test_gpu_flowgather_points.py).

    gather_at64(i0, i1, flows, pix, pair, tau, rev, blend, grad_out)   the definition and, with `grad_out`, d loss / d flows, in float64
                                                   by numpy index arithmetic, one pair of the batch at a time.  It shares no code with
                                                   `flowsynth.gather_at_from` (only the tap lookup of tests/flowgather_refs.py and the
                                                   slope helper of tests/flowgather_grad_refs.py).  Returns (out, budget, dflows,
                                                   dbudget): (R, N, C) twice, (S, 4, N) twice (None without `grad_out`).
    cells_agree(flows, pix, tau, rev, h, w)        every sample takes the same cell in fp32 and in float64 (and is refused by both or by
                                                   neither): the condition under which the budgets hold on EVERY element
    CASES, case(name)                              the cases of the issue, built by rejection: p, q0, q1 have fractional parts in
                                                   [1/16, 15/16] or are exact integers

The definition at point n, p = pix[n] = (py, px), b = pair[n]:

    G1 = flows[0, 0:2, n], c1 = 1 - tau;   G0 = flows[1, 2:4, n], c0 = tau  where S == 2 and not rev[n];  else G0 = G1, c0 = -tau
    q_s = p + c_s G_s;   (W_s, n_s) = sample(I_s[b], q_s);   H_s = sample(I_s[b], p).W
    out[r, c] = (a0 W0_c + a1 W1_c + e (a0 H0_c + a1 H1_c)) / (a0 n0 + a1 n1 + e),   a1 = blend[r] (or tau), a0 = 1 - a1
    d loss / d G_s = sum_r k_sr S_sr,   k_sr = c_s a_sr / D_r,   S_sr = sum_c g_rc (grad_q W_s,c - out_rc grad_q n_s)

The budget bounds |fp32 - float64| to first order with u = 2^-24, derived the way DESIGN 19.4 and 22.4 derive theirs.  Inputs are exact
and both precisions take the same cell (asserted), so only the cell floor(q) enters.  What the point form adds or changes:

  coefficient  c0 = +-tau is exact; c1 = fl(1 - tau) carries u.  The float64 reference uses 1 - tau itself, so the coordinate of sample
               1 carries one more u |c1 G1|:   dq_s <= u ((1 + [s = 1]) |c_s G_s| + |q_s|) per axis.
  sample       inside the cell |dW / dqx| <= max(|t01 - t00|, |t11 - t10|) =: Dx, |dW / dqy| <= Dy likewise: the coordinate error moves
               W by dqx Dx + dqy Dy; the in-cell arithmetic adds 19 u M (four weights of 3u, four products, three sums; M the largest
               |tap| of the cell), as in 19.4.  n: the same on the all-ones image.
  H            H_s = sample(I_s, p) at the exact coordinate p: no coordinate term, the in-cell arithmetic alone, dH_s <= 19 u M_s(p).
               On an integer pixel three weights are exactly 0 and one is 1: H_s = I_s(p) exactly, inside the bound.
  blend        a1 exact, a0 = fl(1 - a1) carries u.  L = a0 H0 + a1 H1:  dL <= a0 dH0 + a1 dH1 + u |H0| + u (|a0 H0| + |a1 H1|) + u |L|;
               num, den, N = num + e L, D = den + e and the quotient as in 19.4.  Each of the R blends is bounded by itself.
  gradient     per blend r as DESIGN 22.4 (slopes 22 u M, the term, the sum over c, the factor), with the forward bound d out_rc above
               and the factor k = c a / D at 5u instead of 4u (the rounding of c1).
  sum over r   the R contributions v_1 .. v_R of one element are added in ascending r: sum_r dv_r + (R - 1) u sum_r |v_r|.
  rev          where G0 = G1 the lane writes dG0 + dG1: both bounds, and one rounding of the sum, u (|dG0| + |dG1|).

A pair outside [0, B) gives zeros with budget 0; a sample whose coordinate is not finite, or 1e9 or more in size, contributes exactly 0
in both precisions.  Second-order terms are covered by the factor 1 + 2^-10 of the forward budget.
"""
import numpy as np
import torch

from flowgather_grad_refs import _slopes
from flowgather_refs import EPS, SECOND_ORDER, U, _cell, _padded, frames

FACTOR_ROUNDINGS = 5


def _resolve(fl, tau, rev):
    """(G0 (2, N), G1 (2, N), c0, c1, back) from flows (S, 4, N) float64"""
    n = fl.shape[2]
    if fl.shape[0] == 1:
        back = np.ones(n, dtype=bool)
    else:
        back = np.zeros(n, dtype=bool) if rev is None else np.asarray(rev).astype(bool)
    g1 = fl[0, 0:2]
    g0 = np.where(back, g1, fl[1, 2:4]) if fl.shape[0] == 2 else g1
    return g0, g1, np.where(back, -tau, tau), 1 - tau, back


def _geom(c, extra, gx, gy, px, py):
    with np.errstate(invalid='ignore', over='ignore'):
        sx, sy = c * gx, c * gy
        qx, qy = px + sx, py + sy
    ok = np.isfinite(qx) & np.isfinite(qy) & (np.abs(qx) < 1e9) & (np.abs(qy) < 1e9)
    qx, qy, sx, sy = (np.where(ok, a, 0.0) for a in (qx, qy, sx, sy))
    return ok, qx, qy, U * ((1 + extra) * np.abs(sx) + np.abs(qx)), U * ((1 + extra) * np.abs(sy) + np.abs(qy))


def _value(plane, ok, qx, qy, dqx, dqy):
    """(W, dW) of one plane at the coordinates q, in the cell floor(q)"""
    fx, fy = np.floor(qx), np.floor(qy)
    ax, ay = qx - fx, qy - fy
    t00, t01, t10, t11 = _cell(_padded(plane), fx.astype(np.int64), fy.astype(np.int64))
    val = (1 - ay) * ((1 - ax) * t00 + ax * t01) + ay * ((1 - ax) * t10 + ax * t11)
    slope_x = np.maximum(np.abs(t01 - t00), np.abs(t11 - t10))
    slope_y = np.maximum(np.abs(t10 - t00), np.abs(t11 - t01))
    big = np.max(np.abs(np.stack([t00, t01, t10, t11])), 0)
    return np.where(ok, val, 0.0), np.where(ok, dqx * slope_x + dqy * slope_y + 19 * U * big, 0.0)


def _np64(t):
    return t.detach().cpu().to(torch.float64).numpy()


def gather_at64(frame1, frame2, flows, pix, pair, tau, rev=None, blend=None, grad_out=None):
    """see the module text.  `blend`: the values as the kernel sees them, rounded to fp32; None: a1 = tau."""
    i0, i1, fl, p, t = (_np64(x) for x in (frame1, frame2, flows, pix, tau))
    who = pair.detach().cpu().numpy().astype(np.int64)
    back_in = None if rev is None else rev.detach().cpu().numpy()
    g = None if grad_out is None else _np64(grad_out)
    b, c, h, w = i0.shape
    s, _, n = fl.shape
    g0, g1, c0, c1, back = _resolve(fl, t, back_in)
    blends = [t] if blend is None else [np.full(n, float(np.float32(v))) for v in blend]
    r_count = len(blends)
    out, budget = np.zeros((r_count, n, c)), np.zeros((r_count, n, c))
    grad, gbudget = np.zeros(fl.shape), np.zeros(fl.shape)
    ones = np.ones((h, w))
    for bb in range(b):
        sel = np.nonzero(who == bb)[0]
        if sel.size == 0:
            continue
        px, py = p[sel, 1], p[sel, 0]
        imgs = (i0[bb], i1[bb])
        geo = (_geom(c0[sel], 0, g0[0, sel], g0[1, sel], px, py), _geom(c1[sel], 1, g1[0, sel], g1[1, sel], px, py))
        here = _geom(np.zeros(sel.size), 0, np.zeros(sel.size), np.zeros(sel.size), px, py)
        here = (here[0], here[1], here[2], np.zeros(sel.size), np.zeros(sel.size))          # p is exact
        wv = [[_value(imgs[k][cc], *geo[k]) for cc in range(c)] for k in range(2)]
        nv = [_value(ones, *geo[k]) for k in range(2)]
        hv = [[_value(imgs[k][cc], *here) for cc in range(c)] for k in range(2)]
        coef = (c0[sel], c1[sel])
        tot = np.zeros((2, 2, sel.size))
        err, mag = np.zeros((2, 2, sel.size)), np.zeros((2, 2, sel.size))
        for r in range(r_count):
            a1 = blends[r][sel]
            a0 = 1 - a1
            a = (a0, a1)
            (n0, dn0), (n1, dn1) = nv
            den = a0 * n0 + a1 * n1
            bottom = den + EPS
            d_den = a0 * dn0 + a1 * dn1 + U * (np.abs(n0) + np.abs(a0 * n0) + np.abs(a1 * n1) + np.abs(den))
            d_bottom = d_den + U * np.abs(bottom)
            assert float((bottom - d_bottom).min()) > 0.5 * EPS
            res, d_res = [], []
            for cc in range(c):
                (w0, dw0), (w1, dw1), (h0, dh0), (h1, dh1) = wv[0][cc], wv[1][cc], hv[0][cc], hv[1][cc]
                lin = a0 * h0 + a1 * h1
                d_lin = a0 * dh0 + a1 * dh1 + U * (np.abs(h0) + np.abs(a0 * h0) + np.abs(a1 * h1) + np.abs(lin))
                num = a0 * w0 + a1 * w1
                d_num = a0 * dw0 + a1 * dw1 + U * (np.abs(w0) + np.abs(a0 * w0) + np.abs(a1 * w1) + np.abs(num))
                top = num + EPS * lin
                d_top = d_num + EPS * d_lin + U * np.abs(top)
                val = top / bottom
                res.append(val)
                d_res.append((d_top + np.abs(val) * d_bottom) / (bottom - d_bottom) + U * np.abs(val))
                out[r, sel, cc] = val
                budget[r, sel, cc] = SECOND_ORDER * d_res[-1]
            if g is None:
                continue
            for k in range(2):
                ok, qx, qy, dqx, dqy = geo[k]
                nx, ny, enx, eny, _ = _slopes(ones, ok, qx, qy, dqx, dqy)
                sums, errs, sizes = [0.0, 0.0], [0.0, 0.0], 0.0
                for cc in range(c):
                    wx, wy, ewx, ewy, big = _slopes(imgs[k][cc], ok, qx, qy, dqx, dqy)
                    gc = g[r, sel, cc]
                    for axis, (sw, sn, ew, en) in enumerate(((wx, nx, ewx, enx), (wy, ny, ewy, eny))):
                        term = sw - res[cc] * sn
                        d_term = ew + d_res[cc] * np.abs(sn) + np.abs(res[cc]) * en + 2 * U * np.abs(res[cc] * sn) + U * np.abs(term)
                        sums[axis] = sums[axis] + gc * term
                        errs[axis] = errs[axis] + np.abs(gc) * d_term
                    sizes = sizes + np.abs(gc) * (2 * big + np.abs(res[cc]))
                factor = coef[k] * a[k] / bottom
                rel = FACTOR_ROUNDINGS * U + d_bottom / (bottom - d_bottom)
                for axis in range(2):
                    val = factor * sums[axis]
                    d_val = np.abs(factor) * (errs[axis] + c * U * sizes) + np.abs(val) * rel
                    val, d_val = np.where(ok, val, 0.0), np.where(ok, d_val, 0.0)
                    tot[k, axis] += val
                    err[k, axis] += d_val
                    mag[k, axis] += np.abs(val)
        if g is None:
            continue
        err = err + U * (r_count - 1) * mag
        bk = back[sel]
        for axis in range(2):
            both = tot[0, axis] + tot[1, axis]
            both_err = err[0, axis] + err[1, axis] + U * (np.abs(tot[0, axis]) + np.abs(tot[1, axis]))
            grad[0, axis, sel] = np.where(bk, both, tot[1, axis])
            gbudget[0, axis, sel] = np.where(bk, both_err, err[1, axis])
            if s == 2:
                grad[1, 2 + axis, sel] = np.where(bk, 0.0, tot[0, axis])
                gbudget[1, 2 + axis, sel] = np.where(bk, 0.0, err[0, axis])
    as_t = torch.from_numpy
    if g is None:
        return as_t(out), as_t(budget), None, None
    return as_t(out), as_t(budget), as_t(grad), as_t(SECOND_ORDER * gbudget)


def _coordinates(flows, pix, tau, rev, dtype):
    """[(qx, qy) of sample 0, of sample 1] evaluated in `dtype` from the fp32 inputs, the product rounded, then the sum"""
    fl = flows.detach().cpu().numpy().astype(np.float32).astype(dtype)
    p = pix.detach().cpu().numpy().astype(np.float32).astype(dtype)
    t = tau.detach().cpu().numpy().astype(np.float32).astype(dtype)
    g0, g1, c0, c1, _ = _resolve(fl, t, None if rev is None else rev.detach().cpu().numpy())
    with np.errstate(invalid='ignore', over='ignore'):
        return [(p[:, 1] + c0 * g0[0], p[:, 0] + c0 * g0[1]), (p[:, 1] + c1 * g1[0], p[:, 0] + c1 * g1[1])]


def cells_agree(flows, pix, tau, rev=None):
    """True where, for every point, sample and axis, the fp32 coordinate and the float64 one are accepted or refused alike and fall
    into the same cell"""
    same = True
    for (x32, y32), (x64, y64) in zip(_coordinates(flows, pix, tau, rev, np.float32), _coordinates(flows, pix, tau, rev, np.float64)):
        with np.errstate(invalid='ignore'):
            ok32 = (np.abs(x32) < np.float32(1e9)) & (np.abs(y32) < np.float32(1e9))
            ok64 = (np.abs(x64) < 1e9) & (np.abs(y64) < 1e9)
        same = same and bool((ok32 == ok64).all())
        both = ok32 & ok64
        for q32, q64 in ((x32, x64), (y32, y64)):
            same = same and bool((np.floor(q32[both]).astype(np.float64) == np.floor(q64[both])).all())
    return same


# ---- inputs ----

def _in_range(q):
    f = q - np.floor(q)
    return (f >= 1 / 16) & (f <= 15 / 16)


def points(seed, n, b, h, w, s, some_rev):
    """(flows (s, 4, n), pix (n, 2), pair (n,) int32, tau (n,), rev (n,) bool or None), fp32, drawn by rejection until p, q0 and q1 of
    every point have fractional parts in [1/16, 15/16] on both axes (p may also be an exact integer: an axis of length 1 has no other
    value).  Every eighth point is an integer pixel with tau = 1/2 and even integer flows: p, q0 and q1 exact integers, half of them
    outside the frame or on its last row and column.  One flow in ten carries its sample far across a border."""
    rng = np.random.default_rng(seed)
    fl = np.zeros((s, 4, n), dtype=np.float32)
    pix, tau = np.zeros((n, 2), dtype=np.float32), np.zeros(n, dtype=np.float32)
    pair = rng.integers(0, b, n).astype(np.int32)
    rev = (rng.random(n) < 0.3) if (s == 2 and some_rev) else None
    todo = np.arange(n)
    while todo.size:
        m = todo.size
        pix[todo, 0], pix[todo, 1] = rng.random(m) * (h - 1), rng.random(m) * (w - 1)
        tau[todo] = 0.05 + 0.9 * rng.random(m)
        draw = (rng.random((s, 4, m)) * 2 - 1) * 6.0
        far = rng.random((s, 4, m)) < 0.1
        draw = np.where(far, draw * np.array([w, h, w, h]).reshape(1, 4, 1), draw)
        fl[:, :, todo] = draw
        whole = todo[todo % 8 == 0]
        pix[whole, 0], pix[whole, 1] = rng.integers(0, h, whole.size), rng.integers(0, w, whole.size)
        tau[whole] = 0.5
        fl[:, :, whole] = 2.0 * rng.integers(-3, 4, (s, 4, whole.size))
        corner = whole[whole % 16 == 0]
        pix[corner, 0], pix[corner, 1] = h - 1, w - 1
        f64, p64, t64 = fl.astype(np.float64), pix.astype(np.float64), tau.astype(np.float64)
        g0, g1, c0, c1, _ = _resolve(f64, t64, rev)
        good = np.ones(n, dtype=bool)
        for axis, col in ((0, 1), (1, 0)):
            pa = p64[:, col]
            good &= _in_range(pa) | (pa == np.floor(pa))
            for q in (pa + c0 * g0[axis], pa + c1 * g1[axis]):
                good &= _in_range(q) | ((np.arange(n) % 8 == 0) & (q == np.floor(q)))
        todo = todo[~good[todo]]
    as_t = torch.from_numpy
    return as_t(fl), as_t(pix), as_t(pair), as_t(tau), None if rev is None else as_t(rev)


def grad_out(seed, r, n, c):
    g = torch.Generator().manual_seed(seed + 1000)
    return (torch.rand(r, n, c, generator=g) * 2 - 1).contiguous()


# name -> (seed, n, b, c, h, w, s, blend, some_rev): the cases of the issue
CASES = {
    '1': (1, 1, 1, 1, 1, 1, 1, (0.5,), False),
    '255': (2, 255, 2, 3, 13, 37, 2, (0.0, 1.0), True),
    '256': (3, 256, 2, 3, 13, 37, 2, (0.0, 1.0), True),
    '257': (4, 257, 2, 3, 13, 37, 2, (0.0, 1.0), True),
    '1031': (5, 1031, 1, 1, 5, 1031, 1, None, False),
    '4099': (6, 4099, 3, 3, 24, 40, 2, (0.0, 1.0, 0.25, 0.6875), False),
}


def case(name):
    """(frame1, frame2, flows, pix, pair, tau, rev, blend, grad_out), fp32 / int32 / bool on the CPU"""
    seed, n, b, c, h, w, s, blend, some_rev = CASES[name]
    i0, i1 = frames(seed, b, c, h, w)
    fl, pix, pair, tau, rev = points(seed, n, b, h, w, s, some_rev)
    return i0, i1, fl, pix, pair, tau, rev, blend, grad_out(seed, 1 if blend is None else len(blend), n, c)
