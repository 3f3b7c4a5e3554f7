"""TEST INFRASTRUCTURE: the float64 reference, the per-element budget and the cases of the occlusion-aware gather tests
(tests/test_flowgather_visible_host.py, tests/test_gpu_flowgather_visible.py).

    gather_visible64(i0, i1, flows, slots, taus, m0, m1)   the definition in float64 with numpy index arithmetic, one (b, k) at a time,
                                                           on the sampler of tests/flowgather_refs.py.  It shares no code with
                                                           `flowsynth.gather_composed`.  Returns (out, budget), (B, K, C, H, W) float64.
    CASES, case(name)                                      the shapes, flows and masks of the tests

The rule, in the notation of csrc/flowgather.hip (m0 is 1 where a pixel of frame 0 is visible in frame 1, m1 the reverse):

    o0 = S(1 - m0, q0), o1 = S(1 - m1, q1);  v0 = 1 - o1, v1 = 1 - o0;  b0 = a0 v0, b1 = a1 v1
    out = (b0 W0 + b1 W1 + e L) / (b0 n0 + b1 n1 + e)

The budget follows the method of tests/flowgather_refs.py (first order in u = 2^-24, inputs exact, times 1 + 2^-10), with these terms
added to its list:

  hidden plane 1 - m carries one rounding, u |1 - m| per tap; the weights inside sum to at most 1:  u max|1 - m| on o
  o            the sample of that plane: the coordinate and in-cell terms of `_sample`, with the plane's own slopes and taps
  v            v0 = 1 - o1:  dv0 <= do1 + u |v0|;  v1 likewise
  b            b0 = a0 v0 with a0 = fl(1 - tau) carrying u:  db0 <= u |b0| + a0 dv0 + u |b0|;   b1 = a1 v1, a1 exact:  db1 <= a1 dv1 + u |b1|
  num          b0 W0 + b1 W1:  dnum <= |b0| dW0 + |W0| db0 + |b1| dW1 + |W1| db1 + u (|b0 W0| + |b1 W1|) + u |num|;   den likewise from n
  L, N, D, quotient   as there, with |D| in place of D: a mask below 0 makes v, and so D, negative

Masks inside [0, 1] keep D >= e.  The cases also hold values outside it; `gather_visible64` asserts |D| - dD > e / 2 on every element, a
condition on the inputs that the reference checks alone.
"""
import numpy as np
import torch

import flowgather_refs as R

U, EPS, SECOND_ORDER = R.U, R.EPS, R.SECOND_ORDER


def gather_visible64(frame1, frame2, flows, slots, taus, mask0, mask1):
    i0, i1, fl, m0, m1 = (t.detach().cpu().to(torch.float64).numpy() for t in (frame1, frame2, flows, mask0, mask1))
    table = slots.numpy()
    coef = table[..., 4:].copy().view(np.float32).astype(np.float64)
    tau = np.asarray([float(t) for t in taus], dtype=np.float32).astype(np.float64)
    b, c, h, w = i0.shape
    assert m0.shape == m1.shape == (b, 1, h, w)
    k = len(tau)
    ys, xs = np.meshgrid(np.arange(h, dtype=np.float64), np.arange(w, dtype=np.float64), indexing='ij')
    ones = np.ones((h, w))
    out, budget = np.zeros((b, k, c, h, w)), np.zeros((b, k, c, h, w))
    for bb in range(b):
        hid0, hid1 = 1 - m0[bb], 1 - m1[bb]                 # (1, H, W)
        for kk in range(k):
            idx0, idx1, ch0, ch1 = (int(v) for v in table[bb, kk, :4])
            s0 = R._sample(np.concatenate([i0[bb], hid0]), ones, coef[bb, kk, 0], fl[idx0, ch0], fl[idx0, ch0 + 1], xs, ys)
            s1 = R._sample(np.concatenate([i1[bb], hid1]), ones, coef[bb, kk, 1], fl[idx1, ch1], fl[idx1, ch1 + 1], xs, ys)
            (w0, o0, dw0, do0), n0, dn0 = _split(s0, c), s0[1], s0[3]
            (w1, o1, dw1, do1), n1, dn1 = _split(s1, c), s1[1], s1[3]
            do0, do1 = do0 + U * np.abs(hid0).max(), do1 + U * np.abs(hid1).max()
            a1 = tau[kk]
            a0 = 1 - a1
            v0, v1 = 1 - o1, 1 - o0
            dv0, dv1 = do1 + U * np.abs(v0), do0 + U * np.abs(v1)
            b0, b1 = a0 * v0, a1 * v1
            db0, db1 = a0 * dv0 + 2 * U * np.abs(b0), a1 * dv1 + U * np.abs(b1)
            lin = a0 * i0[bb] + a1 * i1[bb]
            num = b0 * w0 + b1 * w1
            den = b0 * n0 + b1 * n1
            top, bottom = num + EPS * lin, den + EPS
            res = top / bottom
            d_lin = U * (np.abs(i0[bb]) + np.abs(a0 * i0[bb]) + np.abs(a1 * i1[bb]) + np.abs(lin))
            d_num = (np.abs(b0) * dw0 + np.abs(w0) * db0 + np.abs(b1) * dw1 + np.abs(w1) * db1
                     + U * (np.abs(b0 * w0) + np.abs(b1 * w1) + np.abs(num)))
            d_den = (np.abs(b0) * dn0 + np.abs(n0) * db0 + np.abs(b1) * dn1 + np.abs(n1) * db1
                     + U * (np.abs(b0 * n0) + np.abs(b1 * n1) + np.abs(den)))
            d_top = d_num + EPS * d_lin + U * np.abs(top)
            d_bottom = d_den + U * np.abs(bottom)
            assert float((np.abs(bottom) - d_bottom).min()) > 0.5 * EPS, 'a case whose denominator comes within e / 2 of zero'
            out[bb, kk] = res
            budget[bb, kk] = SECOND_ORDER * ((d_top + np.abs(res) * d_bottom) / (np.abs(bottom) - d_bottom) + U * np.abs(res))
    return torch.from_numpy(out), torch.from_numpy(budget)


def _split(sample, c):
    """(W (C, H, W), o (H, W), dW, do) of a `_sample` over the frame's planes followed by the hidden plane"""
    vals, _, errs, _ = sample
    return vals[:c], vals[c], errs[:c], errs[c]


# ---- inputs ----

def masks(seed, b, h, w):
    """(m0, m1), (b, 1, h, w) fp32: hard 0 / 1 regions with fractional seams; a patch where both are 0; values above 1 in one patch and
    (slightly) below 0 in another"""
    g = torch.Generator().manual_seed(1000 + seed)
    out = []
    for _ in range(2):
        s = R.smooth(g, b, 1, h, w, grid=(4, 5))
        m = ((s - 0.35) * 6).clamp(0, 1)                     # 0 below 0.35, 1 above 0.52, a ramp between
        out.append(m.contiguous())
    m0, m1 = out
    if h >= 5 and w >= 16:
        m0[:, :, 1:3, 2:6] = 0.0
        m1[:, :, 1:3, 2:6] = 0.0
        m0[:, :, h - 3:h - 1, 3:7] = 1.5
        m1[:, :, h - 3:h - 1, w - 9:w - 5] = 1.25
        m0[:, :, 2:4, w - 6:w - 3] = -0.125
        m1[:, :, h // 2:h // 2 + 2, 8:11] = -0.0625
    return m0, m1


# name -> (seed, b, c, h, w, taus, time slices).  7x300: 256-pixel blocks wrap rows; the GPU test alone runs it
CASES = {
    '1x1': (11, 1, 3, 1, 1, (0.5,), 3),
    '2x3': (12, 1, 1, 2, 3, (0.0, 0.5, 1.0), 4),
    '9x33': (13, 2, 3, 9, 33, (0.0, 0.3, 1.0), 7),
    '7x300': (14, 2, 1, 7, 300, (0.25, 0.5, 0.875), 7),
}
HOST_CASES = ('1x1', '2x3', '9x33')


def case(name):
    """(frame1, frame2, flows, slots, taus, m0, m1), fp32 / int32 on the CPU.  The flows are `flowgather_refs.border_flows`: landing
    points outside the frame on every side; on top of them pixels whose landing points are exactly integer pixels (zero and whole-number
    flows under c = 0, 1/2 and 1) and, from 9x33 up, a NaN and an infinite flow."""
    seed, b, c, h, w, taus, slices = CASES[name]
    i0, i1 = R.frames(seed, b, c, h, w)
    if name == '1x1':
        # slice 0: I1 is sampled at (0.3, -0.2) (1 - tau): two taps inside; slice 1: I0 leaves the frame; fractional masks
        fl = torch.tensor([[0.6, -0.4, 9.0, 9.0], [1.0, 1.0, 5.0, 5.0], [0.0, 0.0, 0.0, 0.0]]).reshape(3, 4, 1, 1)
        half = int(np.float32(0.5).view(np.int32))
        table = torch.tensor([[[1, 0, 2, 0, half, half]]], dtype=torch.int32)
        return i0, i1, fl, table, taus, torch.full((1, 1, 1, 1), 0.75), torch.full((1, 1, 1, 1), 0.25)
    fl = R.border_flows(seed, slices, h, w)
    fl[:, :, 0, 0] = 0.0                                     # q = p
    fl[:, :, h - 1, w - 1] = torch.tensor([-2.0, 0.0, 2.0, -2.0])      # whole pixels under c = 1/2 and 1, one of them outside
    if h >= 5:
        fl[:, 0, 4, 7] = float('nan')
        fl[:, 2, 4, 7] = float('nan')
        fl[:, 1, 5, 20] = float('inf')
        fl[:, 3, 5, 20] = float('-inf')
    m0, m1 = masks(seed, b, h, w)
    return i0, i1, fl, R.mixed_slots(b, len(taus), slices, taus, seed), taus, m0, m1
