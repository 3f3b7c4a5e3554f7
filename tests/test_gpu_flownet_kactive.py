"""GPU: `k_active` swept through every skip boundary of the progressive flow networks (PRBF / PFF / PUFF / PRFF of csrc/flownet.hip),
masks with interior zeros, and closed weights that hold NaN.

The launch plan derives four quantities from oe = max(k_active - 3, 0): ksteps = ceil(oe / 16) (layer-1 K loop of the forward),
ktiles = max(1, ceil(oe / 128)) (grid of the layer-1 weight gradient), kcols = 128 ktiles (flownet_reduce_prog_kernel) and
fopen = (oe + 1) / 2 (per-wave skip of flownet_encgrad_kernel, 32 frequencies per wave and 128 per pass, and flownet_reduce_enc_kernel).
KS holds the neighbours of every boundary: ksteps 19 | 20, ktiles 131 | 132, 259 | 260, 387 | 388, fopen 32 | 33 (66, 67 | 68) and
128 | 129 (258, 259 | 260), no encoded feature open (k <= 3), nothing open (k = 0).

Method and budget are those of tests/test_gpu_flownet.py, unchanged (`check`: error against float64 <= min(4 x the deviation of the
same formula in fp32 torch, measured here, 1e-4), max-norm relative to max |ref|, gradients with the kernel's own gates forced).
What is sharper here is exact:
  * the inference and the training forward, and the skipped (k_active = k) and the unskipped (k_active = 515) path, agree bitwise in
    flows, in `saved` and in all eight gradients (nine with gF), from NaN-filled `saved` and workspaces;
  * rows N .. Npad - 1 of every saved layer equal row N - 1 (the clamped point);
  * gW1 where the mask is zero and gF where both features of a frequency are closed are +0 with the sign bit clear; every open
    column / frequency has a nonzero entry (but for the RBF features that are below FLT_MIN at every point of the grid, see
    live_features: their column is honestly zero in fp32);
  * `saved[0][:N]` (h1, what the layer under test writes) is compared with float64, not only asserted finite;
  * gW1 is checked as a whole, on the coordinate columns alone and on every open 128-column tile alone, each relative to its own max;
  * where the float64 reference of a quantity is identically zero (gW1 at k = 0, gF at k <= 3) the kernel's is asserted exact +0;
  * closed columns of W1 that hold NaN change no bit of any output (the promise of flownet_pack_kernel / flownet_encgrad_pack_kernel).
gb4 = scale * sum(up) does not depend on the network, the mask or k_active and stands at 0.90 - 0.94 of a budget whose unit is one
fp32 sum in the sibling files; it is covered by the bitwise assertions here and not compared with float64.

test_reduce_never_reads_an_uncomputed_column: with an honest k_active the `k - 3 >= kcols` clause of flownet_reduce_prog_kernel is
shadowed by its mask test (a column beyond kcols is beyond k_active, so its mask is zero).  The clause is what keeps uninitialised
partial sums out of gW1, so it is pinned on its own: the mask says open, k_active says the tile was not computed, the workspace
holds NaN, and the columns from 3 + kcols on must be +0.

Grids: `sweep`, times (0, 0.25, 1) x 61 x 181: N = 33 123, hw = 11 041 (tiles straddle frames), 518 tiles with a last one of 35
points, 518 > 512 (six blocks of the chain / encgrad kernels take two tiles), 8 or 9 tiles per layer-1 weight-gradient chunk (the
prefetch is live); `single`, (0.5,) x 5 x 7: one partial tile, one chunk, one block.

Measured on an MI355X (worst error / budget over all cases, from the `ratio(...)` lines of a run with -s; where: [error, fp32-torch unit]):
  flows 0.25 (PRBF sweep k=0) [5.33e-08, 5.33e-08]  h1 0.344 (PRBF single k=6) [1.02e-07, 7.44e-08]
  gW1 0.3 (PRBF single k=132) [5.16e-07, 4.30e-07]  coordinate columns 0.292 (PRBF single k=6)  one tile 0.333 (PRBF single k=6, tile 0)
  gb1 0.35 (PRBF single k=132)  gW2 0.29 (PRBF single k=132)  gb2 0.451 (PRBF sweep k=386)  gW3 0.307 (PRBF single k=515)
  gb3 0.568 (PRFF single k=132) [2.60e-07, 1.14e-07]  gW4 0.413 (PRBF single k=132)
  gF 0.306 (PRFF sweep k=67) [1.47e-06, 1.20e-06]  freq.grad 0.383 (PRFF sweep k=67)  gF at frequency 20 under the holes mask 0.065
  15 quantities took the exact branch of check_or_zero (k = 0: gW1 and h1; k <= 3: gF and freq.grad; the coordinate columns at k = 0).
  The clamped-row assertion failed for PRBF at every k >= 18 before encode4 summed the RBF distance with explicit fmaf (the compiler
  had contracted `dt * dt + dy * dy + dx * dx` differently for one of the four points a lane encodes).  80 tests, 7 s.
"""
import os
import sys

import pytest
import torch

pytestmark = pytest.mark.gpu
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import flownet_refs as R  # noqa: E402
import test_flownet_learnable_golden as L  # noqa: E402
import test_flownet_progressive_golden as P  # noqa: E402
from flownet_refs import closed_frequencies, is_plus_zero, nan_buffers, restate  # noqa: E402
from test_gpu_flownet import CEIL, F64, MULT, axes, check  # noqa: E402

assert (MULT, CEIL) == (4.0, 1e-4)                     # the standing budget; this file does not choose one
SCALE = P.SCALE
F32 = torch.float32
GRIDS = {'sweep': ((0.0, 0.25, 1.0), 61, 181), 'single': ((0.5,), 5, 7)}
KS = (0, 1, 3, 4, 18, 19, 20, 66, 67, 68, 130, 131, 132, 258, 259, 260, 386, 387, 388, 514, 515)
K_HOLES = 300
GNAMES = [f'g{k}{l}' for l in (1, 2, 3, 4) for k in ('W', 'b')]
NAN = float('nan')


@pytest.fixture(scope='module')
def dev():
    import sin_inn_amd  # noqa: F401
    assert torch.cuda.is_available(), 'GPU tests need a GPU'
    return torch.device('cuda', 0)


def prefix_mask(k):
    """k leading ones, the last min(3, k) of them at 0.5 as for a block in progress"""
    from sin_inn_amd import flownet
    mask = torch.zeros(515)
    mask[:k] = 1.0
    mask[k - min(3, k):k] = 0.5
    assert flownet.last_open(mask) == k
    return mask


def holes_mask():
    """K_HOLES leading values from {0.25, 0.5, 1} and zeros inside: coordinate y; encoded features 16 - 31 (one K step); feature 40
    (the sin of frequency 20, its cos open); 42 and 43 (frequency 21); 128 - 255 (one weight-gradient tile, frequencies 64 - 127)"""
    from sin_inn_amd import flownet
    pick = torch.randint(0, 3, (515,), generator=torch.Generator().manual_seed(5))
    mask = torch.tensor([0.25, 0.5, 1.0])[pick]
    mask[K_HOLES:] = 0.0
    mask[1] = 0.0
    for a, b in ((16, 32), (40, 41), (42, 44), (128, 256)):
        mask[3 + a:3 + b] = 0.0
    assert flownet.last_open(mask) == K_HOLES and float(mask[3 + 41]) > 0 and float(mask[K_HOLES - 1]) > 0
    return mask


def restate_h1(name, enc, weights, times, ys, xs, scale, dtype, mask, gates=None):
    """`restate` of tests/flownet_refs.py (enc: the buffers of PRBF / PFF / PUFF, or F_eff (3, 256) of PRFF) that also returns h1, the
    output of layer 1; run_case ties its flows to that one's"""
    t, h, w = times.numel(), ys.numel(), xs.numel()
    weights = [p.to(dtype) for p in weights]
    x = R.layer1_input(name, enc, R.poses_of(times, ys, xs, dtype), mask)
    h1 = None
    for l in range(3):
        pre = torch.nn.functional.linear(x, weights[2 * l], weights[2 * l + 1])
        x = torch.relu(pre) if gates is None else pre * gates[l].to(dtype)
        h1 = x if l == 0 else h1
    out = torch.nn.functional.linear(x, weights[6], weights[7])
    return out.view(t, h, w, 4).permute(0, 3, 1, 2) * scale, h1


def check_or_zero(tag, got, r64, r32, signed=True):
    """`check`; where the float64 reference is identically zero, exact +0 instead (check divides by max |ref|; signed=False: a zero
    of either sign, for a quantity torch ops derive from the kernel's); where the fp32 restatement equals the float64 one in every
    element the unit and so the budget are zero, which `check` cannot print: the kernel must then equal the reference as well"""
    if float(r64.abs().max()) == 0.0:
        print(f'exact({tag}): the float64 reference is identically zero')
        assert is_plus_zero(got) if signed else bool((got == 0.0).all()), f'{tag}: not zero where the reference is identically zero'
    elif torch.equal(r32.to(F64), r64):
        print(f'exact({tag}): the fp32 restatement equals the float64 one, budget 0')
        assert torch.equal(got.to(F64), r64), f'{tag}: differs from a reference that fp32 represents exactly'
    else:
        check(tag, got, r64, r32)


class Net:
    """a network on the device with what the kernels and the restatement read"""

    def __init__(self, name, dev):
        self.name, self.prff = name, name == 'PRFF'
        self.net = (L if self.prff else P).build(name).to(dev)
        if self.prff:
            bufs, self.weights = R.net_tensors(self.net, dev)
            self.freq, self.mag = bufs['encode.frequencies'], bufs['encode.magnitudes']
            self.enc = L.f_eff(self.freq, self.mag).contiguous()              # the fp32 matrix the kernels receive
            self.ekw = dict(enc_a=self.enc)
        else:
            self.enc, self.weights = R.net_tensors(self.net, dev)
            self.ekw = {}
        self.weights = [w.clone() for w in self.weights]                    # the reference keeps the clean weights


def live_features(nt, times, ys, xs):
    """(515,) bool: the features that are a normal fp32 number at some point of the grid.  An RBF centre far from the grid with a
    narrow width gives exp(-x) below FLT_MIN at every point; fp32 rounds or flushes that to zero, and the gradient column of such a
    feature is honestly all zero although its mask is open (float64 holds 1e-60 there; the comparison with float64 covers it).  The
    factor 2 is far above the 1e-5 that the fp32 rounding of an exponent of 87 moves the value by.  Fourier features are all live"""
    poses = R.poses_of(times, ys, xs, F64)
    live = torch.ones(515, dtype=torch.bool, device=poses.device)
    if nt.name == 'PRBF':
        live[3:] = R.encode_rbf(nt.enc, poses).abs().amax(dim=0) >= 2 * torch.finfo(F32).tiny
    live[:3] = poses.abs().amax(dim=0) > 0
    return live


def run_kernels(nt, grid, hmask, k, dev):
    """the exact assertions of one case (forward and backward, skipped against unskipped); returns what the float64 part compares"""
    from sin_inn_amd import flownet
    times, ys, xs = axes(GRIDS[grid], dev)
    n = times.numel() * ys.numel() * xs.numel()
    mask = hmask.to(dev)
    skip = dict(nt.ekw, mask=mask, k_active=k)
    full = dict(nt.ekw, mask=mask, k_active=515)

    # ---- forward: both modes, skipped and unskipped, from NaN-filled saved ----
    infer, none = flownet.flownet_forward(nt.net, times, ys, xs, SCALE, False, **skip)
    assert none is None
    saved, ws, ews = nan_buffers(n, dev)
    train, saved = flownet.flownet_forward(nt.net, times, ys, xs, SCALE, True, saved, **skip)
    assert torch.equal(infer, train), 'the inference and the training forward differ'
    assert bool(torch.isfinite(saved).all()) and float(saved.min()) >= 0.0
    saved_full = torch.full_like(saved, NAN)
    flows_full, saved_full = flownet.flownet_forward(nt.net, times, ys, xs, SCALE, True, saved_full, **full)
    assert torch.equal(flows_full, infer), 'skipping the closed features changed the flows'
    assert torch.equal(saved_full, saved), 'skipping the closed features changed saved'
    npad = saved.shape[1]
    assert npad == (n + 63) // 64 * 64 and npad > n
    for l in range(3):
        assert torch.equal(saved[l, n:], saved[l, n - 1:n].expand(npad - n, 256)), f'saved[{l}]: the rows beyond N are not the clamped point'
    del flows_full, saved_full, train

    # ---- backward: two skipped calls and one unskipped, each from NaN-filled workspaces ----
    up = torch.randn(infer.shape, generator=torch.Generator().manual_seed(11)).to(dev)
    runs = []
    for kw in (skip, skip, full):
        ws.fill_(NAN)
        ews.fill_(NAN)
        if nt.prff:
            g_enc = torch.full((3, 256), NAN, device=dev)
            got, gF = flownet.flownet_backward(nt.net, times, ys, xs, SCALE, up, saved, ws, enc_grad=True, enc_workspace=ews, g_enc_a=g_enc, **kw)
            assert gF is g_enc
            runs.append(got + [gF])
        else:
            runs.append(flownet.flownet_backward(nt.net, times, ys, xs, SCALE, up, saved, ws, **kw))
    names = GNAMES + (['gF'] if nt.prff else [])
    for nm, a, b, c in zip(names, *runs):
        assert bool(torch.isfinite(a).all()), nm
        assert torch.equal(a, b), f'{nm}: two backward calls differ'
        assert torch.equal(a, c), f'{nm}: the skipped and the unskipped path differ'
    closed = (hmask == 0).to(dev)
    live = live_features(nt, times, ys, xs)
    for r in (runs[0], runs[2]):
        assert tuple(r[0].shape) == (256, 515)
        assert is_plus_zero(r[0][:, closed]), 'gW1 is not +0 where the mask is zero'
        assert bool((r[0][:, ~closed & live] != 0.0).any(dim=0).all()), 'an open column of gW1 is all zero'
        if nt.prff:
            fclosed = closed_frequencies(hmask).to(dev)
            assert is_plus_zero(r[8][:, fclosed]), 'gF is not +0 at a closed frequency'
            assert bool((r[8][:, ~fclosed] != 0.0).any(dim=0).all()), 'an open frequency has an all-zero gradient'
    return dict(axes=(times, ys, xs), n=n, mask=mask, flows=infer, saved=saved, up=up, grads=runs[0], live=live)


def run_case(dev, name, grid, hmask, k, tag):
    """all assertions of case 1 for one network, grid and mask; returns the kernel's outputs and the references"""
    nt = Net(name, dev)
    out = run_kernels(nt, grid, hmask, k, dev)
    times, ys, xs = out['axes']
    n, mask, saved, up, grads = out['n'], out['mask'], out['saved'], out['up'], out['grads']

    # ---- forward against float64: flows and h1 ----
    with torch.no_grad():
        ref = {}
        for dtype in (F64, F32):
            ref[dtype] = restate_h1(name, nt.enc, nt.weights, times, ys, xs, SCALE, dtype, mask)
            theirs = restate(name, nt.enc, nt.weights, times, ys, xs, SCALE, dtype, mask)
            assert torch.equal(ref[dtype][0], theirs), f'restate_h1 is not the shared restatement ({dtype})'
            del theirs
    check(f'{tag} flows', out['flows'], ref[F64][0], ref[F32][0])
    check_or_zero(f'{tag} h1', saved[0, :n], ref[F64][1], ref[F32][1])
    del ref

    # ---- backward against float64 with the gates the kernel took ----
    gates = [saved[l, :n] > 0 for l in range(3)]
    gref, fref = {}, {}
    for dtype in (F64, F32):
        w = [p.to(dtype).requires_grad_(True) for p in nt.weights]
        if nt.prff:
            fm = nt.enc.to(dtype).requires_grad_(True)
            flows = restate(name, fm, w, times, ys, xs, SCALE, dtype, mask, gates)
            gref[dtype] = torch.autograd.grad((flows * up.to(dtype)).sum(), w + [fm])
            fr = nt.freq.to(dtype).requires_grad_(True)
            flows = restate(name, L.f_eff(fr, nt.mag), nt.weights, times, ys, xs, SCALE, dtype, mask, gates)
            fref[dtype], = torch.autograd.grad((flows * up.to(dtype)).sum(), [fr])
        else:
            flows = restate(name, nt.enc, w, times, ys, xs, SCALE, dtype, mask, gates)
            gref[dtype] = torch.autograd.grad((flows * up.to(dtype)).sum(), w)
        del flows
    r64, r32 = gref[F64], gref[F32]
    for i, nm in enumerate(GNAMES[:7]):                                     # gb4: see the docstring
        check_or_zero(f'{tag} {nm}', grads[i], r64[i], r32[i])
    check_or_zero(f'{tag} gW1 coordinate columns', grads[0][:, :3], r64[0][:, :3], r32[0][:, :3])
    for t in range(4):
        cols = slice(3 + 128 * t, 3 + 128 * t + 128)
        if bool((mask[cols] != 0).any()):
            check(f'{tag} gW1 tile {t}', grads[0][:, cols], r64[0][:, cols], r32[0][:, cols])
    if nt.prff:
        check_or_zero(f'{tag} gF', grads[8], r64[8], r32[8])
        fp = nt.freq.clone().requires_grad_(True)
        freq_grad, = torch.autograd.grad(L.f_eff(fp, nt.mag), [fp], grads[8])   # torch's fp32 normalize backward, as flow_fields applies it
        check_or_zero(f'{tag} freq.grad', freq_grad, fref[F64], fref[F32], signed=False)
    return out, gref


# ---- case 1: the sweep ----
@pytest.mark.parametrize('k', KS)
@pytest.mark.parametrize('name', ('PRBF', 'PFF', 'PRFF'))
def test_k_sweep(dev, name, k):
    run_case(dev, name, 'sweep', prefix_mask(k), k, f'{name} sweep k={k}')


@pytest.mark.parametrize('k', (6, 132, 515))
def test_k_sweep_puff(dev, k):
    """PUFF shares PFF's kernel instantiation"""
    run_case(dev, 'PUFF', 'sweep', prefix_mask(k), k, f'PUFF sweep k={k}')


@pytest.mark.parametrize('k', (6, 132, 515))
@pytest.mark.parametrize('name', ('PRBF', 'PRFF'))
def test_k_sweep_single_tile(dev, name, k):
    run_case(dev, name, 'single', prefix_mask(k), k, f'{name} single k={k}')


# ---- case 2: masks with holes ----
@pytest.mark.parametrize('name', ('PRBF', 'PFF', 'PRFF'))
def test_mask_with_holes(dev, name):
    hmask = holes_mask()
    tag = f'{name} sweep holes'
    out, gref = run_case(dev, name, 'sweep', hmask, K_HOLES, tag)
    gW1 = out['grads'][0]
    assert is_plus_zero(gW1[:, 1]) and is_plus_zero(gW1[:, 3 + 16:3 + 32]) and is_plus_zero(gW1[:, 3 + 128:3 + 256])
    if name == 'PRFF':
        gF = out['grads'][8]
        closed = closed_frequencies(hmask)
        assert not bool(closed[20]) and bool(closed[21]) and bool(closed[64:128].all()) and not bool(closed[63]) and not bool(closed[128])
        assert bool((gF[:, 20] != 0).any())
        check(f'{tag} gF frequency 20', gF[:, 20], gref[F64][8][:, 20], gref[F32][8][:, 20])
        assert is_plus_zero(gF[:, 21]) and is_plus_zero(gF[:, 64:128])


# ---- case 3: closed weights that hold NaN ----
@pytest.mark.parametrize('name', ('PRBF', 'PRFF'))
def test_poisoned_closed_weights(dev, name):
    """NaN in W1[:, mask == 0] of the network the kernels read: flows, saved and every gradient keep their bits.  The float64
    reference is not evaluated on these weights (0 x NaN is NaN in torch; the kernel's exact zero is a stated choice of the port)"""
    hmask = holes_mask()
    nt = Net(name, dev)
    clean = run_kernels(nt, 'sweep', hmask, K_HOLES, dev)
    w1 = nt.net.linears()[0].weight
    with torch.no_grad():
        w1[:, (hmask == 0).to(dev)] = NAN
    assert int(torch.isnan(w1).sum()) == 256 * int((hmask == 0).sum())
    bad = run_kernels(nt, 'sweep', hmask, K_HOLES, dev)
    assert torch.equal(clean['flows'], bad['flows']), 'flows'
    assert torch.equal(clean['saved'], bad['saved']), 'saved'
    for nm, a, b in zip(GNAMES + ['gF'], clean['grads'], bad['grads']):
        assert torch.equal(a, b), nm


# ---- the kcols clause of flownet_reduce_prog_kernel ----
@pytest.mark.parametrize('k', (131, 259, 387))
def test_reduce_never_reads_an_uncomputed_column(dev, k):
    """k - 3 is a multiple of 128: kcols = k - 3.  Under an all-ones mask with k_active = k the columns from k on were not computed
    and the workspace holds NaN there: they must be +0, and the columns before them the bits of the honest call (mask values 1)"""
    from sin_inn_amd import flownet
    nt = Net('PRBF', dev)
    times, ys, xs = axes(GRIDS['sweep'], dev)
    n = times.numel() * ys.numel() * xs.numel()
    honest = torch.zeros(515)
    honest[:k] = 1.0
    honest = honest.to(dev)
    saved, ws, _ = nan_buffers(n, dev)
    flows, saved = flownet.flownet_forward(nt.net, times, ys, xs, SCALE, True, saved, mask=honest, k_active=k)
    up = torch.randn(flows.shape, generator=torch.Generator().manual_seed(11)).to(dev)
    want = flownet.flownet_backward(nt.net, times, ys, xs, SCALE, up, saved, ws, mask=honest, k_active=k)
    ws.fill_(NAN)
    got = flownet.flownet_backward(nt.net, times, ys, xs, SCALE, up, saved, ws, mask=torch.ones(515, device=dev), k_active=k)
    assert bool(torch.isfinite(got[0]).all()), 'gW1 holds a partial sum that was never computed'
    live = live_features(nt, times, ys, xs)
    assert is_plus_zero(got[0][:, k:]) and bool((got[0][:, :k][:, live[:k]] != 0.0).any(dim=0).all())
    for nm, a, b in zip(GNAMES, got, want):
        assert torch.equal(a, b), nm
