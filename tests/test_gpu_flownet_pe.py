"""GPU: the positional encoding of the flow-field network kernels (csrc/flownet.hip, SININN_FLOWNET_PE) for PE and PPE against
float64, with the method and the constants of tests/test_gpu_flownet_grid.py: error against float64 <= min(4 x the deviation of the
same formula in fp32 torch, measured here, 1e-4), max-norm relative to max |ref|, gradients with the kernel's own gates forced
(`saved > 0`), no element excluded.  The reference is `restate` / `encode_pe` of tests/test_flownet_pe_golden.py, which that file
ties to the reference's own model.py / progressive_controller.py through the fixture.

Grids: the fixture's (t = 2, 21 x 28: 1176 points, 18 tiles and one of 24 rows) and a ragged one (times 0, 0.25, 1.0; 37 x 53: 5883
points, neither a multiple of 7 nor of 64, tiles straddling frames).  Nothing runs at production size.

The encoding probe reads the encoding out of the kernel in ONE pass: rows 0 .. 23 of layer 1's weight select +feature k, rows
24 .. 47 select -feature k, the bias is zero, so `saved[0]` holds relu(+-e) exactly and columns k minus 24 + k are every encoded
feature of every point as the kernel generated it.  Compared with the float64 encoding in absolute max-norm (the range is [-1, 1])
against min(4 units, 1e-4), the unit being the fp32-torch encoding's own deviation from float64 on the same points.

Measured on an MI355X (`ratio(...)` lines of a run with -s: error / budget [error, fp32-torch unit]):
  encoding  fixture 0.25 [abs 7.25e-07, unit 7.25e-07]  ragged 0.25 [abs 9.03e-07, unit 9.03e-07]: the kernel is exactly as far from
            float64 as torch's fp32 evaluation, the error is the one rounding of the product freqs[f] * x_d (half an ulp near 8 pi)
  PE fixture   flows 0.248 [3.86e-07, 3.9e-07]  vs fixture 0.228  gW1 0.0639 [4.88e-07, 1.91e-06]  gb1 0.233  gW2 0.117  gb2 0.306
               gW3 0.0924  gb3 0.265  gW4 0.204  gb4 0.667 [2.44e-07, 9.13e-08]
  PE ragged    flows 0.232 [4.66e-07, 5.02e-07]  gW1 0.0579 [3.33e-07, 1.44e-06]  gb1 0.264  gW2 0.0558  gb2 0.366  gW3 0.0336  gb3 0.384
               gW4 0.0945  gb4 0.34 [9.51e-08, 6.99e-08]
  PPE (worst over ones / mid / ramp and both grids)  flows 0.291 (ragged mid, err 3.47e-07)  vs fixture 0.2  gW1 0.116  gW1[:, :3] 0.102
               gb1 0.336  gW2 0.0978  gb2 0.466  gW3 0.0669  gb3 0.352  gW4 0.201  gb4 0.667 (gb4 = scale * sum(up) does not depend on
               the network)
  End to end: the first five losses of the fused and the composed loop agree to 2.7e-07 relative for PE (0.1319209 .. 0.0989356; after
  12 steps 0.0680062 / 0.0684297) and bitwise as printed for PPE (0.1340147 .. 0.1155717; 0.0627617 / 0.0627617).  51 tests, 9.5 s.
"""
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from flownet_refs import encode_pe, is_plus_zero, nan_saved, nan_workspace, net_tensors, poses_of, reference_grads, restate  # noqa: E402
from test_flownet_pe_golden import N_MID, N_RAMP, SCALE, TIMES, GH, GW, build, controller  # noqa: E402
from test_gpu_flownet import CEIL, F64, MULT, axes, check  # noqa: E402

GRIDS = {'fixture': (TIMES, GH, GW), 'ragged': ((0.0, 0.25, 1.0), 37, 53)}
GNAMES = [f'g{k}{l}' for l in (1, 2, 3, 4) for k in ('W', 'b')]
NAN = float('nan')


@pytest.fixture(scope='module')
def dev():
    import sin_inn_amd  # noqa: F401
    assert torch.cuda.is_available(), 'GPU tests need a GPU'
    return torch.device('cuda', 0)


@pytest.fixture(scope='module')
def gold():
    return np.load(os.path.join(ROOT, 'tests', 'golden', 'golden_flownet_pe.npz'))


def masks_of(gold, kind, net=None):
    if kind == 'ones':
        return torch.ones(27), None
    ctl = controller(net)
    for i in range(N_MID if kind == 'mid' else N_RAMP):
        ctl.stash_iteration(torch.tensor(0.5))
    assert np.array_equal(ctl.mask.numpy(), gold[f'mask_{kind}'])
    return ctl.mask.clone(), ctl


@pytest.mark.parametrize('grid', list(GRIDS))
def test_encoding_probe(dev, grid):
    from sin_inn_amd import flownet
    net = build('PE').to(dev)
    bufs, _ = net_tensors(net, dev)
    times, ys, xs = axes(GRIDS[grid], dev)
    n = times.numel() * ys.numel() * xs.numel()
    lin = net.linears()[0]
    with torch.no_grad():
        lin.bias.zero_()
        lin.weight.zero_()
        k = torch.arange(24, device=dev)
        lin.weight[k, k] = 1.0
        lin.weight[24 + k, k] = -1.0
        _, saved = flownet.flownet_forward(net, times, ys, xs, SCALE, True, nan_saved(n, dev))
    pos, neg = saved[0, :n, :24], saved[0, :n, 24:48]
    assert bool(((pos == 0) | (neg == 0)).all()) and is_plus_zero(saved[0, :, 48:])
    got = pos - neg
    assert bool(torch.isfinite(got).all()) and float(got.abs().max()) <= 1.0
    enc64 = encode_pe(bufs, poses_of(times, ys, xs, F64))
    enc32 = encode_pe(bufs, poses_of(times, ys, xs, torch.float32))
    unit = float((enc32.to(F64) - enc64).abs().max())
    err = float((got.to(F64) - enc64).abs().max())
    budget = min(MULT * unit, CEIL)
    print(f'ratio(PE {grid} encoding) = {err / budget:.3g}   [abs err {err:.3g}, fp32-torch unit {unit:.3g}, budget {budget:.3g}]')
    # the probe sees whole periods: both signs of every feature of y and x (the time axis has two or three samples)
    yx = enc64.view(n, 4, 2, 3)[..., 1:]
    assert float(enc64.min()) < -0.99 and float(enc64.max()) > 0.99
    assert bool((yx.amin(0) < -0.5).all()) and bool((yx.amax(0) > 0.5).all())
    assert err <= budget, (err, budget)


@pytest.mark.parametrize('grid', list(GRIDS))
def test_forward_and_backward_against_float64(dev, gold, grid):
    from sin_inn_amd import flownet
    name = 'PE'
    net = build(name).to(dev)
    bufs, weights = net_tensors(net, dev)
    times, ys, xs = axes(GRIDS[grid], dev)
    n = times.numel() * ys.numel() * xs.numel()
    tag = f'{name} {grid}'

    infer, none = flownet.flownet_forward(net, times, ys, xs, SCALE, False)
    assert none is None
    train, saved = flownet.flownet_forward(net, times, ys, xs, SCALE, True, nan_saved(n, dev))
    again_f, saved2 = flownet.flownet_forward(net, times, ys, xs, SCALE, True, nan_saved(n, dev))
    assert torch.equal(infer, train) and torch.equal(train, again_f) and torch.equal(saved, saved2)
    assert bool(torch.isfinite(saved).all()) and float(saved.min()) >= 0.0
    assert torch.equal(saved[:, n:], saved[:, n - 1:n].expand_as(saved[:, n:])), 'a clamped row of the last tile is not row N - 1'
    with torch.no_grad():
        ref64 = restate(name, bufs, weights, times, ys, xs, SCALE, F64)
        ref32 = restate(name, bufs, weights, times, ys, xs, SCALE, torch.float32)
    check(f'{tag} flows', infer, ref64, ref32)
    if grid == 'fixture':
        check(f'{tag} flows vs fixture', infer, torch.from_numpy(gold[f'{name}_out64']).to(dev), torch.from_numpy(gold[f'{name}_out32']).to(dev))

    gates = [saved[l, :n] > 0 for l in range(3)]
    up = torch.randn(infer.shape, generator=torch.Generator().manual_seed(11)).to(dev)
    grads_ref = reference_grads(name, bufs, weights, times, ys, xs, SCALE, up, None, gates)
    got = flownet.flownet_backward(net, times, ys, xs, SCALE, up, saved, nan_workspace(n, dev))
    again = flownet.flownet_backward(net, times, ys, xs, SCALE, up, saved, nan_workspace(n, dev))
    assert tuple(got[0].shape) == (256, 24)
    for nm, a, b in zip(GNAMES, got, again):
        assert bool(torch.isfinite(a).all()), nm
        assert torch.equal(a, b), f'{nm}: two backward calls differ'
    for nm, g, r64, r32 in zip(GNAMES, got, grads_ref[F64], grads_ref[torch.float32]):
        check(f'{tag} {nm}', g, r64, r32)


@pytest.mark.parametrize('grid', list(GRIDS))
@pytest.mark.parametrize('kind', ['ones', 'mid', 'ramp'])
def test_masks(dev, gold, kind, grid):
    from sin_inn_amd import flownet
    name = 'PPE'
    net = build(name).to(dev)
    bufs, weights = net_tensors(net, dev)
    times, ys, xs = axes(GRIDS[grid], dev)
    h, w = ys.numel(), xs.numel()
    n = times.numel() * h * w
    hmask, ctl = masks_of(gold, kind, net)
    mask, ka = hmask.to(dev), flownet.last_open(hmask)
    assert ka == {'ones': 27, 'mid': 18, 'ramp': 12}[kind]
    tag = f'{name} {grid} {kind}'

    infer, _ = flownet.flownet_forward(net, times, ys, xs, SCALE, False, mask=mask, k_active=ka)
    train, saved = flownet.flownet_forward(net, times, ys, xs, SCALE, True, nan_saved(n, dev), mask=mask, k_active=ka)
    assert torch.equal(infer, train)
    assert bool(torch.isfinite(saved).all()) and float(saved.min()) >= 0.0
    with torch.no_grad():
        ref64 = restate(name, bufs, weights, times, ys, xs, SCALE, F64, mask)
        ref32 = restate(name, bufs, weights, times, ys, xs, SCALE, torch.float32, mask)
    check(f'{tag} flows', infer, ref64, ref32)
    if grid == 'fixture':
        check(f'{tag} flows vs fixture', infer, torch.from_numpy(gold[f'{name}_out64_{kind}']).to(dev),
              torch.from_numpy(gold[f'{name}_out32_{kind}']).to(dev))

    gates = [saved[l, :n] > 0 for l in range(3)]
    up = torch.randn(infer.shape, generator=torch.Generator().manual_seed(11)).to(dev)
    grads_ref = reference_grads(name, bufs, weights, times, ys, xs, SCALE, up, mask, gates)
    got = flownet.flownet_backward(net, times, ys, xs, SCALE, up, saved, nan_workspace(n, dev), mask=mask, k_active=ka)
    assert tuple(got[0].shape) == (256, 27)
    closed = mask == 0
    assert is_plus_zero(got[0][:, closed])
    assert bool((got[0][:, ~closed] != 0.0).any(dim=0).all()), 'an open column of gW1 is all zero'
    for nm, g, r64, r32 in zip(GNAMES, got, grads_ref[F64], grads_ref[torch.float32]):
        assert bool(torch.isfinite(g).all()), nm
        check(f'{tag} {nm}', g, r64, r32)
    check(f'{tag} gW1 coordinate columns', got[0][:, :3], grads_ref[F64][0][:, :3], grads_ref[torch.float32][0][:, :3])

    # the public surface: the controller's own mask (k_active from the host mask, skipped) or the bare model against the same mask
    # given as a device tensor (not inspected on the host: all 27 features)
    params = [p for lin in net.linears() for p in (lin.weight, lin.bias)]

    def run(target, **kw):
        for p in params:
            p.grad = None
        f12, f21 = flownet.flow_fields(target, times, h, w, SCALE, **kw)
        (f12 * up[:, :2]).sum().add((f21 * up[:, 2:]).sum()).backward()
        return torch.cat((f12, f21), 1).detach(), [p.grad.clone() for p in params]

    own_f, own_g = run(net if ctl is None else ctl)
    if ctl is not None:
        assert ctl.device_mask(dev)[1] == ka
    over_f, over_g = run(net if ctl is None else ctl, override_mask=mask)
    assert torch.equal(own_f, over_f) and torch.equal(own_f, infer)
    for nm, a, b, c in zip(GNAMES, own_g, over_g, got):
        assert torch.equal(a, b), f'{nm}: k_active and the override mask differ'
        assert torch.equal(a, c), f'{nm}: flow_fields and flownet_backward differ'


@pytest.fixture(scope='module')
def ppe_case(dev):
    net = build('PPE').to(dev)
    times, ys, xs = axes(GRIDS['ragged'], dev)
    up = torch.randn(times.numel(), 4, ys.numel(), xs.numel(), generator=torch.Generator().manual_seed(11)).to(dev)
    return net, times, ys, xs, up


def poisoned(net, k, dev):
    """a copy of the network with NaN in the columns of W1 from k on"""
    import copy
    other = copy.deepcopy(net)
    with torch.no_grad():
        other.linears()[0].weight[:, k:] = NAN
    return other


@pytest.mark.parametrize('ka', list(range(28)))
def test_k_active_sweep(dev, ppe_case, ka):
    """prefix masks of ka ones: EVERY valid k_active, ka (the smallest) .. 27, gives the bits of k_active = 27 on the clean weights
    (flows in both modes, `saved`, the eight gradients), each from NaN-filled buffers and with NaN in the closed columns of W1"""
    from sin_inn_amd import flownet
    net, times, ys, xs, up = ppe_case
    n = times.numel() * ys.numel() * xs.numel()
    mask = torch.zeros(27, device=dev)
    mask[:ka] = 1
    full, saved_full = flownet.flownet_forward(net, times, ys, xs, SCALE, True, nan_saved(n, dev), mask=mask, k_active=27)
    unskipped = flownet.flownet_backward(net, times, ys, xs, SCALE, up, saved_full, nan_workspace(n, dev), mask=mask, k_active=27)
    assert bool(torch.isfinite(full).all())
    assert torch.equal(saved_full[:, n:], saved_full[:, n - 1:n].expand_as(saved_full[:, n:])), 'a clamped row of the last tile is not row N - 1'
    assert is_plus_zero(unskipped[0][:, ka:])
    if ka:
        assert bool((unskipped[0][:, :ka] != 0.0).any(dim=0).all())
    bad = poisoned(net, ka, dev)
    saved, ws = nan_saved(n, dev), nan_workspace(n, dev)
    for kk in range(ka, 28):
        infer, _ = flownet.flownet_forward(bad, times, ys, xs, SCALE, False, mask=mask, k_active=kk)
        flows, saved = flownet.flownet_forward(bad, times, ys, xs, SCALE, True, saved.fill_(NAN), mask=mask, k_active=kk)
        assert torch.equal(flows, full) and torch.equal(infer, full) and torch.equal(saved, saved_full), f'forward at k_active {kk}'
        got = flownet.flownet_backward(bad, times, ys, xs, SCALE, up, saved, ws.fill_(NAN), mask=mask, k_active=kk)
        for nm, a, b in zip(GNAMES, got, unskipped):
            assert torch.equal(a, b) and not bool(torch.signbit(a[a == 0]).any()), \
                f'{nm}: the skipped and the unskipped path differ at k_active {kk} (mask of {ka} ones)'


@pytest.mark.parametrize('k', [3, 8, 16, 19, 24])
def test_reduce_gives_zero_beyond_k_active_under_an_open_mask(dev, ppe_case, k):
    """as test_reduce_never_reads_an_uncomputed_column of tests/test_gpu_flownet_kactive.py: under an all-ones mask with k_active = k
    the columns from k on are +0 and the columns before them the bits of the honest call (prefix mask of k ones)"""
    from sin_inn_amd import flownet
    net, times, ys, xs, up = ppe_case
    n = times.numel() * ys.numel() * xs.numel()
    honest = torch.zeros(27)
    honest[:k] = 1.0
    honest = honest.to(dev)
    ws = nan_workspace(n, dev)
    flows, saved = flownet.flownet_forward(net, times, ys, xs, SCALE, True, nan_saved(n, dev), mask=honest, k_active=k)
    want = flownet.flownet_backward(net, times, ys, xs, SCALE, up, saved, ws, mask=honest, k_active=k)
    ws.fill_(NAN)
    got = flownet.flownet_backward(net, times, ys, xs, SCALE, up, saved, ws, mask=torch.ones(27, device=dev), k_active=k)
    assert bool(torch.isfinite(got[0]).all())
    assert is_plus_zero(got[0][:, k:]) and bool((got[0][:, :k] != 0.0).any(dim=0).all())
    for nm, a, b in zip(GNAMES, got, want):
        assert torch.equal(a, b), nm


@pytest.mark.parametrize('k', [0, 1, 2])
def test_coordinate_columns_follow_the_mask_alone(dev, ppe_case, k):
    """k_active < 3 under an all-ones mask: the encoded columns of gW1 are +0, the three coordinate columns and the other seven
    gradients are the bits of the k_active = 27 call on the same `saved` (include/sininn.h: columns k < 3 are the mask's alone)"""
    from sin_inn_amd import flownet
    net, times, ys, xs, up = ppe_case
    n = times.numel() * ys.numel() * xs.numel()
    ones = torch.ones(27, device=dev)
    _, saved = flownet.flownet_forward(net, times, ys, xs, SCALE, True, nan_saved(n, dev), mask=ones, k_active=k)
    want = flownet.flownet_backward(net, times, ys, xs, SCALE, up, saved, nan_workspace(n, dev), mask=ones, k_active=27)
    got = flownet.flownet_backward(net, times, ys, xs, SCALE, up, saved, nan_workspace(n, dev), mask=ones, k_active=k)
    assert is_plus_zero(got[0][:, 3:]) and bool((got[0][:, :3] != 0.0).any(dim=0).all())
    assert torch.equal(got[0][:, :3], want[0][:, :3])
    for nm, a, b in list(zip(GNAMES, got, want))[1:]:
        assert torch.equal(a, b), nm


@pytest.mark.parametrize('name', ['PE', 'PPE'])
def test_autograd_function_and_inference_mode(dev, name):
    from sin_inn_amd import flownet
    net = build(name).to(dev)
    times, ys, xs = axes(GRIDS['fixture'], dev)
    f12, f21 = flownet.flow_fields(net, times, GH, GW, SCALE)
    assert f12.shape == (2, 2, GH, GW) and f21.shape == (2, 2, GH, GW) and f12.requires_grad
    up = torch.randn(2, 4, GH, GW, generator=torch.Generator().manual_seed(11)).to(dev)
    (f12 * up[:, :2]).sum().add((f21 * up[:, 2:]).sum()).backward()
    kw = dict(mask=torch.ones(27, device=dev)) if name == 'PPE' else {}
    flows, saved = flownet.flownet_forward(net, times, ys, xs, SCALE, True, **kw)
    direct = flownet.flownet_backward(net, times, ys, xs, SCALE, up, saved, **kw)
    for p, g in zip([q for lin in net.linears() for q in (lin.weight, lin.bias)], direct):
        assert torch.equal(p.grad, g)
    with torch.no_grad():
        i12, i21 = flownet.flow_fields(net, times, GH, GW, SCALE)
    assert not i12.requires_grad and torch.equal(i12, f12.detach()) and torch.equal(i21, f21.detach())
    assert torch.equal(torch.cat((i12, i21), 1), flows)
    with pytest.raises(NotImplementedError):
        flownet.flow_fields(net, times.cpu(), GH, GW, SCALE)


@pytest.mark.parametrize('name', ['PE', 'PPE'])
def test_fit_flow_end_to_end(dev, name):
    """12 steps of tools/fit_flow.py at 64 x 96 with the fused network and with the network composed from torch ops (same seed, same
    optimiser): per-step loss within CEIL relative for the first 5 steps.  Wiring, not accuracy."""
    sys.path.insert(0, os.path.join(ROOT, 'tools'))
    import fit_flow
    fused = fit_flow.fit(name, 64, 96, 12, composed=False)
    comp = fit_flow.fit(name, 64, 96, 12, composed=True)
    for s in range(5):
        print(f'{name} step {s}: fused {fused[s]:.7f} composed {comp[s]:.7f} rel {abs(fused[s] - comp[s]) / abs(comp[s]):.3g}')
    print(f'{name} final: fused {fused[-1]:.7f} composed {comp[-1]:.7f}')
    assert all(np.isfinite(fused)) and all(np.isfinite(comp))
    for s in range(5):
        assert abs(fused[s] - comp[s]) <= CEIL * abs(comp[s]), (s, fused[s], comp[s])


def test_command_line_trains_ppe(dev, tmp_path):
    r = subprocess.run([sys.executable, os.path.join(ROOT, 'video-interpolation', 'main.py'), 'train', '--synthetic', '4', '24', '40',
                        '--net', 'PPE', '--batch', '2', '--epochs', '6'], cwd=str(tmp_path), capture_output=True, text=True, timeout=300)
    print(r.stdout[-2000:], r.stderr[-2000:])
    assert r.returncode == 0
    gifs = [f for f in os.listdir(os.path.join(str(tmp_path), 'results')) if f.startswith('flow_synthetic_temp_epe_') and f.endswith('.gif')]
    assert len(gifs) == 1
