"""GPU: the flow-field network kernels (csrc/flownet.hip) for RBF, FFN and UFF against float64, at the fixture's grid
(t = 2, 20 x 28), a ragged one (t = 3, 109 x 253: a partial last tile, tiles straddling two frames) and the production one
(t = 1, 436 x 1024).

Method (that of tests/test_gpu_flowloss_sizes.py):
  * the reference is `restate` of tests/flownet_refs.py in float64 on the GPU, from the fp32 weights, buffers and axis vectors
    the kernel received, widened; test_flownet_golden.py ties it to the reference's own model.py through the fixture, and on the fixture
    grid the kernel is also compared with the fixture's stored outputs directly;
  * the unit of error is the deviation of the same formula evaluated in fp32 torch from float64 on the same inputs, measured in the
    test, max-norm relative to max |ref|.  The kernel is allowed MULT = 4 units (a second, independent summation order and a different
    sin / exp, each at most doubling a per-term bound; the factor tests/test_gpu_flowloss_sizes.py derives) and never more than the
    project's standing 1e-4;
  * outputs are compared with free gates (ReLU is continuous); gradients with FORCED gates, as tests/test_gpu_gates.py does for the
    INN: the gates the kernel took are `saved > 0` and both the float64 reference and the fp32 unit are evaluated with them.  No
    element is excluded;
  * the inference and the training mode of the forward kernel agree bitwise; two backward calls on the same inputs agree bitwise, with
    `saved` (before the forward) and the workspace (before the first backward) filled with NaN.

Measured on an MI355X at the production grid (`ratio(...)` lines of a run with -s: error / budget [error, fp32-torch unit]):
  RBF  flows 0.139 [2.83e-07, 5.09e-07]  gW1 0.0625 [1.21e-06, 4.82e-06]  gb1 0.288  gW2 0.0428 [1.13e-06, 6.61e-06]  gb2 0.275
       gW3 0.0397 [1.27e-06, 8.02e-06]  gb3 0.256  gW4 0.0521 [6.95e-07, 3.34e-06]  gb4 0.279 [2.93e-07, 2.62e-07]
  FFN  flows 0.104 [2.54e-06, 6.10e-06]  gW1 0.122 [4.34e-06, 8.90e-06]  gb1 0.178  gW2 0.0632 [2.29e-06, 9.07e-06]  gb2 0.195
       gW3 0.052 [1.86e-06, 8.94e-06]  gb3 0.162  gW4 0.0928 [1.95e-06, 5.26e-06]  gb4 0.279
  UFF  flows 0.0913 [9.08e-07, 2.49e-06]  gW1 0.0432 [1.32e-06, 7.62e-06]  gb1 0.18  gW2 0.0561 [1.08e-06, 4.81e-06]  gb2 0.227
       gW3 0.0367 [9.43e-07, 6.42e-06]  gb3 0.35  gW4 0.0278 [7.87e-07, 7.07e-06]  gb4 0.279
  The tightest figure of the file is gb4 at the small grids (0.90 fixture, 0.94 ragged: unit 7e-8 .. 1.1e-7, error 2.7e-7 .. 4.1e-7).
  End to end: the first five losses of the fused and the composed loop are equal to all printed digits (0.1310618 .. 0.1218713),
  the final ones 0.0105281 / 0.0105750.  13 tests, 6 s.
"""
import os
import sys

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from flownet_refs import net_tensors, restate  # noqa: E402
from test_flownet_golden import NETS, SCALE, TIMES, GH, GW, build  # noqa: E402

F64 = torch.float64
MULT, CEIL = 4.0, 1e-4
GRIDS = {'fixture': (TIMES, GH, GW), 'ragged': ((0.0, 0.25, 1.0), 109, 253), 'production': ((0.5,), 436, 1024)}


@pytest.fixture(scope='module')
def dev():
    import sin_inn_amd  # noqa: F401
    assert torch.cuda.is_available(), 'GPU tests need a GPU'
    return torch.device('cuda', 0)


def relmax(a, ref):
    a, ref = a.detach().to(F64), ref.detach().to(F64)
    err = (a - ref).abs()
    err = torch.where(torch.isfinite(a), err, torch.full_like(err, float('inf')))
    return float(err.max() / ref.abs().max())


def check(name, got, ref64, ref32):
    """error of the kernel against min(MULT * unit, CEIL); prints ratio(error / budget)"""
    unit = relmax(ref32, ref64)
    budget = min(MULT * unit, CEIL)
    err = relmax(got, ref64)
    print(f'ratio({name}) = {err / budget:.3g}   [err {err:.3g}, fp32-torch unit {unit:.3g}, budget {budget:.3g}]')
    assert err <= budget, (name, err, budget)


def axes(grid, dev):
    times, h, w = grid
    return (torch.tensor(times, device=dev), torch.linspace(-1, 1, h).to(dev), torch.linspace(-1, 1, w).to(dev))


@pytest.mark.parametrize('grid', list(GRIDS))
@pytest.mark.parametrize('name', NETS)
def test_forward_and_backward_against_float64(dev, name, grid):
    from sin_inn_amd import _lib, flownet
    net = build(name).to(dev)
    bufs, weights = net_tensors(net, dev)
    times, ys, xs = axes(GRIDS[grid], dev)
    n = times.numel() * ys.numel() * xs.numel()
    tag = f'{name} {grid}'

    # ---- forward, both modes ----
    infer, none = flownet.flownet_forward(net, times, ys, xs, SCALE, False)
    assert none is None
    nbytes = _lib.lib().sininn_flownet_saved_bytes(n)
    saved = torch.full((3, nbytes // (3 * 256 * 4), 256), float('nan'), device=dev)
    train, saved = flownet.flownet_forward(net, times, ys, xs, SCALE, True, saved)
    assert torch.equal(infer, train)
    assert bool(torch.isfinite(saved).all()) and float(saved.min()) >= 0.0
    with torch.no_grad():
        ref64 = restate(name, bufs, weights, times, ys, xs, SCALE, F64)
        ref32 = restate(name, bufs, weights, times, ys, xs, SCALE, torch.float32)
    check(f'{tag} flows', infer, ref64, ref32)
    if grid == 'fixture':
        gold = np.load(os.path.join(ROOT, 'tests', 'golden', 'golden_flownet.npz'))
        g64 = torch.from_numpy(gold[f'{name}_out64']).to(dev)
        g32 = torch.from_numpy(gold[f'{name}_out32']).to(dev)
        check(f'{tag} flows vs fixture', infer, g64, g32)
    del ref64, ref32

    # ---- backward with the gates the kernel took ----
    gates = [saved[l, :n] > 0 for l in range(3)]
    up = torch.randn(infer.shape, generator=torch.Generator().manual_seed(11)).to(dev)
    grads_ref = {}
    for dtype in (F64, torch.float32):
        w = [p.to(dtype).requires_grad_(True) for p in weights]
        flows = restate(name, bufs, w, times, ys, xs, SCALE, dtype, gates=gates)
        grads_ref[dtype] = torch.autograd.grad((flows * up.to(dtype)).sum(), w)
        del flows
    wbytes = _lib.lib().sininn_flownet_workspace_bytes(n)
    ws = torch.full((wbytes // 4,), float('nan'), device=dev)
    got = flownet.flownet_backward(net, times, ys, xs, SCALE, up, saved, ws)
    again = flownet.flownet_backward(net, times, ys, xs, SCALE, up, saved, ws)
    names = [f'g{k}{l}' for l in (1, 2, 3, 4) for k in ('W', 'b')]
    for nm, a, b in zip(names, got, again):
        assert bool(torch.isfinite(a).all()), nm
        assert torch.equal(a, b), f'{nm}: two backward calls differ'
    for nm, g, r64, r32 in zip(names, got, grads_ref[F64], grads_ref[torch.float32]):
        check(f'{tag} {nm}', g, r64, r32)


@pytest.mark.parametrize('name', NETS)
def test_autograd_function_and_inference_mode(dev, name):
    from sin_inn_amd import flownet
    net = build(name).to(dev)
    times = torch.tensor([0.0, 0.5], device=dev)
    f12, f21 = flownet.flow_fields(net, times, 20, 28, SCALE)
    assert f12.shape == (2, 2, 20, 28) and f21.shape == (2, 2, 20, 28) and f12.requires_grad
    up = torch.randn(2, 4, 20, 28, generator=torch.Generator().manual_seed(11)).to(dev)
    (f12 * up[:, :2]).sum().add((f21 * up[:, 2:]).sum()).backward()
    _, ys, xs = axes(GRIDS['fixture'], dev)
    flows, saved = flownet.flownet_forward(net, times, ys, xs, SCALE, True)
    direct = flownet.flownet_backward(net, times, ys, xs, SCALE, up, saved)
    for p, g in zip([q for lin in net.linears() for q in (lin.weight, lin.bias)], direct):
        assert torch.equal(p.grad, g)
    with torch.no_grad():
        i12, i21 = flownet.flow_fields(net, times, 20, 28, SCALE)
    assert not i12.requires_grad and torch.equal(i12, f12.detach()) and torch.equal(i21, f21.detach())
    with pytest.raises(NotImplementedError):
        flownet.flow_fields(net, times.cpu(), 20, 28, SCALE)


def test_fit_flow_end_to_end(dev):
    """60 steps of tools/fit_flow.py at 64 x 96 with the fused network and with the network composed from torch ops (same seed, same
    optimiser): per-step loss within CEIL relative for the first 5 steps, final loss below the initial one in both.  Wiring, not
    accuracy."""
    sys.path.insert(0, os.path.join(ROOT, 'tools'))
    import fit_flow
    fused = fit_flow.fit('RBF', 64, 96, 60, composed=False)
    comp = fit_flow.fit('RBF', 64, 96, 60, composed=True)
    for s in range(5):
        print(f'step {s}: fused {fused[s]:.7f} composed {comp[s]:.7f} rel {abs(fused[s] - comp[s]) / abs(comp[s]):.3g}')
    print(f'final: fused {fused[-1]:.7f} composed {comp[-1]:.7f}')
    for s in range(5):
        assert abs(fused[s] - comp[s]) <= CEIL * abs(comp[s]), (s, fused[s], comp[s])
    assert fused[-1] < fused[0] and comp[-1] < comp[0]
