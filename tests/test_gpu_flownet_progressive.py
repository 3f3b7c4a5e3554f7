"""GPU: the progressive mode of the flow-field network kernels (csrc/flownet.hip) for PRBF, PFF and PUFF against float64, with the
method, the budget and the three grids of tests/test_gpu_flownet.py, unchanged: error against float64 <= min(4 x the deviation of
the same formula in fp32 torch, measured here, 1e-4), max-norm relative to max |ref|, gradients with the kernel's own gates forced,
no element excluded.  The reference is `restate` of tests/flownet_refs.py (concatenation and mask), which
tests/test_flownet_progressive_golden.py ties to the reference's own model.py / progressive_controller.py through the fixture.

Masks: all ones; `mid`, the controller's mask after 100 iterations (84 leading ones); `init`, the controller's first mask (6 open
features: the three coordinates and three encoded ones); and `ramp`, the mask after 98 iterations, whose block in progress stands at
0.5 (the only one with values other than 0 and 1).  Each case runs the SKIPPED path (k_active = the last open feature, what a
controller passes) and compares it bitwise, flows and all eight gradients, with the UNSKIPPED path (k_active = 515) on the same mask.

Measured on an MI355X (worst error / budget over nets and masks, from the `ratio(...)` lines of a run with -s):
  production  flows 0.19 (PRBF ramp, err 2.2e-7)  gW1 0.13 (PFF ones, err 5.2e-6, unit 1.0e-5)  gW1[:, :3] 0.02  gW2 0.10  gW3 0.05  gW4 0.09
              gb1 0.28  gb2 0.40  gb3 0.31  gb4 0.28
  ragged      flows 0.20  gW1 0.11  gW1[:, :3] 0.05  gW2 - gW4 0.09 - 0.15  gb1 - gb3 0.41 - 0.52  gb4 0.94 (err 2.7e-7, unit 7.1e-8: the same
              figure as in tests/test_gpu_flownet.py, gb4 = scale * sum(up) does not depend on the network)
  fixture     flows 0.34  flows vs fixture 0.26  gW1 0.17  gW1[:, :3] 0.16  gb3 0.59  gb4 0.90
  End to end: the first five losses of the fused and the composed loop are equal to all printed digits (0.1320481 .. 0.1255973), the final
  ones 0.0106249 / 0.0106151, 48 of 515 features open after 60 steps, 32 mask uploads.  40 tests, 9 s.
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
from test_flownet_progressive_golden import NETS, SCALE, build, controller  # noqa: E402
from test_gpu_flownet import CEIL, F64, GRIDS, axes, check  # noqa: E402

MASKS = ('ones', 'mid', 'init', 'ramp')
GNAMES = [f'g{k}{l}' for l in (1, 2, 3, 4) for k in ('W', 'b')]


@pytest.fixture(scope='module')
def dev():
    import sin_inn_amd  # noqa: F401
    assert torch.cuda.is_available(), 'GPU tests need a GPU'
    return torch.device('cuda', 0)


@pytest.fixture(scope='module')
def gold():
    return np.load(os.path.join(ROOT, 'tests', 'golden', 'golden_flownet_progressive.npz'))


def host_mask(gold, kind):
    return torch.ones(515) if kind == 'ones' else torch.from_numpy(gold[f'mask_{kind}'])


@pytest.mark.parametrize('kind', MASKS)
@pytest.mark.parametrize('grid', list(GRIDS))
@pytest.mark.parametrize('name', NETS)
def test_forward_and_backward_against_float64(dev, gold, name, grid, kind):
    from sin_inn_amd import _lib, flownet
    net = build(name).to(dev)
    bufs, weights = net_tensors(net, dev)
    times, ys, xs = axes(GRIDS[grid], dev)
    n = times.numel() * ys.numel() * xs.numel()
    hmask = host_mask(gold, kind)
    mask, ka = hmask.to(dev), flownet.last_open(hmask)
    assert ka == {'ones': 515, 'mid': 84, 'init': 6, 'ramp': 84}[kind]
    tag = f'{name} {grid} {kind}'

    # ---- forward, both modes, skipped and unskipped ----
    infer, none = flownet.flownet_forward(net, times, ys, xs, SCALE, False, mask=mask, k_active=ka)
    assert none is None
    nbytes = _lib.lib().sininn_flownet_saved_bytes(n)
    saved = torch.full((3, nbytes // (3 * 256 * 4), 256), float('nan'), device=dev)
    train, saved = flownet.flownet_forward(net, times, ys, xs, SCALE, True, saved, mask=mask, k_active=ka)
    assert torch.equal(infer, train)
    assert bool(torch.isfinite(saved).all()) and float(saved.min()) >= 0.0
    full, saved_full = flownet.flownet_forward(net, times, ys, xs, SCALE, True, mask=mask, k_active=515)
    assert torch.equal(full, infer), 'skipping the closed features changed the flows'
    assert torch.equal(saved_full, saved)
    with torch.no_grad():
        ref64 = restate(name, bufs, weights, times, ys, xs, SCALE, F64, mask)
        ref32 = restate(name, bufs, weights, times, ys, xs, SCALE, torch.float32, mask)
    check(f'{tag} flows', infer, ref64, ref32)
    if grid == 'fixture' and kind in ('ones', 'mid'):
        g64 = torch.from_numpy(gold[f'{name}_out64_{kind}']).to(dev)
        g32 = torch.from_numpy(gold[f'{name}_out32_{kind}']).to(dev)
        check(f'{tag} flows vs fixture', infer, g64, g32)
    if grid == 'fixture' and kind == 'ramp':
        check(f'{tag} flows vs fixture', infer, torch.from_numpy(gold[f'{name}_out64_ramp']).to(dev), ref32)
    del ref64, ref32, full, saved_full

    # ---- backward with the gates the kernel took ----
    gates = [saved[l, :n] > 0 for l in range(3)]
    up = torch.randn(infer.shape, generator=torch.Generator().manual_seed(11)).to(dev)
    grads_ref = {}
    for dtype in (F64, torch.float32):
        w = [p.to(dtype).requires_grad_(True) for p in weights]
        flows = restate(name, bufs, w, times, ys, xs, SCALE, dtype, mask, gates)
        grads_ref[dtype] = torch.autograd.grad((flows * up.to(dtype)).sum(), w)
        del flows
    wbytes = _lib.lib().sininn_flownet_workspace_bytes(n)
    ws = torch.full((wbytes // 4,), float('nan'), device=dev)
    got = flownet.flownet_backward(net, times, ys, xs, SCALE, up, saved, ws, mask=mask, k_active=ka)
    again = flownet.flownet_backward(net, times, ys, xs, SCALE, up, saved, ws, mask=mask, k_active=ka)
    ws.fill_(float('nan'))
    unskipped = flownet.flownet_backward(net, times, ys, xs, SCALE, up, saved, ws, mask=mask, k_active=515)
    assert tuple(got[0].shape) == (256, 515)
    for nm, a, b, c in zip(GNAMES, got, again, unskipped):
        assert bool(torch.isfinite(a).all()), nm
        assert torch.equal(a, b), f'{nm}: two backward calls differ'
        assert torch.equal(a, c), f'{nm}: the skipped and the unskipped path differ'
    closed = mask == 0
    for g in (got[0], unskipped[0]):
        assert bool((g[:, closed] == 0.0).all()) and not bool(torch.signbit(g[:, closed]).any())
    assert bool((got[0][:, :3] != 0.0).any(dim=0).all()), 'a coordinate column of gW1 is all zero'
    for nm, g, r64, r32 in zip(GNAMES, got, grads_ref[F64], grads_ref[torch.float32]):
        check(f'{tag} {nm}', g, r64, r32)
    check(f'{tag} gW1 coordinate columns', got[0][:, :3], grads_ref[F64][0][:, :3], grads_ref[torch.float32][0][:, :3])


@pytest.mark.parametrize('name', NETS)
def test_flow_fields_controller_override_and_bare_model(dev, gold, name):
    """the public surface: a controller's own mask takes the skipped path, an override_mask on the device the unskipped one, and they
    agree bitwise in flows and parameter gradients; a bare model is the all-ones mask; the device copy is refreshed only on change"""
    from sin_inn_amd import flownet
    net = build(name).to(dev)
    ctl = controller('early', net)
    for i in range(98):
        ctl.stash_iteration(torch.tensor(0.5))
    assert np.array_equal(ctl.mask.numpy(), gold['mask_ramp'])
    times = torch.tensor([0.0, 0.5], device=dev)
    up = torch.randn(2, 4, 20, 28, generator=torch.Generator().manual_seed(11)).to(dev)
    params = [p for lin in net.linears() for p in (lin.weight, lin.bias)]

    def run(target, **kw):
        for p in params:
            p.grad = None
        f12, f21 = flownet.flow_fields(target, times, 20, 28, SCALE, **kw)
        assert f12.shape == (2, 2, 20, 28) and f12.requires_grad
        (f12 * up[:, :2]).sum().add((f21 * up[:, 2:]).sum()).backward()
        return torch.cat((f12, f21), 1).detach(), [p.grad.clone() for p in params]

    own_f, own_g = run(ctl)
    assert ctl.uploads == 1 and ctl.device_mask(dev)[1] == 84
    over_f, over_g = run(ctl, override_mask=ctl.mask.to(dev))
    host_f, host_g = run(net, override_mask=ctl.mask.clone())
    assert ctl.uploads == 1
    for f, g in ((over_f, over_g), (host_f, host_g)):
        assert torch.equal(own_f, f)
        for nm, a, b in zip(GNAMES, own_g, g):
            assert torch.equal(a, b), nm
    assert bool((own_g[0][:, 84:] == 0.0).all()) and bool((own_g[0][:, :84] != 0).any())
    _, ys, xs = axes(GRIDS['fixture'], dev)
    direct, _ = flownet.flownet_forward(net, times, ys, xs, SCALE, False, mask=ctl.mask.to(dev))
    assert torch.equal(direct, own_f)
    # a bare model is evaluated under all ones; an override beats the controller's mask
    ones = torch.ones(515, device=dev)
    bare_f, bare_g = run(net)
    ones_f, ones_g = run(ctl, override_mask=ones)
    assert torch.equal(bare_f, ones_f) and not torch.equal(bare_f, own_f)
    for a, b in zip(bare_g, ones_g):
        assert torch.equal(a, b)
    g64 = torch.from_numpy(gold[f'{name}_out64_ones']).to(dev)
    g32 = torch.from_numpy(gold[f'{name}_out32_ones']).to(dev)
    check(f'{name} bare model vs fixture', bare_f, g64, g32)
    # the device copy follows the host mask
    ctl.stash_iteration(torch.tensor(0.5))                     # iteration 99: the block moves to 0.75
    with torch.no_grad():
        i12, i21 = flownet.flow_fields(ctl, times, 20, 28, SCALE)
        o12, o21 = flownet.flow_fields(net, times, 20, 28, SCALE, override_mask=ctl.mask.to(dev))
    assert ctl.uploads == 2 and not i12.requires_grad
    assert torch.equal(i12, o12) and torch.equal(i21, o21) and not torch.equal(i12, own_f[:, :2])
    with pytest.raises(NotImplementedError):
        flownet.flow_fields(ctl, times.cpu(), 20, 28, SCALE)
    with pytest.raises(ValueError):
        flownet.flow_fields(flownet.RbfModel(flownet.ModelParams()).to(dev), times, 20, 28, SCALE, override_mask=ones)


def test_fit_flow_end_to_end(dev):
    """60 steps of tools/fit_flow.py --net PRBF at 64 x 96 with the fused network and with the network composed from torch ops (same
    seed, same optimiser, same controller): per-step loss within CEIL relative for the first 5 steps (the tolerance of the end-to-end
    test of tests/test_gpu_flownet.py), the loss falls in both, and the controller opens the mask as the reference's does: one block
    of 6 features every 8 iterations."""
    sys.path.insert(0, os.path.join(ROOT, 'tools'))
    import fit_flow
    fi, ci = {}, {}
    fused = fit_flow.fit('PRBF', 64, 96, 60, composed=False, info=fi)
    comp = fit_flow.fit('PRBF', 64, 96, 60, composed=True, info=ci)
    for s in range(5):
        print(f'step {s}: fused {fused[s]:.7f} composed {comp[s]:.7f} rel {abs(fused[s] - comp[s]) / abs(comp[s]):.3g}')
    print(f'final: fused {fused[-1]:.7f} composed {comp[-1]:.7f}; open {fi["net"].cur_block} / 515, uploads {fi["net"].uploads}')
    for s in range(5):
        assert abs(fused[s] - comp[s]) <= CEIL * abs(comp[s]), (s, fused[s], comp[s])
    assert fused[-1] < fused[0] and comp[-1] < comp[0]
    for info in (fi, ci):
        ctl = info['net']
        assert ctl.iteration == 60 and ctl.cur_block == 6 + 6 * (60 // 8) and ctl.next_block == ctl.cur_block + 6
        assert float(ctl.mask.sum()) == ctl.cur_block + 6 * 1.0      # iteration 60: 60 % 8 = 4, the block in progress stands at 1
    assert fi['net'].uploads <= 60
