"""GPU: the radial-basis-grid encoding of the flow-field network kernels (csrc/flownet.hip, SININN_FLOWNET_RBFG) for RBFG and PRBFG
against float64, with the method and the constants of tests/test_gpu_flownet.py: error against float64 <= min(4 x the deviation of
the same formula in fp32 torch, measured here, 1e-4), max-norm relative to max |ref|, gradients with the kernel's own gates forced
(`saved > 0`), no element excluded.  The reference is `restate` / `encode_grid` of tests/test_flownet_grid_golden.py, which that file
ties to the reference's own model.py / progressive_controller.py through the fixture.

Grids: the fixture's (t = 2, 20 x 28: 1120 points, a partial 18th tile) and a ragged one (times 0, 0.25, 1.0; 37 x 53: 5883 points,
tiles straddling frames).  Nothing runs at production size.

The encoding probe reads the encoding out of the kernel: with layer 1's weight a +-one-hot selection and a zero bias, `saved[0]` of
the training-mode forward is relu(+-e) exactly, and relu(e) - relu(-e) is every encoded feature of every point as the kernel
generated it.  It is compared with the float64 encoding in absolute max-norm (the range is [-1, 1]) against 4 units, the unit being
the fp32-torch encoding's own deviation from float64 on the same points.

Measured on an MI355X (`ratio(...)` lines of a run with -s: error / budget [error, fp32-torch unit]):
  encoding  fixture 0.246 [abs 8.32e-06, unit 8.44e-06]  ragged 0.25 [abs 1.03e-05, unit 1.03e-05]: the kernel is as far from float64
            as torch's fp32 evaluation is, it inherits the rounding of x + offset where |xa| reaches 49
  RBFG fixture  flows 0.221 [7.02e-07, 7.93e-07]  vs fixture 0.252  gW1 0.215 [1.59e-06, 1.85e-06]  gb1 0.304  gW2 0.112  gb2 0.206
                gW3 0.0957  gb3 0.501 [2.82e-07, 1.41e-07]  gW4 0.219  gb4 0.9 [4.11e-07, 1.14e-07]
  RBFG ragged   flows 0.245 [1.11e-06, 1.13e-06]  gW1 0.144 [1.8e-06, 3.14e-06]  gb1 0.25  gW2 0.0505  gb2 0.304  gW3 0.0475  gb3 0.243
                gW4 0.0946  gb4 0.34 [9.51e-08, 6.99e-08]
  PRBFG fixture (worst over ones / mid / ramp)  flows 0.302 (ramp, err 3.82e-07)  vs fixture 0.302  gW1 0.147  gW1[:, :3] 0.137  gb1 0.313
                gW2 0.144  gb2 0.457  gW3 0.144  gb3 0.532  gW4 0.256  gb4 0.9 (the figure of tests/test_gpu_flownet.py: gb4 = scale * sum(up)
                does not depend on the network)
  End to end: the first five losses of the fused and the composed loop agree to 9.5e-08 relative (0.1368096 .. 0.0786947), the final ones are
  0.0560618 / 0.0545410.  21 tests, 10 s.
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
from flownet_refs import encode_grid, nan_saved, nan_workspace, net_tensors, poses_of, reference_grads, restate  # noqa: E402
from test_flownet_grid_golden import N_MID, N_RAMP, SCALE, TIMES, GH, GW, build, controller  # noqa: E402
from test_gpu_flownet import CEIL, F64, MULT, axes, check  # noqa: E402

GRIDS = {'fixture': (TIMES, GH, GW), 'ragged': ((0.0, 0.25, 1.0), 37, 53)}
GNAMES = [f'g{k}{l}' for l in (1, 2, 3, 4) for k in ('W', 'b')]
K_ACTIVE = (0, 3, 4, 19, 20, 131, 132, 259, 260, 515)     # the coordinates alone, the 16-feature K step, the 128-column tile


@pytest.fixture(scope='module')
def dev():
    import sin_inn_amd  # noqa: F401
    assert torch.cuda.is_available(), 'GPU tests need a GPU'
    return torch.device('cuda', 0)


@pytest.fixture(scope='module')
def gold():
    return np.load(os.path.join(ROOT, 'tests', 'golden', 'golden_flownet_grid.npz'))


@pytest.mark.parametrize('grid', list(GRIDS))
def test_encoding_probe(dev, grid):
    from sin_inn_amd import flownet
    net = build('RBFG').to(dev)
    bufs, _ = net_tensors(net, dev)
    times, ys, xs = axes(GRIDS[grid], dev)
    n = times.numel() * ys.numel() * xs.numel()
    lin = net.linears()[0]
    got = torch.empty(n, 512, device=dev)
    with torch.no_grad():
        lin.bias.zero_()
        for half in (0, 1):
            parts = []
            for sign in (1.0, -1.0):
                lin.weight.zero_()
                rows = torch.arange(256, device=dev)
                lin.weight[rows, 256 * half + rows] = sign
                _, saved = flownet.flownet_forward(net, times, ys, xs, SCALE, True, nan_saved(n, dev))
                parts.append(saved[0, :n].clone())
            assert bool(((parts[0] == 0) | (parts[1] == 0)).all())
            got[:, 256 * half:256 * half + 256] = parts[0] - parts[1]
    assert bool(torch.isfinite(got).all()) and float(got.abs().max()) <= 1.0
    enc64 = encode_grid(bufs, poses_of(times, ys, xs, F64))
    enc32 = encode_grid(bufs, poses_of(times, ys, xs, torch.float32))
    unit = float((enc32.to(F64) - enc64).abs().max())
    err = float((got.to(F64) - enc64).abs().max())
    budget = MULT * unit
    print(f'ratio(RBFG {grid} encoding) = {err / budget:.3g}   [abs err {err:.3g}, fp32-torch unit {unit:.3g}, budget {budget:.3g}]')
    # the probe exercises the floor-mod of a negative argument and the wrap: xa < 0 exists, and the fastest frequency sees the
    # coordinates in several periods, below and above zero
    xa = poses_of(times, ys, xs, torch.float32)[:, None, :] + bufs['encode.offsets'][None]
    assert bool((xa < 0).any())
    period = 2 / bufs['encode.sigma'][-1]
    cells = torch.floor(xa[:, -1, :] / period)
    assert float(cells.min()) < 0 and float(cells.max()) > 0 and cells.unique().numel() > 2
    assert float(enc64.min()) < -0.99 and float(enc64.max()) > 0.5
    assert err <= budget, (err, budget)


@pytest.mark.parametrize('grid', list(GRIDS))
def test_forward_and_backward_against_float64(dev, gold, grid):
    from sin_inn_amd import flownet
    name = 'RBFG'
    net = build(name).to(dev)
    bufs, weights = net_tensors(net, dev)
    times, ys, xs = axes(GRIDS[grid], dev)
    n = times.numel() * ys.numel() * xs.numel()
    tag = f'{name} {grid}'

    infer, none = flownet.flownet_forward(net, times, ys, xs, SCALE, False)
    assert none is None
    train, saved = flownet.flownet_forward(net, times, ys, xs, SCALE, True, nan_saved(n, dev))
    assert torch.equal(infer, train)
    assert bool(torch.isfinite(saved).all()) and float(saved.min()) >= 0.0
    with torch.no_grad():
        ref64 = restate(name, bufs, weights, times, ys, xs, SCALE, F64)
        ref32 = restate(name, bufs, weights, times, ys, xs, SCALE, torch.float32)
    check(f'{tag} flows', infer, ref64, ref32)
    if grid == 'fixture':
        check(f'{tag} flows vs fixture', infer, torch.from_numpy(gold[f'{name}_out64']).to(dev), torch.from_numpy(gold[f'{name}_out32']).to(dev))

    gates = [saved[l, :n] > 0 for l in range(3)]
    up = torch.randn(infer.shape, generator=torch.Generator().manual_seed(11)).to(dev)
    grads_ref = reference_grads(name, bufs, weights, times, ys, xs, SCALE, up, None, gates)
    ws = nan_workspace(n, dev)
    got = flownet.flownet_backward(net, times, ys, xs, SCALE, up, saved, ws)
    again = flownet.flownet_backward(net, times, ys, xs, SCALE, up, saved, ws)
    for nm, a, b in zip(GNAMES, got, again):
        assert bool(torch.isfinite(a).all()), nm
        assert torch.equal(a, b), f'{nm}: two backward calls differ'
    for nm, g, r64, r32 in zip(GNAMES, got, grads_ref[F64], grads_ref[torch.float32]):
        check(f'{tag} {nm}', g, r64, r32)


@pytest.mark.parametrize('kind', ['ones', 'mid', 'ramp'])
def test_masks(dev, gold, kind):
    from sin_inn_amd import flownet
    name = 'PRBFG'
    net = build(name).to(dev)
    bufs, weights = net_tensors(net, dev)
    times, ys, xs = axes(GRIDS['fixture'], dev)
    n = times.numel() * ys.numel() * xs.numel()
    ctl = None
    if kind == 'ones':
        hmask = torch.ones(515)
    else:
        ctl = controller(net)
        for i in range(N_MID if kind == 'mid' else N_RAMP):
            ctl.stash_iteration(torch.tensor(0.5))
        hmask = ctl.mask.clone()
        assert np.array_equal(hmask.numpy(), gold[f'mask_{kind}'])
    mask, ka = hmask.to(dev), flownet.last_open(hmask)
    assert ka == {'ones': 515, 'mid': 84, 'ramp': 84}[kind]
    tag = f'{name} fixture {kind}'

    infer, _ = flownet.flownet_forward(net, times, ys, xs, SCALE, False, mask=mask, k_active=ka)
    train, saved = flownet.flownet_forward(net, times, ys, xs, SCALE, True, nan_saved(n, dev), mask=mask, k_active=ka)
    assert torch.equal(infer, train)
    assert bool(torch.isfinite(saved).all()) and float(saved.min()) >= 0.0
    with torch.no_grad():
        ref64 = restate(name, bufs, weights, times, ys, xs, SCALE, F64, mask)
        ref32 = restate(name, bufs, weights, times, ys, xs, SCALE, torch.float32, mask)
    check(f'{tag} flows', infer, ref64, ref32)
    g32 = torch.from_numpy(gold[f'{name}_out32_{kind}']).to(dev) if kind != 'ramp' else ref32
    check(f'{tag} flows vs fixture', infer, torch.from_numpy(gold[f'{name}_out64_{kind}']).to(dev), g32)

    gates = [saved[l, :n] > 0 for l in range(3)]
    up = torch.randn(infer.shape, generator=torch.Generator().manual_seed(11)).to(dev)
    grads_ref = reference_grads(name, bufs, weights, times, ys, xs, SCALE, up, mask, gates)
    got = flownet.flownet_backward(net, times, ys, xs, SCALE, up, saved, nan_workspace(n, dev), mask=mask, k_active=ka)
    assert tuple(got[0].shape) == (256, 515)
    closed = mask == 0
    assert bool((got[0][:, closed] == 0.0).all()) and not bool(torch.signbit(got[0][:, closed]).any())
    assert bool((got[0][:, :3] != 0.0).any(dim=0).all()), 'a coordinate column of gW1 is all zero'
    for nm, g, r64, r32 in zip(GNAMES, got, grads_ref[F64], grads_ref[torch.float32]):
        assert bool(torch.isfinite(g).all()), nm
        check(f'{tag} {nm}', g, r64, r32)
    check(f'{tag} gW1 coordinate columns', got[0][:, :3], grads_ref[F64][0][:, :3], grads_ref[torch.float32][0][:, :3])

    # the public surface: the controller's own mask (k_active = 84, skipped) or the bare model against the same mask given as a
    # device tensor (not inspected on the host: all 515 features)
    params = [p for lin in net.linears() for p in (lin.weight, lin.bias)]

    def run(target, **kw):
        for p in params:
            p.grad = None
        f12, f21 = flownet.flow_fields(target, times, GH, GW, SCALE, **kw)
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
def prbfg_case(dev):
    net = build('PRBFG').to(dev)
    times, ys, xs = axes(GRIDS['fixture'], dev)
    up = torch.randn(len(TIMES), 4, GH, GW, generator=torch.Generator().manual_seed(11)).to(dev)
    return net, times, ys, xs, up


@pytest.mark.parametrize('ka', K_ACTIVE)
def test_k_active_boundaries(dev, prbfg_case, ka):
    from sin_inn_amd import flownet
    net, times, ys, xs, up = prbfg_case
    n = times.numel() * ys.numel() * xs.numel()
    mask = torch.zeros(515, device=dev)
    mask[:ka] = 1
    flows, saved = flownet.flownet_forward(net, times, ys, xs, SCALE, True, nan_saved(n, dev), mask=mask, k_active=ka)
    full, saved_full = flownet.flownet_forward(net, times, ys, xs, SCALE, True, nan_saved(n, dev), mask=mask, k_active=515)
    assert bool(torch.isfinite(flows).all())
    assert torch.equal(flows, full) and torch.equal(saved, saved_full)
    got = flownet.flownet_backward(net, times, ys, xs, SCALE, up, saved, nan_workspace(n, dev), mask=mask, k_active=ka)
    unskipped = flownet.flownet_backward(net, times, ys, xs, SCALE, up, saved, nan_workspace(n, dev), mask=mask, k_active=515)
    for nm, a, b in zip(GNAMES, got, unskipped):
        assert bool(torch.isfinite(a).all()), nm
        assert torch.equal(a, b), f'{nm}: the skipped and the unskipped path differ at k_active {ka}'
    assert bool((got[0][:, ka:] == 0.0).all())
    if ka:
        assert bool((got[0][:, :ka] != 0.0).any(dim=0).all())


@pytest.mark.parametrize('name', ['RBFG', 'PRBFG'])
def test_autograd_function_and_inference_mode(dev, name):
    from sin_inn_amd import flownet
    net = build(name).to(dev)
    times, ys, xs = axes(GRIDS['fixture'], dev)
    f12, f21 = flownet.flow_fields(net, times, GH, GW, SCALE)
    assert f12.shape == (2, 2, GH, GW) and f21.shape == (2, 2, GH, GW) and f12.requires_grad
    up = torch.randn(2, 4, GH, GW, generator=torch.Generator().manual_seed(11)).to(dev)
    (f12 * up[:, :2]).sum().add((f21 * up[:, 2:]).sum()).backward()
    kw = dict(mask=torch.ones(515, device=dev)) if name == 'PRBFG' else {}
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


def test_fit_flow_end_to_end(dev):
    """60 steps of tools/fit_flow.py --net RBFG at 64 x 96 with the fused network and with the network composed from torch ops (same
    seed, same optimiser): per-step loss within CEIL relative for the first 5 steps, final loss below the initial one in both.
    Wiring, not accuracy."""
    sys.path.insert(0, os.path.join(ROOT, 'tools'))
    import fit_flow
    fused = fit_flow.fit('RBFG', 64, 96, 60, composed=False)
    comp = fit_flow.fit('RBFG', 64, 96, 60, composed=True)
    for s in range(5):
        print(f'step {s}: fused {fused[s]:.7f} composed {comp[s]:.7f} rel {abs(fused[s] - comp[s]) / abs(comp[s]):.3g}')
    print(f'final: fused {fused[-1]:.7f} composed {comp[-1]:.7f}')
    for s in range(5):
        assert abs(fused[s] - comp[s]) <= CEIL * abs(comp[s]), (s, fused[s], comp[s])
    assert fused[-1] < fused[0] and comp[-1] < comp[0]


def test_command_line_trains_prbfg(dev, tmp_path):
    r = subprocess.run([sys.executable, os.path.join(ROOT, 'video-interpolation', 'main.py'), 'train', '--synthetic', '4', '24', '40',
                        '--net', 'PRBFG', '--batch', '2', '--epochs', '6'], cwd=str(tmp_path), capture_output=True, text=True, timeout=300)
    print(r.stdout[-2000:], r.stderr[-2000:])
    assert r.returncode == 0
    gifs = [f for f in os.listdir(os.path.join(str(tmp_path), 'results')) if f.startswith('flow_synthetic_temp_epe_') and f.endswith('.gif')]
    assert len(gifs) == 1
