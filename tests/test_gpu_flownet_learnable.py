"""GPU: the flow-field networks with learnable Fourier frequencies (RFF / PRFF; sininn_flownet_backward_encgrad of csrc/flownet.hip)
against float64, with the method and the budget of tests/test_gpu_flownet.py, unchanged: the reference is a float64 restatement
(`restate` of tests/test_flownet_learnable_golden.py, which that file ties to the reference's own model.py through the fixture) on
the GPU from the fp32 tensors the kernel received, widened; the unit of error is the same formula in fp32 torch against float64,
measured here; error <= min(4 units, 1e-4), max-norm relative to max |ref|; gradients with the kernel's own gates (`saved > 0`)
forced; no element is excluded.

Two gradients are new.  `gF` (3, 256) is the gradient with respect to the frequency matrix the kernels read,
F_eff = normalize(frequencies) * magnitudes in fp32; its reference differentiates the restatement with respect to that fp32 matrix,
widened.  `freq.grad` is what arrives at `encode.frequencies`: the kernel's gF pushed through torch's fp32 `normalize` backward,
against the float64 chain from the fp32 parameter.

Grids: the fixture's (t = 2, 20 x 28: 17 full tiles and a partial one, fewer tiles than blocks) and the ragged one (t = 3, 109 x 253:
82 731 points, a partial last tile, tiles straddling two frames, more tiles than blocks).  PRFF masks: all ones; `init`, the
controller's first mask (t, y, x, e0, e1, e2 open: the sin of frequency 1 is open and its cos is closed); `mid`, after 100
iterations (84 leading ones); `ramp`, after 98 iterations (the block in progress stands at 0.5).

Measured on an MI355X (worst error / budget over nets and masks, from the `ratio(...)` lines of a run with -s: [error, fp32-torch unit]):
  ragged   flows 0.143 (PRFF ramp) [4.17e-07, 7.28e-07]  gW1 0.0971 (RFF) [4.15e-06, 1.07e-05]  gb1 0.281  gW2 0.0726 [1.62e-06, 5.58e-06]
           gb2 0.454  gW3 0.0793 [1.53e-06, 4.82e-06]  gb3 0.423  gW4 0.105 [8.21e-07, 1.95e-06]  gb4 0.942 [2.67e-07, 7.07e-08]
           gF 0.13 (PRFF ones) [3.40e-06, 6.52e-06]  freq.grad 0.232 (RFF) [7.87e-06, 8.50e-06]
  fixture  flows 0.262 (PRFF init) [3.11e-07, 2.96e-07]  flows vs fixture 0.198  gW1 0.135 (PRFF mid) [4.44e-07, 8.22e-07]  gb1 0.325  gW2 0.113
           gb2 0.397  gW3 0.0997  gb3 0.575 (PRFF mid) [3.28e-07, 1.43e-07]  gW4 0.168  gb4 0.9 [4.11e-07, 1.14e-07]
           gF 0.227 (PRFF init) [3.15e-07, 3.46e-07]  freq.grad 0.249 (RFF) [5.33e-06, 5.36e-06]
  gb4 is the figure of tests/test_gpu_flownet.py: it does not depend on the network.
  End to end: RFF, the first losses of the fused and the composed loop 0.1364782 / 0.1364782, step 4 within 1.3e-05 relative, final
  0.0149109 / 0.0165720, frequencies moved by at most 0.0756 / 0.0755; PRFF, the first five losses equal to all printed digits
  (0.1350149 .. 0.1263025), final 0.0078944 / 0.0079031, frequencies moved by 0.0388 / 0.0384.  20 tests, 5 s.
"""
import os
import sys

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from flownet_refs import closed_frequencies, nan_buffers, net_tensors, restate  # noqa: E402
from test_flownet_learnable_golden import EPSILON, MAX_ITERATION, NETS, SCALE, build, f_eff  # noqa: E402
from test_gpu_flownet import CEIL, F64, GRIDS, axes, check  # noqa: E402

SMALL = ('fixture', 'ragged')
MASKS = {'ones': None, 'init': 0, 'mid': 100, 'ramp': 98}          # controller iterations
GNAMES = [f'g{k}{l}' for l in (1, 2, 3, 4) for k in ('W', 'b')]


@pytest.fixture(scope='module')
def dev():
    import sin_inn_amd  # noqa: F401
    assert torch.cuda.is_available(), 'GPU tests need a GPU'
    return torch.device('cuda', 0)


@pytest.fixture(scope='module')
def gold():
    return np.load(os.path.join(ROOT, 'tests', 'golden', 'golden_flownet_learnable.npz'))


def host_mask(kind):
    """the mask of the port's own controller after MASKS[kind] iterations (tests/test_flownet_learnable_golden.py ties it to the
    reference's)"""
    if MASKS[kind] is None:
        return torch.ones(515)
    from sin_inn_amd import progressive
    ctl = progressive.LinearControllerEarly(build('PRFF'), MAX_ITERATION, epsilon=EPSILON)
    for _ in range(MASKS[kind]):
        ctl.stash_iteration(torch.tensor(0.5))
    return ctl.mask.clone()


def run_case(dev, gold, name, grid, kind):
    """everything of cases 1 and 3 for one network, grid and mask; returns nothing, asserts"""
    from sin_inn_amd import flownet
    net = build(name).to(dev)
    bufs, weights = net_tensors(net, dev)
    freq, mag = bufs['encode.frequencies'], bufs['encode.magnitudes']
    feff = f_eff(freq, mag).contiguous()                           # the fp32 matrix the kernels receive
    times, ys, xs = axes(GRIDS[grid], dev)
    n = times.numel() * ys.numel() * xs.numel()
    prog = name == 'PRFF'
    hmask = host_mask(kind) if prog else None
    mkw = dict(mask=hmask.to(dev), k_active=flownet.last_open(hmask)) if prog else {}
    full = dict(mkw, k_active=515) if prog else {}
    rmask = mkw.get('mask')
    tag = f'{name} {grid} {kind}'

    # ---- forward, both modes ----
    infer, none = flownet.flownet_forward(net, times, ys, xs, SCALE, False, enc_a=feff, **mkw)
    assert none is None
    saved, ws, ews = nan_buffers(n, dev)
    train, saved = flownet.flownet_forward(net, times, ys, xs, SCALE, True, saved, enc_a=feff, **mkw)
    assert torch.equal(infer, train)
    assert bool(torch.isfinite(saved).all()) and float(saved.min()) >= 0.0
    own, _ = flownet.flownet_forward(net, times, ys, xs, SCALE, False, **mkw)          # F_eff computed by the module itself
    assert torch.equal(own, infer)
    with torch.no_grad():
        ref64 = restate(name, feff, weights, times, ys, xs, SCALE, F64, rmask)
        ref32 = restate(name, feff, weights, times, ys, xs, SCALE, torch.float32, rmask)
    check(f'{tag} flows', infer, ref64, ref32)
    if grid == 'fixture' and kind in ('plain', 'ones', 'init', 'ramp'):
        g64 = torch.from_numpy(gold[f'{name}_out64_{kind}']).to(dev)
        g32 = torch.from_numpy(gold[f'{name}_out32_{kind}']).to(dev)
        check(f'{tag} flows vs fixture', infer, g64, g32)
    del ref64, ref32

    # ---- backward with the gates the kernel took ----
    gates = [saved[l, :n] > 0 for l in range(3)]
    up = torch.randn(infer.shape, generator=torch.Generator().manual_seed(11)).to(dev)
    ref, ref_freq = {}, {}
    for dtype in (F64, torch.float32):
        w = [p.to(dtype).requires_grad_(True) for p in weights]
        fm = feff.to(dtype).requires_grad_(True)
        flows = restate(name, fm, w, times, ys, xs, SCALE, dtype, rmask, gates)
        ref[dtype] = torch.autograd.grad((flows * up.to(dtype)).sum(), w + [fm])
        fr = freq.to(dtype).requires_grad_(True)
        flows = restate(name, f_eff(fr, mag), weights, times, ys, xs, SCALE, dtype, rmask, gates)
        ref_freq[dtype], = torch.autograd.grad((flows * up.to(dtype)).sum(), [fr])
        del flows
    g_enc = torch.full((3, 256), float('nan'), device=dev)
    got, gF = flownet.flownet_backward(net, times, ys, xs, SCALE, up, saved, ws, enc_a=feff, enc_grad=True, enc_workspace=ews, g_enc_a=g_enc,
                                       **mkw)
    assert gF is g_enc and bool(torch.isfinite(gF).all())
    plain = flownet.flownet_backward(net, times, ys, xs, SCALE, up, saved, enc_a=feff, **mkw)
    for nm, a, b in zip(GNAMES, got, plain):
        assert bool(torch.isfinite(a).all()), nm
        assert torch.equal(a, b), f'{nm}: the new entry point and sininn_flownet_backward differ'
    for nm, g, r64, r32 in zip(GNAMES + ['gF'], got + [gF], ref[F64], ref[torch.float32]):
        check(f'{tag} {nm}', g, r64, r32)
    fp = freq.clone().requires_grad_(True)
    freq_grad, = torch.autograd.grad(f_eff(fp, mag), [fp], gF)       # torch's fp32 normalize backward, as flow_fields applies it
    check(f'{tag} freq.grad', freq_grad, ref_freq[F64], ref_freq[torch.float32])

    if prog:
        # closed frequencies are exact +0; the skipped and the unskipped path agree bitwise
        closed = closed_frequencies(hmask).to(dev)
        ews.fill_(float('nan'))
        _, gF_full = flownet.flownet_backward(net, times, ys, xs, SCALE, up, saved, ws, enc_a=feff, enc_grad=True, enc_workspace=ews, **full)
        assert torch.equal(gF, gF_full), 'gF: the skipped and the unskipped path differ'
        for g in (gF, gF_full):
            assert bool((g[:, closed] == 0.0).all()) and not bool(torch.signbit(g[:, closed]).any())
            assert bool((g[:, ~closed] != 0.0).any(dim=0).all()), 'an open frequency has an all-zero gradient'
        assert int(closed.sum()) == {'ones': 0, 'init': 254, 'mid': 215, 'ramp': 215}[kind]


@pytest.mark.parametrize('grid', SMALL)
@pytest.mark.parametrize('name', NETS)
def test_forward_and_backward_against_float64(dev, gold, name, grid):
    run_case(dev, gold, name, grid, 'plain' if name == 'RFF' else 'ones')


@pytest.mark.parametrize('kind', list(MASKS))
@pytest.mark.parametrize('grid', SMALL)
def test_prff_under_masks(dev, gold, grid, kind):
    run_case(dev, gold, 'PRFF', grid, kind)


@pytest.mark.parametrize('grid', SMALL)
@pytest.mark.parametrize('name', NETS)
def test_two_backward_calls_are_bitwise_equal(dev, name, grid):
    """all nine outputs, with `saved`, both workspaces and g_enc_a filled with NaN beforehand"""
    from sin_inn_amd import flownet
    net = build(name).to(dev)
    times, ys, xs = axes(GRIDS[grid], dev)
    n = times.numel() * ys.numel() * xs.numel()
    feff = net.encode.effective_frequencies().detach().contiguous()
    mkw = {}
    if name == 'PRFF':
        hmask = host_mask('ramp')
        mkw = dict(mask=hmask.to(dev), k_active=flownet.last_open(hmask))
    saved, ws, ews = nan_buffers(n, dev)
    _, saved = flownet.flownet_forward(net, times, ys, xs, SCALE, True, saved, enc_a=feff, **mkw)
    up = torch.randn(times.numel(), 4, ys.numel(), xs.numel(), generator=torch.Generator().manual_seed(11)).to(dev)
    runs = []
    for _ in range(2):
        ws.fill_(float('nan'))
        ews.fill_(float('nan'))
        g_enc = torch.full((3, 256), float('nan'), device=dev)
        got, gF = flownet.flownet_backward(net, times, ys, xs, SCALE, up, saved, ws, enc_a=feff, enc_grad=True, enc_workspace=ews,
                                           g_enc_a=g_enc, **mkw)
        runs.append(got + [gF])
    for nm, a, b in zip(GNAMES + ['gF'], *runs):
        assert bool(torch.isfinite(a).all()), nm
        assert torch.equal(a, b), f'{nm}: two backward calls differ'


@pytest.mark.parametrize('name', NETS)
def test_autograd_surface(dev, name):
    from sin_inn_amd import flownet, progressive
    net = build(name).to(dev)
    target = net
    mkw = {}
    if name == 'PRFF':                                             # under a controller, as main.py wraps it
        target = progressive.LinearControllerEarly(net, MAX_ITERATION, epsilon=EPSILON)
        for _ in range(98):
            target.stash_iteration(torch.tensor(0.5))
        mkw = dict(mask=target.mask.to(dev), k_active=flownet.last_open(target.mask))
    times = torch.tensor([0.0, 0.5], device=dev)
    up = torch.randn(2, 4, 20, 28, generator=torch.Generator().manual_seed(11)).to(dev)
    params = [q for lin in net.linears() for q in (lin.weight, lin.bias)]
    freq = net.encode.frequencies

    def run():
        for p in params + [freq]:
            p.grad = None
        f12, f21 = flownet.flow_fields(target, times, 20, 28, SCALE)
        assert f12.shape == (2, 2, 20, 28) and f12.requires_grad
        (f12 * up[:, :2]).sum().add((f21 * up[:, 2:]).sum()).backward()
        return torch.cat((f12, f21), 1).detach()

    flows = run()
    _, ys, xs = axes(GRIDS['fixture'], dev)
    feff = net.encode.effective_frequencies()
    direct_f, saved = flownet.flownet_forward(net, times, ys, xs, SCALE, True, enc_a=feff.detach().contiguous(), **mkw)
    assert torch.equal(direct_f, flows)
    direct, gF = flownet.flownet_backward(net, times, ys, xs, SCALE, up, saved, enc_a=feff.detach().contiguous(), enc_grad=True, **mkw)
    for p, g in zip(params, direct):
        assert torch.equal(p.grad, g)
    want, = torch.autograd.grad(feff, [freq], gF)                  # the direct call's gF through torch's normalize backward
    assert freq.grad is not None and torch.equal(freq.grad, want) and bool((freq.grad != 0).any())
    along = (freq.grad * freq.detach()).sum(0).abs().max() / freq.grad.abs().max()
    assert float(along) < 1e-5                                     # normalize projects out the component along each column
    if name == 'PRFF':                                             # a bare model is the all-ones mask, an override beats the controller
        target_grad = freq.grad.clone()
        for p in params + [freq]:
            p.grad = None
        o12, _ = flownet.flow_fields(net, times, 20, 28, SCALE, override_mask=target.mask.clone())
        assert torch.equal(o12.detach(), flows[:, :2])
        b12, b21 = flownet.flow_fields(net, times, 20, 28, SCALE)
        c12, _ = flownet.flow_fields(target, times, 20, 28, SCALE, override_mask=torch.ones(515, device=dev))
        assert torch.equal(b12, c12) and not torch.equal(b12.detach(), flows[:, :2])
        (b12 * up[:, :2]).sum().add((b21 * up[:, 2:]).sum()).backward()
        assert not torch.equal(freq.grad, target_grad) and bool((freq.grad != 0).any(dim=0).all())
    # frozen frequencies: the other parameters get bitwise the same gradients from the plain backward
    flows = run()
    grads = [p.grad.clone() for p in params]
    freq.requires_grad_(False)
    frozen = run()
    assert torch.equal(frozen, flows) and freq.grad is None
    for p, g in zip(params, grads):
        assert torch.equal(p.grad, g)
    freq.requires_grad_(True)
    # no_grad: inference mode, nothing saved
    with torch.no_grad():
        i12, i21 = flownet.flow_fields(target, times, 20, 28, SCALE)
    assert not i12.requires_grad and i12.grad_fn is None and torch.equal(torch.cat((i12, i21), 1), flows)
    with pytest.raises(NotImplementedError):
        flownet.flow_fields(target, times.cpu(), 20, 28, SCALE)


@pytest.mark.parametrize('name', NETS)
def test_fit_flow_end_to_end(dev, name):
    """60 steps of tools/fit_flow.py at 64 x 96 with the fused network and with the network composed from torch ops (same seed, same
    optimiser), the size, step count and criterion of the end-to-end case of tests/test_gpu_flownet.py: per-step loss within CEIL
    relative for the first 5 steps, final loss below the initial one in both; and the frequencies have moved."""
    sys.path.insert(0, os.path.join(ROOT, 'tools'))
    import fit_flow
    fi, ci = {}, {}
    fused = fit_flow.fit(name, 64, 96, 60, composed=False, info=fi)
    comp = fit_flow.fit(name, 64, 96, 60, composed=True, info=ci)
    for s in range(5):
        print(f'step {s}: fused {fused[s]:.7f} composed {comp[s]:.7f} rel {abs(fused[s] - comp[s]) / abs(comp[s]):.3g}')
    print(f'final: fused {fused[-1]:.7f} composed {comp[-1]:.7f}')
    for s in range(5):
        assert abs(fused[s] - comp[s]) <= CEIL * abs(comp[s]), (s, fused[s], comp[s])
    assert fused[-1] < fused[0] and comp[-1] < comp[0]
    from sin_inn_amd import flownet
    torch.manual_seed(0)                                            # fit's seed: the initial frequencies
    init = flownet.learnable_model_dict[name](flownet.ModelParams()).encode.frequencies.detach()
    for info in (fi, ci):
        model = info['net'].model if name == 'PRFF' else info['net']
        now = model.encode.frequencies.detach().cpu()
        moved = float((now - init).abs().max())
        print(f'frequencies moved by at most {moved:.3g}')
        assert bool(torch.isfinite(now).all()) and moved > 0
