"""GPU: the SIREN flow network kernels (csrc/siren.hip) against float64.

Method (that of tests/test_gpu_flownet.py, whose `check`, `axes`, MULT and CEIL are used):
  * the reference is `siren_restate` of tests/siren_refs.py in float64 on the GPU, from the fp32 weights and axis vectors the kernel
    received, widened; test_flownet_siren_golden.py ties it to the reference's own model.py through the fixture, and on the fixture
    grid the kernel is also compared with the fixture's stored outputs directly;
  * the unit of error is the deviation of the same formula evaluated in fp32 torch from float64 on the same inputs, measured in the
    test, max-norm relative to max |ref|.  The kernel is allowed MULT = 4 units and never more than the project's standing 1e-4.  Sine
    has no gates: nothing is forced and no element is excluded;
  * the inference and the training mode of the forward kernel agree bitwise; two training calls give bitwise the same flows and
    `saved`; two backward calls agree bitwise; `saved` (before the forward) and the workspace (before the first backward) are filled
    with NaN and every result is finite.

Grids, the smallest that reach each way the kernels can go wrong:
    tiny     (0.5,), 1 x 5                  5 points: one partial tile, more blocks than tiles in the weight gradient's split
    exact    (0,), 8 x 16                   128 points: tiles with no padding
    fixture  (0, 0.5), 21 x 28              1176 points: the reference's own numbers, a tile straddling a frame
    ragged   (0, 0.25, 1.0), 37 x 53        5883 points: neither H nor W a multiple of anything
    strided  (-1, 1), 130 x 257             66 820 points: 1045 tiles, more than the 512-block cap (the grid-stride loops) and every chunk
                                            of the split weight gradient; the extreme time coordinates give the largest layer-1 phases

Measured on an MI355X (`ratio(...)` lines of a run with -s: error / budget [error, fp32-torch unit]):
  grid      flows                          gW1    gb1    gW2    gb2    gW3    gb3    gW4    gb4    gW5    gb5
  tiny      0.228 [4.50e-07, 4.93e-07]     0.193  0.193  0.236  0.208  0.262  0.236  0.243  0.217  0.251  0.250
  exact     0.250 [8.07e-07, 8.07e-07]     0.232  0.255  0.242  0.242  0.229  0.239  0.242  0.223  0.279  0.117
  fixture   0.244 [8.00e-07, 8.21e-07]     0.217  0.231  0.207  0.253  0.216  0.211  0.121  0.258  0.251  0.115
            vs fixture 0.257 [8.00e-07, 7.80e-07]
  ragged    0.270 [9.39e-07, 8.68e-07]     0.221  0.255  0.103  0.245  0.131  0.265  0.0729 0.291  0.186  0.135
  strided   0.258 [1.01e-06, 9.80e-07]     0.202  0.268  0.0835 0.267  0.076  0.275  0.0631 0.232  0.106  0.122
  The kernels sit at one fp32-torch unit (a quarter of the budget) nearly everywhere; the units are 0.5 - 1.0e-6 for the flows and
  0.6e-6 - 5.3e-6 for the weight gradients.  gb5, a plain sum of up to 66 820 values whose fp32-torch unit is below one ulp, stood at 0.96
  on `strided` and 0.667 on `fixture` while every chain block rounded its double sum to one float; since the blocks' sums travel as two
  floats it is at 0.12 - 0.25 (`strided` 0.122: unit 7.39e-08, error 3.60e-08).
  omega = 1 with the weights x 30 on `ragged`: flows 0.244 [8.46e-07, 8.68e-07] (omega = 30: 0.270), gradients 0.083 - 0.34.
  End to end: fused / composed losses 0.1347243 / 0.1347243, 0.1342991 / 0.1342991, 0.1259129 / 0.1259127, 0.1219991 / 0.1219940,
  0.1179408 / 0.1179501 (relative 0, 1.1e-07, 1.5e-06, 4.2e-05, 7.9e-05: a sine network amplifies the last bit quickly), after 12 steps
  0.0717662 / 0.0705338.  Trainer: six losses 0.04279 .. 0.04168.  9 tests, 5 s.
"""
import os
import sys

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from siren_refs import siren_restate, siren_tensors  # noqa: E402
from test_gpu_flownet import CEIL, MULT, axes, check  # noqa: E402,F401
from test_flownet_siren_golden import GH, GW, SCALE, SHAPES, TIMES, build  # noqa: E402

F64 = torch.float64
GRIDS = {'tiny': ((0.5,), 1, 5), 'exact': ((0.0,), 8, 16), 'fixture': (TIMES, GH, GW), 'ragged': ((0.0, 0.25, 1.0), 37, 53),
         'strided': ((-1.0, 1.0), 130, 257)}
NAMES = [f'g{k}{l}' for l in (1, 2, 3, 4, 5) for k in ('W', 'b')]


@pytest.fixture(scope='module')
def dev():
    import sin_inn_amd  # noqa: F401
    assert torch.cuda.is_available(), 'GPU tests need a GPU'
    return torch.device('cuda', 0)


def nan_buffers(n, dev):
    from sin_inn_amd import _lib
    saved = torch.full((_lib.lib().sininn_siren_saved_bytes(n) // 4,), float('nan'), device=dev)
    ws = torch.full((_lib.lib().sininn_siren_workspace_bytes(n) // 4,), float('nan'), device=dev)
    return saved, ws


@pytest.mark.parametrize('grid', list(GRIDS))
def test_forward_and_backward_against_float64(dev, grid):
    from sin_inn_amd import flownet
    net = build().to(dev)
    weights = siren_tensors(net)
    times, ys, xs = axes(GRIDS[grid], dev)
    n = times.numel() * ys.numel() * xs.numel()
    tag = f'siren {grid}'

    # ---- forward, both modes, twice ----
    infer, none = flownet.siren_forward(net, times, ys, xs, SCALE, False)
    assert none is None
    saved, ws = nan_buffers(n, dev)
    saved2 = torch.full_like(saved, float('nan'))
    train, saved = flownet.siren_forward(net, times, ys, xs, SCALE, True, saved)
    train2, saved2 = flownet.siren_forward(net, times, ys, xs, SCALE, True, saved2)
    assert torch.equal(infer, train) and torch.equal(train, train2) and torch.equal(saved, saved2)
    assert bool(torch.isfinite(saved).all()) and bool(torch.isfinite(infer).all())
    with torch.no_grad():
        ref64 = siren_restate(weights, times, ys, xs, SCALE, F64)
        ref32 = siren_restate(weights, times, ys, xs, SCALE, torch.float32)
    check(f'{tag} flows', infer, ref64, ref32)
    if grid == 'fixture':
        gold = np.load(os.path.join(ROOT, 'tests', 'golden', 'golden_flownet_siren.npz'))
        check(f'{tag} flows vs fixture', infer, torch.from_numpy(gold['out64']).to(dev), torch.from_numpy(gold['out32']).to(dev))
    del ref64, ref32

    # ---- backward ----
    up = torch.randn(infer.shape, generator=torch.Generator().manual_seed(11)).to(dev)
    grads_ref = {}
    for dtype in (F64, torch.float32):
        w = [p.to(dtype).requires_grad_(True) for p in weights]
        flows = siren_restate(w, times, ys, xs, SCALE, dtype)
        grads_ref[dtype] = torch.autograd.grad((flows * up.to(dtype)).sum(), w)
        del flows
    got = flownet.siren_backward(net, times, ys, xs, SCALE, up, saved, ws)
    again = flownet.siren_backward(net, times, ys, xs, SCALE, up, saved, ws)
    assert [tuple(g.shape) for g in got] == SHAPES
    for nm, a, b in zip(NAMES, got, again):
        assert bool(torch.isfinite(a).all()), nm
        assert torch.equal(a, b), f'{nm}: two backward calls differ'
    for nm, g, r64, r32 in zip(NAMES, got, grads_ref[F64], grads_ref[torch.float32]):
        check(f'{tag} {nm}', g, r64, r32)


def test_autograd_function_and_inference_mode(dev):
    from sin_inn_amd import flownet
    net = build().to(dev)
    times = torch.tensor(TIMES, device=dev)
    f12, f21 = flownet.flow_fields(net, times, GH, GW, SCALE)
    assert f12.shape == (2, 2, GH, GW) and f21.shape == (2, 2, GH, GW) and f12.requires_grad
    up = torch.randn(2, 4, GH, GW, generator=torch.Generator().manual_seed(11)).to(dev)
    (f12 * up[:, :2]).sum().add((f21 * up[:, 2:]).sum()).backward()
    _, ys, xs = axes(GRIDS['fixture'], dev)
    flows, saved = flownet.siren_forward(net, times, ys, xs, SCALE, True)
    direct = flownet.siren_backward(net, times, ys, xs, SCALE, up, saved)
    for p, g in zip([q for lin in net.linears() for q in (lin.weight, lin.bias)], direct):
        assert torch.equal(p.grad, g)
    with torch.no_grad():
        i12, i21 = flownet.flow_fields(net, times, GH, GW, SCALE)
    assert not i12.requires_grad and torch.equal(i12, f12.detach()) and torch.equal(i21, f21.detach())
    # nothing trainable: the inference kernel runs, and a backward through it raises
    for p in net.parameters():
        p.requires_grad_(False)
    n12, _ = flownet.flow_fields(net, times, GH, GW, SCALE)
    assert not n12.requires_grad and torch.equal(n12, i12)
    with pytest.raises(RuntimeError, match='inference-mode forward'):
        flownet._SirenFields.apply(net, times, ys, xs, SCALE, False, *[p.requires_grad_(True) for p in net.parameters()]).sum().backward()
    with pytest.raises(ValueError):
        flownet.flow_fields(net, times, GH, GW, SCALE, override_mask=torch.ones(3))
    with pytest.raises(NotImplementedError):
        flownet.flow_fields(net, times.cpu(), GH, GW, SCALE)


def test_omega_is_a_runtime_argument(dev):
    """omega = 1 with 30 W_l, 30 b_l (l = 1 .. 4) has the phases of omega = 30 up to the rounding of the products, so the flows agree
    within the budget of the forward test; a kernel with a baked-in 30 would be off by whole radians"""
    from sin_inn_amd import flownet
    net = build().to(dev)
    weights = siren_tensors(net)
    times, ys, xs = axes(GRIDS['ragged'], dev)
    scaled = build().to(dev)
    with torch.no_grad():
        for lin in scaled.linears()[:4]:
            lin.weight.mul_(30.0)
            lin.bias.mul_(30.0)
    got, _ = flownet.siren_forward(scaled, times, ys, xs, SCALE, False, omega=1.0)
    own, _ = flownet.siren_forward(net, times, ys, xs, SCALE, False)
    with torch.no_grad():
        ref64 = siren_restate(weights, times, ys, xs, SCALE, F64)
        ref32 = siren_restate(weights, times, ys, xs, SCALE, torch.float32)
    check('siren ragged flows at omega 30', own, ref64, ref32)
    check('siren ragged flows at omega 1, weights x 30', got, ref64, ref32)
    # training mode and the backward take the same omega
    n = times.numel() * ys.numel() * xs.numel()
    saved, ws = nan_buffers(n, dev)
    train, saved = flownet.siren_forward(scaled, times, ys, xs, SCALE, True, saved, omega=1.0)
    assert torch.equal(train, got)
    up = torch.randn(got.shape, generator=torch.Generator().manual_seed(11)).to(dev)
    g1 = flownet.siren_backward(scaled, times, ys, xs, SCALE, up, saved, ws, omega=1.0)
    grads_ref = {}
    for dtype in (F64, torch.float32):
        w = [p.to(dtype).requires_grad_(True) for p in siren_tensors(scaled)]
        flows = siren_restate(w, times, ys, xs, SCALE, dtype, omega=1.0)
        grads_ref[dtype] = torch.autograd.grad((flows * up.to(dtype)).sum(), w)
    for nm, g, r64, r32 in zip(NAMES, g1, grads_ref[F64], grads_ref[torch.float32]):
        check(f'siren ragged omega 1 {nm}', g, r64, r32)


def test_trainer_trains_checkpoints_and_reloads(dev, tmp_path):
    """FlowTrainer with a SirenModel on SyntheticClip(4, 24, 40), batch 2: 6 steps of its own optimiser (FusedLAMB), then checkpoint ->
    load_from_checkpoint -> the same flows"""
    import argparse
    from sin_inn_amd import FusedLAMB, flowdata, flownet, flowtrainer

    def args_of(net):
        return argparse.Namespace(lr=1e-4, loss_l1=1, loss_census=0.1, loss_ssim=0.05, census_width=3, loss_smooth1=0.1, edge_constant=150,
                                  edge_func='gauss', occl='wang', occl_thresh=0.7, net=net)
    model = flowtrainer.FlowTrainer(args_of(build())).to(dev)
    opt = model.attach_optimizer()
    assert isinstance(opt.optimizer, FusedLAMB)
    clip = flowdata.SyntheticClip(4, 24, 40)
    params = list(model.net.parameters())
    assert len(params) == 10
    before = [p.detach().clone() for p in params]
    losses = []
    for step in range(6):
        i = step % 2
        batch = [clip.video[i:i + 2].to(dev), clip.video[i + 1:i + 3].to(dev), clip.T[i:i + 2].to(dev),
                 torch.tensor([clip.flow_scale] * 2, dtype=F64).to(dev), clip.flow[i:i + 2].to(dev)]
        opt.zero_grad()
        loss = model.training_step(batch, step)
        loss.backward()
        opt.step()
        losses.append(float(loss.detach()))
    print('siren trainer losses', losses)
    assert all(np.isfinite(losses))
    for p, b in zip(params, before):
        assert bool(torch.isfinite(p).all()) and not torch.equal(p.detach(), b)
    path = os.path.join(str(tmp_path), 'siren.ckpt')
    model.trainer.save_checkpoint(model, path)
    torch.manual_seed(5)
    again = flowtrainer.FlowTrainer.load_from_checkpoint(path, args=args_of(flownet.SirenModel(flownet.ModelParams()))).to(dev)
    assert all(k.startswith('net.model.') for k in again.state_dict())
    times = torch.tensor([0.0, 0.5], device=dev)
    with torch.no_grad():
        a12, a21 = flownet.flow_fields(model.net, times, 24, 40, 2.0)
        b12, b21 = flownet.flow_fields(again.net, times, 24, 40, 2.0)
    assert torch.equal(a12, b12) and torch.equal(a21, b21)


def test_fit_flow_end_to_end(dev):
    """12 steps of tools/fit_flow.py at 64 x 96 with the fused network and with the network composed from torch ops (same seed, same
    optimiser): per-step loss within CEIL relative for the first 5 steps.  Wiring, not accuracy."""
    sys.path.insert(0, os.path.join(ROOT, 'tools'))
    import fit_flow
    fused = fit_flow.fit('siren', 64, 96, 12, composed=False)
    comp = fit_flow.fit('siren', 64, 96, 12, composed=True)
    for s in range(5):
        print(f'step {s}: fused {fused[s]:.7f} composed {comp[s]:.7f} rel {abs(fused[s] - comp[s]) / abs(comp[s]):.3g}')
    print(f'final: fused {fused[-1]:.7f} composed {comp[-1]:.7f}')
    for s in range(5):
        assert abs(fused[s] - comp[s]) <= CEIL * abs(comp[s]), (s, fused[s], comp[s])
