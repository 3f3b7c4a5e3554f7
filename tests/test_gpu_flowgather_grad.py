"""GPU: the gradient of the fused gather synthesis with respect to its flows (csrc/flowgather.hip: flowgather_bwd_kernel and
flowgather_reduce_kernel; sin_inn_amd.flowsynth.gather(.., flow_grad=True)) per element against float64, and the
in-between consistency loss of the flow trainer built on it.

The reference and the budget are those of tests/flowgather_grad_refs.py, checked on every element: the flows are built from target
coordinates whose fractional parts lie in [1/16, 15/16], and every case first checks on the CPU that fp32 and float64 take the same cell.

Parameter gradients of the between term, fused against composed: the unit is the composed fp32 chain against the composed float64
chain through the same network kernels, max |g32 - g64| / max |g64| per parameter tensor, and the fused chain is allowed MULT = 4
units from the composed fp32 one.  Both chains end in the network's fp32 backward kernels, so both gradients are fp32 numbers and their
difference is a whole number of ulps, possibly none: a unit below one rounding of the result, 2^-24 of the largest value, cannot be
measured this way and is taken as 2^-24; the test prints which tensors needed the floor.  On an MI355X: RBF parameters 3 (measured
5.3e-08), 5 (5.4e-08) and 7 (the last bias, four values: measured 8.0e-09, fused - composed 6.4e-08 = 1.07 * 2^-24); PRBF parameters 1, 3
and 5.  Every other tensor's measured unit is above 2^-24 and is used as measured.
Measured on an MI355X, RBF and PRBF: units 6.0e-08 .. 2.5e-07, fused - composed 4.3e-08 .. 2.2e-07, ratios 0.13 .. 0.5 of the MULT = 4 budget;
the fused backward against float64, worst error / budget: 1x1 0.004, 13x37 0.094, 5x1031 0.117, 24x40 0.116, 17x300 (K = 64) 0.650;
fused against composed on the device, largest difference 4.0e-07 (13x37, largest gradient 0.49) and 3.1e-07 (5x1031, 0.27); the
trainer's d loss_between / d flows 0.025 (RBF) and 0.026 (PRBF) of the budget with every element in one cell in both precisions.
"""
import ctypes as C
import os
import sys

import pytest
import torch

pytestmark = pytest.mark.gpu
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import flowgather_grad_refs as G  # noqa: E402
from sin_inn_amd import _lib, flowsynth, flowtrainer  # noqa: E402

F64 = torch.float64
MULT = 4


@pytest.fixture(scope='module')
def dev():
    assert torch.cuda.is_available(), 'GPU tests need a GPU'
    return torch.device('cuda', 0)


@pytest.fixture(scope='module')
def refs():
    """name -> (inputs, float64 gradient, budget), computed once and left unchanged"""
    out = {}
    for name in G.CASES:
        inputs = G.case(name)
        i0, i1, fl, slots, taus, g = inputs
        assert G.cells_agree(fl, slots, *i0.shape[-2:]), name
        out[name] = (inputs, *G.gather_grad64(*inputs))
    return out


def _ratio(got, x64, budget):
    err = (got.to(F64).cpu() - x64).abs()
    err = torch.where(torch.isfinite(err), err, torch.full_like(err, float('inf')))
    return float(torch.where(err == 0, torch.zeros_like(err), err / budget).max())


def fused_grad(dev, i0, i1, fl, slots, taus, g, flows=None, **kw):
    flows = fl.to(dev).clone().requires_grad_(True) if flows is None else flows
    out = flowsynth.gather(i0.to(dev), i1.to(dev), flows, slots, taus, flow_grad=True, **kw)
    assert out.requires_grad
    out.backward(g.to(dev))
    return flows.grad


# ---- 1. the fused backward against float64 ----

# both forward launch shapes at the three host cases (the backward pass has one shape); the stride and the K = 64 case once
@pytest.mark.parametrize('name,k_loop', [(n, kl) for n in G.HOST_CASES for kl in (False, True)] + [('24x40', False), ('17x300', False)])
def test_fused_gradient_within_budget_everywhere(dev, refs, name, k_loop):
    inputs, d64, budget = refs[name]
    i0, i1, fl, slots, taus, g = inputs
    flows = None
    if name == '24x40':                    # a slice stride larger than 4 H W: every other slice of a wider tensor
        wide = torch.full((fl.shape[0], 2, *fl.shape[1:]), float('nan'), device=dev)
        wide[:, 0] = fl.to(dev)
        flows = wide[:, 0].detach().requires_grad_(True)
        assert flows.stride(0) == 8 * fl.shape[-2] * fl.shape[-1] and not flows.is_contiguous()
    got = fused_grad(dev, *inputs, flows=flows, k_loop=k_loop)
    assert got.shape == d64.shape and got.dtype == torch.float32
    ratio = _ratio(got, d64, budget)
    print(f'flowgather_bwd {name} {tuple(i0.shape)} K={len(taus)} k_loop={k_loop}: worst err / budget {ratio:.3f}')
    assert ratio <= 1.0
    assert float(got[-1].abs().max()) == 0.0                            # the unnamed slice: exactly 0


def test_repeated_calls_and_both_paths_give_equal_bits(dev, refs):
    inputs, _, _ = refs['13x37']
    first, again = fused_grad(dev, *inputs), fused_grad(dev, *inputs)
    assert torch.equal(first, again)
    # a table with distinct targets: the one-launch path and the reduce path
    i0, i1, fl, slots, taus, g = refs['24x40'][0]
    assert flowsynth.gather_reduce_list(slots, fl.shape[0])[1]
    assert flowsynth.BWD_IN_PLACE is None
    try:
        flowsynth.BWD_IN_PLACE = True
        direct = fused_grad(dev, i0, i1, fl, slots, taus, g)
        with pytest.raises(ValueError, match='distinct'):
            fused_grad(dev, *inputs)                                    # 13x37 has reverse rows and a shared slice
        flowsynth.BWD_IN_PLACE = False
        reduced = fused_grad(dev, i0, i1, fl, slots, taus, g)
    finally:
        flowsynth.BWD_IN_PLACE = None
    default = fused_grad(dev, i0, i1, fl, slots, taus, g)
    assert torch.equal(direct.view(torch.int32), reduced.view(torch.int32)) and torch.equal(direct, default)


def test_non_contiguous_grad_out(dev, refs):
    i0, i1, fl, slots, taus, g = refs['13x37'][0]
    want = fused_grad(dev, i0, i1, fl, slots, taus, g)
    flows = fl.to(dev).clone().requires_grad_(True)
    out = flowsynth.gather(i0.to(dev), i1.to(dev), flows, slots, taus, flow_grad=True)
    strided = g.to(dev).permute(0, 1, 3, 4, 2).contiguous().permute(0, 1, 4, 2, 3)
    assert not strided.is_contiguous()
    out.backward(strided)
    assert torch.equal(flows.grad, want)


@pytest.mark.parametrize('name', ['13x37', '5x1031'])
def test_fused_against_composed_on_the_device(dev, refs, name):
    (i0, i1, fl, slots, taus, g), d64, budget = refs[name]
    fused = fused_grad(dev, i0, i1, fl, slots, taus, g)
    flows = fl.to(dev).clone().requires_grad_(True)
    flowsynth.gather_composed(i0.to(dev), i1.to(dev), flows, slots, taus, flow_grad=True).backward(g.to(dev))
    diff = float((fused - flows.grad).abs().max())
    print(f'fused against composed on the device, {name}: largest difference {diff:.3g} (largest gradient {float(d64.abs().max()):.3g}); '
          f'composed err / budget {_ratio(flows.grad, d64, budget):.3f}')
    assert _ratio(flows.grad, d64, budget) <= 1.0
    assert float(((fused - flows.grad).abs().cpu().to(F64) / (2 * budget)).nan_to_num(0.0).max()) <= 1.0      # both within one budget


# ---- 2. borders and non-finite flows ----

def _integer_case(h=6, w=9):
    g = torch.Generator().manual_seed(7)
    i0, i1 = torch.rand(1, 3, h, w, generator=g), torch.rand(1, 3, h, w, generator=g)
    half = G._bits(0.5)
    slots = torch.tensor([[[1, 0, 2, 0, half, half]]], dtype=torch.int32)
    go = torch.rand(1, 1, 3, h, w, generator=g) + 0.5
    return i0, i1, torch.zeros(2, 4, h, w), slots, (0.5,), go


def test_borders_on_the_device(dev):
    i0, i1, fl, slots, taus, go = _integer_case()
    w = i0.shape[-1]
    fl[0, 0] = 2.0                         # integer targets: the right-hand derivative
    fl[0, 0, :, 0] = -1.0                  # q in (-1, 0)
    fl[0, 0, :, w - 1] = 1.0               # q in (W - 1, W)
    fl[0, 0, :, 4] = 2.0 * w               # fully outside
    fl[1, 3] = -2.0
    d64, budget = G.gather_grad64(i0, i1, fl, slots, taus, go)
    got = fused_grad(dev, i0, i1, fl, slots, taus, go)
    assert _ratio(got, d64, budget) <= 1.0
    assert float(d64[0, 0, :, 0].abs().min()) > 1e-3 and float(d64[0, 0, :, w - 1].abs().min()) > 1e-3
    assert float(got[0, :2, :, 4].abs().max()) == 0.0


@pytest.mark.parametrize('bad', [float('nan'), float('inf'), float('-inf')])
def test_non_finite_flow_on_the_device(dev, bad):
    i0, i1, fl, slots, taus, go = _integer_case()
    fl[1, 2:] = 0.5
    fl[0, 0, 3, 5] = bad
    far = fl.clone()
    far[0, 0, 3, 5] = 4.0e9
    want, budget = G.gather_grad64(i0, i1, far, slots, taus, go)
    got = fused_grad(dev, i0, i1, fl, slots, taus, go)
    assert bool(torch.isfinite(got).all()) and float(got[0, :2, 3, 5].abs().max()) == 0.0
    assert _ratio(got, want, budget) <= 1.0 and float(got[1, 2:, 3, 5].abs().max()) > 0


# ---- 3. the trainer ----

def _trainer(dev, net, weight='1', fused=True, **kw):
    argv = ['--loss-between', weight, '--between-taus', '2'] if weight != '0' else []
    model = flowtrainer.FlowTrainer(G.trainer_args(net=net, argv=argv, between_dt=2 / 3, **kw)).to(dev)
    model.fused = fused
    return model


def _between_grads(model, batch):
    frame1, frame2, times, scale = batch[:4]
    loss = model.between_loss(frame1, frame2, [float(t) for t in times.tolist()], scale)
    model.between_frames.retain_grad()
    params = list(model.net.parameters())
    flows = model.between_flows
    flows.retain_grad()
    for p in params:
        p.grad = None
    loss.backward()
    return loss.detach(), [p.grad.clone() if p.grad is not None else None for p in params], flows, model.between_frames


@pytest.mark.parametrize('net', ['RBF', 'PRBF'])
def test_training_step_with_the_between_loss(dev, net):
    model = _trainer(dev, net)
    batch = [t.to(dev) for t in G.trainer_batch()]
    logged = {}
    model.log = lambda name, value, **_: logged.__setitem__(name, value)
    loss = model.training_step(batch, 0)
    loss.backward()
    assert 'train/between' in logged and float(logged['train/between'].detach()) > 0
    for p in model.net.parameters():
        if p.requires_grad:
            assert p.grad is not None and bool(torch.isfinite(p.grad).all())
    assert any(float(p.grad.abs().max()) > 0 for p in model.net.parameters() if p.grad is not None)


@pytest.mark.parametrize('net', ['RBF', 'PRBF'])
def test_between_loss_gradients(dev, net):
    batch = [t.to(dev) for t in G.trainer_batch()]
    frame1, frame2, times = batch[0], batch[1], batch[2]
    model = _trainer(dev, net)
    state = model.between_rng.getstate()
    loss, grads, flows, frames = _between_grads(model, batch)
    assert float(loss) > 0 and all(g is not None and bool(torch.isfinite(g).all()) and float(g.abs().max()) > 0 for g in grads)
    # the generator's state fixed: equal bits
    model.between_rng.setstate(state)
    loss2, grads2, _, _ = _between_grads(model, batch)
    assert torch.equal(loss, loss2) and all(torch.equal(a, b) for a, b in zip(grads, grads2))
    # d loss_between / d flows against float64, for the upstream gradient the loss handed the operator
    model.between_rng.setstate(state)
    taus = [model.between_rng.random() for _ in range(2)]
    _, table, blend = model.between_table([float(t) for t in times.tolist()], taus)
    fl = flows.detach().cpu()
    d64, budget = G.gather_grad64(frame1.cpu(), frame2.cpu(), fl, table, blend, frames.grad.cpu())
    same = _same_cells(fl, table, 24, 40)
    err = (flows.grad.cpu().to(F64) - d64).abs()
    ratio = float(torch.where(same & (err > 0), err / budget, torch.zeros_like(err)).max())
    print(f'between {net}: d loss / d flows worst err / budget {ratio:.3f}; fp32 and float64 take the same cell on {int(same.sum())} '
          f'of {same.numel()} elements')
    assert ratio <= 1.0 and bool(same.all())                           # no element is left out
    # the parameter gradients, fused against composed, in units of composed fp32 against composed float64
    composed = _trainer(dev, net, fused=False)
    composed.between_rng.setstate(state)
    _, g32, _, _ = _between_grads(composed, batch)
    wide = _trainer(dev, net, fused=False)
    wide.between_rng.setstate(state)
    real = flowsynth.gather_composed
    try:
        flowsynth.gather_composed = lambda f1, f2, fl_, tab, tau, **kw: real(f1.double(), f2.double(), fl_.double(), tab, tau, **kw)
        _, g64, _, _ = _between_grads(wide, batch)
    finally:
        flowsynth.gather_composed = real
    for i, (gf, gc, gw) in enumerate(zip(grads, g32, g64)):
        top = float(gw.abs().max())
        measured = float((gc.to(F64) - gw.to(F64)).abs().max()) / top
        unit = max(measured, 2.0 ** -24)                                # not below one rounding of an fp32 result
        err = float((gf.to(F64) - gc.to(F64)).abs().max()) / top
        print(f'between {net} parameter {i}: fused - composed {err:.3g}, fp32-torch unit {unit:.3g}'
              f'{f" (measured {measured:.3g}, floored at 2^-24)" if measured < unit else ""}, ratio {err / (MULT * unit):.3g}')
        assert err <= MULT * unit, (i, err, unit)


def _same_cells(fl, table, h, w):
    """(T', 4, H, W) bool: elements all of whose readers take the same cell in fp32 and float64"""
    import numpy as np
    same = torch.ones(fl.shape, dtype=torch.bool)
    ys, xs = np.meshgrid(np.arange(h, dtype=np.float32), np.arange(w, dtype=np.float32), indexing='ij')
    fl32 = fl.numpy()
    coef = table[..., 4:].contiguous().view(torch.float32).reshape(-1, 2).numpy()
    for row, cf in zip(table.reshape(-1, 6).tolist(), coef):
        for s in range(2):
            ok = np.ones((h, w), dtype=bool)
            for g, p in ((fl32[row[s], row[2 + s]], xs), (fl32[row[s], row[2 + s] + 1], ys)):
                q32 = p + cf[s] * g
                q64 = p.astype(np.float64) + np.float64(cf[s]) * g.astype(np.float64)
                ok &= np.floor(q32).astype(np.float64) == np.floor(q64)
            same[row[s], row[2 + s]] &= torch.from_numpy(ok)
            same[row[s], row[2 + s] + 1] &= torch.from_numpy(ok)
    return same


def test_weight_zero_is_the_parent_step(dev):
    """--loss-between 0: no generator, exactly one `forward` call and no `between_*` call -- the step is the code path it was.  The
    full loss cannot be compared bitwise between two passes: the softmax splat adds with fp32 atomics, so l1, census and their
    gradients differ in the last bits from run to run, on the parent commit too.  What is deterministic -- the network's flows, the
    smoothness term and its gradient to the parameters -- is bitwise that of a trainer built from a namespace without the switches."""
    batch = [t.to(dev) for t in G.trainer_batch()]
    outs = []
    for strip in (False, True):                     # no switch at all, and the switch with weight 0
        args = G.trainer_args(net='RBF')
        if strip:
            args = G.trainer_args(net='RBF', argv=['--loss-between', '0'])
        model = flowtrainer.FlowTrainer(args).to(dev)
        assert model.between_rng is None
        calls = []
        real = model.forward
        model.forward = lambda *a: calls.append(1) or real(*a)

        def never(*a, **kw):
            raise AssertionError('a between_* call at weight 0')
        model.between_loss = model.between_table = model._host_times = never
        logged = {}
        model.log = lambda name, value, **_: logged.__setitem__(name, value)
        kept = {}
        losses = model.losses
        model.losses = lambda f1, f2, a, b: kept.setdefault('flows', (a, b)) and losses(f1, f2, a, b)
        loss = model.training_step(batch, 0)
        assert len(calls) == 1 and 'train/between' not in logged
        smooth = logged['train/smooth']
        grads = torch.autograd.grad(smooth, list(model.net.parameters()), retain_graph=True, allow_unused=True)
        outs.append((kept['flows'][0].detach(), kept['flows'][1].detach(), smooth.detach(), grads, sorted(logged)))
        assert bool(torch.isfinite(loss))
    a, b = outs
    assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1]) and torch.equal(a[2], b[2]) and a[4] == b[4]
    assert all((x is None and y is None) or torch.equal(x, y) for x, y in zip(a[3], b[3]))


# ---- 4. the C entry point refuses before any launch ----

def test_c_entry_point_refusals(dev):
    lib = _lib.lib()
    b, k, c, h, w, t = 1, 2, 3, 4, 8, 5
    need = lib.sininn_flow_gather_bwd_workspace(b, k, h, w)
    assert need == b * k * 4 * h * w and lib.sininn_flow_gather_bwd_workspace(0, k, h, w) == 0
    i0 = torch.zeros(b, c, h, w, device=dev)
    fl = torch.zeros(t, 4, h, w, device=dev)
    slots = torch.zeros(b, k, 6, dtype=torch.int32, device=dev)
    tau = torch.zeros(k, device=dev)
    go = torch.zeros(b, k, c, h, w, device=dev)
    ws = torch.zeros(need, device=dev)
    rl = torch.zeros(2 * t + 1 + 2 * b * k, dtype=torch.int32, device=dev)
    out = torch.full((t, 4, h, w), 7.0, device=dev)
    P = lambda x: C.c_void_p(x.data_ptr()) if x is not None else None      # noqa: E731

    def call(i0=i0, i1=i0, fl=fl, stride=4 * h * w, slots=slots, tau=tau, go=go, k=k, c=c, rl=rl, n_rl=rl.numel(), ws=ws,
             n_ws=need, out=out):
        return lib.sininn_flow_gather_bwd(P(i0), P(i1), P(fl), stride, P(slots), P(tau), P(go), b, k, c, h, w, t, P(rl), n_rl, P(ws),
                                          n_ws, P(out), None)

    for what, kw in (('null', dict(i0=None)), ('null', dict(slots=None)), ('gradient of the output is null', dict(go=None)),
                     ('gradient of the flows is null', dict(out=None)), ('workspace is null', dict(ws=None)),
                     ('1 or 3 channels', dict(c=2)), ('K = 65', dict(k=65)), ('workspace holds', dict(n_ws=need - 1)),
                     ('sample stride', dict(stride=4 * h * w - 1)), ('reduce list', dict(n_rl=2 * t))):
        assert call(**kw) != 0, what
        assert what in lib.sininn_last_error().decode(), (what, lib.sininn_last_error().decode())
    torch.cuda.synchronize()
    assert float(out.min()) == 7.0 and float(out.max()) == 7.0             # nothing was launched
