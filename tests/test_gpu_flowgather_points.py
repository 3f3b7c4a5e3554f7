"""GPU: the fused gather rule at a list of points (csrc/flowgather.hip: flowgather_points_kernel, flowgather_points_bwd_kernel;
sin_inn_amd.flowsynth.gather_at) per element against float64, forward and gradient, and the trainer's between loss at
sampled points built on it.

The reference and the budgets are those of tests/flowgather_points_refs.py, checked on every element: every case first checks on the
CPU that fp32 and float64 take the same cell at every point.  A list that spells out a frame's integer pixels must give the bits of the
grid operator `gather`, forward and gradient.  Parameter gradients of the between term, fused against composed, by the measured-unit
method of DESIGN 22.5: the unit is the composed fp32 chain against the composed float64 chain through the same network kernels,
max |g32 - g64| / max |g64| per parameter tensor, floored at one fp32 rounding (2^-24), and the fused chain is allowed MULT = 4 units
from the composed fp32 one.  The measured ratios are printed and recorded in DESIGN 23.5.
"""
import os
import sys

import pytest
import torch

pytestmark = pytest.mark.gpu
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import flowgather_grad_refs as G  # noqa: E402
import flowgather_points_refs as P  # noqa: E402
from sin_inn_amd import flowsynth, flowtrainer  # noqa: E402

F64 = torch.float64
MULT = 4


@pytest.fixture(scope='module')
def dev():
    assert torch.cuda.is_available(), 'GPU tests need a GPU'
    return torch.device('cuda', 0)


@pytest.fixture(scope='module')
def refs():
    """name -> (inputs, out64, budget, grad64, grad budget), computed once and left unchanged"""
    out = {}
    for name in P.CASES:
        inputs = P.case(name)
        i0, i1, fl, pix, pair, tau, rev, blend, g = inputs
        assert P.cells_agree(fl, pix, tau, rev), name
        out[name] = (inputs, *P.gather_at64(i0, i1, fl, pix, pair, tau, rev, blend, g))
    return out


def _ratio(got, x64, budget):
    err = (got.to(F64).cpu() - x64).abs()
    err = torch.where(torch.isfinite(err), err, torch.full_like(err, float('inf')))
    return float(torch.where(err == 0, torch.zeros_like(err), err / budget).max())


def _to(dev, t):
    return None if t is None else t.to(dev)


def fused(dev, inputs):
    """(out, d flows) of gather_at on the device for the case's upstream gradient"""
    i0, i1, fl, pix, pair, tau, rev, blend, g = inputs
    flows = fl.to(dev).clone().requires_grad_(True)
    out = flowsynth.gather_at(i0.to(dev), i1.to(dev), flows, pix.to(dev), pair.to(dev), tau.to(dev), _to(dev, rev), blend=blend,
                              flow_grad=True)
    assert out.requires_grad and out.dtype == torch.float32
    out.backward(g.to(dev))
    return out.detach(), flows.grad


# ---- 1. forward and gradient against float64, every element ----

@pytest.mark.parametrize('name', list(P.CASES))
def test_fused_within_budget_everywhere(dev, refs, name):
    inputs, o64, ob, d64, db = refs[name]
    out, grad = fused(dev, inputs)
    assert out.shape == o64.shape and grad.shape == d64.shape
    fwd, bwd = _ratio(out, o64, ob), _ratio(grad, d64, db)
    print(f'flowgather_points {name} frames {tuple(inputs[0].shape)} S={inputs[2].shape[0]} R={out.shape[0]}: worst err / budget '
          f'forward {fwd:.3f}, gradient {bwd:.3f}')
    assert fwd <= 1.0 and bwd <= 1.0
    assert float(grad[0, 2:].abs().max()) == 0.0                            # unused values of a column: exact zeros
    if grad.shape[0] == 2:
        assert float(grad[1, :2].abs().max()) == 0.0
    plain = flowsynth.gather_at(*(_to(dev, t) for t in inputs[:7]), blend=inputs[7])
    assert not plain.requires_grad and torch.equal(plain, out)              # the inference call: the same bits


def test_two_calls_give_equal_bits(dev, refs):
    inputs = refs['4099'][0]
    (o1, g1), (o2, g2) = fused(dev, inputs), fused(dev, inputs)
    assert torch.equal(o1.view(torch.int32), o2.view(torch.int32)) and torch.equal(g1.view(torch.int32), g2.view(torch.int32))


# ---- 2. planted rows at block boundaries ----

def test_planted_rows_at_block_boundaries(dev, refs):
    i0, i1, fl, pix, pair, tau, rev, blend, g = refs['4099'][0]
    b, _, h, w = i0.shape
    clean_out, clean_grad = fused(dev, (i0, i1, fl, pix, pair, tau, rev, blend, g))
    fl2, pix2, pair2, tau2 = fl.clone(), pix.clone(), pair.clone(), tau.clone()
    edges = [255, 256, 257, 511, 512, 1023, 1024, 4095, 4096, 4098]
    # both samples refused: NaN, inf and huge flows in both slabs -- the row is H alone, its gradient exactly 0
    for k, bad in zip(edges[:4], (float('nan'), float('inf'), float('-inf'), 4.0e9)):
        fl2[0, 0, k], fl2[1, 3, k] = bad, bad
    # the point itself far outside the frame, not finite, and its pair out of range: rows of exact zeros
    pix2[edges[4]] = torch.tensor([-50.0, 3.0])
    fl2[:, :, edges[4]] = 0.0
    pix2[edges[5]] = torch.tensor([float('nan'), 2.0])
    pix2[edges[6]] = torch.tensor([3.0e9, 2.0])
    pair2[edges[7]], pair2[edges[8]] = -1, b
    # the last row and column, flows zero: an integer pixel whose east and south taps are outside -- the frame's own value
    pix2[edges[9]] = torch.tensor([h - 1.0, w - 1.0])
    fl2[:, :, edges[9]] = 0.0
    tau2[edges[9]] = 0.5
    inputs = (i0, i1, fl2, pix2, pair2, tau2, rev, blend, g)
    out, grad = fused(dev, inputs)
    assert bool(torch.isfinite(out).all()) and bool(torch.isfinite(grad).all())
    assert float(grad[:, :, edges[:9]].abs().max()) == 0.0
    assert float(out[:, edges[4:9]].abs().max()) == 0.0
    o64, ob, d64, db = P.gather_at64(*inputs)
    assert _ratio(out, o64, ob) <= 1.0 and _ratio(grad, d64, db) <= 1.0
    for k in edges[:4]:                                                     # no tap: (e (a0 H0 + a1 H1)) / e
        assert float(out[:, k].abs().max()) > 0
    corner = edges[9]
    for r, a1 in enumerate(blend):
        want = ((1 - a1) * i0[int(pair[corner]), :, h - 1, w - 1] + a1 * i1[int(pair[corner]), :, h - 1, w - 1]).to(F64)
        assert float((out[r, corner].cpu().to(F64) - want).abs().max()) <= float(ob[r, corner].max())
    same = torch.ones(4099, dtype=torch.bool)
    same[edges] = False
    assert torch.equal(out[:, same].view(torch.int32), clean_out[:, same].view(torch.int32))
    assert torch.equal(grad[:, :, same].view(torch.int32), clean_grad[:, :, same].view(torch.int32))


def test_pair_out_of_range_gives_a_zero_row(dev, refs):
    i0, i1, fl, pix, pair, tau, rev, blend, g = refs['256'][0]
    pair2 = pair.clone()
    pair2[0], pair2[100], pair2[255] = 2, -7, 2 ** 31 - 1
    out, grad = fused(dev, (i0, i1, fl, pix, pair2, tau, rev, blend, g))
    rows = [0, 100, 255]
    assert float(out[:, rows].abs().max()) == 0.0 and float(grad[:, :, rows].abs().max()) == 0.0
    clean_out, clean_grad = fused(dev, refs['256'][0])
    keep = torch.ones(256, dtype=torch.bool)
    keep[rows] = False
    assert torch.equal(out[:, keep], clean_out[:, keep]) and torch.equal(grad[:, :, keep], clean_grad[:, :, keep])


# ---- 3. a list that spells out the grid gives the grid operator's bits ----

def _grid_case(dev, k_rows):
    """two pairs of 13 x 37 frames, positive random values; pair 0 is the clip's first pair (a reverse row), pair 1 a network row"""
    gen = torch.Generator().manual_seed(21)
    b, c, h, w = 2, 3, 13, 37
    i0, i1 = torch.rand(b, c, h, w, generator=gen) + 0.1, torch.rand(b, c, h, w, generator=gen) + 0.1
    stamps, slots = flowsynth.gather_slots([-1.0, -1 / 3], [0.3], 2 / 3, 'network')
    assert len(stamps) == 3 and int(slots[0, 0, 2]) == 0 and int(slots[1, 0, 2]) == 2       # reverse, then network
    flows = ((torch.rand(3, 4, h, w, generator=gen) * 2 - 1) * 5).to(dev)
    ys, xs = torch.meshgrid(torch.arange(h), torch.arange(w), indexing='ij')
    pix = torch.stack((ys.reshape(-1), xs.reshape(-1)), 1).float().repeat(b, 1)
    pair = torch.arange(b, dtype=torch.int32).repeat_interleave(h * w)
    listed = torch.full((2, 4, b * h * w), float('nan'), device=dev)
    for bb in range(b):
        cols = slice(bb * h * w, (bb + 1) * h * w)
        listed[0, :, cols] = flows[int(slots[bb, 0, 1])].reshape(4, -1)
        if int(slots[bb, 0, 2]) == 2:
            listed[1, :, cols] = flows[int(slots[bb, 0, 0])].reshape(4, -1)
    rev = (pair == 0)
    tau = torch.full((b * h * w,), 0.3)
    table = torch.cat([slots] * k_rows, dim=1).contiguous()
    return i0.to(dev), i1.to(dev), flows, table, listed, pix.to(dev), pair.to(dev), tau.to(dev), rev.to(dev), slots


@pytest.mark.parametrize('blend', [None, (0.0, 1.0)])
def test_list_of_integer_pixels_gives_the_grid_bits(dev, blend):
    rows = 1 if blend is None else 2
    i0, i1, flows, table, listed, pix, pair, tau, rev, slots = _grid_case(dev, rows)
    b, c, h, w = i0.shape
    gen = torch.Generator().manual_seed(22)
    g = (torch.rand(b, rows, c, h, w, generator=gen) * 2 - 1).to(dev)
    gflows = flows.clone().requires_grad_(True)
    want = flowsynth.gather(i0, i1, gflows, table, [0.3] if blend is None else list(blend), flow_grad=True)
    want.backward(g)
    lflows = listed.clone().requires_grad_(True)
    got = flowsynth.gather_at(i0, i1, lflows, pix, pair, tau, rev, blend=blend, flow_grad=True)
    got.backward(g.permute(1, 0, 3, 4, 2).reshape(rows, b * h * w, c).contiguous())
    assert torch.equal(got.reshape(rows, b, h, w, c).permute(1, 0, 4, 2, 3), want.detach())
    dl, dg = lflows.grad, gflows.grad
    assert bool(torch.isfinite(dl).all()) and float(dg.abs().max()) > 0
    for bb in range(b):
        cols = slice(bb * h * w, (bb + 1) * h * w)
        idx0, idx1, ch0 = (int(slots[bb, 0, k]) for k in (0, 1, 2))
        assert torch.equal(dl[0, :2, cols].reshape(2, h, w), dg[idx1, :2])                  # dG1, and under reverse dG0 + dG1
        if ch0 == 2:
            assert torch.equal(dl[1, 2:, cols].reshape(2, h, w), dg[idx0, 2:]) and float(dg[idx0, 2:].abs().max()) > 0
        else:
            assert float(dl[1, :, cols].abs().max()) == 0.0
    assert float(dl[0, 2:].abs().max()) == 0.0 and float(dl[1, :2].abs().max()) == 0.0


# ---- 4. the trainer ----

def _trainer(dev, fused_path=True, net='RBF'):
    model = flowtrainer.FlowTrainer(G.trainer_args(net=net, argv=['--loss-between', '1', '--between-points', '512'],
                                                   between_dt=2 / 3)).to(dev)
    model.fused = fused_path
    return model


def _between_grads(model, batch):
    frame1, frame2, times, scale = batch[:4]
    loss = model.between_points_loss(frame1, frame2, times, scale)
    model.between_frames.retain_grad()
    model.between_flows.retain_grad()
    params = list(model.net.parameters())
    for p in params:
        p.grad = None
    loss.backward()
    return loss.detach(), [p.grad.clone() for p in params], model.between_flows, model.between_frames, model.between_sample


def test_trainer_step_fused_against_composed(dev):
    batch = [t.to(dev) for t in G.trainer_batch()]
    frame1, frame2 = batch[0], batch[1]
    model = _trainer(dev)
    loss, grads, flows, frames, (pix, pair, tau, rev) = _between_grads(model, batch)
    assert float(loss) > 0 and tuple(flows.shape) == (2, 4, 512) and tuple(frames.shape) == (2, 512, 3)
    assert all(bool(torch.isfinite(g).all()) and float(g.abs().max()) > 0 for g in grads)
    # a fresh trainer repeats the draw: equal bits
    loss2, grads2, _, _, sample2 = _between_grads(_trainer(dev), batch)
    assert torch.equal(sample2[0], pix) and torch.equal(loss, loss2) and all(torch.equal(a, b) for a, b in zip(grads, grads2))
    # d loss_between / d flows against float64, for the upstream gradient the loss handed the operator
    fl = flows.detach().cpu()
    assert P.cells_agree(fl, pix.cpu(), tau.cpu(), rev.cpu())              # no element is left out
    o64, ob, d64, db = P.gather_at64(frame1.cpu(), frame2.cpu(), fl, pix.cpu(), pair.cpu(), tau.cpu(), rev.cpu(), (0.0, 1.0),
                                     frames.grad.cpu())
    fwd, bwd = _ratio(frames.detach(), o64, ob), _ratio(flows.grad, d64, db)
    print(f'between points RBF N=512: forward worst err / budget {fwd:.3f}, d loss / d flows {bwd:.3f}')
    assert fwd <= 1.0 and bwd <= 1.0
    # the whole step runs and trains
    step = _trainer(dev)
    logged = {}
    step.log = lambda name, value, **_: logged.__setitem__(name, value)
    step.training_step(batch, 0).backward()
    assert float(logged['train/between'].detach()) > 0 and torch.equal(logged['train/between'].detach(), loss)
    # the parameter gradients, fused against composed, in units of composed fp32 against composed float64
    _, g32, _, _, sample32 = _between_grads(_trainer(dev, fused_path=False), batch)
    assert torch.equal(sample32[0], pix)
    real = flowsynth.gather_at_composed
    try:
        flowsynth.gather_at_composed = lambda f1, f2, fl_, *a, **kw: real(f1.double(), f2.double(), fl_.double(), *a, **kw)
        _, g64, _, _, _ = _between_grads(_trainer(dev, fused_path=False), batch)
    finally:
        flowsynth.gather_at_composed = real
    for i, (gf, gc, gw) in enumerate(zip(grads, g32, g64)):
        top = float(gw.abs().max())
        measured = float((gc.to(F64) - gw.to(F64)).abs().max()) / top
        unit = max(measured, 2.0 ** -24)                                    # not below one rounding of an fp32 result
        err = float((gf.to(F64) - gc.to(F64)).abs().max()) / top
        print(f'between points RBF parameter {i}: fused - composed {err:.3g}, fp32-torch unit {unit:.3g}'
              f'{f" (measured {measured:.3g}, floored at 2^-24)" if measured < unit else ""}, ratio {err / (MULT * unit):.3g}')
        assert err <= MULT * unit, (i, err, unit)
