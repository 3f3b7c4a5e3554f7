"""GPU: the flow-field network kernels (csrc/flownet.hip) per ELEMENT against float64, for RBF, FFN, RBFG, PE (the narrow layer 1) and the
progressive PRBF and PPE under the fixture's `mask_ramp` with the k_active a controller would pass.  The budgets, the cases and the
references are those of tests/flownet_element_refs.py; tests/test_flownet_elements_host.py has established on the CPU that every budget
and precondition is satisfiable and that seeded defects fall outside them.  DESIGN 14.13

Part A, the backward pass on exact integers.  `flownet_backward` is fed a synthetic `saved` in {0, 1, 2} (rows N .. Npad - 1 hold 3 and
must not matter), sparse W2 / W3 and a W4 in {-1, 0, 1} written into the network's parameters, dflows in {-1, 0, 1} and scale = 2.
Everything downstream of layer 1 is then sums of products of small integers, exact in fp32 in any order of tiles, chunks and partials
(sum |terms| < 2^23, asserted from float64): gb1, gW2, gb2, gW3, gb3, gW4, gb4 must EQUAL float64 in every element, and two calls are
bitwise equal with the workspace filled with NaN before the first.  gW1 regenerates the encoding and is held per element to
    |gW1[j][k] - ref64| <= (chain + partials + c) u S[j][k] + MULT D[j][k]
with S = sum_p |dh1[p][j]| |x_k(p)|, D = sum_p |dh1[p][j]| delta_k, delta_k = max(2 u, max_p |x_k in fp32 torch - x_k in float64|),
chain = 64 x the most tiles a chunk walks, partials = the chunks (both from the plan rebuilt here and asserted), c = 2 (the product and
the store) or 3 (progressive: the folded mask), MULT = 4.  Closed columns of a progressive gW1 are an exact +0; PRBF is also run with the
unskipped k_active, which must give the same bits.
Shapes: one point; 171 points as a pose list (three tiles, the last ragged, every block and chunk owns one tile); the grid 3 x 113 x 200
(1060 tiles: chain blocks walk 2 or 3 tiles, hidden chunks 8 or 9, layer-1 chunks 16 or 17, narrow chunks 4 or 5; tiles straddle frames,
the last tile has 24 live rows).

Part B, the forward pass layer by layer from the kernel's own `saved` (random normal weights as built, scale = 3, `saved` NaN-filled
first): saved[0] against relu(x W1^T + b1) with x in float64, budget (K + c) u (|x| |W1|^T + |b1|) + MULT delta |W1|^T (K the live
inputs; progressive: W1 * mask, c = 3); saved[l] against relu(saved[l - 1] W^T + b), budget (256 + 2) u (..); flows against
(saved[2] W4^T + b4) scale, budget (256 + 3) u (..) scale.  Single-stage bounds, ReLU is 1-Lipschitz, no element excluded; rows
N .. Npad - 1 of `saved` are finite; the inference-mode flows are bitwise the training-mode ones.
Shapes: one point; 3 x 13 x 37 (1443 points, tiles straddling frames, a ragged last tile); 3 x 151 x 290 (2053 tiles, five forward blocks
take a second tile; RBF and PRBF).

Measured on an MI355X (`ratio(...)` lines of a run with -s: error / budget): see DESIGN 14.13.
"""
import os
import sys

import pytest
import torch

pytestmark = pytest.mark.gpu
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import flownet_element_refs as R  # noqa: E402
from flownet_refs import PROGRESSIVE, is_plus_zero, nan_saved, nan_workspace, net_tensors  # noqa: E402

F64 = torch.float64
A_CASES = [(name, shape, False) for name in R.NETS for shape in R.A_SHAPES] + [('PRBF', shape, True) for shape in R.A_SHAPES]
B_CASES = [(name, shape) for name in R.NETS for shape in R.B_SHAPES if shape != 'past_cap' or name in R.B_PAST_CAP_NETS]
_integer = {}


@pytest.fixture(scope='module')
def dev():
    import sin_inn_amd  # noqa: F401
    assert torch.cuda.is_available(), 'GPU tests need a GPU'
    return torch.device('cuda', 0)


def integer_case(shape, dev):
    """(points, inputs, float64 gradients, dh1, worst sum |terms|) of a part A shape on the device, computed once and left unchanged"""
    if shape not in _integer:
        pts = R.Points(R.A_SHAPES[shape], dev)
        inp = {k: v.to(dev) for k, v in R.integer_inputs(pts.n, R.Plan(pts.n).npad).items()}
        grads, dh, _, worst = R.backward_ref(inp, pts.n)
        _integer[shape] = (pts, inp, grads, dh[0], worst)
    return _integer[shape]


def forward(net, pts, scale, train, saved=None, mask=None, k_active=None):
    """(flows (4, N), saved)"""
    from sin_inn_amd import flownet
    if pts.grid is None:
        return flownet.flownet_forward_points(net, pts.list, scale, train, saved, mask=mask, k_active=k_active)
    flows, saved = flownet.flownet_forward(net, pts.times, pts.ys, pts.xs, scale, train, saved, mask=mask, k_active=k_active)
    assert tuple(flows.shape) == (pts.grid[0], 4, *pts.grid[1:])
    return pts.planar(flows), saved


def backward(net, pts, scale, dflows, saved, workspace, mask=None, k_active=None):
    from sin_inn_amd import flownet
    if pts.grid is None:
        return flownet.flownet_backward_points(net, pts.list, scale, dflows, saved, workspace, mask=mask, k_active=k_active)
    return flownet.flownet_backward(net, pts.times, pts.ys, pts.xs, scale, pts.shaped(dflows), saved, workspace, mask=mask, k_active=k_active)


def test_plans_are_the_ones_the_cases_rely_on():
    wide, narrow = R.Plan(67800, 'RBF'), R.Plan(67800, 'PE')
    assert (wide.ntiles, wide.chain_walk, wide.hidden_walk, wide.l1_walk, narrow.l1_walk) == (1060, (2, 3), (8, 9), (16, 17), (4, 5))
    assert (wide.chain_blocks, wide.hidden_chunks, wide.l1_chunks, narrow.l1_chunks) == (512, 128, 64, 256)
    few = R.Plan(171, 'RBF')
    assert (few.ntiles, few.chain_walk, few.hidden_walk, few.l1_walk) == (3, (1, 1), (1, 1), (1, 1))
    cap = R.Plan(3 * 151 * 290)
    assert (cap.ntiles, cap.fwd_blocks, cap.fwd_walk) == (2053, 2048, (1, 2))


@pytest.mark.parametrize('name,shape,unskipped', A_CASES)
def test_backward_on_exact_integers(dev, name, shape, unskipped):
    pts, inp, grads, dh1, worst = integer_case(shape, dev)
    n, plan = pts.n, R.Plan(pts.n, name)
    assert (R.Points(R.A_SHAPES[shape]).n, tuple(inp['saved'].shape)) == (n, (3, plan.npad, 256))
    assert max(worst.values()) < R.EXACT_LIMIT, worst
    net = R.build(name).to(dev)
    with torch.no_grad():
        for lin, key in zip(net.linears()[1:], ('W2', 'W3', 'W4')):
            lin.weight.copy_(inp[key])
    bufs, weights = net_tensors(net, dev)
    host, k_active = R.ramp(name)
    mask = None if host is None else host.to(dev)
    kw = dict(mask=mask, k_active=host.numel() if unskipped else k_active)
    assert tuple(nan_saved(n, dev).shape) == tuple(inp['saved'].shape)
    ws = nan_workspace(n, dev)
    got = backward(net, pts, R.SCALE_A, inp['dflows'], inp['saved'], ws, **kw)
    again = backward(net, pts, R.SCALE_A, inp['dflows'], inp['saved'], ws, **kw)
    got, again = dict(zip(R.GRAD_NAMES, got)), dict(zip(R.GRAD_NAMES, again))
    for nm in R.GRAD_NAMES:
        assert torch.equal(got[nm], again[nm]), f'{nm}: two backward calls differ'
    wrong = [nm for nm in R.EXACT_NAMES if not torch.equal(got[nm].to(F64), grads[nm].view_as(got[nm]))]
    for nm in wrong:
        bad = got[nm].to(F64) != grads[nm].view_as(got[nm])
        print(f'{name} {shape} {nm}: {int(bad.sum())} of {bad.numel()} elements differ from float64, first at {torch.nonzero(bad)[0].tolist()}')
    assert not wrong, wrong
    ref, budget, _ = R.gw1_ref(name, bufs, pts, mask, dh1, plan)
    ratio = R.element_ratio(got['gW1'], ref, budget)
    print(f'ratio({name} {shape}{" unskipped" if unskipped else ""} gW1) = {ratio:.3g}   '
          f'[chain {plan.p * plan.l1_walk[1]}, partials {plan.l1_chunks}, worst sum|terms| {max(worst.values()):.0f}]')
    assert tuple(got['gW1'].shape) == tuple(ref.shape)
    assert ratio <= 1
    if name in PROGRESSIVE:
        closed = R.closed_columns(mask, k_active)
        assert bool(closed.any()) and is_plus_zero(got['gW1'][:, closed])
    if unskipped:
        skipped = backward(net, pts, R.SCALE_A, inp['dflows'], inp['saved'], nan_workspace(n, dev), mask=mask, k_active=k_active)
        for nm, a in zip(R.GRAD_NAMES, skipped):
            assert torch.equal(a, got[nm]), f'{nm}: the skipped and the unskipped path differ'


@pytest.mark.parametrize('name,shape', B_CASES)
def test_forward_layer_by_layer(dev, name, shape):
    pts = R.Points(R.B_SHAPES[shape], dev)
    n, plan = pts.n, R.Plan(pts.n)
    net = R.build(name).to(dev)
    bufs, weights = net_tensors(net, dev)
    host, k_active = R.ramp(name)
    mask = None if host is None else host.to(dev)
    infer, none = forward(net, pts, R.SCALE_B, False, mask=mask, k_active=k_active)
    assert none is None
    flows, saved = forward(net, pts, R.SCALE_B, True, nan_saved(n, dev), mask=mask, k_active=k_active)
    assert torch.equal(infer, flows), 'the inference-mode flows are not the training-mode ones'
    assert tuple(saved.shape) == (3, plan.npad, 256) and bool(torch.isfinite(saved[:, n:]).all())
    ratios = {}
    for stage, (got, ref, budget) in R.forward_stages(name, bufs, weights, pts, mask, saved, flows).items():
        ratios[stage] = R.element_ratio(got, ref, budget)
        print(f'ratio({name} {shape} {stage}) = {ratios[stage]:.3g}')
    assert all(v <= 1 for v in ratios.values()), ratios
