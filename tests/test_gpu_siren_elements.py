"""GPU: the SIREN flow-network kernels (csrc/siren.hip) per ELEMENT against float64: siren_fwd_kernel, siren_bwd_chain_kernel<false|true>,
siren_transpose_kernel, siren_reduce_kernel and their use of hidden_wgrad_launch.  The budgets, the cases and the references are those of
tests/siren_element_refs.py; tests/test_siren_elements_host.py has established on the CPU that every budget and precondition is satisfiable
and that seeded defects fall outside them.  DESIGN 14.14

Part A1, the backward pass on exact integers.  `siren_backward` is fed omega = 1 and a `saved` of phases 0.0 (pad rows included), so
sincosf gives exactly (0, 1); W1 .. W5 and dflows in {-1, 0, 1} (W2 .. W4 sparse, density 1/32), quarter-integer coordinates, scale 1.
Every dz_l is then an integer and every sum exact in fp32 in any order (sum |terms| < 2^23, asserted from float64): gb1 .. gb5, gW1 and
(pose_grad) g_poses must EQUAL float64 in every element, gW2 .. gW5 and `hin` are an exact +0, dz_2 .. dz_4 in the workspace equal float64
in rows below N and are exactly 0 in rows N .. Npad - 1, the transposed weights in the workspace are bitwise the transposes, and the
pose_grad kernel gives bitwise the ten weight gradients of the plain one.
Part A2, the backward pass stage by stage on real phases: (a) those of a training-mode forward call of the network as built, (b) uniform
in [-512, 512] rad, written into `saved` directly.  Each of hin, dz_4, dz_3, dz_2, gW2 .. gW4, gb2 .. gb4, gW5, gb5, gW1, gb1, g_poses is
compared in float64 from the inputs the kernel itself used for it (`saved`, the kernel's own dz and hin), within the single-stage budgets
of `backward_stages`; the sine / cosine allowance is MULT x torch's own fp32 error on the same phases on the same device, at least 2 u.
Part B, the forward pass stage by stage from the kernel's own `saved`: u_1 from the coordinates, u_2 .. u_4 and flows from the previous
layer's phases; pad rows finite; inference flows bitwise the training flows; once more with W1, b1 x 8 (phases of some hundreds of rad).
The workspace and `saved` are NaN-filled before use; two backward calls are bitwise equal.

Shapes: one point; 171 points as a pose list (three tiles, 43 live rows in the last; pose_grad); 3 x 13 x 37 (1443 points, tiles
straddling frames); 3 x 109 x 118 as a grid and as a pose list (38 586 points, 603 tiles, 58 live rows in the last, the 512 chain blocks
walk one or two tiles, the 128 hidden chunks 4 or 5; the list with pose_grad).

Measured on an MI355X (`ratio(...)` lines of a run with -s: worst error / budget; in brackets the fp32 torch restatement on the CPU):
  A1: every element equal at all five shapes, pose_grad included (worst sum |terms| 4 849 619, gW1 at 3 x 109 x 118).
  A2, regime (a) / (b); d_sin = d_cos = 2 u (the floor) on the device in every case:
  stage      one            few            ragged           past_cap           past_cap_list      [CPU, worst]
  hin        0.108 / 0.104  0.139 / 0.139  0.139 / 0.142    0.146 / 0.146      0.150 / 0.146      [0.075]
  dz4        0.136 / 0.147  0.224 / 0.254  0.238 / 0.283    0.303 / 0.301      0.302 / 0.301      [0.31]
  dz3, dz2   0.0097/ 0.0095 0.016 / 0.021  0.019 / 0.020    0.030 / 0.026      0.027 / 0.026      [0.028]
  gW2 .. gW4 0.015 / 0.015  0.032 / 0.030  0.0082 / 0.0085  0.00077 / 0.00087  0.00076 / 0.00087  [0.080]
  gb2 .. gb4 0 / 0          0.015 / 0.014  0.0042 / 0.0032  0.00014 / 0.00016  0.00014 / 0.00016  [0.015]
  gW5        0.022 / 0.025  0.010 / 0.014  0.0045 / 0.0045  0.00034 / 0.00043  0.00053 / 0.00043  [0.034]
  gb5        0 / 0          0.35 / 0.35    0.28 / 0.28      0.30 / 0.30        0.30 / 0.30        [0.35]
  gW1        0.0083/ 0.0087 0.0008/ 0.0009 0.00026/ 0.00027 8.7e-5 / 9.5e-5    8.9e-5 / 1.1e-4    [0.0066]
  gb1        0.0083/ 0.0087 0.0005/ 0.0006 0.00021/ 0.00019 5.5e-5 / 7.1e-5    5.3e-5 / 7.1e-5    [0.0066]
  g_poses    -              0.0007/ 0.0005 -                -                  0.00097 / 0.00089  [0.0019]
  B: u1 0.345, 0.409, 0.492, 0.518, 0.648 [0.52]; u2 .. u4 at most 0.019 [0.019]; flows at most 0.0051 [0.010];
     W1, b1 x 8 on `ragged` (|u_1| <= 310): u1 0.492, u2 .. u4 0.017, flows 0.0038.
  Finding: before its fix gb5 stood at 0.97 (few) and 1.40 (ragged) of 2 u |sum| + u^2 N sum |dout|: every chain block rounded its double
  sum to one float before siren_reduce_kernel added the blocks in double.  The partial is now two floats (hi, lo); 0.35 and 0.28 since.
  The worst ratio is u1 at 0.65 (a budget of six roundings on a three-term sum; 0.52 for fp32 torch); nothing else is above 0.5.
  22 tests, 4 s.
"""
import os
import sys

import pytest
import torch

pytestmark = pytest.mark.gpu
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import siren_element_refs as R  # noqa: E402
from flownet_refs import is_plus_zero  # noqa: E402
from siren_refs import OMEGA, siren_tensors  # noqa: E402

F64 = torch.float64
NAN = float('nan')


@pytest.fixture(scope='module')
def dev():
    import sin_inn_amd  # noqa: F401
    assert torch.cuda.is_available(), 'GPU tests need a GPU'
    return torch.device('cuda', 0)


def nan_buffers(n, dev):
    """(saved, workspace) of a call at n points, flat and NaN"""
    from sin_inn_amd import _lib
    return (torch.full((_lib.lib().sininn_siren_saved_bytes(n) // 4,), NAN, device=dev),
            torch.full((_lib.lib().sininn_siren_workspace_bytes(n) // 4,), NAN, device=dev))


def forward(net, pts, scale, train, saved=None, omega=None):
    """(flows (4, N), saved)"""
    from sin_inn_amd import flownet
    if pts.grid is None:
        return flownet.siren_forward_points(net, pts.list, scale, train, saved, omega=omega)
    flows, saved = flownet.siren_forward(net, pts.times, pts.ys, pts.xs, scale, train, saved, omega=omega)
    assert tuple(flows.shape) == (pts.grid[0], 4, *pts.grid[1:])
    return pts.planar(flows), saved


def backward(net, pts, scale, dflows, saved, workspace, omega=None, pose_grad=False):
    """(the ten gradients, g_poses or None)"""
    from sin_inn_amd import flownet
    if pts.grid is None:
        out = flownet.siren_backward_points(net, pts.list, scale, dflows, saved, workspace, omega=omega, pose_grad=pose_grad)
        return out if pose_grad else (out, None)
    assert not pose_grad
    return flownet.siren_backward(net, pts.times, pts.ys, pts.xs, scale, pts.shaped(dflows), saved, workspace, omega=omega), None


def backward_twice(net, pts, scale, dflows, saved, ws, omega, pose_grad):
    got, gp = backward(net, pts, scale, dflows, saved, ws, omega, pose_grad)
    again, gp2 = backward(net, pts, scale, dflows, saved, ws, omega, pose_grad)
    for nm, a, b in zip(R.GRAD_NAMES, got, again):
        assert torch.equal(a, b), f'{nm}: two backward calls differ'
    assert gp is None or torch.equal(gp, gp2)
    return got, gp


def test_plans_are_the_ones_the_cases_rely_on():
    cap, few, ragged = R.Plan(38586), R.Plan(171), R.Plan(1443)
    assert (cap.ntiles, cap.npad - cap.n, cap.chain_blocks, cap.chain_walk, cap.hidden_chunks, cap.hidden_walk) == (603, 6, 512, (1, 2), 128, (4, 5))
    assert (few.ntiles, few.npad - few.n, few.chain_walk, few.hidden_walk) == (3, 21, (1, 1), (1, 1))
    assert (ragged.ntiles, ragged.chain_walk, ragged.hidden_walk) == (23, (1, 1), (1, 1))
    assert {s: R.Points(v).n for s, v in R.SHAPES.items()} == {'one': 1, 'few': 171, 'ragged': 1443, 'past_cap': 38586, 'past_cap_list': 38586}


@pytest.mark.parametrize('shape', list(R.SHAPES))
def test_backward_on_exact_integers(dev, shape):
    pts = R.quarter_points(R.SHAPES[shape], dev)
    n, plan = pts.n, R.Plan(pts.n)
    inp = {k: v.to(dev) for k, v in R.integer_inputs(n).items()}
    grads, dz_ref, gp_ref, worst = R.integer_ref(inp, pts.poses(F64))
    assert max(worst.values()) < R.EXACT_LIMIT, worst
    net = R.build().to(dev)
    with torch.no_grad():
        for lin, key in zip(net.linears(), ('W1', 'W2', 'W3', 'W4', 'W5')):
            lin.weight.copy_(inp[key])
    nan_saved, ws = nan_buffers(n, dev)
    saved = torch.zeros_like(nan_saved)
    assert saved.numel() == 4 * plan.lstride and ws.numel() >= plan.ws_floats
    pose_grad = shape in R.POSE_GRAD
    got, gp = backward_twice(net, pts, R.SCALE_A1, inp['dflows'], saved, ws, 1.0, pose_grad)
    dz, hin, wt, _ = R.views(ws, saved, plan.ntiles)
    dz, hin, wt = dz.clone(), hin.clone(), wt.clone()
    got = dict(zip(R.GRAD_NAMES, got))
    wrong = [nm for nm in grads if not torch.equal(got[nm].to(F64), grads[nm].view_as(got[nm]))]
    for nm in wrong:
        bad = got[nm].to(F64) != grads[nm].view_as(got[nm])
        print(f'{shape} {nm}: {int(bad.sum())} of {bad.numel()} elements differ from float64, first at {torch.nonzero(bad)[0].tolist()}')
    assert sorted(grads) == ['gW1', 'gb1', 'gb2', 'gb3', 'gb4', 'gb5'] and not wrong, wrong
    for nm in ('gW2', 'gW3', 'gW4', 'gW5'):
        assert is_plus_zero(got[nm]), f'{nm} is not an exact +0'
    assert bool((hin == 0).all()), 'hin is not exactly 0'
    for l in range(3):
        assert torch.equal(dz[l, :n].to(F64), dz_ref[l + 1]), f'dz_{l + 2} in the workspace differs from float64'
    assert bool((dz[:, n:] == 0).all()), 'rows N .. Npad - 1 of dz are not exactly 0'
    for l, key in enumerate(('W2', 'W3', 'W4')):
        assert torch.equal(wt[l], inp[key].t()), f'{key}^T in the workspace'
    if pose_grad:
        assert tuple(gp.shape) == (n, 3) and torch.equal(gp.to(F64), gp_ref), 'g_poses differs from float64'
        plain, none = backward(net, pts, R.SCALE_A1, inp['dflows'], saved, nan_buffers(n, dev)[1], 1.0, False)
        assert none is None
        for nm, a in zip(R.GRAD_NAMES, plain):
            assert torch.equal(a, got[nm]), f'{nm}: the pose_grad kernel and the plain one differ'
    print(f'exact({shape}{" pose_grad" if pose_grad else ""}): every element equal; worst sum|terms| {max(worst.values()):.0f} ({max(worst, key=worst.get)})')


@pytest.mark.parametrize('regime', ['a', 'b'])
@pytest.mark.parametrize('shape', list(R.SHAPES))
def test_backward_stage_by_stage(dev, shape, regime):
    pts = R.Points(R.SHAPES[shape], dev)
    n, plan = pts.n, R.Plan(pts.n)
    net = R.build().to(dev)
    weights = siren_tensors(net)
    saved, ws = nan_buffers(n, dev)
    if regime == 'a':
        _, saved = forward(net, pts, R.SCALE, True, saved)
    else:
        saved = R.synthetic_phases(plan.npad).to(dev).reshape(-1).contiguous()
    assert saved.numel() == 4 * plan.lstride and bool(torch.isfinite(saved).all())
    dflows = R.upstream(n).to(dev)
    pose_grad = shape in R.POSE_GRAD
    got, gp = backward_twice(net, pts, R.SCALE, dflows, saved, ws, None, pose_grad)
    dz, hin, wt, sv = R.views(ws, saved, plan.ntiles)
    assert bool((dz[:, n:] == 0).all()), 'rows N .. Npad - 1 of dz are not exactly 0'
    assert bool(torch.isfinite(hin[:, n:]).all()), 'rows N .. Npad - 1 of hin are not finite'
    for l in range(3):
        assert torch.equal(wt[l], weights[2 * l + 2].t()), f'W{l + 2}^T in the workspace'
    stages = R.backward_stages(weights, pts, OMEGA, R.SCALE, dflows, sv, dz, hin, got, plan, gp)
    assert ('g_poses' in stages) == pose_grad
    ratios = {k: R.element_ratio(*v) for k, v in stages.items()}
    d_sin, d_cos = R.trig_delta(sv[:, :n])
    print(f'ratio({shape} regime {regime}): ' + '  '.join(f'{k} {v:.3g}' for k, v in ratios.items())
          + f'   [max |phase| {float(sv.abs().max()):.4g}, d_sin {d_sin / R.U:.3g} u, d_cos {d_cos / R.U:.3g} u]')
    assert all(v <= 1 for v in ratios.values()), ratios
    if pose_grad:
        plain, _ = backward(net, pts, R.SCALE, dflows, saved, nan_buffers(n, dev)[1], None, False)
        for nm, a, b in zip(R.GRAD_NAMES, plain, got):
            assert torch.equal(a, b), f'{nm}: the pose_grad kernel and the plain one differ'


@pytest.mark.parametrize('shape', list(R.SHAPES) + ['ragged x8'])
def test_forward_stage_by_stage(dev, shape):
    pts = R.Points(R.SHAPES[shape.split()[0]], dev)
    n, plan = pts.n, R.Plan(pts.n)
    net = R.build().to(dev)
    if shape not in R.SHAPES:
        with torch.no_grad():
            net.linears()[0].weight.mul_(8.0)
            net.linears()[0].bias.mul_(8.0)
    weights = siren_tensors(net)
    infer, none = forward(net, pts, R.SCALE, False)
    assert none is None
    flows, saved = forward(net, pts, R.SCALE, True, nan_buffers(n, dev)[0])
    assert torch.equal(infer, flows), 'the inference-mode flows are not the training-mode ones'
    sv = saved.view(4, plan.npad, 256)
    assert bool(torch.isfinite(sv[:, n:]).all()), 'rows N .. Npad - 1 of saved are not finite'
    stages = R.forward_stages(weights, pts, OMEGA, R.SCALE, sv, flows)
    ratios = {k: R.element_ratio(*v) for k, v in stages.items()}
    print(f'ratio({shape}): ' + '  '.join(f'{k} {v:.3g}' for k, v in ratios.items()) + f'   [max |u_1| {float(sv[0, :n].abs().max()):.4g}]')
    assert all(v <= 1 for v in ratios.values()), ratios
