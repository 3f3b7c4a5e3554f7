"""GPU: the piecewise-linear encoding of the flow-field network kernels (csrc/flownet.hip, SININN_FLOWNET_PIECEWISE) for MPFF against
float64, with the method and the constants of tests/test_gpu_flownet_grid.py: error against float64 <= min(4 x the deviation of the same
formula in fp32 torch, measured here, 1e-4), max-norm relative to max |ref|, gradients with the kernel's own gates forced (`saved > 0`),
backward calls made twice and bitwise equal.  The reference is `encode_piecewise` of tests/flownet_piecewise_refs.py under the
restatements of tests/flownet_refs.py / flownet_points_refs.py / flownet_spatial_refs.py, which tests/test_flownet_piecewise_golden.py ties
to the reference's own model.py / progressive_controller.py through the fixture.

Grids: the fixture's (t = 2, 20 x 28: 1120 points, a partial 18th tile) and a ragged one (times 0, 0.25, 1.0; 37 x 53: 5883 points, tiles
straddling frames).  Nothing runs at production size.

  1. the encoding probe of tests/test_gpu_flownet_grid.py on the 515-wide layer 1: one-hot +-1 columns 3 + k, zero bias, relu(e) - relu(-e)
     of `saved[0]` is every feature as the kernel made it; absolute max-norm against 4 units.  Both branches of tri, several periods and
     max |u| > 40 are asserted.
  2. forward and every parameter gradient under the masks ones / mid / ramp, and against the fixture.
  3. k_active through every skip boundary: exact zeros from the closed features, the bits of the unskipped call.
  4. a pose list that spells out the fixture grid gives the grid call's bits; 4096 random points of [-1, 1]^3 against float64.
  5. out of domain, 4096 points of [-1.5, 1.5]^3: where u < 0 the reference's fmod truncates and its values jump at negative integers of
     u.  A point is left out if the float64 u of any of its frequencies lies within delta = 8 x 2^-24 x max |u| of an integer <= -1.  From the
     float64 reference alone: at most 5 % of the points are left out, and u < 0 in more than 1 % of the remaining (point, frequency) pairs.
  6. StashedSpatialController(net, res=7) with a grid that is neither ones nor a prefix, on the fixture grid and at 4096 points; the list
     that spells out the grid is bitwise the grid call.
  7. the pose gradient on the ragged grid spelt out as a pose list, under the ramp mask.  The derivative is piecewise constant and jumps by
     4 |F[d][f]| at every integer of u, so per point and coordinate the bound is the plain budget (4 units of max |ref|) plus
     sum over the frequencies whose float64 u is within delta of an integer of 4 |G_k| |F[d][f]|, G = (dh1 W1)_k mask_k in float64.  From
     the reference alone: at most 5 % of the points have a non-zero allowance; the unit is measured on the others, and they are held to the
     plain budget.
  8. end to end: tools/fit_flow.py --net MPFF, fused against composed; one FlowTrainer step, checkpoint and reload.

Measured on an MI355X (`ratio(...)` lines of a run with -s: error / budget [error, fp32-torch unit]; the table is in DESIGN 14.10):
  ratio(MPFF fixture encoding) = 0.25   [abs err 8.42e-06, fp32-torch unit 8.42e-06, budget 3.37e-05, max u 42.8]
  ratio(MPFF ragged encoding) = 0.25   [abs err 8.56e-06, fp32-torch unit 8.56e-06, budget 3.42e-05, max u 46.3]: the kernel is as far from
            float64 as torch's fp32 evaluation is, both inherit the rounding of u where its ulp is 3.8e-6 and the slope is 2
  ratio(MPFF fixture ones flows) = 0.238   [err 2.42e-06, fp32-torch unit 2.55e-06]  vs fixture 0.25  gW1 0.244  gb1 0.209  gW2 0.227  gb2 0.375
            gW3 0.222  gb3 0.424  gW4 0.236  gb4 0.12  gW1[:, :3] 0.0842
  ratio(MPFF fixture mid flows) = 0.276   [err 4.14e-07, fp32-torch unit 3.76e-07]  vs fixture 0.246  worst gradient gb3 0.519 [2.41e-07, 1.16e-07]
  ratio(MPFF fixture ramp flows) = 0.229   [err 4.04e-07, fp32-torch unit 4.4e-07]  vs fixture 0.229  worst gradient gb3 0.405
  ratio(MPFF ragged ones flows) = 0.242   [err 2.64e-06, fp32-torch unit 2.73e-06]  worst gradient gb1 0.471 [5.74e-07, 3.05e-07]
  ratio(MPFF ragged ramp flows) = 0.231   [err 3.49e-07, fp32-torch unit 3.77e-07]  worst gradient gb1 0.364
  ratio(MPFF points ones flows) = 0.237   [err 2.05e-06, fp32-torch unit 2.16e-06]  worst gradient gb1 0.265
  ratio(MPFF points ramp flows) = 0.273   [err 3.47e-07, fp32-torch unit 3.18e-07]  worst gradient gb1 0.411
  MPFF out of domain: delta 2.68e-05, 2 of 4096 points left out (0.049%), u < 0 in 4.132% of the remaining pairs, min u -9.35
  ratio(MPFF out of domain flows) = 0.24   [err 1.83e-06, fp32-torch unit 1.9e-06, budget 7.6e-06]
  ratio(MPFF spatial fixture flows) = 0.275   [err 4.66e-07, fp32-torch unit 4.24e-07]  worst gradient gb2 0.241
  ratio(MPFF spatial points flows) = 0.253   [err 4.26e-07, fp32-torch unit 4.21e-07]  worst gradient gb1, gb2 0.268; controller(poses) the same
  MPFF g_poses: delta 2.21e-05; 4.98e-05 of the (point, frequency) pairs near a kink; 9 of 5883 points (0.153%) have a non-zero allowance,
            largest 0.119 against max |ref| 0.824
  ratio(MPFF g_poses, points without allowance) = 0.243   [err 3.15e-07, fp32-torch unit 3.25e-07, budget 1.3e-06]
  ratio(MPFF g_poses, error beyond the allowance, every point) = 0.243   columns t 0.254  y 0.183  x 0.287
  End to end: the first five losses of the fused and the composed loop agree to the 7 digits printed (0.1307229 .. 0.1232553), the final ones
  are 0.0482327 / 0.0482307.  25 tests, 6 s.
Speed (tools/bench_flownet.py, 446 464 points): MPFF 2.079 ms forward / 6.389 ms step against PFF's 2.409 / 6.751 and the composed
network's 7.331 / 15.375 (3.53 x / 2.41 x); --k-active 128: 1.274 / 5.120 (5.73 x / 2.99 x); --points 446464 --pose-grad: step 7.529 against
6.369 without and 19.616 composed (2.61 x).
"""
import argparse
import os
import sys

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import flownet_piecewise_refs as P  # noqa: E402
from flownet_piecewise_refs import GH, GW, N_MID, N_RAMP, NAME, SCALE, TIMES, build, controller, encode_piecewise, piecewise_arg  # noqa: E402
from flownet_points_refs import grid_poses, reference_grads_points, restate_points  # noqa: E402
from flownet_refs import nan_saved, nan_workspace, net_tensors, poses_of, reference_grads, restate  # noqa: E402
from flownet_spatial_refs import interp_mask  # noqa: E402
from flownet_spatial_refs import restate_points as restate_spatial_points  # noqa: E402
from test_gpu_flownet import CEIL, F64, MULT, axes, check  # noqa: E402

F32 = torch.float32
NAN = float('nan')
GRIDS = {'fixture': (TIMES, GH, GW), 'ragged': ((0.0, 0.25, 1.0), 37, 53)}
GNAMES = [f'g{k}{l}' for l in (1, 2, 3, 4) for k in ('W', 'b')]
K_ACTIVE = (0, 3, 4, 19, 20, 131, 132, 259, 260, 515)     # the coordinates alone, the 16-feature K step, the 128-column tile
N_POINTS = 4096
SEED_IN, SEED_OUT = 21, 22                                 # the pose lists of 4 / 6 and of 5


@pytest.fixture(scope='module')
def dev():
    import sin_inn_amd  # noqa: F401
    assert torch.cuda.is_available(), 'GPU tests need a GPU'
    return torch.device('cuda', 0)


@pytest.fixture(scope='module')
def gold():
    return P.gold()


@pytest.fixture(scope='module')
def case(dev):
    """the network of the fixture's seed on the device, its tensors, and the three host masks with their k_active"""
    from sin_inn_amd import flownet
    net = build().to(dev)
    bufs, weights = net_tensors(net, dev)
    masks = {'ones': torch.ones(515)}
    ctl = controller(net)
    for i in range(N_MID):
        ctl.stash_iteration(torch.tensor(0.5))
        if i + 1 == N_RAMP:
            masks['ramp'] = ctl.mask.clone()
    masks['mid'] = ctl.mask.clone()
    return argparse.Namespace(net=net, bufs=bufs, weights=weights, masks=masks, ka={k: flownet.last_open(m) for k, m in masks.items()})


def random_poses(seed, half, dev):
    return ((torch.rand(N_POINTS, 3, generator=torch.Generator().manual_seed(seed)) * 2 - 1) * half).to(dev)


def upstream(n, dev):
    return torch.randn(4, n, generator=torch.Generator().manual_seed(11)).to(dev)


# ---- 1 ----
@pytest.mark.parametrize('grid', list(GRIDS))
def test_encoding_probe(dev, case, grid):
    from sin_inn_amd import flownet
    net = build().to(dev)
    times, ys, xs = axes(GRIDS[grid], dev)
    n = times.numel() * ys.numel() * xs.numel()
    lin = net.linears()[0]
    ones = torch.ones(515, device=dev)
    got = torch.empty(n, 512, device=dev)
    with torch.no_grad():
        lin.bias.zero_()
        for half in (0, 1):
            parts = []
            for sign in (1.0, -1.0):
                lin.weight.zero_()
                rows = torch.arange(256, device=dev)
                lin.weight[rows, 3 + 256 * half + rows] = sign
                _, saved = flownet.flownet_forward(net, times, ys, xs, SCALE, True, nan_saved(n, dev), mask=ones, k_active=515)
                parts.append(saved[0, :n].clone())
            assert bool(((parts[0] == 0) | (parts[1] == 0)).all())
            got[:, 256 * half:256 * half + 256] = parts[0] - parts[1]
    assert bool(torch.isfinite(got).all()) and float(got.abs().max()) <= 1.0
    enc64 = encode_piecewise(case.bufs, poses_of(times, ys, xs, F64))
    enc32 = encode_piecewise(case.bufs, poses_of(times, ys, xs, F32))
    unit = float((enc32.to(F64) - enc64).abs().max())
    err = float((got.to(F64) - enc64).abs().max())
    budget = MULT * unit
    u = piecewise_arg(case.bufs, poses_of(times, ys, xs, F64))
    print(f'ratio({NAME} {grid} encoding) = {err / budget:.3g}   [abs err {err:.3g}, fp32-torch unit {unit:.3g}, budget {budget:.3g}, '
          f'max u {float(u.max()):.3g}]')
    # both branches of tri, for both features of a frequency; several periods; arguments where an fp32 ulp of u is 4e-6
    for w in (u, u + 1):
        r = torch.fmod(w, 2) - 1
        assert 0.25 < float((r < 0).double().mean()) < 0.75
    assert float(u.min()) >= 0 and torch.floor(u / 2).unique().numel() > 10 and float(u.abs().max()) > 40
    assert float(enc64.min()) < -0.99 and float(enc64.max()) > 0.99
    assert err <= budget, (err, budget)


# ---- 2 ----
@pytest.mark.parametrize('grid,kind', [('fixture', 'ones'), ('fixture', 'mid'), ('fixture', 'ramp'), ('ragged', 'ones'), ('ragged', 'ramp')])
def test_forward_and_backward_against_float64(dev, gold, case, grid, kind):
    from sin_inn_amd import flownet
    net, bufs, weights = case.net, case.bufs, case.weights
    times, ys, xs = axes(GRIDS[grid], dev)
    n = times.numel() * ys.numel() * xs.numel()
    hmask, ka = case.masks[kind], case.ka[kind]
    if kind != 'ones':
        assert np.array_equal(hmask.numpy(), gold[f'mask_{kind}'])
    assert ka == {'ones': 515, 'mid': 84, 'ramp': 84}[kind]
    mask = hmask.to(dev)
    tag = f'{NAME} {grid} {kind}'

    infer, none = flownet.flownet_forward(net, times, ys, xs, SCALE, False, mask=mask, k_active=ka)
    assert none is None
    train, saved = flownet.flownet_forward(net, times, ys, xs, SCALE, True, nan_saved(n, dev), mask=mask, k_active=ka)
    assert torch.equal(infer, train)
    assert bool(torch.isfinite(saved).all()) and float(saved.min()) >= 0.0
    with torch.no_grad():
        ref64 = restate(NAME, bufs, weights, times, ys, xs, SCALE, F64, mask)
        ref32 = restate(NAME, bufs, weights, times, ys, xs, SCALE, F32, mask)
    check(f'{tag} flows', infer, ref64, ref32)
    if grid == 'fixture':
        g32 = torch.from_numpy(gold[f'{NAME}_out32_{kind}']).to(dev) if kind != 'ramp' else ref32
        check(f'{tag} flows vs fixture', infer, torch.from_numpy(gold[f'{NAME}_out64_{kind}']).to(dev), g32)

    gates = [saved[l, :n] > 0 for l in range(3)]
    up = torch.randn(infer.shape, generator=torch.Generator().manual_seed(11)).to(dev)
    grads_ref = reference_grads(NAME, bufs, weights, times, ys, xs, SCALE, up, mask, gates)
    ws = nan_workspace(n, dev)
    got = flownet.flownet_backward(net, times, ys, xs, SCALE, up, saved, ws, mask=mask, k_active=ka)
    again = flownet.flownet_backward(net, times, ys, xs, SCALE, up, saved, ws, mask=mask, k_active=ka)
    assert tuple(got[0].shape) == (256, 515)
    closed = mask == 0
    assert bool((got[0][:, closed] == 0.0).all()) and not bool(torch.signbit(got[0][:, closed]).any())
    assert bool((got[0][:, :3] != 0.0).any(dim=0).all()), 'a coordinate column of gW1 is all zero'
    for nm, a, b in zip(GNAMES, got, again):
        assert bool(torch.isfinite(a).all()), nm
        assert torch.equal(a, b), f'{nm}: two backward calls differ'
    for nm, g, r64, r32 in zip(GNAMES, got, grads_ref[F64], grads_ref[F32]):
        check(f'{tag} {nm}', g, r64, r32)
    check(f'{tag} gW1 coordinate columns', got[0][:, :3], grads_ref[F64][0][:, :3], grads_ref[F32][0][:, :3])
    if grid != 'fixture':
        return

    # the public surface: the controller's own mask (k_active = 84, skipped) or the same mask given as a device tensor (not inspected on
    # the host: all 515 features); get_mask returns the mask in use
    params = [p for lin in net.linears() for p in (lin.weight, lin.bias)]
    target = net
    if kind != 'ones':
        target = controller(net)
        for i in range(N_MID if kind == 'mid' else N_RAMP):
            target.stash_iteration(torch.tensor(0.5))
        assert torch.equal(target.mask, hmask) and target.device_mask(dev)[1] == ka

    def run(**kw):
        for p in params:
            p.grad = None
        f12, f21 = flownet.flow_fields(target, times, GH, GW, SCALE, **kw)
        (f12 * up[:, :2]).sum().add((f21 * up[:, 2:]).sum()).backward()
        return torch.cat((f12, f21), 1).detach(), [p.grad.clone() for p in params]

    own_f, own_g = run()
    over_f, over_g = run(override_mask=mask)
    assert torch.equal(own_f, over_f) and torch.equal(own_f, infer)
    for nm, a, b, c in zip(GNAMES, own_g, over_g, got):
        assert torch.equal(a, b), f'{nm}: k_active and the override mask differ'
        assert torch.equal(a, c), f'{nm}: flow_fields and flownet_backward differ'
    with torch.no_grad():
        i12, i21, used = flownet.flow_fields(target, times, GH, GW, SCALE, get_mask=True)
    assert not i12.requires_grad and torch.equal(torch.cat((i12, i21), 1), infer) and torch.equal(used, mask)
    for p in params:
        p.grad = None


# ---- 3 ----
@pytest.mark.parametrize('ka', K_ACTIVE)
def test_k_active_boundaries(dev, case, ka):
    from sin_inn_amd import flownet
    net = case.net
    times, ys, xs = axes(GRIDS['fixture'], dev)
    n = times.numel() * ys.numel() * xs.numel()
    up = torch.randn(len(TIMES), 4, GH, GW, generator=torch.Generator().manual_seed(11)).to(dev)
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
    assert bool((got[0][:, ka:] == 0.0).all()) and not bool(torch.signbit(got[0][:, ka:]).any())
    if ka:
        assert bool((got[0][:, :ka] != 0.0).any(dim=0).all())
    # the closed features contribute exact zeros to the flows: NaN in their columns of W1 changes nothing
    if 3 <= ka < 515:
        lin = net.linears()[0]
        keep = lin.weight.detach().clone()
        try:
            with torch.no_grad():
                lin.weight[:, ka:] = NAN
            poisoned, _ = flownet.flownet_forward(net, times, ys, xs, SCALE, False, mask=mask, k_active=ka)
        finally:
            with torch.no_grad():
                lin.weight.copy_(keep)
        assert torch.equal(poisoned, flows)


# ---- 4 ----
def test_a_grid_spelled_out_as_poses_gives_the_grid_call_bitwise(dev, case):
    from sin_inn_amd import flownet
    net = case.net
    times, ys, xs = axes(GRIDS['fixture'], dev)
    n = times.numel() * ys.numel() * xs.numel()
    poses = grid_poses(times, ys, xs)
    mask, ka = case.masks['ramp'].to(dev), case.ka['ramp']
    up = torch.randn(len(TIMES), 4, GH, GW, generator=torch.Generator().manual_seed(11)).to(dev)
    flows_g, saved_g = flownet.flownet_forward(net, times, ys, xs, SCALE, True, nan_saved(n, dev), mask=mask, k_active=ka)
    want = flownet.flownet_backward(net, times, ys, xs, SCALE, up, saved_g, nan_workspace(n, dev), mask=mask, k_active=ka)
    flows_p, saved_p = flownet.flownet_forward_points(net, poses, SCALE, True, nan_saved(n, dev), mask=mask, k_active=ka)
    assert flows_p.shape == (4, n) and torch.equal(flows_p.view(4, len(TIMES), GH, GW).permute(1, 0, 2, 3), flows_g)
    assert torch.equal(saved_p, saved_g)
    up_p = up.permute(1, 0, 2, 3).reshape(4, n).contiguous()
    got = flownet.flownet_backward_points(net, poses, SCALE, up_p, saved_p, nan_workspace(n, dev), mask=mask, k_active=ka)
    gp = torch.full((n, 3), NAN, device=dev)
    with_pg, gp_out = flownet.flownet_backward_points(net, poses, SCALE, up_p, saved_p, nan_workspace(n, dev), mask=mask, k_active=ka,
                                                      pose_grad=True, g_poses=gp)
    assert gp_out is gp and bool(torch.isfinite(gp).all()) and bool((gp != 0).any(dim=0).all())
    for nm, a, b, c in zip(GNAMES, got, want, with_pg):
        assert bool(torch.isfinite(a).all()) and torch.equal(a, b), f'{nm}: points and grid differ'
        assert torch.equal(a, c), f'{nm}: the posegrad call and the call without it differ'
    ctl = controller(net)
    ctl.mask = case.masks['ramp'].clone()
    with torch.no_grad():
        out = ctl(poses)                                          # net(poses): (N, 4), scale 1
        bare = net(poses, override_mask=mask)
    one, _ = flownet.flownet_forward_points(net, poses, 1.0, False, mask=mask, k_active=ka)
    assert out.shape == (n, 4) and torch.equal(out.t(), one) and torch.equal(bare, out)


@pytest.mark.parametrize('kind', ['ones', 'ramp'])
def test_random_points_against_float64(dev, case, kind):
    from sin_inn_amd import flownet
    net, bufs, weights = case.net, case.bufs, case.weights
    poses, up = random_poses(SEED_IN, 1.0, dev), upstream(N_POINTS, dev)
    n = N_POINTS
    mask, ka = case.masks[kind].to(dev), case.ka[kind]
    tag = f'{NAME} points {kind}'
    infer, none = flownet.flownet_forward_points(net, poses, SCALE, False, mask=mask, k_active=ka)
    flows, saved = flownet.flownet_forward_points(net, poses, SCALE, True, nan_saved(n, dev), mask=mask, k_active=ka)
    assert none is None and torch.equal(infer, flows)
    gates = [saved[l, :n] > 0 for l in range(3)]
    with torch.no_grad():
        f64, f32 = (restate_points(NAME, bufs, weights, poses, SCALE, dt, mask) for dt in (F64, F32))
    check(f'{tag} flows', flows, f64, f32)
    ref = reference_grads_points(NAME, bufs, weights, poses, SCALE, up, mask, gates)
    ws = nan_workspace(n, dev)
    got = flownet.flownet_backward_points(net, poses, SCALE, up, saved, ws, mask=mask, k_active=ka)
    again = flownet.flownet_backward_points(net, poses, SCALE, up, saved, ws, mask=mask, k_active=ka)
    for nm, g, a, r64, r32 in zip(GNAMES, got, again, ref[F64][1], ref[F32][1]):
        assert torch.equal(g, a), f'{nm}: two backward calls differ'
        check(f'{tag} {nm}', g, r64, r32)


# ---- 5 ----
def test_out_of_domain_against_float64(dev, case):
    from sin_inn_amd import flownet
    net, bufs, weights = case.net, case.bufs, case.weights
    poses = random_poses(SEED_OUT, 1.5, dev)
    mask = case.masks['ones'].to(dev)
    u = piecewise_arg(bufs, poses.to(F64))
    delta = P.kink_delta(u)
    out = P.near_integer(u, delta, negative_only=True).any(1)
    left_out = float(out.double().mean())
    negative = float((u[~out] < 0).double().mean())
    print(f'{NAME} out of domain: delta {delta:.3g}, {int(out.sum())} of {N_POINTS} points left out ({left_out:.3%}), u < 0 in {negative:.3%} of '
          f'the remaining pairs, min u {float(u.min()):.3g}')
    assert left_out <= 0.05 and negative > 0.01
    enc64 = encode_piecewise(bufs, poses.to(F64))
    assert float(enc64.min()) < -4.0                             # the reference's own values below -1, down to almost -5
    flows, _ = flownet.flownet_forward_points(net, poses, SCALE, False, mask=mask, k_active=515)
    assert bool(torch.isfinite(flows).all())
    with torch.no_grad():
        f64, f32 = (restate_points(NAME, bufs, weights, poses, SCALE, dt, mask) for dt in (F64, F32))
    keep = ~out
    check(f'{NAME} out of domain flows', flows[:, keep], f64[:, keep], f32[:, keep])


# ---- 6 ----
RES = 7


def spatial_controller(net, dev):
    """a StashedSpatialController whose cells differ: random levels in the first 200 columns, zero beyond (k_active = 200)"""
    from sin_inn_amd import progressive
    ctl = progressive.StashedSpatialController(net, RES)
    g = torch.rand(RES ** 3, 515, generator=torch.Generator().manual_seed(6))
    g[:, 200:] = 0
    ctl.mask.copy_(g.to(dev))
    ctl.mask_ = None
    ctl.cur_block = ctl.next_block = 200
    assert ctl.device_grid(dev).k_active == 200 and ctl.device_grid(dev).res == RES
    return ctl


def test_spatial_controller_on_the_grid_and_at_points(dev, case):
    from sin_inn_amd import flownet
    net, bufs, weights = case.net, case.bufs, case.weights
    ctl = spatial_controller(net, dev)
    grid, cs = ctl.get_mask(), ctl.centre_scale_host()
    params = [p for lin in net.linears() for p in (lin.weight, lin.bias)]

    def float64_parity(tag, poses, flows, saved, sampled):
        n = poses.shape[0]
        m64 = interp_mask(grid, RES, poses, F64, cs)
        assert float((sampled.double() - m64).abs().max()) <= 4e-6 and float(m64[:, :200].std()) > 0.01 and bool((m64[:, 200:] == 0).all())
        gates = [saved[l, :n] > 0 for l in range(3)]
        with torch.no_grad():
            f64, f32 = (restate_spatial_points(NAME, bufs, weights, poses, dt, m64.to(dt)).t() * SCALE for dt in (F64, F32))
        check(f'{tag} flows', flows, f64, f32)                   # free gates: ReLU is continuous
        up = upstream(n, dev)
        ref = {}
        for dt in (F64, F32):
            w = [p.to(dt).requires_grad_(True) for p in weights]
            out = restate_spatial_points(NAME, bufs, w, poses, dt, m64.to(dt), gates).t() * SCALE
            ref[dt] = torch.autograd.grad((out * up.to(dt)).sum(), w)
        return up, ref

    # the fixture grid through the raw calls, and the pose list that spells it out
    times, ys, xs = axes(GRIDS['fixture'], dev)
    n = times.numel() * ys.numel() * xs.numel()
    poses = grid_poses(times, ys, xs)
    flows_g, saved_g = flownet.flownet_forward_spatial(net, times, ys, xs, SCALE, True, grid, RES, cs, 200, nan_saved(n, dev))
    sampled = flownet.flownet_sample_mask(net, times, ys, xs, grid, RES, cs)
    planar = flows_g.permute(1, 0, 2, 3).reshape(4, n)
    up, ref = float64_parity(f'{NAME} spatial fixture', poses, planar, saved_g, sampled)
    up_g = up.view(4, len(TIMES), GH, GW).permute(1, 0, 2, 3).contiguous()
    ws = nan_workspace(n, dev)
    got = flownet.flownet_backward_spatial(net, times, ys, xs, SCALE, up_g, saved_g, grid, RES, cs, 200, ws)
    again = flownet.flownet_backward_spatial(net, times, ys, xs, SCALE, up_g, saved_g, grid, RES, cs, 200, ws)
    for nm, g, a, r64, r32 in zip(GNAMES, got, again, ref[F64], ref[F32]):
        assert torch.equal(g, a), f'{nm}: two backward calls differ'
        check(f'{NAME} spatial fixture {nm}', g, r64, r32)
    assert bool((got[0][:, 200:] == 0).all())
    flows_p, saved_p = flownet.flownet_forward_spatial_points(net, poses, SCALE, True, grid, RES, cs, 200, nan_saved(n, dev))
    assert torch.equal(flows_p, planar) and torch.equal(saved_p, saved_g)
    got_p = flownet.flownet_backward_spatial_points(net, poses, SCALE, up, saved_p, grid, RES, cs, 200, nan_workspace(n, dev))
    for nm, a, b in zip(GNAMES, got_p, got):
        assert torch.equal(a, b), f'{nm}: points and grid differ'
    assert torch.equal(flownet.flownet_sample_mask_points(net, poses, grid, RES, cs), sampled)
    # the public surface on the grid: flow_fields(controller) is that call
    for p in params:
        p.grad = None
    f12, f21, used = flownet.flow_fields(ctl, times, GH, GW, SCALE, get_mask=True)
    assert torch.equal(torch.cat((f12, f21), 1).detach(), flows_g) and torch.equal(used, sampled)
    torch.autograd.backward([f12, f21], [up_g[:, :2], up_g[:, 2:]])
    for nm, p, g in zip(GNAMES, params, got):
        assert torch.equal(p.grad, g), nm

    # 4096 random points through controller(poses)
    poses = random_poses(SEED_IN, 1.0, dev)
    n = N_POINTS
    flows, saved = flownet.flownet_forward_spatial_points(net, poses, SCALE, True, grid, RES, cs, 200, nan_saved(n, dev))
    sampled = flownet.flownet_sample_mask_points(net, poses, grid, RES, cs)
    up, ref = float64_parity(f'{NAME} spatial points', poses, flows, saved, sampled)
    ws = nan_workspace(n, dev)
    got = flownet.flownet_backward_spatial_points(net, poses, SCALE, up, saved, grid, RES, cs, 200, ws)
    again = flownet.flownet_backward_spatial_points(net, poses, SCALE, up, saved, grid, RES, cs, 200, ws)
    for nm, g, a, r64, r32 in zip(GNAMES, got, again, ref[F64], ref[F32]):
        assert torch.equal(g, a), f'{nm}: two backward calls differ'
        check(f'{NAME} spatial points {nm}', g, r64, r32)
    for p in params:
        p.grad = None
    out, used = ctl(poses, get_mask=True)
    assert out.shape == (n, 4) and torch.equal(used, sampled)
    out.backward(up.t().contiguous() * SCALE)                     # controller(poses) has scale 1: the upstream carries it
    one, _ = flownet.flownet_forward_spatial_points(net, poses, 1.0, False, grid, RES, cs, 200)
    assert torch.equal(out.detach().t(), one)
    for nm, p, r64, r32 in zip(GNAMES, params, ref[F64], ref[F32]):
        check(f'{NAME} controller(poses) {nm}', p.grad, r64, r32)
        p.grad = None


# ---- 7 ----
def test_pose_gradient_with_the_kink_allowance(dev, case):
    from sin_inn_amd import flownet
    net, bufs, weights = case.net, case.bufs, case.weights
    times, ys, xs = axes(GRIDS['ragged'], dev)
    poses = grid_poses(times, ys, xs)
    n = poses.shape[0]
    hmask, ka = case.masks['ramp'], case.ka['ramp']
    mask = hmask.to(dev)
    ctl = controller(net)
    ctl.mask = hmask.clone()
    up = torch.randn(n, 4, generator=torch.Generator().manual_seed(11)).to(dev)
    params = [p for lin in net.linears() for p in (lin.weight, lin.bias)]

    # the raw call twice, every buffer NaN before it, then the same through flow_at(controller, p, pose_grad=True)
    _, saved = flownet.flownet_forward_points(net, poses, SCALE, True, nan_saved(n, dev), mask=mask, k_active=ka)
    raw = []
    for _ in range(2):
        gp = torch.full((n, 3), NAN, device=dev)
        flownet.flownet_backward_points(net, poses, SCALE, up.t().contiguous(), saved, nan_workspace(n, dev), mask=mask, k_active=ka,
                                        pose_grad=True, g_poses=gp)
        raw.append(gp)
    assert bool(torch.isfinite(raw[0]).all()) and torch.equal(raw[0], raw[1])
    for q in params:
        q.grad = None
    p = poses.clone().requires_grad_(True)
    flownet.flow_at(ctl, p, SCALE, pose_grad=True).backward(up)
    got = p.grad
    assert torch.equal(got, raw[0])
    for q in params:
        q.grad = None

    gates = [saved[l, :n] > 0 for l in range(3)]
    ref = {}
    for dt in (F64, F32):
        x = poses.to(dt).requires_grad_(True)
        flows = restate_points(NAME, bufs, weights, x, SCALE, dt, mask, gates)
        ref[dt] = torch.autograd.grad((flows * up.t().to(dt)).sum(), x)[0]
    u = piecewise_arg(bufs, poses.to(F64))
    delta = P.kink_delta(u)
    near = P.near_integer(u, delta)
    G = P.layer1_gradient(bufs, weights, poses, SCALE, up.t(), mask, gates)
    allow = P.kink_allowance(bufs, G, near)                       # (N, 3), float64, from the reference alone
    touched = (allow > 0).any(1)
    share, pairs = float(touched.double().mean()), float(near.double().mean())
    print(f'{NAME} g_poses: delta {delta:.3g}; {pairs:.3g} of the (point, frequency) pairs near a kink; {int(touched.sum())} of {n} points '
          f'({share:.3%}) have a non-zero allowance, largest {float(allow.max()):.3g} against max |ref| {float(ref[F64].abs().max()):.3g}')
    assert share <= 0.05
    plain = ~touched
    scale = float(ref[F64].abs().max())
    unit = float((ref[F32][plain].to(F64) - ref[F64][plain]).abs().max()) / scale
    budget = min(MULT * unit, CEIL)
    err = (got.to(F64) - ref[F64]).abs()
    worst = float(err[plain].max()) / scale
    print(f'ratio({NAME} g_poses, points without allowance) = {worst / budget:.3g}   [err {worst:.3g}, fp32-torch unit {unit:.3g}, budget {budget:.3g}]')
    over = float((err - allow).max()) / scale
    print(f'ratio({NAME} g_poses, error beyond the allowance, every point) = {over / budget:.3g}')
    assert worst <= budget, (worst, budget)
    assert bool((err <= budget * scale + allow).all()), (over, budget)
    for d, axis in enumerate('tyx'):                              # each column against its own max |ref| and unit, as the other posegrad tests
        sc = float(ref[F64][:, d].abs().max())
        un = float((ref[F32][plain, d].to(F64) - ref[F64][plain, d]).abs().max()) / sc
        bd = min(MULT * un, CEIL)
        e = float(err[plain, d].max()) / sc
        print(f'ratio({NAME} g_poses column {axis}) = {e / bd:.3g}   [err {e:.3g}, fp32-torch unit {un:.3g}, budget {bd:.3g}]')
        assert e <= bd, (axis, e, bd)
        assert bool((err[:, d] <= bd * sc + allow[:, d]).all()), axis


# ---- 8 ----
def test_fit_flow_end_to_end(dev):
    """tools/fit_flow.py --net MPFF at its smallest size (64 x 96) with the fused network and with the network composed from torch ops
    (same seed, same optimiser): per-step loss within CEIL relative for the first 5 steps, as the RBFG test asks; the loss falls in both.
    Wiring, not accuracy."""
    sys.path.insert(0, os.path.join(ROOT, 'tools'))
    import fit_flow
    fused = fit_flow.fit(NAME, 64, 96, 30, composed=False)
    comp = fit_flow.fit(NAME, 64, 96, 30, composed=True)
    for s in range(5):
        print(f'step {s}: fused {fused[s]:.7f} composed {comp[s]:.7f} rel {abs(fused[s] - comp[s]) / abs(comp[s]):.3g}')
    print(f'final: fused {fused[-1]:.7f} composed {comp[-1]:.7f}')
    for s in range(5):
        assert abs(fused[s] - comp[s]) <= CEIL * abs(comp[s]), (s, fused[s], comp[s])
    assert fused[-1] < fused[0] and comp[-1] < comp[0]


def test_flow_trainer_trains_checkpoints_and_reloads(dev, tmp_path):
    from sin_inn_amd import flowdata, flownet, flowtrainer, progressive

    def args_of(net):
        return argparse.Namespace(lr=1e-4, loss_l1=1, loss_census=0.1, loss_ssim=0.05, census_width=3, loss_smooth1=0.1, edge_constant=150,
                                  edge_func='gauss', occl='wang', occl_thresh=0.7, net=net)

    torch.manual_seed(0)
    net = progressive.LinearControllerEarly(flownet.MPFFModel(flownet.ModelParams()), 1000, epsilon=1e-3).to(dev)
    model = flowtrainer.FlowTrainer(args_of(net)).to(dev)
    opt = model.attach_optimizer()
    clip = flowdata.SyntheticClip(3, 24, 40, seed=0)
    batch = [clip.video[0:2].to(dev), clip.video[1:3].to(dev), clip.T[0:2].to(dev), torch.tensor([clip.flow_scale] * 2, dtype=F64).to(dev),
             clip.flow[0:2].to(dev)]
    params = list(model.net.parameters())
    assert len(params) == 8
    before = [p.detach().clone() for p in params]
    opt.zero_grad()
    loss = model.training_step(batch, 0)
    assert bool(torch.isfinite(loss)) and float(loss) > 0
    loss.backward()
    for p in params:
        assert p.grad is not None and bool(torch.isfinite(p.grad).all()) and float(p.grad.abs().max()) > 0
    opt.step()
    for p, b in zip(params, before):
        assert bool(torch.isfinite(p).all()) and not torch.equal(p.detach(), b)
    assert net.iteration == 1
    model.trainer.global_step = 1
    path = os.path.join(str(tmp_path), 'mpff.ckpt')
    model.trainer.save_checkpoint(model, path)
    ck = torch.load(path, map_location='cpu')
    assert 'net.model.encode.frequencies' in ck['state_dict'] and 'net.mask_stashed' in ck['state_dict']
    torch.manual_seed(1)
    fresh = progressive.LinearControllerEarly(flownet.MPFFModel(flownet.ModelParams()), 1000, epsilon=1e-3)
    again = flowtrainer.FlowTrainer.load_from_checkpoint(path, args=args_of(fresh)).to(dev)
    for (ka, va), (kb, vb) in zip(model.state_dict().items(), again.state_dict().items()):
        assert ka == kb and torch.equal(va.cpu(), vb.cpu()), ka
    # the mask comes back as a checkpoint keeps it, floor(sum) ones and the fraction (6 ones and a block at 0.25 -> 7 ones, 0.5): the
    # reloaded trainer is the trained network under that mask, to the bit
    assert again.net.iteration == 1 and float(ck['state_dict']['net.mask_stashed'][0]) == 7.5
    assert torch.equal(again.net.mask[:9], torch.tensor([1.0] * 7 + [0.5, 0.0]))
    with torch.no_grad():
        h, w = batch[0].shape[-2:]
        a = flownet.flow_fields(model.net, batch[2].to(F32), h, w, model._scale(batch[3], batch[0]), override_mask=again.net.mask)
        b = again(batch[0], batch[2], batch[3])
    assert bool(torch.isfinite(b[0]).all()) and torch.equal(a[0], b[0]) and torch.equal(a[1], b[1])
