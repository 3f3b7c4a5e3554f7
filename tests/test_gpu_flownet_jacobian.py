"""GPU: the flow Jacobian of the fused kernels (flow_at(.., jacobian=); csrc/flownet_jacobian.h; sininn_flownet_jacobian_forward / _backward).

  1. the fused call against the float64 reference of tests/flownet_jacobian_refs.py (the kernel's own gates forced, saved > 0) under its
     budget rule -- jac as a whole, per direction, per channel pair, per parameter gradient -- and the composed form under the same rule:
     RBF, FFN, UFF plain, PRBF, PFF, PUFF with k_active in {0, 3, 16, 19, 515}; directions 'yx', 't', 'tyx'; N in {1, 63, 64, 65, 129} and
     2048 * 64 + 65 (past one sweep of the forward grid; forward and one backward).
  2. exact: the flows are bitwise the plain call's; djac = 0 gives the plain backward's gradients; two calls agree; a small grid spelled out
     as a pose list gives the same bits whatever its order within a tile; k_active past the last open feature gives equal bits; rows with
     NaN / inf poses leave every other row's bits unchanged.
  3. the autograd surface: shapes, a None upstream for either output, net(poses, jacobian=), controller(poses, jacobian=).
  4. one trainer step, fused against composed, by the measured-unit method of DESIGN 22.5: the composed step in float64 is the reference,
     the composed step in fp32 the unit.
Ratios (error / budget) are printed with -s; the table is in DESIGN 24.
"""
import os
import sys

import pytest
import torch

pytestmark = pytest.mark.gpu
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import flownet_jacobian_refs as J  # noqa: E402
from flownet_refs import net_tensors  # noqa: E402

F32, F64 = torch.float32, torch.float64
SCALE = 3.0
NAN = float('nan')
BIG = 2048 * 64 + 65
_nets = {}


@pytest.fixture(scope='module')
def dev():
    import sin_inn_amd  # noqa: F401
    assert torch.cuda.is_available(), 'GPU tests need a GPU'
    return torch.device('cuda', 0)


def net_of(name, dev):
    from sin_inn_amd import flownet
    if name not in _nets:
        torch.manual_seed(40 + len(_nets))
        _nets[name] = flownet.all_model_dict[name](flownet.ModelParams()).to(dev)
    return _nets[name]


def mask_of(net, k_active, dev):
    """(device mask, host-known k_active) of a progressive network: ones up to k_active, a block in progress at its end"""
    if not net.is_progressive:
        return None, None
    m = torch.zeros(net.encoding_dim)
    m[:k_active] = 1.0
    if k_active > 4:
        m[k_active - 2:k_active] = torch.tensor([0.75, 0.25])
    return m.to(dev), k_active


def inputs(n, nd, dev, seed=5):
    g = torch.Generator().manual_seed(seed)
    poses = torch.rand(n, 3, generator=g) * 2 - 1
    return poses.to(dev), torch.randn(4, n, generator=g).to(dev), torch.randn(nd, 4, n, generator=g).to(dev)


def fused(net, poses, dirs, up, upj, mask, k_active):
    """the raw calls: (flows, jac, grads, saved)"""
    from sin_inn_amd import flownet
    flows, jac, saved, tsaved = flownet.flownet_jacobian_forward_points(net, poses, SCALE, dirs, mask=mask, k_active=k_active)
    grads = flownet.flownet_jacobian_backward_points(net, poses, SCALE, dirs, up, upj, saved, tsaved, mask=mask, k_active=k_active)
    return flows, jac, grads, saved


def against_reference(label, name, net, poses, dirs, up, upj, mask, k_active, worst=None, composed=True):
    from sin_inn_amd import flownet
    n = poses.shape[0]
    flows, jac, grads, saved = fused(net, poses, dirs, up, upj, mask, k_active)
    assert bool(torch.isfinite(jac).all()) and (n < 8 or k_active == 0 or bool((jac != 0).any()))
    gates = [saved[l, :n] > 0 for l in range(3)]
    bufs, weights = net_tensors(net, poses.device)
    ref = J.reference(name, bufs, weights, poses, SCALE, dirs, up, upj, mask, gates)
    J.check_all(f'fused {label}', dirs, flows, jac, grads, ref, worst)
    if composed:
        params = [p for lin in net.linears() for p in (lin.weight, lin.bias)]
        for p in params:
            p.grad = None
        cf, cj = flownet.flow_jacobian_composed(net, poses, SCALE, ''.join('tyx'[d] for d in dirs), override_mask=mask, planar=True, gates=gates)
        ((cf * up).sum() + (cj * upj).sum()).backward()
        J.check_all(f'composed {label}', dirs, cf, cj, [p.grad for p in params], ref)
        for p in params:
            p.grad = None
    return flows, jac, grads


# ---- 1 ----
PLAIN = [(name, None, dirs) for name in ('RBF', 'FFN', 'UFF') for dirs in ((1, 2), (0,), (0, 1, 2))]
PROG = [(name, k, dirs) for name in ('PRBF', 'PFF', 'PUFF') for k in (0, 3, 16, 19, 515) for dirs in ((1, 2), (0,), (0, 1, 2))]


@pytest.mark.parametrize('name,k_active,dirs', PLAIN + PROG)
def test_against_float64(dev, name, k_active, dirs):
    net = net_of(name, dev)
    mask, k = mask_of(net, k_active, dev)
    poses, up, upj = inputs(129, len(dirs), dev)
    worst = []
    against_reference(f'{name} k={k_active} {"".join("tyx"[d] for d in dirs)} N=129', name, net, poses, dirs, up, upj, mask, k, worst)
    print('worst: %.3g at %s' % max(worst))


@pytest.mark.parametrize('name', ['RBF', 'PFF'])
@pytest.mark.parametrize('n', [1, 63, 64, 65])
def test_tile_edges_against_float64(dev, name, n):
    net = net_of(name, dev)
    mask, k = mask_of(net, 131, dev)
    dirs = (1, 2)
    poses, up, upj = inputs(n, len(dirs), dev, seed=6)
    against_reference(f'{name} N={n}', name, net, poses, dirs, up, upj, mask, k)


@pytest.mark.parametrize('name', ['RBF', 'PRBF'])
def test_past_one_sweep_of_the_forward_grid(dev, name):
    net = net_of(name, dev)
    mask, k = mask_of(net, 67, dev)
    dirs = (1, 2)
    poses, up, upj = inputs(BIG, len(dirs), dev, seed=7)
    flows, jac, grads = against_reference(f'{name} N={BIG}', name, net, poses, dirs, up, upj, mask, k, composed=False)
    # the last tile is the partial one of the second sweep: its rows are the small call's rows, bit for bit
    tail = slice(BIG - 65, BIG)
    f2, j2, _, _ = fused(net, poses[tail].contiguous(), dirs, up[:, tail].contiguous(), upj[:, :, tail].contiguous(), mask, k)
    assert torch.equal(f2, flows[:, tail]) and torch.equal(j2, jac[:, :, tail])


# ---- 2 ----
@pytest.mark.parametrize('name', ['RBF', 'FFN', 'PRBF', 'PUFF'])
def test_exact_properties(dev, name):
    from sin_inn_amd import flownet
    net = net_of(name, dev)
    mask, k = mask_of(net, 19, dev)
    dirs = (0, 1, 2)
    n = 129
    poses, up, upj = inputs(n, len(dirs), dev)
    kw = dict(mask=mask, k_active=k)
    flows, jac, grads, saved = fused(net, poses, dirs, up, upj, mask, k)
    # the plain call's flows and hidden layers
    pf, psaved = flownet.flownet_forward_points(net, poses, SCALE, True, **kw)
    assert torch.equal(flows, pf) and torch.equal(saved, psaved)
    # djac = 0: the plain backward's gradients
    plain = flownet.flownet_backward_points(net, poses, SCALE, up, psaved, **kw)
    _, _, zero, _ = fused(net, poses, dirs, up, torch.zeros_like(upj), mask, k)
    assert all(bool((a == b).all()) for a, b in zip(zero, plain))
    # two calls
    f2, j2, g2, _ = fused(net, poses, dirs, up, upj, mask, k)
    assert torch.equal(j2, jac) and torch.equal(f2, flows) and all(torch.equal(a, b) for a, b in zip(g2, grads))
    assert any(not torch.equal(a, b) for a, b in zip(grads, plain))                     # and djac does reach the parameters
    # a direction subset is the matching slice of the full set
    _, jyx, _, _ = fused(net, poses, (1, 2), up, upj[1:], mask, k)
    assert torch.equal(jyx, jac[1:])
    if net.is_progressive:
        # k_active past the last open feature
        for other in (20, 32, 131, 515):
            f3, j3, g3, _ = fused(net, poses, dirs, up, upj, mask, other)
            assert torch.equal(j3, jac) and torch.equal(f3, flows) and all(torch.equal(a, b) for a, b in zip(g3, grads)), other


@pytest.mark.parametrize('name', ['RBF', 'PRBF'])
def test_a_small_grid_in_any_order_within_a_tile(dev, name):
    net = net_of(name, dev)
    mask, k = mask_of(net, 19, dev)
    dirs = (1, 2)
    gt, gy, gx = torch.meshgrid(torch.tensor([-0.5, 0.5]), torch.linspace(-1, 1, 8), torch.linspace(-1, 1, 8), indexing='ij')
    poses = torch.stack((gt, gy, gx), dim=-1).view(-1, 3).to(dev)                       # 128 points: two whole tiles
    n = poses.shape[0]
    _, up, upj = inputs(n, len(dirs), dev)
    perm = torch.cat([torch.randperm(64, generator=torch.Generator().manual_seed(3 + t)) + 64 * t for t in range(2)]).to(dev)
    f, j, _, _ = fused(net, poses, dirs, up, upj, mask, k)
    fp, jp, _, _ = fused(net, poses[perm].contiguous(), dirs, up[:, perm].contiguous(), upj[:, :, perm].contiguous(), mask, k)
    assert torch.equal(fp, f[:, perm]) and torch.equal(jp, j[:, :, perm])
    # the bits in question are the per-point outputs.  The parameter gradients are sums over a tile's rows in row order, so a permuted tile
    # adds the same terms in another order: they are held to the float64 reference (test_against_float64), not to each other


@pytest.mark.parametrize('name', ['RBF', 'PFF'])
def test_non_finite_poses_stay_in_their_rows(dev, name):
    from sin_inn_amd import flownet
    net = net_of(name, dev)
    mask, k = mask_of(net, 515, dev)
    dirs = (0, 1, 2)
    n = 129
    poses = inputs(n, 3, dev)[0]
    clean = flownet.flownet_jacobian_forward_points(net, poses, SCALE, dirs, mask=mask, k_active=k)
    bad = poses.clone()
    rows = [0, 63, 64, 128]
    bad[0, 1], bad[63, 0], bad[64, 2], bad[128] = NAN, float('inf'), float('-inf'), NAN
    got = flownet.flownet_jacobian_forward_points(net, bad, SCALE, dirs, mask=mask, k_active=k)
    keep = torch.ones(n, dtype=torch.bool, device=dev)
    keep[rows] = False
    assert torch.equal(got[0][:, keep], clean[0][:, keep]) and torch.equal(got[1][:, :, keep], clean[1][:, :, keep])


# ---- 3 ----
def test_autograd_surface(dev):
    from sin_inn_amd import flownet, progressive
    rbf = net_of('RBF', dev)
    poses, up, upj = inputs(40, 2, dev)
    params = [p for lin in rbf.linears() for p in (lin.weight, lin.bias)]
    flows, jac, grads, _ = fused(rbf, poses, (1, 2), up, upj, None, None)
    for p in params:
        p.grad = None
    out, j = flownet.flow_at(rbf, poses.view(5, 8, 3), SCALE, jacobian=True)
    assert tuple(out.shape) == (5, 8, 4) and tuple(j.shape) == (5, 8, 4, 2) and out.requires_grad and j.requires_grad
    assert torch.equal(out.detach(), flownet.flow_at(rbf, poses.view(5, 8, 3), SCALE).detach())            # bitwise the call without the keyword
    assert torch.equal(j.detach().view(40, 4, 2).permute(2, 1, 0), jac)
    ((out.view(40, 4).t() * up).sum() + (j.view(40, 4, 2).permute(2, 1, 0) * upj).sum()).backward()
    assert all(torch.equal(p.grad, g) for p, g in zip(params, grads))
    # planar, and a None upstream for either output
    plain = flownet.flownet_backward_points(rbf, poses, SCALE, up, flownet.flownet_forward_points(rbf, poses, SCALE, True)[1])
    for p in params:
        p.grad = None
    out, j = flownet.flow_at(rbf, poses, SCALE, planar=True, jacobian='yx')
    assert tuple(out.shape) == (4, 40) and tuple(j.shape) == (2, 4, 40)
    (out * up).sum().backward()
    assert all(torch.equal(p.grad, g) for p, g in zip(params, plain))
    for p in params:
        p.grad = None
    out, j = flownet.flow_at(rbf, poses, SCALE, planar=True, jacobian='yx')
    (j * upj).sum().backward()
    _, _, only, _ = fused(rbf, poses, (1, 2), torch.zeros_like(up), upj, None, None)
    assert all(torch.equal(p.grad, g) for p, g in zip(params, only))
    assert not bool(params[1].grad.any()) and not bool(params[7].grad.any())                               # no bias enters a tangent
    for p in params:
        p.grad = None
    with torch.no_grad():
        out, j = flownet.flow_at(rbf, poses, SCALE, planar=True, jacobian='t')
    assert not j.requires_grad and tuple(j.shape) == (1, 4, 40)
    # net(poses, jacobian=) and a controller
    o1, j1 = rbf(poses, jacobian='yx')
    o2, j2 = flownet.flow_at(rbf, poses, 1.0, jacobian='yx')
    assert torch.equal(o1, o2) and torch.equal(j1, j2)
    ctrl = progressive.LinearControllerEarly(net_of('PRBF', dev), 1000, epsilon=1e-3)
    o1, j1 = ctrl(poses, jacobian='yx')
    o2, j2 = flownet.flow_at(ctrl, poses, 1.0, jacobian='yx')
    assert torch.equal(o1, o2) and torch.equal(j1, j2) and tuple(j1.shape) == (40, 4, 2)
    assert torch.equal(o1.detach(), ctrl(poses).detach())
    for p in ctrl.parameters():
        p.grad = None


# ---- 4 ----
@pytest.mark.parametrize('net_name', ['RBF', 'PRBF'])
def test_one_trainer_step_fused_against_composed(dev, net_name):
    """the smoothness term of one step and its parameter gradients: composed in float64 is the reference (frames, poses and weights widened),
    composed in fp32 the unit, fused within MULT x the unit.  The term is continuous in the ReLU gates, so they are free here"""
    import flowgather_grad_refs as G
    from sin_inn_amd import flownet, flowtrainer
    args = G.trainer_args(net=net_name, argv=['--loss-smooth-at', '0.7', '--smooth-points', '4096'])
    args.net = args.net.to(dev)
    model = flowtrainer.FlowTrainer(args)
    batch = [t.to(dev) for t in G.trainer_batch()[:4]]
    params = [p for p in model.net.parameters()]

    def step(fused_path, dtype=F32):
        m = flowtrainer.FlowTrainer(args)                                              # a fresh generator: the same draw
        m.fused = fused_path
        for p in params:
            p.grad = None
        if dtype == F64:
            real = flownet.flow_jacobian_composed
            flownet.flow_jacobian_composed = lambda net, poses, *a, **kw: real(net, poses.to(F64), *a, **kw)
        try:
            loss = m.smooth_at_loss(batch[0].to(dtype), batch[1].to(dtype), batch[2], 8.0)
        finally:
            if dtype == F64:
                flownet.flow_jacobian_composed = real
        loss.backward()
        return loss.detach(), [torch.zeros_like(p) if p.grad is None else p.grad.clone() for p in params]   # composed: a bias is in no tangent, no grad

    ref, unit, got = step(False, F64), step(False), step(True)
    J.check(f'trainer {net_name} smooth_at', got[0], ref[0], unit[0])
    for i, (g, r64, r32) in enumerate(zip(got[1], ref[1], unit[1])):
        if bool((r64 != 0).any()):
            J.check(f'trainer {net_name} grad {i}', g, r64, r32)
        else:
            assert not bool(g.any()), i
    for p in params:
        p.grad = None
