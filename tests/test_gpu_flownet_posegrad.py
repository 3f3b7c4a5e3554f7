"""GPU: the gradient of the flow networks with respect to the coordinates (flow_at(.., pose_grad=True); flownet_posegrad_kernel of
csrc/flownet.hip, the POSEGRAD chain kernel of csrc/siren.hip; sininn_flownet_backward_posegrad_points / sininn_siren_backward_posegrad_points).

  1. g_poses at N = 1000 scattered points against torch.autograd.grad of the float64 restatement with the poses as a leaf and the kernel's own
     ReLU gates forced (RFF: g_enc_a from the same call as well).  Error and unit are max-norms relative to the max-norm of the float64
     gradient; budget = 4 x the unit, the unit the error of the same restatement in fp32 -- derived from the restatement, never from the
     kernel.  RBFG: the points whose float64 remainder operand lies within 1e-6 of a wrap are excluded from both (at most 3 % of them;
     17 of 1000 with the seeds used here, counted on the CPU); no other encoding excludes anything.
  2. bits (RBF, PRBF, siren; every output NaN before the call): two calls agree, N in {1, 64, 65} agree on their common points, a permuted
     list gives the permuted gradient, PRBF: every valid k_active gives the bits of 515 and a mask closed beyond the coordinates gives
     m_d dz_d; the parameter gradients (and g_enc_a) of the posegrad call are those of the existing points calls.
  3. the autograd surface: p.grad of flow_at(.., pose_grad=True) is the raw call's g_poses for (..., 3) shapes and planar=True; a chained
     query reaches the parameters through p' within the budget of 1; a double backward raises; without pose_grad the old error; under
     no_grad nothing is saved.
  4. end to end: tools/fit_flow.fit_points(cycle=True), the forward-backward consistency term at continuous points, fused against composed:
     the first loss of each within 1e-4 relative of the float64 restatement's loss (the bound of the project's other end-to-end tests; the
     loss is continuous in the ReLU gates, so they are free), and the loss falls in both.

Measured on an MI355X (`ratio(...)` lines of a run with -s: error / budget); the table is in DESIGN 14.8.
"""
import os
import sys

import pytest
import torch

pytestmark = pytest.mark.gpu
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from flownet_posegrad_refs import chained, rbfg_near_wrap, reference_pose_grads  # noqa: E402
from flownet_points_refs import siren_restate_points  # noqa: E402
from flownet_refs import net_tensors  # noqa: E402
from siren_refs import siren_tensors  # noqa: E402
from test_gpu_flownet import F64, MULT, SCALE, relmax  # noqa: E402
from test_gpu_flownet_points import N_SCATTER, Case, scattered  # noqa: E402

F32 = torch.float32
NAN = float('nan')
NETS = ('RBF', 'FFN', 'RBFG', 'PE', 'RFF', 'PRBF', 'PPE', 'siren')
BIT_NETS = ('RBF', 'PRBF', 'siren')
_cache = {}


@pytest.fixture(scope='module')
def dev():
    import sin_inn_amd  # noqa: F401
    assert torch.cuda.is_available(), 'GPU tests need a GPU'
    return torch.device('cuda', 0)


def case(name, dev):
    if name not in _cache:
        _cache[name] = Case(name, dev)
    return _cache[name]


def upstream(n, dev):
    return torch.randn(4, n, generator=torch.Generator().manual_seed(11)).to(dev)


def posegrad(c, poses, up, **over):
    """forward, then the posegrad call with every buffer NaN before it: (the gradients as Case.backward_points lists them, g_poses)"""
    from sin_inn_amd import flownet
    n = poses.shape[0]
    bufs = c.nan(n)
    _, saved = c.forward_points(poses, bufs[0], **over)
    g_poses = torch.full((n, 3), NAN, device=c.dev)
    if c.siren:
        return flownet.siren_backward_points(c.net, poses, SCALE, up, saved, bufs[1], pose_grad=True, g_poses=g_poses) + (saved,)
    kw = {**c.kw, **over}
    res, gp = flownet.flownet_backward_points(c.net, poses, SCALE, up, saved, bufs[1], enc_grad=c.learnable, pose_grad=True, g_poses=g_poses, **kw)
    if c.learnable:
        res = res[0] + [res[1]]
    assert gp is g_poses
    return res, gp, saved


def check(name, got, ref64, ref32, keep=None):
    """error of the kernel against MULT x the fp32-torch unit, rows `keep` only; prints ratio(error / budget)"""
    if keep is not None:
        got, ref64, ref32 = got[keep], ref64[keep], ref32[keep]
    unit = relmax(ref32, ref64)
    budget = MULT * unit
    err = relmax(got, ref64)
    print(f'ratio({name}) = {err / budget:.3g}   [err {err:.3g}, fp32-torch unit {unit:.3g}, budget {budget:.3g}]')
    assert err <= budget, (name, err, budget)


# ---- 1 ----
@pytest.mark.parametrize('name', NETS)
def test_g_poses_against_float64(dev, name):
    c = case(name, dev)
    n = N_SCATTER
    poses, up = scattered(n, dev), upstream(n, dev)
    got, g_poses, saved = posegrad(c, poses, up)
    assert g_poses.shape == (n, 3) and bool(torch.isfinite(g_poses).all())
    keep = None
    if c.siren:
        ebufs, weights, gates = None, siren_tensors(c.net, dev), None
    else:
        ebufs, weights = net_tensors(c.net, dev)
        if name == 'RBFG':
            near = rbfg_near_wrap(ebufs, poses)
            print(f'RBFG: {int(near.sum())} of {n} points within 1e-6 of a wrap, excluded')
            assert int(near.sum()) <= 0.03 * n
            keep = ~near
        if c.learnable:
            ebufs = c.kw['enc_a']
        gates = [saved[l, :n] > 0 for l in range(3)]
    mask = c.hmask.to(dev) if c.hmask is not None else None
    ref = reference_pose_grads(name, ebufs, weights, poses, SCALE, up, mask, gates, with_enc=c.learnable)
    check(f'{name} g_poses', g_poses, ref[F64][0], ref[F32][0], keep)
    if c.learnable:
        check(f'{name} g_enc_a (same call)', got[-1], ref[F64][1], ref[F32][1])


# ---- 2 ----
@pytest.mark.parametrize('name', BIT_NETS + ('RFF',))
def test_two_calls_agree_and_the_other_gradients_are_the_points_calls(dev, name):
    c = case(name, dev)
    n = N_SCATTER
    poses, up = scattered(n, dev), upstream(n, dev)
    a, ga, saved = posegrad(c, poses, up)
    b, gb, _ = posegrad(c, poses, up)
    assert bool(torch.isfinite(ga).all()) and torch.equal(ga, gb)
    plain = c.backward_points(poses, up, saved, *c.nan(n)[1:])
    assert len(a) == len(b) == len(plain) == len(c.names())
    for nm, x, y, z in zip(c.names(), a, b, plain):
        assert bool(torch.isfinite(x).all()) and torch.equal(x, y) and torch.equal(x, z), nm


@pytest.mark.parametrize('name', BIT_NETS)
def test_tile_edges_and_permutation(dev, name):
    c = case(name, dev)
    poses, up = scattered(N_SCATTER, dev), upstream(N_SCATTER, dev)
    g = {n: posegrad(c, poses[:n].contiguous(), up[:, :n].contiguous())[1] for n in (1, 64, 65, N_SCATTER)}
    assert torch.equal(g[65][:64], g[64]) and torch.equal(g[1][0], g[64][0]) and torch.equal(g[N_SCATTER][:65], g[65])
    perm = torch.randperm(N_SCATTER, generator=torch.Generator().manual_seed(3)).to(dev)
    gp = posegrad(c, poses[perm].contiguous(), up[:, perm].contiguous())[1]
    assert torch.equal(gp, g[N_SCATTER][perm])


def test_k_active_and_a_closed_mask(dev):
    c = case('PRBF', dev)
    n = 200
    poses, up = scattered(n, dev), upstream(n, dev)
    assert c.kw['k_active'] == 12
    want = posegrad(c, poses, up, k_active=515)[1]
    for k in (12, 13, 64, 67, 131, 259, 323):
        assert torch.equal(posegrad(c, poses, up, k_active=k)[1], want), k
    # closed beyond the coordinates: the encoded part is an exact zero, what is left is m_d dz_d; powers of two scale it exactly.  The
    # forward pass, and with it dh1, reads m_d as well, so dh1 is held fixed: the same `saved`, the mask changed for the backward call only
    from sin_inn_amd import flownet
    ones = torch.zeros(515, device=dev)
    ones[:3] = 1.0
    scaled = ones.clone()
    scaled[:3] = torch.tensor([0.5, 0.25, 2.0])
    saved, ws = c.nan(n)
    _, saved = c.forward_points(poses, saved, mask=ones, k_active=3)
    out = {}
    for key, m, k in (('ones', ones, 3), ('ones515', ones, 515), ('scaled', scaled, 3), ('zero', torch.zeros(515, device=dev), 0)):
        gp = torch.full((n, 3), NAN, device=dev)
        flownet.flownet_backward_points(c.net, poses, SCALE, up, saved, ws, mask=m, k_active=k, pose_grad=True, g_poses=gp)
        out[key] = gp
    assert bool(torch.isfinite(out['ones']).all()) and bool((out['ones'] != 0).any())
    assert torch.equal(out['ones'], out['ones515'])
    assert torch.equal(out['scaled'], out['ones'] * scaled[:3])
    assert bool((out['zero'] == 0).all()) and not bool(torch.signbit(out['zero']).any())


# ---- 3 ----
@pytest.mark.parametrize('name', ['RBF', 'RFF', 'PRBF', 'siren'])
def test_autograd_fills_the_pose_gradient_with_the_raw_values(dev, name):
    from sin_inn_amd import flownet
    c = case(name, dev)
    n = 5 * 8
    poses = scattered(n, dev, seed=9)
    up = torch.randn(n, 4, generator=torch.Generator().manual_seed(11)).to(dev)
    grads, want, _ = posegrad(c, poses, up.t().contiguous())
    leaves = c.params + ([c.net.encode.frequencies] if c.learnable else [])
    for shape, planar in (((n, 3), False), ((5, 8, 3), False), ((2, 2, 10, 3), False), ((5, 8, 3), True)):
        for q in leaves:
            q.grad = None
        p = poses.view(shape).clone().requires_grad_(True)
        out = flownet.flow_at(c.target, p, SCALE, planar=planar, pose_grad=True)
        assert out.shape == ((4, n) if planar else shape[:-1] + (4,)) and out.requires_grad
        out.backward(up.t().contiguous() if planar else up.view(shape[:-1] + (4,)))
        assert p.grad.shape == shape and torch.equal(p.grad.view(n, 3), want), (shape, planar)
        for nm, q, g in zip(c.names(), c.params, grads):           # the parameters get what they always got
            assert torch.equal(q.grad, g), nm
    for q in leaves:
        q.grad = None
    # net(poses, pose_grad=True) and the controller pass the keyword on
    p = poses.clone().requires_grad_(True)
    c.target(p, pose_grad=True).backward(up)
    q = poses.clone().requires_grad_(True)
    flownet.flow_at(c.target, q, 1.0, pose_grad=True).backward(up)
    assert torch.equal(p.grad, q.grad)
    # frozen parameters: the poses alone carry the graph
    for t in leaves:
        t.requires_grad_(False)
    try:
        p = poses.clone().requires_grad_(True)
        flownet.flow_at(c.target, p, SCALE, pose_grad=True).backward(up)
        assert torch.equal(p.grad, want)
    finally:
        for t in leaves:
            t.requires_grad_(True)
            t.grad = None


def test_double_backward_raises_and_the_old_refusal_stands(dev):
    from sin_inn_amd import flownet
    c = case('RBF', dev)
    poses = scattered(40, dev, seed=9)
    p = poses.clone().requires_grad_(True)
    out = flownet.flow_at(c.net, p, pose_grad=True)
    g, = torch.autograd.grad(out.sum(), p, create_graph=True)
    with pytest.raises(RuntimeError):
        g.sum().backward()
    with pytest.raises(NotImplementedError, match='no gradient with respect to the coordinates'):
        flownet.flow_at(c.net, p)
    with torch.no_grad():
        out = flownet.flow_at(c.net, p, pose_grad=True)
    assert not out.requires_grad and out.grad_fn is None           # inference mode: nothing saved
    assert torch.equal(out, flownet.flow_at(c.net, poses).detach())
    out = flownet.flow_at(c.net, poses, pose_grad=True)            # the keyword alone changes nothing for poses that ask for no gradient
    assert torch.equal(out.detach(), flownet.flow_at(c.net, poses).detach())
    for q in c.params:
        q.grad = None


def test_a_chained_query_reaches_the_parameters_through_the_moved_points(dev):
    """p' = p + (0, flow12(p)), then the flow at p': the gradient of the second query reaches the parameters of the first through p'.
    SIREN: no gates to force, the composition is smooth; float64 and fp32 restatements of the SAME composition give reference and unit"""
    from sin_inn_amd import flownet
    c = case('siren', dev)
    n = N_SCATTER
    poses = scattered(n, dev)
    up = torch.randn(n, 4, generator=torch.Generator().manual_seed(11)).to(dev)
    for q in c.params:
        q.grad = None
    p = poses.clone().requires_grad_(True)
    out = chained(lambda x: flownet.flow_at(c.net, x, 1.0, pose_grad=True), p)
    out.backward(up)
    got = [q.grad.clone() for q in c.params]
    got_p = p.grad.clone()
    for q in c.params:
        q.grad = None
    ref = {}
    for dtype in (F64, F32):
        w = [t.to(dtype).requires_grad_(True) for t in siren_tensors(c.net, dev)]
        x = poses.to(dtype).requires_grad_(True)
        o = chained(lambda y: siren_restate_points(w, y, 1.0, dtype).t(), x)
        ref[dtype] = torch.autograd.grad((o * up.to(dtype)).sum(), w + [x])
    for nm, g, r64, r32 in zip(c.names() + ['g_poses'], got + [got_p], ref[F64], ref[F32]):
        check(f'siren chained {nm}', g, r64, r32)
    # without the first query's pose gradient the parameters see the second query only: the feature is what closes the gap
    detached = chained(lambda x: flownet.flow_at(c.net, x.detach(), 1.0), poses)
    detached.backward(up)
    assert relmax(c.params[0].grad, ref[F64][0]) > MULT * relmax(ref[F32][0], ref[F64][0])
    for q in c.params:
        q.grad = None


# ---- 4 ----
def test_fit_points_with_the_cycle_term_end_to_end(dev):
    from sin_inn_amd import flownet
    from flownet_points_refs import restate_points
    sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), 'tools'))
    import fit_flow
    info = {}
    fused = fit_flow.fit_points('RBF', 2048, 30, composed=False, info=info, cycle=True)
    comp = fit_flow.fit_points('RBF', 2048, 30, composed=True, cycle=True)
    first = info['first']
    net0 = flownet.RbfModel(flownet.ModelParams()).to(dev)
    net0.load_state_dict(first['state'])
    bufs, weights = net_tensors(net0, dev)
    with torch.no_grad():
        query = lambda x: restate_points('RBF', bufs, weights, x, 1.0, F64).t()  # noqa: E731
        p64 = first['poses'].to(F64)
        out = query(p64)
        loss64 = float((out - first['target'].to(F64)).pow(2).mean() + fit_flow.cycle_term(query, p64, out))
    print(f'step 0: float64 {loss64:.9f}  fused off by {abs(fused[0] - loss64) / loss64:.3g}  composed off by '
          f'{abs(comp[0] - loss64) / loss64:.3g} (relative; bound 1e-4)   final: fused {fused[-1]:.6f} composed {comp[-1]:.6f}')
    assert abs(fused[0] - loss64) <= 1e-4 * loss64 and abs(comp[0] - loss64) <= 1e-4 * loss64
    assert fused[-1] < fused[0] and comp[-1] < comp[0]
