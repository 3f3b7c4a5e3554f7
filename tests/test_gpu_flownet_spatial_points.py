"""GPU: per-point masks at pose lists (controller(poses) of a StashedSpatialController, flow_at under a mask grid;
sininn_flownet_*_spatial_points, sininn_flownet_sample_mask_points; the SPATIAL form of flownet_posegrad_kernel, csrc/flownet.hip).

  1. a pose list that spells out a 2 x 5 x 13 grid (130 points: two full tiles and a part) under a random res-3 grid gives the bits of the
     spatial grid call: flows, `saved`, the eight parameter gradients, g_enc_a (PRFF) and the sampled mask; again with both time values
     outside [-1, 1] (the corner indices are clamped).  PRBF, PFF, PRFF, PRBFG.
  2. bits (PRBF, PRFF; every output NaN before the call): two calls agree; N in {1, 63, 64, 65, 129} agree on their common points (flows and
     g_poses); a permuted list gives permuted flows and g_poses; k_active in {3, 9, 19, 67, 259, 515} gives the bits of 515 where the grid is
     zero from that column on; a grid closed beyond its coordinate columns gives g_poses[p][d] == sample_mask[p][d] * g, g the global-mask
     call's g_poses under (1, 1, 1, 0, ..) on the same `saved`; the parameter gradients of the posegrad call are those of the call without it.
  3. float64 parity at N = 1000 scattered points, res 3 (identity scale) and res 7 (a centre_scale that is not the identity): the per-point
     mask is computed once from the fp32 cells (flownet_spatial_refs.cells / interp_mask) and is a CONSTANT of both restatements, the gates
     are the kernel's (`saved` > 0).  Flows and parameter gradients by tests/test_gpu_flownet.py's `check` (min(MULT x the fp32-torch unit,
     1e-4)), g_poses by tests/test_gpu_flownet_posegrad.py's (MULT x the unit); the unit is the fp32 evaluation of the same restatement.
     PRBFG excludes the points within 1e-6 of a wrap from g_poses (rbfg_near_wrap): 12 of 1000 with the seeds used here, counted on the CPU,
     at most 3 %.  Nothing else excludes anything.
  4. the autograd surface of controller(poses): pose_grad, a chained query, get_mask, a grid that moved on, double backward, no_grad, stash.
  5. end to end: tools/fit_flow.fit_points(controller='spatial', res=3), with and without the cycle term, fused against composed: the first
     loss of each within 1e-4 relative of the float64 loss (the bound of the project's other end-to-end tests), the loss falls in both.

Measured on an MI355X (`ratio(...)` lines of a run with -s: error / budget); the table is in DESIGN 14.9.
"""
import os
import sys

import pytest
import torch

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from flownet_points_refs import grid_poses  # noqa: E402
from flownet_posegrad_refs import chained, rbfg_near_wrap  # noqa: E402
from flownet_refs import nan_buffers, net_tensors  # noqa: E402
from flownet_spatial_refs import interp_mask, restate_points  # noqa: E402
from test_gpu_flownet import F64, MULT, check, relmax  # noqa: E402
from test_gpu_flownet_points import N_SCATTER, scattered  # noqa: E402
from test_gpu_flownet_posegrad import check as check_unit  # noqa: E402

F32 = torch.float32
NAN = float('nan')
NETS = {'PRBF': 404, 'PFF': 505, 'PRFF': 707, 'PRBFG': 808}
SCALE = 3.0
GNAMES = [f'g{k}{l}' for l in (1, 2, 3, 4) for k in ('W', 'b')]
CS7 = (0.1, -0.05, 0.02, 0.9, 1.1, 0.8)                # keeps every scaled coordinate of [-1, 1]^3 inside (-1.2, 1.2): no clamped corner
_cache = {}


@pytest.fixture(scope='module')
def dev():
    import sin_inn_amd  # noqa: F401
    assert torch.cuda.is_available(), 'GPU tests need a GPU'
    return torch.device('cuda', 0)


class Net:
    def __init__(self, name, dev):
        from sin_inn_amd import flownet
        torch.manual_seed(NETS[name])
        self.name, self.dev = name, dev
        self.net = flownet.all_model_dict[name](flownet.ModelParams()).to(dev)
        self.fourier = name == 'PRFF'
        self.enc_a = self.net.encode.effective_frequencies().detach().contiguous() if self.fourier else None
        self.bufs, self.weights = net_tensors(self.net, dev)
        if self.fourier:
            self.bufs = self.enc_a
        self.names = GNAMES + (['g_enc_a'] if self.fourier else [])


def net_of(name, dev):
    if name not in _cache:
        _cache[name] = Net(name, dev)
    return _cache[name]


def rand_grid(res, dev, zero_from=515, seed=5):
    g = torch.rand(res ** 3, 515, generator=torch.Generator().manual_seed(seed))
    g[:, zero_from:] = 0
    return g.to(dev)


def upstream(n, dev):
    return torch.randn(4, n, generator=torch.Generator().manual_seed(11)).to(dev)


def run_points(c, poses, up, grid, res, cs=None, ka=None, pose_grad=True, saved_from=None, scale=SCALE):
    """forward and backward at a pose list, every buffer NaN before: dict(flows, saved, grads (list, g_enc_a last), g_poses)"""
    from sin_inn_amd import flownet
    n = poses.shape[0]
    saved, ws, _ = nan_buffers(n, c.dev)
    flows, saved = flownet.flownet_forward_spatial_points(c.net, poses, scale, True, grid, res, cs, ka, saved, c.enc_a)
    kw = dict(centre_scale=cs, k_active=ka, workspace=ws, enc_a=c.enc_a, enc_grad=c.fourier)
    use = saved if saved_from is None else saved_from
    gp = None
    if pose_grad:
        gp = torch.full((n, 3), NAN, device=c.dev)
        out, got = flownet.flownet_backward_spatial_points(c.net, poses, scale, up, use, grid, res, pose_grad=True, g_poses=gp, **kw)
        assert got is gp
    else:
        _, _, ews = nan_buffers(n, c.dev)
        out = flownet.flownet_backward_spatial_points(c.net, poses, scale, up, use, grid, res, enc_workspace=ews if c.fourier else None, **kw)
    grads = list(out[0]) + [out[1]] if c.fourier else list(out)
    return dict(flows=flows, saved=saved, grads=grads, g_poses=gp)


# ---- 1 ----
@pytest.mark.parametrize('times', [(0.0, 0.5), (-1.9, 2.4)])
@pytest.mark.parametrize('name', list(NETS))
def test_a_grid_spelled_out_as_poses_gives_the_spatial_grid_call_bitwise(dev, name, times):
    from sin_inn_amd import flownet
    c = net_of(name, dev)
    times = torch.tensor(times, device=dev)
    ys, xs = torch.linspace(-1, 1, 5).to(dev), torch.linspace(-1, 1, 13).to(dev)
    n = 2 * 5 * 13
    poses = grid_poses(times, ys, xs)
    assert poses.shape == (n, 3) and n // 64 == 2 and n % 64
    grid = rand_grid(3, dev)
    up = torch.randn(2, 4, 5, 13, generator=torch.Generator().manual_seed(11)).to(dev)
    saved, ws, ews = nan_buffers(n, dev)
    flows_g, saved_g = flownet.flownet_forward_spatial(c.net, times, ys, xs, SCALE, True, grid, 3, saved=saved, enc_a=c.enc_a)
    out = flownet.flownet_backward_spatial(c.net, times, ys, xs, SCALE, up, saved_g, grid, 3, workspace=ws, enc_a=c.enc_a, enc_grad=c.fourier,
                                           enc_workspace=ews if c.fourier else None)
    want = list(out[0]) + [out[1]] if c.fourier else list(out)
    for pose_grad in (False, True):
        p = run_points(c, poses, up.permute(1, 0, 2, 3).reshape(4, n).contiguous(), grid, 3, pose_grad=pose_grad)
        assert p['flows'].shape == (4, n) and torch.equal(p['flows'].view(4, 2, 5, 13).permute(1, 0, 2, 3), flows_g)
        assert bool(torch.isfinite(p['saved']).all()) and torch.equal(p['saved'], saved_g)
        assert len(p['grads']) == len(want) == len(c.names)
        for nm, a, b in zip(c.names, p['grads'], want):
            assert bool(torch.isfinite(a).all()) and torch.equal(a, b), f'{name} {nm} (pose_grad={pose_grad}): points and grid differ'
    assert bool(torch.isfinite(p['g_poses']).all())
    m_g = flownet.flownet_sample_mask(c.net, times, ys, xs, grid, 3)
    m_p = flownet.flownet_sample_mask_points(c.net, poses, grid, 3)
    assert m_p.shape == (n, 515) and torch.equal(m_p, m_g)


# ---- 2 ----
@pytest.mark.parametrize('name', ['PRBF', 'PRFF'])
def test_two_calls_tile_edges_and_permutation(dev, name):
    c = net_of(name, dev)
    grid = rand_grid(3, dev)
    poses, up = scattered(129, dev), upstream(129, dev)
    full = run_points(c, poses, up, grid, 3)
    again = run_points(c, poses, up, grid, 3)
    plain = run_points(c, poses, up, grid, 3, pose_grad=False)
    assert bool(torch.isfinite(full['g_poses']).all()) and bool((full['g_poses'] != 0).any())
    assert torch.equal(full['g_poses'], again['g_poses']) and torch.equal(full['flows'], again['flows'])
    for nm, a, b, d in zip(c.names, full['grads'], again['grads'], plain['grads']):
        assert bool(torch.isfinite(a).all()) and torch.equal(a, b), nm
        assert torch.equal(a, d), f'{nm}: the posegrad call and the call without it differ'
    for n in (1, 63, 64, 65):
        part = run_points(c, poses[:n].contiguous(), up[:, :n].contiguous(), grid, 3)
        assert torch.equal(part['flows'], full['flows'][:, :n]), n
        assert torch.equal(part['g_poses'], full['g_poses'][:n]), n
    perm = torch.randperm(129, generator=torch.Generator().manual_seed(3)).to(dev)
    p = run_points(c, poses[perm].contiguous(), up[:, perm].contiguous(), grid, 3)
    assert torch.equal(p['flows'], full['flows'][:, perm]) and torch.equal(p['g_poses'], full['g_poses'][perm])


@pytest.mark.parametrize('name', ['PRBF', 'PRFF'])
def test_k_active_gives_the_bits_of_515(dev, name):
    """3, 9, 19, 67, 259, 515: nothing encoded, inside the first K step, past it, past the first wave's 64 columns, past the first pass of 256"""
    c = net_of(name, dev)
    poses, up = scattered(129, dev), upstream(129, dev)
    for k in (3, 9, 19, 67, 259, 515):
        grid = rand_grid(3, dev, zero_from=k)
        a, b = run_points(c, poses, up, grid, 3, ka=k), run_points(c, poses, up, grid, 3, ka=515)
        assert torch.equal(a['flows'], b['flows']) and torch.equal(a['g_poses'], b['g_poses']), k
        assert bool(torch.isfinite(a['g_poses']).all())
        for nm, x, y in zip(c.names, a['grads'], b['grads']):
            assert torch.equal(x, y), (k, nm)


@pytest.mark.parametrize('name', ['PRBF', 'PRFF'])
def test_a_grid_closed_beyond_the_coordinates_is_the_sampled_mask_times_the_global_gradient(dev, name):
    from sin_inn_amd import flownet
    c = net_of(name, dev)
    n = 129
    poses, up = scattered(n, dev), upstream(n, dev)
    grid = rand_grid(3, dev, zero_from=3)
    ones = torch.zeros(515, device=dev)
    ones[:3] = 1.0
    # dh1 is held fixed: one `saved` (of the global forward) for both backward calls, as tests/test_gpu_flownet_posegrad.py does
    saved, ws, _ = nan_buffers(n, dev)
    _, saved = flownet.flownet_forward_points(c.net, poses, SCALE, True, saved, mask=ones, k_active=3, enc_a=c.enc_a)
    g = torch.full((n, 3), NAN, device=dev)
    flownet.flownet_backward_points(c.net, poses, SCALE, up, saved, ws, mask=ones, k_active=3, enc_a=c.enc_a, pose_grad=True, g_poses=g)
    m = flownet.flownet_sample_mask_points(c.net, poses, grid, 3)
    for ka in (3, 515):
        got = run_points(c, poses, up, grid, 3, ka=ka, saved_from=saved)['g_poses']
        assert bool(torch.isfinite(got).all()) and bool((got != 0).any())
        assert torch.equal(got, m[:, :3] * g), ka


# ---- 3 ----
@pytest.mark.parametrize('res,cs,zero_from', [(3, None, 515), (7, CS7, 200)])
@pytest.mark.parametrize('name', list(NETS))
def test_scattered_points_against_float64(dev, name, res, cs, zero_from):
    from sin_inn_amd import flownet
    c = net_of(name, dev)
    n = N_SCATTER
    poses, up = scattered(n, dev), upstream(n, dev)
    grid = rand_grid(res, dev, zero_from, seed=6)
    got = run_points(c, poses, up, grid, res, cs, zero_from)
    infer, none = flownet.flownet_forward_spatial_points(c.net, poses, SCALE, False, grid, res, cs, zero_from, enc_a=c.enc_a)
    assert none is None and torch.equal(infer, got['flows'])
    m64 = interp_mask(grid, res, poses, F64, cs or (0.0, 0.0, 0.0, 1.0, 1.0, 1.0))
    sampled = flownet.flownet_sample_mask_points(c.net, poses, grid, res, cs)
    assert float((sampled.double() - m64).abs().max()) <= 4e-6
    gates = [got['saved'][l, :n] > 0 for l in range(3)]
    tag = f'{name} res {res}'
    with torch.no_grad():
        f64, f32 = (restate_points(name, c.bufs, c.weights, poses, dt, m64.to(dt)).t() * SCALE for dt in (F64, F32))
    check(f'{tag} flows', got['flows'], f64, f32)                                   # free gates: ReLU is continuous
    ref = {}
    for dt in (F64, F32):
        w = [p.to(dt).requires_grad_(True) for p in c.weights]
        x = poses.to(dt).requires_grad_(True)
        enc = [c.bufs.to(dt).requires_grad_(True)] if c.fourier else []
        flows = restate_points(name, enc[0] if c.fourier else c.bufs, w, x, dt, m64.to(dt), gates).t() * SCALE
        ref[dt] = torch.autograd.grad((flows * up.to(dt)).sum(), w + enc + [x])
    for nm, g, r64, r32 in zip(c.names, got['grads'], ref[F64], ref[F32]):
        check(f'{tag} {nm}', g, r64, r32)
    keep = None
    if name == 'PRBFG':
        near = rbfg_near_wrap(c.bufs, poses)
        print(f'PRBFG: {int(near.sum())} of {n} points within 1e-6 of a wrap, excluded')
        assert int(near.sum()) <= 0.03 * n
        keep = ~near
    check_unit(f'{tag} g_poses', got['g_poses'], ref[F64][-1], ref[F32][-1], keep)


# ---- 4 ----
def ramped_controller(name, dev, res=3):
    """a StashedSpatialController three iterations into its first ramp (block in progress at 0.75, k_active 12), called on pose lists"""
    from sin_inn_amd import progressive
    c = net_of(name, dev)
    ctl = progressive.StashedSpatialController(c.net, res, block_iterations=8)
    pts = scattered(64, dev, seed=2)
    for _ in range(3):
        with torch.no_grad():
            ctl(pts)
        ctl.stash_iteration(torch.full((64,), 0.5, device=dev))
    assert ctl.iteration == 3 and ctl.k_active == 12
    return c, ctl


@pytest.mark.parametrize('name', ['PRBF', 'PRFF'])
def test_controller_on_poses_fills_the_pose_gradient_with_the_raw_values(dev, name):
    from sin_inn_amd import flownet
    c, ctl = ramped_controller(name, dev)
    n = 40
    poses = scattered(n, dev, seed=9)
    up = torch.randn(n, 4, generator=torch.Generator().manual_seed(11)).to(dev)
    m = ctl.device_grid(dev)
    assert m.spatial and m.k_active == 12
    raw = run_points(c, poses, up.t().contiguous(), m.tensor, m.res, m.centre_scale, m.k_active, scale=1.0)   # controller(poses) has scale 1
    leaves = [p for lin in c.net.linears() for p in (lin.weight, lin.bias)]
    for shape, planar in (((n, 3), False), ((5, 8, 3), False), ((5, 8, 3), True)):
        for q in leaves:
            q.grad = None
        p = poses.view(shape).clone().requires_grad_(True)
        out = flownet.flow_at(ctl, p, 1.0, planar=True, pose_grad=True) if planar else ctl(p, pose_grad=True)
        assert out.shape == ((4, n) if planar else shape[:-1] + (4,)) and out.requires_grad
        assert torch.equal(out.detach().reshape(4, n) if planar else out.detach().reshape(n, 4).t(), raw['flows'])
        out.backward(up.t().contiguous() if planar else up.view(shape[:-1] + (4,)))
        assert p.grad.shape == shape and torch.equal(p.grad.view(n, 3), raw['g_poses']), (shape, planar)
        for nm, q, g in zip(GNAMES, leaves, raw['grads']):
            assert torch.equal(q.grad, g), nm
    for q in leaves:
        q.grad = None
    if c.fourier:
        c.net.encode.frequencies.grad = None
    # a raw grid as override_mask goes the same way, under the spatial and under a linear controller: all 515 features
    from sin_inn_amd import progressive
    lin = progressive.LinearController(c.net)
    with torch.no_grad():
        own = ctl(poses)
        assert torch.equal(own, ctl(poses, override_mask=m.tensor.clone())) and torch.equal(own, lin(poses, override_mask=m.tensor.clone()))
        out, mask = ctl(poses.view(5, 8, 3), get_mask=True)
    assert not out.requires_grad and out.grad_fn is None                     # no_grad: nothing saved
    assert mask.shape == (5, 8, 515)
    assert torch.equal(mask.view(n, 515), flownet.flownet_sample_mask_points(c.net, poses, m.tensor, m.res, m.centre_scale))
    assert float((mask.view(n, 515) - ctl.interpolate(poses)).abs().max()) <= 8e-6
    with pytest.raises(NotImplementedError):
        flownet.flow_at(c.net, poses, override_mask=m.tensor)                # a bare model: the interpolation is a controller's


def test_backward_after_the_grid_moved_on_and_double_backward_raise(dev):
    c, ctl = ramped_controller('PRBF', dev)
    poses = scattered(40, dev, seed=9)
    out = ctl(poses)
    assert out.requires_grad
    ctl.stash_iteration(torch.full((40,), 0.5, device=dev))
    ctl.get_mask()
    with pytest.raises(RuntimeError, match='changed between'):
        out.sum().backward()
    p = poses.clone().requires_grad_(True)
    g, = torch.autograd.grad(ctl(p, pose_grad=True).sum(), p, create_graph=True)
    with pytest.raises(RuntimeError):
        g.sum().backward()
    with pytest.raises(NotImplementedError, match='no gradient with respect to the coordinates'):
        ctl(p)
    for q in c.net.parameters():
        q.grad = None


def test_stash_after_controller_on_poses_is_the_composed_stash(dev):
    """the reference's indexed `+=` keeps ONE write where indices repeat, and on the device which one is not fixed; so the lists here put
    every point into a 2 x 2 x 2 block of cells of its own (res 9: blocks (1, 2), (3, 4), (5, 6) per axis, 27 points), where it is a sum"""
    from sin_inn_amd import progressive
    c = net_of('PRBF', dev)
    a, b = (progressive.StashedSpatialController(c.net, 9) for _ in range(2))
    gen = torch.Generator().manual_seed(4)
    base = torch.cartesian_prod(*[torch.tensor([1.0, 3.0, 5.0])] * 3)
    for _ in range(3):
        u = base + 0.1 + 0.8 * torch.rand(27, 3, generator=gen)
        poses = (((u - 0.5) / 7) * 2 - 1).to(dev)
        loss = torch.rand(27, generator=gen).to(dev)
        with torch.no_grad():
            a(poses.view(3, 9, 3))
        a.stash_iteration(loss)
        b.interpolate(poses)
        b.stash_iteration(loss)
        inds = b.stash[0].flatten()
        assert inds.unique().numel() == inds.numel() == 27 * 8
    assert int((a.log_counter != 0).sum()) == 27 * 8
    assert torch.equal(a.log_buffer, b.log_buffer) and torch.equal(a.log_counter, b.log_counter)
    assert torch.equal(a.get_mask(), b.get_mask())


def test_a_chained_query_reaches_the_parameters_through_the_moved_points(dev):
    """p' = p + (0, flow12(p)), then the flow at p', both under the controller's mask.  The gates of each query are the kernel's (a raw
    forward at p and at the kernel's p'), the masks constants of each restatement, taken at the restatement's own points"""
    from sin_inn_amd import flownet
    c, ctl = ramped_controller('PRBF', dev)
    n = N_SCATTER
    poses = scattered(n, dev)
    up = torch.randn(n, 4, generator=torch.Generator().manual_seed(11)).to(dev)
    leaves = [p for lin in c.net.linears() for p in (lin.weight, lin.bias)]
    for q in leaves:
        q.grad = None
    p = poses.clone().requires_grad_(True)
    moved = []

    def query(x):
        moved.append(x.detach())
        return ctl(x, pose_grad=True)

    chained(query, p).backward(up)
    got = [q.grad.clone() for q in leaves] + [p.grad.clone()]
    for q in leaves:
        q.grad = None
    m = ctl.device_grid(dev)
    gates = []
    for x in moved:
        _, saved = flownet.flownet_forward_spatial_points(c.net, x.contiguous(), 1.0, True, m.tensor, m.res, m.centre_scale, m.k_active)
        gates.append([saved[l, :n] > 0 for l in range(3)])
    ref = {}
    for dt in (F64, F32):
        w = [t.to(dt).requires_grad_(True) for t in c.weights]
        x = poses.to(dt).requires_grad_(True)
        calls = iter(gates)
        o = chained(lambda y: restate_points('PRBF', c.bufs, w, y, dt, interp_mask(m.tensor, m.res, y.detach().float(), dt), next(calls)), x)
        ref[dt] = torch.autograd.grad((o * up.to(dt)).sum(), w + [x])
    for nm, g, r64, r32 in zip(GNAMES + ['g_poses'], got, ref[F64], ref[F32]):
        check_unit(f'PRBF chained under the spatial controller {nm}', g, r64, r32)
    # without the first query's pose gradient the parameters see the second query only
    chained(lambda x: ctl(x.detach()), poses).backward(up)
    assert relmax(leaves[0].grad, ref[F64][0]) > MULT * relmax(ref[F32][0], ref[F64][0])
    for q in leaves:
        q.grad = None


# ---- 5 ----
@pytest.mark.parametrize('cycle', [False, True])
def test_fit_points_under_the_spatial_controller_end_to_end(dev, cycle):
    from sin_inn_amd import flownet, progressive
    sys.path.insert(0, os.path.join(ROOT, 'tools'))
    import fit_flow
    info = {}
    fused = fit_flow.fit_points('PRBF', 2048, 30, composed=False, info=info, cycle=cycle, controller='spatial', res=3)
    comp = fit_flow.fit_points('PRBF', 2048, 30, composed=True, cycle=cycle, controller='spatial', res=3)
    assert info['progress'] == 1 and info['net'].cur_block == 12
    first = info['first']
    net0 = flownet.PRBFModel(flownet.ModelParams()).to(dev)
    net0.load_state_dict({k[len('model.'):]: v for k, v in first['state'].items() if k.startswith('model.')})
    grid = progressive.StashedSpatialController(net0, 3).get_mask()
    bufs, weights = net_tensors(net0, dev)
    with torch.no_grad():
        query = lambda x: restate_points('PRBF', bufs, weights, x, F64, interp_mask(grid, 3, x.float(), F64))  # noqa: E731
        p64 = first['poses'].to(F64)
        out = query(p64)
        loss64 = float((out - first['target'].to(F64)).pow(2).mean() + (fit_flow.cycle_term(query, p64, out) if cycle else 0.0))
    print(f'cycle={cycle} step 0: float64 {loss64:.9f}  fused off by {abs(fused[0] - loss64) / loss64:.3g}  composed off by '
          f'{abs(comp[0] - loss64) / loss64:.3g} (relative; bound 1e-4)   final: fused {fused[-1]:.6f} composed {comp[-1]:.6f}')
    assert abs(fused[0] - loss64) <= 1e-4 * loss64 and abs(comp[0] - loss64) <= 1e-4 * loss64
    assert fused[-1] < fused[0] and comp[-1] < comp[0]
