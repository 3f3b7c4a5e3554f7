"""GPU: the SPATIAL mode of the flow-field network kernels (csrc/flownet.hip): a per-point mask interpolated from a grid
[res^3][515], for PRBF, PFF, PRFF and PRBFG, with the method and the budget of tests/test_gpu_flownet.py unchanged: error against float64
<= min(4 x the deviation of the same formula in fp32 torch, measured here, 1e-4), max-norm relative to max |ref|, gradients with the
kernel's own gates forced, no element excluded.  The reference is tests/flownet_spatial_refs.py (cells and weights in fp32 on the
CPU as the reference computes them, the weighted sum and the network in float64), which tests/test_flownet_spatial_golden.py ties to
the reference's own progressive_controller.py.

Grids of points: `fixture` (t = 2, 20 x 28) and `ragged` (t = 3, 109 x 253: 64-point tiles wrap rows and frames) of
tests/test_gpu_flownet.py.  Mask grids at res 7: `init`, the controller's first grid; `mid`, the controller after five blocks with the
cells of one side closed by update_progress and the block in progress at 0.75; `random`, uniform in [0, 1] in the first 200 columns.
One forward-only case at res 50 (125 000 rows of 2060 bytes: the large strides).

sample_mask bound: 4e-6 absolute: 8 products and 7 adds of non-negative terms that total at most 2, each within 2^-24 relative.
"""
import os
import sys

import pytest
import torch

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from flownet_refs import is_plus_zero, nan_buffers, net_tensors, poses_of, restate  # noqa: E402
from flownet_spatial_refs import cells, interp_mask, restate_spatial  # noqa: E402
from test_gpu_flownet import F64, GRIDS, axes, check  # noqa: E402

NETS = {'PRBF': 404, 'PFF': 505, 'PRFF': 707, 'PRBFG': 808}
PGRIDS = ('fixture', 'ragged')
KINDS = ('init', 'mid', 'random')
SCALE, RES, MASK_TOL = 3.0, 7, 4e-6
GNAMES = [f'g{k}{l}' for l in (1, 2, 3, 4) for k in ('W', 'b')]
_cache = {}


@pytest.fixture(scope='module')
def dev():
    import sin_inn_amd  # noqa: F401
    assert torch.cuda.is_available(), 'GPU tests need a GPU'
    return torch.device('cuda', 0)


def build(name, dev):
    from sin_inn_amd import flownet
    torch.manual_seed(NETS[name])
    return flownet.all_model_dict[name](flownet.ModelParams()).to(dev)


def mask_grid(kind, dev):
    """(grid (343, 515) on the device, k_active); made once, never modified"""
    if kind in _cache:
        return _cache[kind]
    from sin_inn_amd import progressive
    if kind == 'random':
        g = torch.rand(RES ** 3, 515, generator=torch.Generator().manual_seed(5)).to(dev)
        g[:, 200:] = 0
        out = (g, 200)
    else:
        ctl = progressive.StashedSpatialController(build('PRBF', dev), RES, block_iterations=8)
        if kind == 'mid':
            pts = poses_of(*axes(((0.3,), 8, 12), dev), torch.float32)
            loss = torch.where(pts[:, 2] > 0.8, 1.0, 1e-6)

            def rounds(n):
                for _ in range(n):
                    ctl.interpolate(pts)
                    ctl.stash_iteration(loss)
            for _ in range(5):
                rounds(8)
                ctl.update_progress()
            rounds(3)
            closed = int((~ctl.in_progress).sum())
            assert 0 < closed < RES ** 3 and ctl.next_block == 42
        out = (ctl.get_mask().clone(), ctl.k_active)
        assert bool((out[0][:, out[1]:] == 0).all())
    _cache[kind] = out
    return out


def reference_mask(grid, res, times, ys, xs):
    return interp_mask(grid, res, poses_of(times, ys, xs, torch.float32))


@pytest.mark.parametrize('kind', KINDS)
@pytest.mark.parametrize('pgrid', PGRIDS)
def test_sample_mask(dev, pgrid, kind):
    from sin_inn_amd import flownet
    net = build('PRBF', dev)
    times, ys, xs = axes(GRIDS[pgrid], dev)
    grid, _ = mask_grid(kind, dev)
    got = flownet.flownet_sample_mask(net, times, ys, xs, grid, RES)
    again = flownet.flownet_sample_mask(net, times, ys, xs, grid, RES)
    ref = reference_mask(grid, RES, times, ys, xs)
    err = float((got.double() - ref).abs().max())
    print(f'sample_mask {pgrid} {kind}: max abs error {err:.3g} (bound {MASK_TOL:g}), max mask {float(ref.max()):.3g}')
    assert tuple(got.shape) == (times.numel() * ys.numel() * xs.numel(), 515) and torch.equal(got, again)
    assert err <= MASK_TOL


def test_sample_mask_and_forward_at_res_50(dev):
    """125 000 grid rows: row offsets up to 6.4e7 floats"""
    from sin_inn_amd import flownet
    net = build('PRBF', dev)
    bufs, weights = net_tensors(net, dev)
    times, ys, xs = axes(GRIDS['fixture'], dev)
    grid = torch.rand(50 ** 3, 515, generator=torch.Generator().manual_seed(6)).to(dev)
    got = flownet.flownet_sample_mask(net, times, ys, xs, grid, 50)
    ref = reference_mask(grid, 50, times, ys, xs)
    err = float((got.double() - ref).abs().max())
    print(f'sample_mask res 50: max abs error {err:.3g}')
    assert err <= MASK_TOL
    flows, _ = flownet.flownet_forward_spatial(net, times, ys, xs, SCALE, False, grid, 50)
    with torch.no_grad():
        ref64 = restate_spatial('PRBF', bufs, weights, times, ys, xs, SCALE, F64, ref)
        ref32 = restate_spatial('PRBF', bufs, weights, times, ys, xs, SCALE, torch.float32, ref.float())
    check('PRBF fixture res 50 flows', flows, ref64, ref32)


def test_out_of_range_time_reads_the_edge_cell(dev):
    """times outside [-1, 1]: the reference would raise an index error, the kernels clamp every corner index to the grid.  The
    expectation is built here from the clamped indices and the unclamped weights; bound: 4e-6 per unit of sum |weight|"""
    from sin_inn_amd import flownet
    net = build('PRBF', dev)
    times, ys, xs = axes(((-1.9, 2.4), 9, 11), dev)
    grid, ka = mask_grid('random', dev)
    p = poses_of(times, ys, xs, torch.float32).cpu()
    u = ((p + 1) / 2) * (RES - 2) + .5
    lo, hi = torch.floor(u), torch.ceil(u + 1e-6)
    assert float(lo.min()) < 0 and float(hi.max()) > RES - 1
    a, i = (hi - u, u - lo), (lo.clamp(0, RES - 1).long(), hi.clamp(0, RES - 1).long())
    ref = torch.zeros(p.shape[0], 515, dtype=F64)
    wsum = torch.zeros(p.shape[0], dtype=F64)
    g = grid.cpu().double()
    for c in range(8):
        s = ((c >> 2) & 1, (c >> 1) & 1, c & 1)
        w = (a[s[0]][:, 0] * a[s[1]][:, 1]) * a[s[2]][:, 2]
        ref += w.double()[:, None] * g[i[s[0]][:, 0] + i[s[1]][:, 1] * RES + i[s[2]][:, 2] * RES * RES]
        wsum += w.double().abs()
    got = flownet.flownet_sample_mask(net, times, ys, xs, grid, RES).cpu().double()
    err = float(((got - ref).abs() / wsum.clamp(min=1.0)[:, None]).max())
    print(f'out-of-range time: max abs error per unit weight {err:.3g}')
    assert err <= MASK_TOL
    flows, _ = flownet.flownet_forward_spatial(net, times, ys, xs, SCALE, False, grid, RES, k_active=ka)
    assert bool(torch.isfinite(flows).all())


@pytest.mark.parametrize('pgrid', PGRIDS)
@pytest.mark.parametrize('name', ['PRBF', 'PFF'])
def test_constant_grid_is_the_global_mask(dev, name, pgrid):
    """a grid whose every row is one global vector v: the interpolated mask is v times the sum s(p) of the point's eight weights.
    s = 1 to rounding, except where a coordinate lies within 1e-6 below a cell boundary: there a0 + a1 = 2 in the reference (a quirk
    the kernels keep) and the mask is 2 v.  Every point of the fixture grid has s = 1 (asserted), and there the flows are those of
    the existing global-mask path within the budget, not bitwise (the operand is masked, not the weight).  The ragged grid has
    such points (max s = 2), so its reference is the global restatement under v s(p), all points, and the
    comparison with the global-mask kernel is made on the fixture grid."""
    from sin_inn_amd import flownet
    net = build(name, dev)
    bufs, weights = net_tensors(net, dev)
    times, ys, xs = axes(GRIDS[pgrid], dev)
    v = torch.zeros(515)
    v[:84], v[84:90] = 1.0, 0.5
    v = v.to(dev)
    grid = v[None, :].repeat(RES ** 3, 1).contiguous()
    s = cells(poses_of(times, ys, xs, torch.float32), RES)[1].double().sum(1).to(dev)
    print(f'{name} {pgrid}: sum of weights in [{float(s.min()):.7f}, {float(s.max()):.7f}]')
    spatial, _ = flownet.flownet_forward_spatial(net, times, ys, xs, SCALE, False, grid, RES, k_active=90)
    m64 = v.double()[None, :] * s[:, None]
    with torch.no_grad():
        ref64 = restate_spatial(name, bufs, weights, times, ys, xs, SCALE, F64, m64)
        ref32 = restate_spatial(name, bufs, weights, times, ys, xs, SCALE, torch.float32, m64.float())
    check(f'{name} {pgrid} constant grid', spatial, ref64, ref32)
    if pgrid == 'fixture':
        assert float((s - 1).abs().max()) < 1e-6
        glob, _ = flownet.flownet_forward(net, times, ys, xs, SCALE, False, mask=v, k_active=90)
        with torch.no_grad():
            g64 = restate(name, bufs, weights, times, ys, xs, SCALE, F64, v)
            g32 = restate(name, bufs, weights, times, ys, xs, SCALE, torch.float32, v)
        check(f'{name} global path', glob, g64, g32)
        check(f'{name} constant grid vs the global mask', spatial, g64, g32)


@pytest.mark.parametrize('kind', KINDS)
@pytest.mark.parametrize('pgrid', PGRIDS)
@pytest.mark.parametrize('name', list(NETS))
def test_forward_and_backward_against_float64(dev, name, pgrid, kind):
    from sin_inn_amd import flownet
    net = build(name, dev)
    bufs, weights = net_tensors(net, dev)
    fourier = name == 'PRFF'
    enc_a = net.encode.effective_frequencies().detach().contiguous() if fourier else None
    if fourier:
        bufs = enc_a
    times, ys, xs = axes(GRIDS[pgrid], dev)
    n = times.numel() * ys.numel() * xs.numel()
    grid, ka = mask_grid(kind, dev)
    tag = f'{name} {pgrid} {kind}'
    m64 = reference_mask(grid, RES, times, ys, xs)
    m32 = m64.float()

    # ---- forward, both modes, skipped and unskipped ----
    saved, ws, ews = nan_buffers(n, dev)
    infer, none = flownet.flownet_forward_spatial(net, times, ys, xs, SCALE, False, grid, RES, k_active=ka, enc_a=enc_a)
    assert none is None
    train, saved = flownet.flownet_forward_spatial(net, times, ys, xs, SCALE, True, grid, RES, k_active=ka, saved=saved, enc_a=enc_a)
    assert torch.equal(infer, train)
    assert bool(torch.isfinite(saved).all()) and float(saved.min()) >= 0.0
    full, saved_full = flownet.flownet_forward_spatial(net, times, ys, xs, SCALE, True, grid, RES, k_active=515, enc_a=enc_a)
    assert torch.equal(full, infer), 'skipping the closed features changed the flows'
    assert torch.equal(saved_full, saved)
    with torch.no_grad():
        ref64 = restate_spatial(name, bufs, weights, times, ys, xs, SCALE, F64, m64)
        ref32 = restate_spatial(name, bufs, weights, times, ys, xs, SCALE, torch.float32, m32)
    check(f'{tag} flows', infer, ref64, ref32)
    del ref64, ref32, full, saved_full

    # ---- backward with the gates the kernel took ----
    gates = [saved[l, :n] > 0 for l in range(3)]
    up = torch.randn(infer.shape, generator=torch.Generator().manual_seed(11)).to(dev)
    grads_ref = {}
    for dtype, m in ((F64, m64), (torch.float32, m32)):
        w = [p.to(dtype).requires_grad_(True) for p in weights]
        leaves = w + ([bufs.to(dtype).requires_grad_(True)] if fourier else [])
        flows = restate_spatial(name, leaves[8] if fourier else bufs, w, times, ys, xs, SCALE, dtype, m, gates)
        grads_ref[dtype] = torch.autograd.grad((flows * up.to(dtype)).sum(), leaves)
        del flows
    kw = dict(workspace=ws, enc_a=enc_a, enc_grad=fourier, enc_workspace=ews if fourier else None)

    def backward(k_active):
        out = flownet.flownet_backward_spatial(net, times, ys, xs, SCALE, up, saved, grid, RES, k_active=k_active, **kw)
        return list(out[0]) + [out[1]] if fourier else out

    got = backward(ka)
    again = backward(ka)
    ws.fill_(float('nan'))
    ews.fill_(float('nan'))
    unskipped = backward(515)
    assert tuple(got[0].shape) == (256, 515)
    names = GNAMES + (['g_enc_a'] if fourier else [])
    for nm, a, b, c in zip(names, got, again, unskipped):
        assert bool(torch.isfinite(a).all()), nm
        assert torch.equal(a, b), f'{nm}: two backward calls differ'
        assert torch.equal(a, c), f'{nm}: the skipped and the unskipped path differ'
    closed = (grid == 0).all(dim=0)
    assert bool(closed[ka:].all()) and int(closed.sum()) >= 515 - ka
    for g in (got[0], unskipped[0]):
        assert is_plus_zero(g[:, closed]), 'gW1 of an all-zero grid column is not +0'
    assert bool((got[0][:, :3] != 0.0).any(dim=0).all()), 'a coordinate column of gW1 is all zero'
    if fourier:
        fclosed = closed[3::2] & closed[4::2]
        assert is_plus_zero(got[8][:, fclosed]) and bool((got[8][:, ~fclosed] != 0).any())
    for nm, g, r64, r32 in zip(names, got, grads_ref[F64], grads_ref[torch.float32]):
        check(f'{tag} {nm}', g, r64, r32)
    check(f'{tag} gW1 coordinate columns', got[0][:, :3], grads_ref[F64][0][:, :3], grads_ref[torch.float32][0][:, :3])


def test_flow_fields_controller_override_and_get_mask(dev):
    from sin_inn_amd import flownet, progressive
    net = build('PFF', dev)
    ctl = progressive.StashedSpatialController(net, RES, block_iterations=8)
    times = torch.tensor([0.0, 0.5], device=dev)
    _, ys, xs = axes(GRIDS['fixture'], dev)
    up = torch.randn(2, 4, 20, 28, generator=torch.Generator().manual_seed(11)).to(dev)
    params = [p for lin in net.linears() for p in (lin.weight, lin.bias)]

    def run(target, **kw):
        for p in params:
            p.grad = None
        f12, f21 = flownet.flow_fields(target, times, 20, 28, SCALE, **kw)
        assert f12.shape == (2, 2, 20, 28) and f12.requires_grad
        (f12 * up[:, :2]).sum().add((f21 * up[:, 2:]).sum()).backward()
        return torch.cat((f12, f21), 1).detach(), [p.grad.clone() for p in params]

    for i in range(3):                                   # the block in progress ramps to 0.75
        flownet.flow_fields(ctl, times, 20, 28, SCALE)
        ctl.stash_iteration(torch.full((2 * 20 * 28,), 0.5, device=dev))
    assert ctl.iteration == 3 and tuple(ctl.stash[0].shape) == (1120, 8) and ctl.k_active == 12
    own_f, own_g = run(ctl)                              # k_active = next_block
    over_f, over_g = run(net, override_mask=ctl.get_mask().clone())   # a raw grid: all 515 features
    assert torch.equal(own_f, over_f)
    for nm, a, b in zip(GNAMES, own_g, over_g):
        assert torch.equal(a, b), nm
    direct, _ = flownet.flownet_forward_spatial(net, times, ys, xs, SCALE, False, ctl.get_mask(), RES, k_active=12)
    assert torch.equal(direct, own_f)
    assert is_plus_zero(own_g[0][:, 12:]) and bool((own_g[0][:, :12] != 0).any(dim=0).all())
    with torch.no_grad():
        g12, g21, m = flownet.flow_fields(ctl, times, 20, 28, SCALE, get_mask=True)
    assert not g12.requires_grad and torch.equal(torch.cat((g12, g21), 1), own_f)
    assert torch.equal(m, flownet.flownet_sample_mask(net, times, ys, xs, ctl.get_mask(), RES))
    assert float((m - ctl.interpolate(poses_of(times, ys, xs, torch.float32))).abs().max()) <= 2 * MASK_TOL
    # backward through an inference-mode forward, and after the grid moved on
    with torch.no_grad():
        i12, _ = flownet.flow_fields(ctl, times, 20, 28, SCALE)
    assert not i12.requires_grad
    f12, f21 = flownet.flow_fields(ctl, times, 20, 28, SCALE)
    ctl.stash_iteration(torch.full((1120,), 0.5, device=dev))
    ctl.get_mask()
    with pytest.raises(RuntimeError, match='changed between'):
        f12.sum().backward()
    with pytest.raises(RuntimeError, match='PPE'):
        flownet.flow_fields(build_ppe(dev), times, 20, 28, SCALE, override_mask=torch.ones(RES ** 3, 27, device=dev))


def build_ppe(dev):
    from sin_inn_amd import flownet
    torch.manual_seed(1)
    return flownet.PPEModel(flownet.ModelParams()).to(dev)


def test_fit_flow_spatial_controller(dev):
    """30 steps of tools/fit_flow.py --net PRBF --controller spatial --res 7 at 32 x 48: the loss falls and update_progress runs"""
    sys.path.insert(0, os.path.join(ROOT, 'tools'))
    import fit_flow
    info = {}
    losses = fit_flow.fit('PRBF', 32, 48, 30, controller='spatial', res=7, info=info)
    ctl = info['net']
    print(f'first {losses[0]:.6f} last {losses[-1]:.6f}; update_progress x {info["progress"]}, open {ctl.cur_block} / 515, '
          f'cells in progress {int(ctl.in_progress.sum())} / {RES ** 3}')
    assert losses[-1] < losses[0] and info['progress'] >= 1 and ctl.cur_block == 12 and ctl.next_block == 18
