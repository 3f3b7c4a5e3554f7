"""GPU: the flow networks at arbitrary points (sin_inn_amd.flownet.flow_at, net(poses), controller(poses); sininn_flownet_*_points /
sininn_siren_*_points).  The mode adds no kernel: point_coord (csrc/flownet_tile.h) reads row p of the pose list where the grid mode reads
the three axis vectors, so the central tests are EXACT comparisons with the grid path, not tolerances.

  1. a pose list that spells out the grid (2, 20, 28) (1120 points: 17 full tiles and a ragged one), built as the reference builds it,
     gives bitwise the grid call's flows and parameter gradients (RFF: and g_enc_a), for RBF, FFN, RBFG, PE, RFF, PRBF under a
     LinearControllerEarly stopped mid-ramp (mask entries of 0.25, k_active = 12), PPE under its controller, and siren; `saved` and the
     workspaces are NaN before every call;
  2. tile edges: N in {1, 64, 65} on the same leading points give the same flows, bitwise;
  3. a point's value does not depend on where it stands in the list (N = 1000, a fixed permutation), bitwise;
  4. scattered points (N = 1000, uniform in [-1, 1]^3, on no grid) against the float64 restatement of tests/flownet_points_refs.py, flows
     and all gradients with the kernel's own gates forced, by the budget method of tests/test_gpu_flownet.py unchanged (its `check`):
     budget = min(4 x the deviation of the fp32 torch evaluation from float64, measured here, 1e-4), max-norm relative to max |ref|;
  5. two backward calls are bitwise equal (NaN-filled buffers before each), any valid k_active gives the bits of 515;
  6. the surface: net(poses), leading dimensions, planar, controller(poses, get_mask= / override_mask=), no_grad, autograd;
  7. end to end: tools/fit_flow.fit_points fused against composed.

The loss of point 7: a scalar has no max-norm, and the deviation of ONE fp32 number from float64 can be zero by chance, which would make
"4 units" an equality; so the unit is measured where point 4 measures it, on the flows of the first step's points (fp32 torch against
float64, max-norm relative to max |flows64|), B = min(4 unit, 1e-4), and carried to the loss L = mean((o - y)^2): flows within
d = B max |o64| of o64 move L by at most 2 mean|o64 - y| d + d^2 <= 2 sqrt(L64) d + d^2 (Cauchy-Schwarz).  On top come the roundings of
the fp32 loss itself (y is fp32 already; a subtraction, a square and a pairwise mean: 4 eps32 relative at most) -- 2^-22 L64.  Both loops
must be within that of the float64 loss; never more than 1e-4 L64, the bound of the other end-to-end tests.

Measured on an MI355X (`ratio(...)` lines of a run with -s: error / budget); the table is in DESIGN 14.7.
"""
import ctypes as C
import os
import sys

import pytest
import torch

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from flownet_points_refs import grid_poses, reference_grads_points, restate_points, siren_restate_points  # noqa: E402
from flownet_refs import nan_buffers, nan_saved, nan_workspace, net_tensors  # noqa: E402
from siren_refs import siren_tensors  # noqa: E402
from test_gpu_flownet import CEIL, F64, MULT, SCALE, check, relmax  # noqa: E402

F32 = torch.float32
NAN = float('nan')
NETS = ('RBF', 'FFN', 'RBFG', 'PE', 'RFF', 'PRBF', 'PPE', 'siren')
SEED = {name: 1100 + 7 * i for i, name in enumerate(NETS)}
TIMES, GH, GW = (0.0, 0.5), 20, 28
N_SCATTER = 1000                                       # 15 tiles + 40
_cache = {}


@pytest.fixture(scope='module')
def dev():
    import sin_inn_amd  # noqa: F401
    assert torch.cuda.is_available(), 'GPU tests need a GPU'
    return torch.device('cuda', 0)


class Case:
    """a network on the device, the controller it runs under (progressive ones: LinearControllerEarly one iteration into its first
    ramp, the block in progress at 0.25), and what its low-level calls take"""

    def __init__(self, name, dev):
        from sin_inn_amd import flownet, progressive
        torch.manual_seed(SEED[name])
        self.name, self.dev = name, dev
        self.net = flownet.flow_model_dict[name](flownet.ModelParams()).to(dev)
        self.siren = name == 'siren'
        self.target, self.hmask, self.kw = self.net, None, {}
        if self.net.is_progressive:
            self.target = progressive.LinearControllerEarly(self.net, 1000, epsilon=1e-3)
            self.target.stash_iteration(torch.tensor(0.5))
            self.hmask = self.target.mask.clone()
            m = self.target.device_mask(dev)
            width = self.net.encoding_dim
            assert 0 < m.k_active < width and bool(((self.hmask > 0) & (self.hmask < 1)).any()), 'a mask stopped mid-ramp'
            self.kw = dict(mask=m.tensor, k_active=m.k_active)
        self.learnable = name == 'RFF'
        if self.learnable:
            self.kw['enc_a'] = self.net.encode.effective_frequencies().detach().contiguous()
        self.params = [p for lin in self.net.linears() for p in (lin.weight, lin.bias)]

    def nan(self, n):
        """(saved, workspace[, the frequency gradient's workspace]) for n points, all NaN"""
        from sin_inn_amd import _lib
        if self.siren:
            lib = _lib.lib()
            return (torch.full((lib.sininn_siren_saved_bytes(n) // 4,), NAN, device=self.dev),
                    torch.full((lib.sininn_siren_workspace_bytes(n) // 4,), NAN, device=self.dev))
        return nan_buffers(n, self.dev) if self.learnable else (nan_saved(n, self.dev), nan_workspace(n, self.dev))

    def forward_points(self, poses, saved=None, train=True, **over):
        from sin_inn_amd import flownet
        fn = flownet.siren_forward_points if self.siren else flownet.flownet_forward_points
        return fn(self.net, poses, SCALE, train, saved, **{**self.kw, **over})

    def backward_points(self, poses, up, saved, ws, ews=None, **over):
        """the gradients as one list: gW1, gb1, .. and (RFF) gF last"""
        from sin_inn_amd import flownet
        if self.siren:
            return flownet.siren_backward_points(self.net, poses, SCALE, up, saved, ws)
        if self.learnable:
            grads, gF = flownet.flownet_backward_points(self.net, poses, SCALE, up, saved, ws, enc_grad=True, enc_workspace=ews,
                                                        **{**self.kw, **over})
            return grads + [gF]
        return flownet.flownet_backward_points(self.net, poses, SCALE, up, saved, ws, **{**self.kw, **over})

    def forward_grid(self, times, ys, xs, saved):
        from sin_inn_amd import flownet
        fn = flownet.siren_forward if self.siren else flownet.flownet_forward
        return fn(self.net, times, ys, xs, SCALE, True, saved, **self.kw)

    def backward_grid(self, times, ys, xs, up, saved, ws, ews=None):
        from sin_inn_amd import flownet
        if self.siren:
            return flownet.siren_backward(self.net, times, ys, xs, SCALE, up, saved, ws)
        if self.learnable:
            grads, gF = flownet.flownet_backward(self.net, times, ys, xs, SCALE, up, saved, ws, enc_grad=True, enc_workspace=ews, **self.kw)
            return grads + [gF]
        return flownet.flownet_backward(self.net, times, ys, xs, SCALE, up, saved, ws, **self.kw)

    def names(self):
        nl = 5 if self.siren else 4
        return [f'g{k}{l}' for l in range(1, nl + 1) for k in ('W', 'b')] + (['gF'] if self.learnable else [])


def case(name, dev):
    if name not in _cache:
        _cache[name] = Case(name, dev)
    return _cache[name]


def scattered(n, dev, seed=5):
    return (torch.rand(n, 3, generator=torch.Generator().manual_seed(seed)) * 2 - 1).to(dev)


def grid(dev):
    return torch.tensor(TIMES, device=dev), torch.linspace(-1, 1, GH).to(dev), torch.linspace(-1, 1, GW).to(dev)


# ---- 1 ----
@pytest.mark.parametrize('name', NETS)
def test_a_grid_spelled_out_as_poses_gives_the_grid_path_bitwise(dev, name):
    from sin_inn_amd import flownet
    c = case(name, dev)
    times, ys, xs = grid(dev)
    n = times.numel() * GH * GW
    poses = grid_poses(times, ys, xs)
    assert poses.shape == (n, 3) and poses.is_contiguous() and n % 64 != 0 and n // 64 == 17
    # the public surface
    with torch.no_grad():
        f12, f21 = flownet.flow_fields(c.target, times, GH, GW, SCALE)
        at = flownet.flow_at(c.target, poses, SCALE)
    assert at.shape == (n, 4) and at.is_contiguous()
    assert torch.equal(at.view(len(TIMES), GH, GW, 4).permute(0, 3, 1, 2), torch.cat((f12, f21), 1))
    # the calls themselves, every buffer NaN before them
    up = torch.randn(len(TIMES), 4, GH, GW, generator=torch.Generator().manual_seed(11)).to(dev)
    up_planar = up.permute(1, 0, 2, 3).reshape(4, n)
    bufs_g, bufs_p = c.nan(n), c.nan(n)
    flows_g, saved_g = c.forward_grid(times, ys, xs, bufs_g[0])
    flows_p, saved_p = c.forward_points(poses, bufs_p[0])
    assert flows_p.shape == (4, n) and torch.equal(flows_p.view(4, len(TIMES), GH, GW).permute(1, 0, 2, 3), flows_g)
    assert torch.equal(flows_g, torch.cat((f12, f21), 1))
    assert bool(torch.isfinite(saved_p).all()) and torch.equal(saved_p, saved_g)
    got_g = c.backward_grid(times, ys, xs, up, saved_g, *bufs_g[1:])
    got_p = c.backward_points(poses, up_planar, saved_p, *bufs_p[1:])
    assert len(got_g) == len(got_p) == len(c.names())
    for nm, g, p in zip(c.names(), got_g, got_p):
        assert bool(torch.isfinite(p).all()), nm
        assert torch.equal(g, p), f'{name} {nm}: points and grid differ'
    # and through autograd on both sides, the same upstream gradient
    leaves = c.params + ([c.net.encode.frequencies] if c.learnable else [])
    for p in leaves:
        p.grad = None
    f12, f21 = flownet.flow_fields(c.target, times, GH, GW, SCALE)
    torch.autograd.backward([f12, f21], [up[:, :2], up[:, 2:]])
    want = [p.grad.clone() for p in leaves]
    for p in leaves:
        p.grad = None
    flownet.flow_at(c.target, poses, SCALE).backward(up.permute(0, 2, 3, 1).reshape(n, 4))
    for i, (p, w) in enumerate(zip(leaves, want)):
        assert torch.equal(p.grad, w), f'{name} leaf {i}'
        p.grad = None


# ---- 2 ----
@pytest.mark.parametrize('name', ['RBF', 'siren'])
def test_tile_edges(dev, name):
    c = case(name, dev)
    poses = scattered(65, dev)
    f65, _ = c.forward_points(poses, train=False)
    f64, _ = c.forward_points(poses[:64].contiguous(), train=False)
    f1, _ = c.forward_points(poses[:1].contiguous(), train=False)
    assert f65.shape == (4, 65) and f64.shape == (4, 64) and f1.shape == (4, 1)
    assert bool(torch.isfinite(f65).all())
    assert torch.equal(f65[:, :64], f64) and torch.equal(f1[:, 0], f64[:, 0])


# ---- 3 ----
@pytest.mark.parametrize('name', ['RBF', 'PRBF', 'siren'])
def test_a_value_does_not_depend_on_the_position_in_the_list(dev, name):
    from sin_inn_amd import flownet
    c = case(name, dev)
    poses = scattered(N_SCATTER, dev)
    perm = torch.randperm(N_SCATTER, generator=torch.Generator().manual_seed(3)).to(dev)
    with torch.no_grad():
        a = flownet.flow_at(c.target, poses[perm], SCALE)
        b = flownet.flow_at(c.target, poses, SCALE)[perm]
    assert a.shape == (N_SCATTER, 4) and torch.equal(a, b)


# ---- 4 ----
@pytest.mark.parametrize('name', NETS)
def test_scattered_points_against_float64(dev, name):
    c = case(name, dev)
    n = N_SCATTER
    poses = scattered(n, dev)
    bufs = c.nan(n)
    infer, none = c.forward_points(poses, train=False)
    flows, saved = c.forward_points(poses, bufs[0])
    assert none is None and torch.equal(infer, flows) and bool(torch.isfinite(saved).all())
    up = torch.randn(4, n, generator=torch.Generator().manual_seed(11)).to(dev)
    if c.siren:
        ebufs, weights, gates = None, siren_tensors(c.net, dev), None
    else:
        ebufs, weights = net_tensors(c.net, dev)
        if c.learnable:
            ebufs = c.kw['enc_a']                      # the fp32 matrix the kernels receive
        gates = [saved[l, :n] > 0 for l in range(3)]   # the decisions the kernel took
    mask = c.hmask.to(dev) if c.hmask is not None else None
    with torch.no_grad():
        if c.siren:
            ref64, ref32 = (siren_restate_points(weights, poses, SCALE, dt) for dt in (F64, F32))
        else:
            ref64, ref32 = (restate_points(name, ebufs, weights, poses, SCALE, dt, mask) for dt in (F64, F32))
    check(f'{name} points flows', flows, ref64, ref32)                       # free gates: ReLU is continuous
    ref = reference_grads_points(name, ebufs, weights, poses, SCALE, up, mask, gates)
    got = c.backward_points(poses, up, saved, *bufs[1:])
    assert len(got) == len(ref[F64][1]) == len(c.names())
    for nm, g, r64, r32 in zip(c.names(), got, ref[F64][1], ref[F32][1]):
        check(f'{name} points {nm}', g, r64, r32)


# ---- 5 ----
@pytest.mark.parametrize('name', ['RBF', 'RFF'])
def test_two_backward_calls_are_bitwise_equal(dev, name):
    c = case(name, dev)
    n = N_SCATTER
    poses = scattered(n, dev)
    up = torch.randn(4, n, generator=torch.Generator().manual_seed(11)).to(dev)
    runs = []
    for _ in range(2):
        bufs = c.nan(n)
        _, saved = c.forward_points(poses, bufs[0])
        runs.append(c.backward_points(poses, up, saved, *bufs[1:]))
    for nm, a, b in zip(c.names(), *runs):
        assert bool(torch.isfinite(a).all()) and torch.equal(a, b), nm


def test_any_valid_k_active_gives_the_bits_of_515(dev):
    c = case('PRBF', dev)
    n = N_SCATTER
    poses = scattered(n, dev)
    up = torch.randn(4, n, generator=torch.Generator().manual_seed(11)).to(dev)
    out = {}
    assert c.kw['k_active'] == 12
    for k in (12, 13, 64, 131, 515):
        saved, ws = c.nan(n)
        flows, saved = c.forward_points(poses, saved, k_active=k)
        out[k] = [flows] + c.backward_points(poses, up, saved, ws, k_active=k)
    for k in out:
        for nm, a, b in zip(['flows'] + c.names(), out[k], out[515]):
            assert torch.equal(a, b), (k, nm)


# ---- 6 ----
def test_surface(dev):
    from sin_inn_amd import flownet
    c, p, s = case('RBF', dev), case('PRBF', dev), case('siren', dev)
    poses = scattered(40, dev).view(5, 8, 3)
    for k in (c, p, s):
        with torch.no_grad():
            out = k.net(poses)
            assert out.shape == (5, 8, 4) and out.is_contiguous() and not out.requires_grad
            assert torch.equal(out, flownet.flow_at(k.net, poses, 1.0))
            assert torch.equal(out.view(-1, 4), k.net(poses.view(-1, 3)))
            planar = flownet.flow_at(k.net, poses, 1.0, planar=True)
            again = flownet.flow_at(k.net, poses, 1.0, planar=True)
        assert planar.shape == (4, 40) and torch.equal(planar.t(), out.view(-1, 4))
        assert planar.data_ptr() != again.data_ptr() and torch.equal(planar, again)
        train = flownet.flow_at(k.net, poses, 1.0)                 # training mode: the same flows, a graph behind them
        assert train.requires_grad and torch.equal(train.detach(), out)
    # the controller: its own mask (and get_mask), an override
    ctl = p.target
    out, mask = ctl(poses, get_mask=True)
    assert mask is ctl.mask and torch.equal(out, flownet.flow_at(ctl, poses, 1.0))
    assert not torch.equal(out, p.net(poses))                      # the bare model runs under all ones
    m = torch.linspace(1, 0, 515)
    with torch.no_grad():
        over, back = ctl(poses, override_mask=m, get_mask=True)
        assert back is m and torch.equal(over, flownet.flow_at(p.net, poses, override_mask=m))
        assert torch.equal(over, flownet.flow_at(ctl, poses, override_mask=m.to(dev)))
        _, used = flownet.flow_at(ctl, poses, get_mask=True)
    assert used.is_cuda and torch.equal(used.cpu(), ctl.mask)
    with pytest.raises(ValueError):
        flownet.flow_at(c.net, poses, override_mask=m)             # a mask needs a progressive network
    with pytest.raises(NotImplementedError):
        flownet.flow_at(p.net, poses, override_mask=torch.ones(27, 515, device=dev))    # a grid: per-point masks are flow_fields'


@pytest.mark.parametrize('name', ['RBF', 'RFF', 'PRBF', 'siren'])
def test_autograd_equals_the_direct_backward_call(dev, name):
    from sin_inn_amd import flownet
    c = case(name, dev)
    n = 200
    poses = scattered(n, dev, seed=9)
    up = torch.randn(n, 4, generator=torch.Generator().manual_seed(11)).to(dev)
    leaves = c.params + ([c.net.encode.frequencies] if c.learnable else [])
    for p in leaves:
        p.grad = None
    flownet.flow_at(c.target, poses, SCALE).backward(up)
    _, saved = c.forward_points(poses)
    direct = c.backward_points(poses, up.t().contiguous(), saved, None)
    if c.learnable:                                                # gF through torch's normalize backward, as flow_at carries it
        direct[-1], = torch.autograd.grad(c.net.encode.effective_frequencies(), [c.net.encode.frequencies], direct[-1])
    for nm, p, g in zip(c.names(), leaves, direct):
        assert torch.equal(p.grad, g), nm
        p.grad = None
    with torch.no_grad():
        assert not flownet.flow_at(c.target, poses, SCALE).requires_grad


# ---- 7 ----
def test_fit_points_end_to_end(dev):
    """60 steps of tools/fit_flow.fit_points('RBF', 4096) with flow_at and with the network composed from torch ops, same seed: the
    first loss of each within the bound of the module text of the float64 loss, the loss falls in both."""
    from sin_inn_amd import flownet
    sys.path.insert(0, os.path.join(ROOT, 'tools'))
    import fit_flow
    info = {}
    fused = fit_flow.fit_points('RBF', 4096, 60, composed=False, info=info)
    comp = fit_flow.fit_points('RBF', 4096, 60, composed=True)
    for s in range(5):
        print(f'step {s}: fused {fused[s]:.7f} composed {comp[s]:.7f} rel {abs(fused[s] - comp[s]) / abs(comp[s]):.3g}')
    print(f'final: fused {fused[-1]:.7f} composed {comp[-1]:.7f}')
    first = info['first']
    net0 = flownet.RbfModel(flownet.ModelParams()).to(dev)
    net0.load_state_dict(first['state'])
    bufs, weights = net_tensors(net0, dev)
    with torch.no_grad():
        o64 = restate_points('RBF', bufs, weights, first['poses'], 1.0, F64).t()
        o32 = restate_points('RBF', bufs, weights, first['poses'], 1.0, F32).t()
    unit = relmax(o32, o64)
    budget = min(MULT * unit, CEIL)
    loss64 = float((o64 - first['target'].to(F64)).pow(2).mean())
    d = budget * float(o64.abs().max())
    bound = min(2 * loss64 ** 0.5 * d + d * d + 2.0 ** -22 * loss64, CEIL * loss64)
    print(f'step 0: float64 loss {loss64:.9f}  flows unit {unit:.3g} budget {budget:.3g}  loss bound {bound:.3g} '
          f'(relative {bound / loss64:.3g})  fused off by {abs(fused[0] - loss64):.3g}  composed off by {abs(comp[0] - loss64):.3g}')
    assert abs(fused[0] - loss64) <= bound, (fused[0], loss64, bound)
    assert abs(comp[0] - loss64) <= bound, (comp[0], loss64, bound)
    assert fused[-1] < fused[0] and comp[-1] < comp[0]
