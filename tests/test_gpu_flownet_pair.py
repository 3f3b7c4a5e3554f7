"""GPU: the flow-field network kernels on TWO coordinates per point (csrc/flownet.hip, the DIM = 2 instantiations behind
sininn_flownet_*_dim; ModelParams(domain_dim=2), the networks of video-interpolation/pair_flow.py) for RBF, FFN, UFF, RBFG and their
progressive forms PRBF, PFF, PUFF, PRBFG against float64.

Shapes: the grids 1 x 1 (one point, one ragged tile), 13 x 37 (481 points: seven full tiles and a ragged one) and 7 x W just past the
forward launch's grid cap (FN_FWD_MAX_BLOCKS of csrc/flownet.hip, read from the source: cap + 3 tiles of 64 points, the last ragged, so
three blocks take a second tile), and the fixture's pose list of 37 points.

Method (that of tests/test_gpu_flownet.py):
  * the reference is `restate_at` of tests/flownet_pair_refs.py in float64 on the GPU, from the fp32 weights, buffers and poses the kernel
    received, widened; tests/test_flownet_pair_golden.py ties it to the reference's own model.py through the fixture, and at the fixture's
    pose list the kernel is also compared with the fixture's stored outputs directly;
  * the unit of error is the deviation of the same formula in fp32 torch from float64 on the same inputs, measured in the test, max-norm
    relative to max |ref|; the kernel is allowed MULT = 4 units and never more than 1e-4;
  * gradients are taken with FORCED gates, `saved > 0`, in the float64 reference and in the fp32 unit alike.  No element is excluded;
  * progressive networks run under the fixture's `mask_ramp` (a block in progress at 0.8) with the k_active a controller would pass;
  * bitwise: inference forward == training forward; two backward calls with `saved` and the workspace filled with NaN first; a pose list
    that spells out the grid == the grid call, flows and gradients; every k_active == the unskipped call.

Measured on an MI355X (`ratio(...)` lines of a run with -s: error / budget): see DESIGN 14.11.
"""
import argparse
import os
import re
import sys

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from flownet_refs import is_plus_zero, nan_saved, nan_workspace, net_tensors  # noqa: E402
from flownet_pair_refs import NETS, PROGRESSIVE, build, grid_poses, reference_grads_at, restate_at  # noqa: E402

F64 = torch.float64
MULT, CEIL, SCALE = 4.0, 1e-4, 3.0
GRAD_NAMES = [f'g{k}{l}' for l in (1, 2, 3, 4) for k in ('W', 'b')]


def forward_grid_cap():
    """the forward launch's block cap, from the host code"""
    src = open(os.path.join(ROOT, 'sin-inn_amd', 'csrc', 'flownet.hip')).read()
    m = re.search(r'constexpr int FN_FWD_MAX_BLOCKS = (\d+);', src)
    assert m and 'q.ntiles < FN_FWD_MAX_BLOCKS ? q.ntiles : FN_FWD_MAX_BLOCKS' in src
    return int(m.group(1))


def past_cap_grid():
    cap = forward_grid_cap()
    h = 7
    w = ((cap + 2) * 64 + 43) // h + 1
    n = h * w
    assert cap * 64 < (cap + 2) * 64 < n < (cap + 3) * 64 and n % 64 != 0 and n <= 300000
    return h, w


SHAPES = {'one': (1, 1), 'ragged': (13, 37), 'past_cap': None, 'list': 'poses'}


@pytest.fixture(scope='module')
def dev():
    import sin_inn_amd  # noqa: F401
    assert torch.cuda.is_available(), 'GPU tests need a GPU'
    return torch.device('cuda', 0)


@pytest.fixture(scope='module')
def gold():
    return np.load(os.path.join(ROOT, 'tests', 'golden', 'golden_flownet_pair.npz'))


def relmax(a, ref):
    a, ref = a.detach().to(F64), ref.detach().to(F64)
    err = (a - ref).abs()
    err = torch.where(torch.isfinite(a), err, torch.full_like(err, float('inf')))
    return float(err.max() / ref.abs().max())


def check(name, got, ref64, ref32):
    """error of the kernel against min(MULT * unit, CEIL); prints ratio(error / budget)"""
    unit = relmax(ref32, ref64)
    budget = min(MULT * unit, CEIL)
    err = relmax(got, ref64)
    print(f'ratio({name}) = {err / budget:.3g}   [err {err:.3g}, fp32-torch unit {unit:.3g}, budget {budget:.3g}]')
    assert err <= budget, (name, err, budget)


class Call:
    """one network at one set of points: the grid call (ys, xs) or the points call (a pose list), the same arguments either way"""

    def __init__(self, net, dev, shape=None, poses=None, mask=None, k_active=None):
        self.net, self.dev, self.kw = net, dev, dict(mask=mask, k_active=k_active)
        if poses is None:
            h, w = shape
            self.ys, self.xs = torch.linspace(-1, 1, h).to(dev), torch.linspace(-1, 1, w).to(dev)
            self.poses, self.n, self.grid = grid_poses(h, w, device=dev), h * w, (h, w)
        else:
            self.poses, self.n, self.grid = poses.to(dev).contiguous(), poses.shape[0], None

    def forward(self, train, saved=None):
        """flows as (4, N), saved"""
        from sin_inn_amd import flownet
        if self.grid:
            flows, saved = flownet.flownet_forward(self.net, None, self.ys, self.xs, SCALE, train, saved, **self.kw)
            assert tuple(flows.shape) == (1, 4, *self.grid)
            return flows.view(4, -1), saved
        flows, saved = flownet.flownet_forward_points(self.net, self.poses, SCALE, train, saved, **self.kw)
        assert tuple(flows.shape) == (4, self.n)
        return flows, saved

    def backward(self, up, saved, workspace=None):
        """up (4, N)"""
        from sin_inn_amd import flownet
        if self.grid:
            return flownet.flownet_backward(self.net, None, self.ys, self.xs, SCALE, up.view(1, 4, *self.grid), saved, workspace, **self.kw)
        return flownet.flownet_backward_points(self.net, self.poses, SCALE, up, saved, workspace, **self.kw)


def ramp_mask(gold, name, dev):
    """(the device mask, k_active, the host mask) of a progressive network, else (None, None, None)"""
    from sin_inn_amd import flownet
    if name not in PROGRESSIVE:
        return None, None, None
    host = torch.from_numpy(gold['mask_ramp']).clone()
    assert host.shape == (514,) and 0.0 < float(host[flownet.last_open(host) - 1]) < 1.0
    return host.to(dev), flownet.last_open(host), host


@pytest.mark.parametrize('shape', list(SHAPES))
@pytest.mark.parametrize('name', NETS)
def test_forward_and_backward_against_float64(dev, gold, name, shape):
    net = build(name).to(dev)
    bufs, weights = net_tensors(net, dev)
    mask, k_active, host = ramp_mask(gold, name, dev)
    if shape == 'list':
        call = Call(net, dev, poses=torch.from_numpy(gold['poses']), mask=mask, k_active=k_active)
    else:
        call = Call(net, dev, shape=past_cap_grid() if shape == 'past_cap' else SHAPES[shape], mask=mask, k_active=k_active)
    n, tag = call.n, f'{name} {shape}'

    # ---- forward, both modes ----
    infer, none = call.forward(False)
    assert none is None
    train, saved = call.forward(True, nan_saved(n, dev))
    assert torch.equal(infer, train)
    assert bool(torch.isfinite(saved).all()) and float(saved.min()) >= 0.0
    with torch.no_grad():
        ref64 = restate_at(name, bufs, weights, call.poses, SCALE, F64, mask).t()
        ref32 = restate_at(name, bufs, weights, call.poses, SCALE, torch.float32, mask).t()
    check(f'{tag} flows', infer, ref64, ref32)
    if shape == 'list':
        sfx = '' if mask is None else '_ramp'
        with torch.no_grad():
            bare = Call(net, dev, poses=call.poses, mask=None if mask is None else torch.ones(514, device=dev)).forward(False)[0]
        check(f'{tag} flows vs fixture', bare, torch.from_numpy(gold[f'{name}_out64']).to(dev).t() * SCALE,
              torch.from_numpy(gold[f'{name}_out32']).to(dev).t() * SCALE)
        if sfx:
            g64 = torch.from_numpy(gold[f'{name}_out64{sfx}']).to(dev).t() * SCALE
            assert relmax(ref64, g64) < 1e-12
    del ref64, ref32

    # ---- backward with the gates the kernel took ----
    gates = [saved[l, :n] > 0 for l in range(3)]
    up = torch.randn(4, n, generator=torch.Generator().manual_seed(11)).to(dev)
    grads_ref = reference_grads_at(name, bufs, weights, call.poses, SCALE, up.t(), mask, gates)
    ws = nan_workspace(n, dev)
    got = call.backward(up, saved, ws)
    again = call.backward(up, saved, ws)
    for nm, a, b in zip(GRAD_NAMES, got, again):
        assert bool(torch.isfinite(a).all()), nm
        assert torch.equal(a, b), f'{nm}: two backward calls differ'
    assert tuple(got[0].shape) == (256, 514 if mask is not None else 512)
    for nm, g, r64, r32 in zip(GRAD_NAMES, got, grads_ref[F64], grads_ref[torch.float32]):
        check(f'{tag} {nm}', g, r64, r32)
    if mask is not None:
        assert is_plus_zero(got[0][:, host == 0]) and float(got[0][:, host != 0].abs().max()) > 0


@pytest.mark.parametrize('name', NETS)
def test_pose_list_that_spells_out_the_grid_is_the_grid_call(dev, gold, name):
    net = build(name).to(dev)
    mask, k_active, _ = ramp_mask(gold, name, dev)
    grid = Call(net, dev, shape=SHAPES['ragged'], mask=mask, k_active=k_active)
    pts = Call(net, dev, poses=grid.poses, mask=mask, k_active=k_active)
    up = torch.randn(4, grid.n, generator=torch.Generator().manual_seed(12)).to(dev)
    fg, sg = grid.forward(True)
    fp, sp = pts.forward(True)
    assert torch.equal(fg, fp) and torch.equal(sg, sp)
    for nm, a, b in zip(GRAD_NAMES, grid.backward(up, sg), pts.backward(up, sp)):
        assert torch.equal(a, b), nm


@pytest.mark.parametrize('k', [0, 2, 3, 16, 17, 130, 513, 514])
@pytest.mark.parametrize('name', PROGRESSIVE)
def test_k_active_skips_exactly(dev, name, k):
    """a prefix mask of k entries whose last one is fractional: the call that skips from k_active = k on is bitwise the call that runs all
    514 features; gW1 is [256][514], an exact +0 where the mask is zero; its two coordinate columns against float64"""
    net = build(name).to(dev)
    bufs, weights = net_tensors(net, dev)
    host = torch.zeros(514)
    host[:k] = 1.0
    if k:
        host[k - 1] = 0.375
    mask = host.to(dev)
    skip = Call(net, dev, shape=SHAPES['ragged'], mask=mask, k_active=k)
    full = Call(net, dev, shape=SHAPES['ragged'], mask=mask, k_active=514)
    n = skip.n
    up = torch.randn(4, n, generator=torch.Generator().manual_seed(13)).to(dev)
    fs, ss = skip.forward(True, nan_saved(n, dev))
    ff, sf = full.forward(True, nan_saved(n, dev))
    assert torch.equal(fs, ff) and torch.equal(ss, sf)
    gs, gf = skip.backward(up, ss, nan_workspace(n, dev)), full.backward(up, sf, nan_workspace(n, dev))
    for nm, a, b in zip(GRAD_NAMES, gs, gf):
        assert bool(torch.isfinite(a).all()) and torch.equal(a, b), nm
    gw1 = gs[0]
    assert tuple(gw1.shape) == (256, 514)
    assert is_plus_zero(gw1[:, host == 0])
    with torch.no_grad():
        check(f'{name} k_active {k} flows', fs, restate_at(name, bufs, weights, skip.poses, SCALE, F64, mask).t(),
              restate_at(name, bufs, weights, skip.poses, SCALE, torch.float32, mask).t())
    if k:
        gates = [ss[l, :n] > 0 for l in range(3)]
        ref = reference_grads_at(name, bufs, weights, skip.poses, SCALE, up.t(), mask, gates)
        cols = min(k, 2)
        check(f'{name} k_active {k} gW1 coordinate columns', gw1[:, :cols], ref[F64][0][:, :cols], ref[torch.float32][0][:, :cols])
        check(f'{name} k_active {k} gW1', gw1, ref[F64][0], ref[torch.float32][0])


@pytest.mark.parametrize('name', ['RBF', 'UFF', 'PRBF', 'PRBFG'])
def test_public_calls_and_autograd(dev, name):
    """flow_fields(net_or_controller, None, h, w, scale) -> (1, 4, h, w) in two views; flow_at / net(poses) / controller(poses): (..., 2) ->
    (..., 4); gradients are those of the raw calls; inference mode equals training mode"""
    from sin_inn_amd import flownet, progressive
    net = build(name).to(dev)
    target = net
    kw = {}
    if net.is_progressive:
        target = progressive.LinearControllerEarly(net, 1000, epsilon=1e-3).to(dev)
        for _ in range(97):
            target.stash_iteration(torch.tensor(0.5))
        m = target.device_mask(dev)
        kw = dict(mask=m.tensor, k_active=m.k_active)
        assert m.k_active == flownet.last_open(target.mask) < 514
    h, w = SHAPES['ragged']
    f12, f21 = flownet.flow_fields(target, None, h, w, SCALE)
    assert f12.shape == (1, 2, h, w) and f21.shape == (1, 2, h, w) and f12.requires_grad
    up = torch.randn(1, 4, h, w, generator=torch.Generator().manual_seed(14)).to(dev)
    (f12 * up[:, :2]).sum().add((f21 * up[:, 2:]).sum()).backward()
    call = Call(net, dev, shape=(h, w), **kw)
    flows, saved = call.forward(True)
    assert torch.equal(flows.view(1, 4, h, w)[:, :2], f12.detach())
    params = [q for lin in net.linears() for q in (lin.weight, lin.bias)]
    for p, g in zip(params, call.backward(up.view(4, -1), saved)):
        assert torch.equal(p.grad, g)
        p.grad = None
    with torch.no_grad():
        i12, i21 = flownet.flow_fields(target, None, h, w, SCALE)
    assert not i12.requires_grad and torch.equal(i12, f12.detach()) and torch.equal(i21, f21.detach())
    # pose lists: (..., 2) -> (..., 4), the reference's layout; the grid spelt out gives the grid's flows
    poses = call.poses.view(h, w, 2)
    out = target(poses)
    assert out.shape == (h, w, 4) and out.requires_grad
    assert torch.equal(out.detach(), flownet.flow_at(target, poses, 1.0).detach())
    at = flownet.flow_at(target, poses, SCALE)
    assert torch.equal(at.detach().permute(2, 0, 1), torch.cat((f12, f21), 1).detach()[0])
    (at * up[0].permute(1, 2, 0)).sum().backward()
    for p, g in zip(params, call.backward(up.view(4, -1), saved)):
        assert torch.equal(p.grad, g)
    if net.is_progressive:
        got, used = target(poses, get_mask=True)
        assert torch.equal(got.detach(), out.detach()) and torch.equal(used, target.mask)
        f12o, _, used = flownet.flow_fields(target, None, h, w, SCALE, override_mask=torch.ones(514), get_mask=True)
        b12, _ = flownet.flow_fields(net, None, h, w, SCALE)
        assert torch.equal(f12o, b12) and used.shape == (514,)
    with pytest.raises(ValueError, match='domain_dim 2'):
        flownet.flow_fields(target, torch.zeros(1, device=dev), h, w, SCALE)
    with pytest.raises(ValueError, match='domain_dim 2'):
        flownet.flow_at(target, torch.zeros(4, 3, device=dev))
    with pytest.raises(ValueError, match='domain_dim 2.*pose_grad'):
        flownet.flow_at(target, poses.clone().requires_grad_(True), pose_grad=True)


# ---- the first step of the pair fit ----

PAIR_SEED = 0


def pair_module():
    import importlib.util
    spec = importlib.util.spec_from_file_location('pair_flow_cmd', os.path.join(ROOT, 'video-interpolation', 'pair_flow.py'))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def test_first_step_of_the_pair_fit_against_float64(dev):
    """24 x 40 synthetic pair, PRBF under LinearControllerEarly, the loop of video-interpolation/pair_flow.py: the loss terms and the EPE of
    the first step against the float64 composition of the oracles on the kernel's own flows, the way tests/test_gpu_flowtrainer.py compares
    its step.  Budget: 4 fp32-torch units per term; masks: at most 0.5 % of the pixels differ from float64's, the fp32 oracle's own
    included (PAIR_SEED was checked for that on the CPU).  Six steps give finite losses that move"""
    import flowtrainer_refs as R
    from sin_inn_amd import flowdata
    pf = pair_module()
    clip = flowdata.SyntheticClip(3, 24, 40, seed=PAIR_SEED)
    frame1, frame2, _, scale, gt = clip[0]
    frame1, frame2, gt = frame1[None].to(dev).contiguous(), frame2[None].to(dev).contiguous(), gt.to(dev)
    info = {}
    history = pf.fit_pair(frame1, frame2, float(scale), gt, 'PRBF', epochs=6, seed=PAIR_SEED, info=info)
    assert info['net'].encoding_dim == 514 and info['net'].iteration == 6
    first = info['first']
    flow12, flow21 = first['flow12'], first['flow21']
    assert flow12.shape == (1, 2, 24, 40) and flow21.shape == (1, 2, 24, 40)

    args = argparse.Namespace(occl='wang', occl_thresh=0.7, loss_l1=1, loss_census=0.1, census_width=3, loss_ssim=0, loss_smooth1=0.1,
                              edge_func='gauss', edge_constant=150)
    cpu = [t.detach().cpu() for t in (frame1, frame2, flow12, flow21)]
    m64 = R.step_masks_ref(*[t.to(F64) for t in cpu], args.occl, args.occl_thresh)[:2]
    m32 = R.step_masks_ref(*cpu, args.occl, args.occl_thresh)[:2]
    for i, (a, b, k) in enumerate(zip(m64, m32, first['masks'])):
        oracle_diff = float((a.to(torch.float32) != b).float().mean())
        kernel_diff = float((a.to(torch.float32) != k.cpu()).float().mean())
        print(f'mask{i + 1}: fp32 oracle differs from float64 on {oracle_diff:.3%} of pixels, the kernels on {kernel_diff:.3%}; '
              f'open {float(a.mean()):.3f}')
        assert oracle_diff <= 0.005, 'PAIR_SEED: the oracle itself sits on a threshold'
        assert kernel_diff <= 0.005
    kmasks = tuple(m.cpu() for m in first['masks'])
    ref64, _ = R.step_losses_ref(*[t.to(F64) for t in cpu], args, masks=kmasks)
    ref32, _ = R.step_losses_ref(*cpu, args, masks=kmasks)
    for ref in (ref64, ref32):
        ref['loss'] = ref['l1'] + ref['census'] + ref['smooth']
    ref64['epe'] = R.epe_ref(cpu[2].to(F64), gt.cpu().to(F64)[None])
    ref32['epe'] = R.epe_ref(cpu[2], gt.cpu()[None])
    failures = []
    for term in ('loss', 'l1', 'census', 'smooth', 'epe'):
        want = float(ref64[term])
        unit = abs(float(ref32[term].to(F64)) - want) / abs(want)
        err = abs(history[0][term] - want) / abs(want)
        print(f'pair step {term}: value {want:.6g}  err {err:.3g}  fp32-torch unit {unit:.3g}  budget {MULT * unit:.3g}')
        if not err <= MULT * unit:
            failures.append((term, err, MULT * unit))
    assert not failures, failures

    losses = [rec['loss'] for rec in history]
    print('pair fit losses:', ' '.join(f'{v:.6f}' for v in losses))
    assert len(losses) == 6 and all(np.isfinite(v) for v in losses) and len(set(losses)) > 1
    for p in info['net'].parameters():
        assert bool(torch.isfinite(p).all())
