"""Fit a flow-field network to one synthetic frame pair: flow_fields -> warp / softmax splatting / L1 / census / smoothness
-> backward -> FusedAdam or FusedLAMB, the training step of video-interpolation/trainer.py:47-87 on this project's kernels.

    python tools/fit_flow.py --net RBF --height 64 --width 96 --steps 60
    python tools/fit_flow.py --net PRBF --max-iteration 1000
    python tools/fit_flow.py --net RFF
    python tools/fit_flow.py --net RBFG
    python tools/fit_flow.py --net PPE
    python tools/fit_flow.py --net siren
    python tools/fit_flow.py --net MPFF
    python tools/fit_flow.py --optimizer lamb
    python tools/fit_flow.py --net PRBF --controller spatial --res 7
    python tools/fit_flow.py --net RBF --points 4096
    python tools/fit_flow.py --net RBF --points 4096 --cycle
    python tools/fit_flow.py --net PRBF --points 4096 --controller spatial --res 7 [--cycle]
    python tools/fit_flow.py --net PRBF --dim 2

`--optimizer lamb` steps with FusedLAMB(net.parameters(), lr=lr), the optimiser of FlowTrainer.configure_optimizers
(trainer.py:134-135); the default stays FusedAdam.

A progressive network (PRBF, PFF, PUFF, PRFF, PRBFG, PPE, MPFF) is wrapped in LinearControllerEarly(net, max_iteration, epsilon=1e-3) as
video-interpolation/main.py:136-143 does, and the controller sees the loss after every step (trainer.py:75), which opens the mask.

`--controller spatial [--res R]` wraps a 515-wide progressive network in StashedSpatialController(net, R) instead (the reference's
--spatially-adaptive): after every step the controller stashes the per-pixel squared error of flow12 against the pair's known flow,
and every `block_iterations` (20) steps `update_progress()` closes the cells that are fitted and opens the next block in the others.

RFF / PRFF train `encode.frequencies` as well: the optimiser gets net.parameters(), which includes them.

`siren` (flownet.siren_model_dict) is the sine network on the raw coordinates; composed, it is its five nn.Linears with
torch.sin(30 * .) between them, model.py:145-146.

`--points N` (fit_points) is the other way such a network is trained: every step draws N uniform points in [-1, 1]^3 from a seeded
generator and fits net(poses) (flownet.flow_at, or the composed network) to the analytic flow of flowdata.SyntheticClip at those points,
MSE and FusedAdam; no warping, no images.  `--cycle` adds a forward-backward consistency term at those continuous points: p' = p moved by
flow12(p) (pixels turned into the pose units of the clip, the time unchanged: the clip's flow21 at a pose is the flow back onto that pose's
frame), and flow21(p') + flow12(p) should vanish.  The second query is a chained one: its gradient reaches the parameters through p' as
well (flow_at(.., pose_grad=True); composed: torch's autograd).  It runs the fused and the composed loop and prints the losses of both.
`--points N --controller spatial --res R` puts a 515-wide progressive network under StashedSpatialController(net, R) and calls it the
reference's way, controller(poses): fresh random points every step, the per-point squared error of flow12 stashed after the step (with
`--cycle` the controller attributes it to the cells of the list it evaluated last, p', as the reference's stash does), `update_progress()`
every `block_iterations` steps as on a grid.  Composed, the mask is the controller's `interpolate` (gather + einsum), (N, 515).

The pair is seeded and analytic: frame1 is a smooth texture, frame2 the same texture displaced by a known smooth flow.
`--composed` evaluates the network with torch's own ops (nn.functional.linear and elementwise ops) instead of the fused
kernels; everything after the network is the same, which is what tests/test_gpu_flownet.py compares.
"""
import argparse
import math
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)


def texture(x, y, gen_seed):
    """3-channel sum of 12 low-frequency plane waves per channel, values in about [0, 1]; x, y in pixels (any shape)"""
    g = torch.Generator().manual_seed(gen_seed)
    k = (torch.rand(3, 12, 2, generator=g) - 0.5) * 0.6          # radians per pixel
    ph = torch.rand(3, 12, generator=g) * 2 * math.pi
    k, ph = k.to(x), ph.to(x)
    arg = k[:, :, 0, None, None] * x[None, None] + k[:, :, 1, None, None] * y[None, None] + ph[:, :, None, None]
    return 0.5 + torch.sin(arg).mean(1) * 1.2


def make_pair(h, w, seed, device):
    """frame1, frame2 (1, 3, h, w) and the flow12 (1, 2, h, w) that produced frame2(x) = frame1(x - flow)"""
    yy, xx = torch.meshgrid(torch.arange(h, dtype=torch.float32), torch.arange(w, dtype=torch.float32), indexing='ij')
    u = 1.5 * torch.sin(yy / h * math.pi) + 0.5
    v = 1.0 * torch.cos(xx / w * math.pi)
    f1 = texture(xx, yy, seed)
    f2 = texture(xx - u, yy - v, seed)
    return f1[None].to(device).contiguous(), f2[None].to(device).contiguous(), torch.stack((u, v))[None].to(device)


PIECEWISE = 5                                                     # sin_inn_amd.flownet.PIECEWISE: the `kind` of MPFF's encoding


def composed_piecewise(enc, x):
    """PieceWiseEncoding.forward, model.py:634-646 line by line, on the port's buffer (out of place where the reference assigns
    through a mask: autograd-safe, the same values)"""
    out = torch.matmul(x + 1, enc.frequencies)
    out = torch.stack((out, out + 1), dim=2).view(-1, enc.output_channels)
    out = torch.fmod(out, 2) - 1
    return torch.where(out.lt(0), 2 * out + 1, 1 - 2 * out)


def composed_flow_fields(net, times, h, w, scale, override_mask=None):
    """FlowTrainer.forward (trainer.py:37-45) with torch's own GPU ops on the port's buffers and parameters: what a user of the
    reference runs, and the baseline of tools/bench_flownet.py.  A progressive network reads cat((poses, encoding)) times the
    mask of its controller (or `override_mask`; a bare network: no mask), model.py:532-535 and 89-99.  A learnable encoding (RFF /
    PRFF) normalises its frequencies and scales them by the magnitudes on every call, model.py:274.  The radial-basis grid (RBFG / PRBFG)
    is model.py:375-387 line by line, with its N x 256 x 2 x 3 intermediate; the positional encoding (PE / PPE) is the einsum / cat of
    model.py:331-332, without the `.view(-1, 21)` that raises unless N is a multiple of 7 (the cat is already (N, 4, 6)); the piecewise-linear
    encoding (MPFF) is composed_piecewise.  A SirenModel has
    no encoding: sin(omega_0 * linear(x)) four times and the last nn.Linear, model.py:145-146, 163-171.  A network on two coordinates
    (ModelParams(domain_dim=2)) takes `times=None`: the poses are (y, x) on the h x w grid and the encoders, written over the last axis, are
    the reference's two-term expressions."""
    mask = override_mask
    spatial = None
    if hasattr(net, 'mask'):                                      # a controller
        if hasattr(net, 'interpolate'):                           # spatially adaptive: the reference's gather + einsum, (N, 8, 515)
            spatial = net
        else:
            mask = net.mask if mask is None else mask
        net = net.model
    if net.domain_dim == 2:                                       # one frame pair, pair_flow.py:55-58: poses (y, x), no times
        assert times is None, 'a network on (y, x) has no times'
        like = next(net.parameters())
        gh, gw = torch.meshgrid(torch.linspace(-1, 1, h).to(like), torch.linspace(-1, 1, w).to(like), indexing='ij')
        x = poses = torch.stack((gh, gw), dim=-1).view(-1, 2)
        times = like.new_zeros(1)                                 # one frame: flows (1, 4, h, w)
    else:
        ys = torch.linspace(-1, 1, h).to(times)
        xs = torch.linspace(-1, 1, w).to(times)
        gt, gh, gw = torch.meshgrid(times, ys, xs, indexing='ij')
        x = poses = torch.stack((gt, gh, gw), dim=-1).view(-1, 3)
    if spatial is not None and mask is None:
        mask = spatial.interpolate(poses)                         # (N, 515), one row per point
    if not hasattr(net, 'encode'):                                # siren
        for layer in net.model:
            x = torch.sin(layer.omega_0 * layer.linear(x)) if hasattr(layer, 'omega_0') else layer(x)
        flows = x.view(times.numel(), h, w, 4).permute(0, 3, 1, 2) * scale
        return flows[:, :2], flows[:, 2:]
    enc = net.encode
    if hasattr(enc, 'centres'):
        x = (x[:, None, :] - enc.centres[None, :, :]).pow(2).sum(2)
        x = torch.exp(-(x * enc.sigma[None, :] ** 2))
    elif hasattr(enc, 'freqs'):
        x = torch.einsum('f,nd->nfd', enc.freqs, x)
        x = torch.cat((torch.cos(x), torch.sin(x)), dim=2).view(x.shape[0], -1)
    elif getattr(enc, 'kind', None) == PIECEWISE:
        x = composed_piecewise(enc, x)
    elif hasattr(enc, 'offsets'):
        x_a = x[:, None, :] + enc.offsets[None, :]
        x_b = x_a + (1 / enc.sigma[None, :, None])
        x = torch.stack((x_a, x_b), dim=2)
        x = (x % (2 / enc.sigma[None, :, None, None])) * 2 - (2 / enc.sigma[None, :, None, None])
        x = x.pow(2).sum(3) * enc.sigma[None, :, None] ** 2
        x = torch.exp(-x.view(-1, enc.output_channels)) * 2 - 1
    else:
        freq = enc.effective_frequencies() if hasattr(enc, 'magnitudes') else enc.frequencies
        x = torch.matmul(x * 2 * math.pi, freq)
        x = torch.stack((torch.sin(x), torch.cos(x)), dim=2).view(x.shape[0], -1)
    if net.is_progressive:
        x = torch.cat((poses, x), dim=-1)
        if mask is not None:
            x = x * (mask.to(x) if mask.dim() == 2 else mask.to(x)[None, :])
    flows = net.model.model(x).view(times.numel(), h, w, 4).permute(0, 3, 1, 2) * scale
    return flows[:, :2], flows[:, 2:]


def composed_flow_at(net, poses, scale=1.0, override_mask=None):
    """net(poses) * scale, (N, 3) -> (N, 4), with torch's own GPU ops: composed_flow_fields on a pose list (one frame of N x 1 points
    whose coordinates are the list), the baseline of `bench_flownet.py --points`"""
    mask = override_mask
    if hasattr(net, 'mask'):                                      # a controller
        if hasattr(net, 'interpolate'):                           # spatially adaptive: the reference's gather + einsum, (N, 515)
            mask = net.interpolate(poses) if mask is None else mask
        else:
            mask = net.mask if mask is None else mask
        net = net.model
    x = poses
    if not hasattr(net, 'encode'):                                # siren
        for layer in net.model:
            x = torch.sin(layer.omega_0 * layer.linear(x)) if hasattr(layer, 'omega_0') else layer(x)
        return x * scale
    enc = net.encode
    if hasattr(enc, 'centres'):
        x = (x[:, None, :] - enc.centres[None, :, :]).pow(2).sum(2)
        x = torch.exp(-(x * enc.sigma[None, :] ** 2))
    elif hasattr(enc, 'freqs'):
        x = torch.einsum('f,nd->nfd', enc.freqs, x)
        x = torch.cat((torch.cos(x), torch.sin(x)), dim=2).view(x.shape[0], -1)
    elif getattr(enc, 'kind', None) == PIECEWISE:
        x = composed_piecewise(enc, x)
    elif hasattr(enc, 'offsets'):
        x_a = x[:, None, :] + enc.offsets[None, :]
        x_b = x_a + (1 / enc.sigma[None, :, None])
        x = torch.stack((x_a, x_b), dim=2)
        x = (x % (2 / enc.sigma[None, :, None, None])) * 2 - (2 / enc.sigma[None, :, None, None])
        x = x.pow(2).sum(3) * enc.sigma[None, :, None] ** 2
        x = torch.exp(-x.view(-1, enc.output_channels)) * 2 - 1
    else:
        freq = enc.effective_frequencies() if hasattr(enc, 'magnitudes') else enc.frequencies
        x = torch.matmul(x * 2 * math.pi, freq)
        x = torch.stack((torch.sin(x), torch.cos(x)), dim=2).view(x.shape[0], -1)
    if net.is_progressive:
        x = torch.cat((poses, x), dim=-1)
        if mask is not None:
            x = x * (mask.to(x) if mask.dim() == 2 else mask.to(x)[None, :])
    return net.model.model(x) * scale


def analytic_flow(poses, h=64, w=96, frames=3):
    """(N, 4) fp32: the ground-truth flow of flowdata.SyntheticClip(frames, h, w) as a function of continuous (t, y, x) in [-1, 1]^3,
    in pixels: columns 0:2 the flow that carries the frame at time t onto the frame one step later (SyntheticClip.flow between its
    frames), columns 2:4 the flow back.  s = (t + 1) / 2 is the clip's displacement factor, one step is 1 / (frames - 1).  Evaluated in
    float64 with the clip's own fixed-point iteration."""
    p = poses.to(torch.float64)
    s0 = (p[:, 0] + 1) / 2
    yy, xx = (p[:, 1] + 1) / 2 * (h - 1), (p[:, 2] + 1) / 2 * (w - 1)
    s1 = s0 + 1.0 / (frames - 1)

    def disp(x, y):
        return 1.5 * torch.sin(y / h * math.pi) + 0.5, 1.0 * torch.cos(x / w * math.pi)

    def carry(sa, sb):                                            # the frame at factor sa -> the frame at factor sb
        u, v = disp(xx, yy)
        px, py = xx - sa * u, yy - sa * v
        x1, y1 = xx.clone(), yy.clone()
        for _ in range(60):                                       # a contraction of ratio < 0.15: far below 1e-13 after 60
            du, dv = disp(x1, y1)
            x1, y1 = px + sb * du, py + sb * dv
        return x1 - xx, y1 - yy

    return torch.stack((*carry(s0, s1), *carry(s1, s0)), dim=1).to(torch.float32)


def follow(poses, out, h=64, w=96):
    """p' (N, 3): `poses` moved by flow12 = out[:, :2] (x then y displacement, in pixels of the h x w clip) in pose units, the time unchanged"""
    zero = torch.zeros_like(out[:, 0])
    return poses + torch.stack((zero, out[:, 1] * (2.0 / (h - 1)), out[:, 0] * (2.0 / (w - 1))), dim=1)


def cycle_term(query, poses, out):
    """mean |flow21(p') + flow12(p)|^2 with p' = follow(poses, out), out = query(poses) already evaluated"""
    back = query(follow(poses, out))
    return (back[:, 2:] + out[:, :2]).pow(2).mean()


def _spatial_only(name, dim=3):
    from sin_inn_amd import flowcaps
    if flowcaps.TABLE[name].spatial is not flowcaps.OK or dim != 3:
        raise ValueError(f'--controller spatial needs a 515-wide progressive network ({", ".join(flowcaps.names("spatial"))}); got {name}')


def fit_points(name='RBF', n_points=4096, steps=60, composed=False, info=None, lr=1e-3, seed=0, device='cuda', log=None,
               max_iteration=1000, cycle=False, cycle_weight=1.0, controller='early', res=7, smooth_at=0.0):
    """fit net(poses) to analytic_flow at `n_points` fresh uniform points of [-1, 1]^3 per step (a seeded generator): MSE, FusedAdam.
    `cycle`: plus cycle_weight x cycle_term, the forward-backward consistency at p' (a chained query).
    Returns the list of per-step losses (floats).  `info`: a dict that receives the network (the controller of a progressive one)
    as info['net'] and, as info['first'], the first step's `poses`, `target` and the network's `state` before that step.
    `smooth_at`: plus smooth_at x the first-order smoothness of the network's analytic Jacobian at the same points:
    0.5 (mean robust_l1(d flow / d y per pixel) + mean robust_l1(d flow / d x per pixel)), robust_l1(v) = sqrt(v^2 + 1e-6), no guide image;
    flow_at(.., jacobian='yx'), or with `composed` flownet.flow_jacobian_composed.
    `controller='spatial'`: a StashedSpatialController(net, res) called on the pose list; it stashes the per-point squared error of flow12
    and runs update_progress every block_iterations steps (their number: info['progress'])"""
    from sin_inn_amd import FusedAdam, flownet, progressive
    torch.manual_seed(seed)
    net = flownet.flow_model_dict[name](flownet.ModelParams()).to(device)
    assert controller in ('early', 'spatial'), controller
    spatial = controller == 'spatial'
    if spatial:
        _spatial_only(name)
        net = progressive.StashedSpatialController(net, res)
    elif net.is_progressive:
        net = progressive.LinearControllerEarly(net, max_iteration, epsilon=1e-3)
    opt = FusedAdam(net.parameters(), lr=lr)
    gen = torch.Generator().manual_seed(seed + 1)
    at = composed_flow_at if composed else flownet.flow_at
    query = (lambda x: composed_flow_at(net, x, 1.0)) if composed else (lambda x: flownet.flow_at(net, x, 1.0, pose_grad=True))
    if info is not None:
        info['net'], info['progress'] = net, 0
    losses = []
    for step in range(steps):
        poses = (torch.rand(n_points, 3, generator=gen) * 2 - 1).to(device)
        target = analytic_flow(poses)
        if info is not None and step == 0:
            info['first'] = dict(poses=poses, target=target, state={k: v.detach().clone() for k, v in net.state_dict().items()})
        opt.zero_grad()
        if smooth_at:
            out, jac = flownet.flow_jacobian_composed(net, poses, 1.0, 'yx') if composed else flownet.flow_at(net, poses, 1.0, jacobian='yx')
        else:
            out = at(net, poses, 1.0)
        loss = torch.nn.functional.mse_loss(out, target)
        if smooth_at:
            gy, gx = jac[..., 0] * (2.0 / 63), jac[..., 1] * (2.0 / 95)      # per pixel of analytic_flow's 64 x 96 clip
            loss = loss + smooth_at * 0.5 * (torch.sqrt(gy * gy + 1e-6).mean() + torch.sqrt(gx * gx + 1e-6).mean())
        if cycle:
            loss = loss + cycle_weight * cycle_term(query, poses, out)
        loss.backward()
        opt.step()
        if spatial:
            net.stash_iteration((out.detach()[:, :2] - target[:, :2]).pow(2).sum(1))
            if (step + 1) % net.block_iterations == 0:
                net.update_progress()
                if info is not None:
                    info['progress'] += 1
        else:
            net.stash_iteration(loss.detach())
        losses.append(float(loss.detach()))
        if log:
            extra = f'  open {net.cur_block:3d} / {net.encoding_dim}' if net.is_progressive else ''
            log(f'step {step:3d}  loss {losses[-1]:.6f}{extra}')
    return losses


def fit(net_name='RBF', h=64, w=96, steps=60, lr=1e-3, seed=0, composed=False, device='cuda', log=None, max_iteration=1000,
        info=None, optimizer='adam', controller='early', res=7, dim=3):
    """returns the list of per-step losses (floats); `info`: a dict that receives the network (the controller of a progressive one,
    and under `controller='spatial'` the number of update_progress calls as info['progress']).  `dim=2`: the network is built on two
    coordinates, ModelParams(domain_dim=2), and evaluated on the (y, x) grid of the pair"""
    from sin_inn_amd import FusedAdam, FusedLAMB, flowloss as FL, flownet, progressive
    from sin_inn_amd.functional import flow_warp_l1
    torch.manual_seed(seed)
    assert dim in (2, 3), dim
    net = flownet.flow_model_dict[net_name](flownet.ModelParams(domain_dim=dim)).to(device)
    assert controller in ('early', 'spatial'), controller
    spatial = controller == 'spatial'
    if spatial:
        _spatial_only(net_name, dim)
        net = progressive.StashedSpatialController(net, res)
    elif net.is_progressive:
        net = progressive.LinearControllerEarly(net, max_iteration, epsilon=1e-3)
    if info is not None:
        info['net'] = net
    assert optimizer in ('adam', 'lamb'), optimizer
    opt = (FusedLAMB if optimizer == 'lamb' else FusedAdam)(net.parameters(), lr=lr)
    frame1, frame2, true_flow = make_pair(h, w, seed + 1, device)
    if info is not None:
        info['progress'] = 0
    times = torch.zeros(1, device=device) if dim == 3 else None
    l1, census, smooth = FL.L1Loss(1.0), FL.CensusLoss(0.1, max_distance=3), FL.BilateralSmooth(0.1, 'gauss', 150, 1)
    fields = composed_flow_fields if composed else flownet.flow_fields
    losses = []
    for step in range(steps):
        opt.zero_grad()
        flow12, flow21 = fields(net, times, h, w, 1.0)
        flow12, flow21 = flow12.contiguous(), flow21.contiguous()
        mask1 = FL.occlusion_wang(flow12, flow21, 0.5)
        mask2 = FL.occlusion_wang(flow21, flow12, 0.5)
        _, metric = flow_warp_l1(frame1, flow21, frame2)
        softmax1 = FL.FunctionSoftsplat(frame2, flow21, -20 * metric, strType='softmax')
        mask1 = mask1 * (softmax1 != 0)
        _, metric = flow_warp_l1(frame2, flow12, frame1)
        softmax2 = FL.FunctionSoftsplat(frame1, flow12, -20 * metric, strType='softmax')
        mask2 = mask2 * (softmax2 != 0)
        loss = (l1(softmax1, frame1, mask1) + l1(softmax2, frame2, mask2)
                + census(softmax1, frame1, mask1) + census(softmax2, frame2, mask2)
                + smooth(frame1, flow12) + smooth(frame2, flow21))
        loss.backward()
        opt.step()
        if spatial:
            net.stash_iteration((flow12.detach() - true_flow).pow(2).sum(1).flatten())
            if (step + 1) % net.block_iterations == 0:
                net.update_progress()
                if info is not None:
                    info['progress'] += 1
        else:
            net.stash_iteration(loss.detach())
        losses.append(float(loss))
        if log:
            extra = f'  open {net.cur_block:3d} / {net.encoding_dim}' if net.is_progressive else ''
            log(f'step {step:3d}  loss {losses[-1]:.6f}{extra}')
    return losses


def main():
    from sin_inn_amd import flownet
    ap = argparse.ArgumentParser(description=__doc__.split('\n')[0])
    ap.add_argument('--net', default='RBF', choices=list(flownet.flow_model_dict))
    ap.add_argument('--max-iteration', type=int, default=1000, help='progressive nets: the controller opens the mask over 3/4 of it')
    ap.add_argument('--height', type=int, default=64)
    ap.add_argument('--width', type=int, default=96)
    ap.add_argument('--steps', type=int, default=60)
    ap.add_argument('--lr', type=float, default=1e-3)
    ap.add_argument('--seed', type=int, default=0)
    ap.add_argument('--composed', action='store_true')
    ap.add_argument('--optimizer', default='adam', choices=['adam', 'lamb'])
    ap.add_argument('--controller', default='early', choices=['early', 'spatial'], help='progressive nets: the mask is global / per grid cell')
    ap.add_argument('--res', type=int, default=7, help='--controller spatial: cells per axis of the mask grid')
    ap.add_argument('--dim', type=int, default=3, choices=[2, 3], help='coordinates per point: 3 (t, y, x), or 2 (y, x), the network of '
                    'video-interpolation/pair_flow.py (RBF, FFN, UFF, RBFG and their progressive forms; not with --points)')
    ap.add_argument('--points', type=int, default=0, metavar='N', help='fit net(poses) at N random points per step (fit_points) instead of a frame pair')
    ap.add_argument('--cycle', action='store_true', help='--points: add the forward-backward consistency term at p + flow12(p); runs the '
                    'fused and the composed loop and prints both')
    ap.add_argument('--smooth-at', type=float, default=0.0, metavar='W', help='--points: add W x the smoothness of the analytic flow Jacobian '
                    'at the sampled points (flow_at(.., jacobian=); DESIGN 24)')
    a = ap.parse_args()
    assert a.points or not a.smooth_at, '--smooth-at is a term of the --points loop'
    assert a.points or not a.cycle, '--cycle is a term of the --points loop'
    assert a.dim == 3 or not a.points, '--points fits the three-coordinate clip; --dim 2 is the frame-pair loop'
    if a.cycle:
        for what, comp in (('fused', False), ('composed', True)):
            losses = fit_points(a.net, a.points, a.steps, comp, lr=a.lr, seed=a.seed, log=lambda m, w=what: print(w, m),
                                max_iteration=a.max_iteration, cycle=True, controller=a.controller, res=a.res)
            print(f'{what}: first {losses[0]:.6f}  last {losses[-1]:.6f}')
        return
    if a.points:
        losses = fit_points(a.net, a.points, a.steps, a.composed, lr=a.lr, seed=a.seed, log=print, max_iteration=a.max_iteration,
                            controller=a.controller, res=a.res, smooth_at=a.smooth_at)
        print(f'first {losses[0]:.6f}  last {losses[-1]:.6f}')
        return
    losses = fit(a.net, a.height, a.width, a.steps, a.lr, a.seed, a.composed, log=print, max_iteration=a.max_iteration,
                 optimizer=a.optimizer, controller=a.controller, res=a.res, dim=a.dim)
    print(f'first {losses[0]:.6f}  last {losses[-1]:.6f}')


if __name__ == '__main__':
    main()
