"""Time the flow-field network (sin_inn_amd.flownet): forward (inference mode) and forward + backward (training mode), with
device events, after a warm-up, over a window of at least --seconds; one JSON line.

    python tools/bench_flownet.py --net RBF --frames 1 --height 436 --width 1024 [--baseline]

FLOP counts come from the shapes (2 N (E*256 + 2*256*256 + 256*4) forward, E = 512, for PE / PPE the network's own 24 / 27; backward adds the data gradients of layers 2-4 and
the weight gradients of all four); `mfma_peak_share` is those executed FLOPs over the event time against the 157.3 TFLOP/s f32
matrix peak of an MI355X -- the share of the whole call, not of one kernel.  --baseline times the same module composed from
torch's own GPU ops (tools/fit_flow.composed_flow_fields) in the same process, alternating windows with the fused path.
The progressive nets (PRBF, PFF, PUFF, PRBFG, PPE, MPFF) run under a prefix mask of --k-active leading ones (default 515: all ones; clamped to
the network's width, 27 for PPE), given as a
host tensor so that the kernels skip the closed features as they do under a controller; the FLOP counts stay those of the full
network, so the share of a skipped run is not a utilisation.  The mask sits in a controller, which uploads it once.
RFF / PRFF (learnable frequencies) add the data gradient through layer 1 to the step (2 N 512*256 more FLOPs, counted) and the torch ops
that make F_eff and carry its gradient to `encode.frequencies`; PRFF runs under the prefix mask like the other progressive nets.
--spatial R (515-wide progressive nets) puts the network under a StashedSpatialController(net, R) whose every cell has the prefix mask of
--k-active ones: the fused path samples the grid [R^3][515] in the kernels (the SPATIAL mode of the call descriptor, k_active = --k-active), the
--baseline is composed_flow_fields with the reference's own gather + einsum, `get_mask()[inds]` (N, 8, 515) times the weights, on every
call.  The FLOP counts stay those of the network; the interpolation is not counted.
`siren` is 3-256-256-256-256-4: 2 N (3*256 + 3*256*256 + 256*4) FLOPs forward; backward adds the data gradients of layers 2-5 and the
weight gradients of all five.  Its 4 * 256 sines per point (and as many cosines in the backward pass) are not counted.
--points N times the network at a pose list of N uniform random points of [-1, 1]^3 (flownet.flow_at, planar output: the kernels' own
layout) instead of a grid; the --baseline is tools/fit_flow.composed_flow_at on the same list.  The FLOP counts are those of N points.
--points N --spatial R [--pose-grad] calls the StashedSpatialController on the pose list (AT_POINTS | SPATIAL); the --baseline is
composed_flow_at under the controller's `interpolate` (gather + einsum, (N, 8, 515)) on every call.
--dim 2 builds the network on two coordinates, ModelParams(domain_dim=2) (the networks with `pair` in sin_inn_amd/flowcaps.py), and
times flow_fields(net, None, height, width, .), the call of video-interpolation/pair_flow.py: one frame, no times; the --baseline is
composed_flow_fields on the same network.  Grids only (no --points, --spatial, --frames).
"""
import argparse
import json
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, 'tools')):
    if p not in sys.path:
        sys.path.insert(0, p)

PEAK_F32_MFMA = 157.3e12


def flops(n, learnable=False, enc_dim=512):
    fwd = 2 * n * (enc_dim * 256 + 2 * 256 * 256 + 256 * 4)
    dgrad = 2 * n * (2 * 256 * 256 + 256 * 4 + (enc_dim * 256 if learnable else 0))
    return fwd, fwd + dgrad + fwd


def flops_siren(n):
    fwd = 2 * n * (3 * 256 + 3 * 256 * 256 + 256 * 4)
    dgrad = 2 * n * (3 * 256 * 256 + 256 * 4)
    return fwd, fwd + dgrad + fwd


def window(fn, seconds, warmup):
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    times, total = [], 0.0
    while total < seconds * 1e3:
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        for _ in range(5):
            fn()
        b.record()
        b.synchronize()
        times.append(a.elapsed_time(b) / 5)
        total += times[-1] * 5
    times.sort()
    return dict(median_ms=times[len(times) // 2], min_ms=times[0], max_ms=times[-1], samples=len(times))


def main():
    from sin_inn_amd import _lib, flowcaps, flownet, progressive
    ap = argparse.ArgumentParser(description=__doc__.split('\n')[0])
    ap.add_argument('--net', default='RBF', choices=list(flownet.flow_model_dict))
    ap.add_argument('--k-active', type=int, default=515, help='progressive nets: leading open features of the mask (0 .. 515, clamped to the network\'s width: 27 for PPE)')
    ap.add_argument('--frames', type=int, default=1)
    ap.add_argument('--height', type=int, default=436)
    ap.add_argument('--width', type=int, default=1024)
    ap.add_argument('--seconds', type=float, default=1.0)
    ap.add_argument('--warmup', type=int, default=5)
    ap.add_argument('--rounds', type=int, default=2, help='alternations of the fused and the baseline windows')
    ap.add_argument('--baseline', action='store_true')
    ap.add_argument('--points', type=int, default=0, metavar='N', help='a pose list of N random points instead of the frames x height x width grid')
    ap.add_argument('--spatial', type=int, default=0, metavar='R', help='progressive nets: a per-point mask from an R^3 grid (0: the global mask)')
    ap.add_argument('--pose-grad', action='store_true', help='--points: the step also differentiates the poses (flow_at(.., pose_grad=True); the '
                    'baseline: the composed network with the poses as a leaf); adds no_pose_grad_step_ms, the same step without it, and pose_grad_cost_ms / pose_grad_cost_ratio')
    ap.add_argument('--jacobian', metavar='D', help='--points: time flow_at(.., jacobian=D) (D from tyx, e.g. yx: DESIGN 24), forward and the step with '
                    'upstream gradients for both outputs; adds plain_*_ms, the call without the keyword at the same N, and jacobian_ratio_*; the '
                    '--baseline is flownet.flow_jacobian_composed')
    ap.add_argument('--dim', type=int, default=3, choices=[2, 3], help='coordinates per point: 3 (t, y, x) or 2 (y, x), one frame pair')
    a = ap.parse_args()
    assert a.dim == 3 or not (a.points or a.spatial or a.frames > 1), '--dim 2: one frame on its (y, x) grid'
    assert a.points or not a.pose_grad, '--pose-grad: the coordinate gradient exists at pose lists (--points)'
    assert not a.jacobian or (a.points and not a.spatial and not a.pose_grad and a.dim == 3), '--jacobian: a pose list (--points), a global mask, three coordinates'
    from fit_flow import composed_flow_at, composed_flow_fields
    dev = torch.device('cuda', 0)
    torch.manual_seed(0)
    learnable = a.net in flownet.learnable_model_dict
    siren = a.net in flownet.siren_model_dict
    net = flownet.flow_model_dict[a.net](flownet.ModelParams(domain_dim=a.dim)).to(dev)
    prog = net.is_progressive
    target = net
    if a.spatial:
        assert flowcaps.TABLE[a.net].spatial is flowcaps.OK, '--spatial needs a 515-wide progressive network'
        assert 6 <= a.k_active <= 515
        target = progressive.StashedSpatialController(net, a.spatial)
        target.mask.zero_()
        target.mask[:, :a.k_active] = 1
        target.mask_ = None
        target.cur_block = target.next_block = a.k_active          # k_active of the kernels
        assert target.device_grid(dev).k_active == a.k_active
    elif prog:
        assert 0 <= a.k_active <= 515
        a.k_active = min(a.k_active, net.encoding_dim)
        target = progressive.LinearController(net)
        target.mask = torch.zeros(net.encoding_dim)
        target.mask[:a.k_active] = 1
        mask_dev = target.mask.to(dev)
    times = torch.linspace(0, 1, a.frames, device=dev) if a.frames > 1 else torch.zeros(1, device=dev)
    if a.dim == 2:
        times = None
    n = a.points if a.points else a.frames * a.height * a.width
    up = torch.randn(a.frames, 4, a.height, a.width, device=dev) if not a.points else None
    params = list(net.parameters())

    def point_paths(at, pose_grad=False, **fixed):
        poses = (torch.rand(n, 3, generator=torch.Generator().manual_seed(1)) * 2 - 1).to(dev)
        if pose_grad:
            poses.requires_grad_(True)
            fixed = dict(fixed, pose_grad=True) if at is flownet.flow_at else fixed
        kw = dict(override_mask=mask_dev) if prog and not a.spatial and at is composed_flow_at else {}
        up_p = torch.randn(4, n, device=dev)
        up_p = up_p if fixed else up_p.t().contiguous()          # the composed network returns (N, 4)

        def fwd():
            with torch.no_grad():
                at(target, poses, 2.0, **kw, **fixed)

        def step():
            for p in params:
                p.grad = None
            poses.grad = None
            at(target, poses, 2.0, **kw, **fixed).backward(up_p)
        return fwd, step

    def paths(fields):
        kw = dict(override_mask=mask_dev) if prog and not a.spatial and fields is composed_flow_fields else {}

        def fwd():
            with torch.no_grad():
                fields(target, times, a.height, a.width, 2.0, **kw)

        def step():
            for p in params:
                p.grad = None
            f12, f21 = fields(target, times, a.height, a.width, 2.0, **kw)
            torch.autograd.backward([f12, f21], [up[:, :2], up[:, 2:]])
        return fwd, step

    def jacobian_paths(composed):
        poses = (torch.rand(n, 3, generator=torch.Generator().manual_seed(1)) * 2 - 1).to(dev)
        nd = len(flownet.jacobian_dirs(a.jacobian))
        up_p, up_j = torch.randn(4, n, device=dev), torch.randn(nd, 4, n, device=dev)
        if composed:
            kw = dict(override_mask=mask_dev) if prog else {}
            call = lambda: flownet.flow_jacobian_composed(target, poses, 2.0, a.jacobian, planar=True, **kw)  # noqa: E731
        else:
            call = lambda: flownet.flow_at(target, poses, 2.0, planar=True, jacobian=a.jacobian)  # noqa: E731

        def fwd():
            with torch.no_grad():
                call()

        def step():
            for p in params:
                p.grad = None
            torch.autograd.backward(list(call()), [up_p, up_j])
        return fwd, step

    if a.jacobian:
        todo = {'fused': jacobian_paths(False), 'plain': point_paths(flownet.flow_at, planar=True)}
        if a.baseline:
            todo['torch'] = jacobian_paths(True)
    elif a.points:
        todo = {'fused': point_paths(flownet.flow_at, a.pose_grad, planar=True)}
        if a.pose_grad:
            todo['no_pose_grad'] = point_paths(flownet.flow_at, planar=True)
        if a.baseline:
            todo['torch'] = point_paths(composed_flow_at, a.pose_grad)
    else:
        todo = {'fused': paths(flownet.flow_fields)}
        if a.baseline:
            todo['torch'] = paths(composed_flow_fields)
    res = {k: {'forward': [], 'step': []} for k in todo}
    for _ in range(a.rounds):
        for k, (fwd, step) in todo.items():
            res[k]['forward'].append(window(fwd, a.seconds, a.warmup))
            res[k]['step'].append(window(step, a.seconds, a.warmup))
    f_fwd, f_step = flops_siren(n) if siren else flops(n, learnable, net.encoding_dim if a.net in flownet.positional_model_dict else 512)
    sizes = (_lib.lib().sininn_siren_saved_bytes, _lib.lib().sininn_siren_workspace_bytes) if siren else \
        (_lib.lib().sininn_flownet_saved_bytes, _lib.lib().sininn_flownet_workspace_bytes)
    out = dict(net=a.net, **(dict(dim=a.dim) if a.dim != 3 else {}), **(dict(k_active=a.k_active) if prog else {}), **(dict(spatial_res=target.res) if a.spatial else {}), **(dict(jacobian=a.jacobian) if a.jacobian else {}), **(dict(mode='points', pose_grad=a.pose_grad) if a.points else dict(frames=a.frames, height=a.height, width=a.width)), points=n, flop_forward=f_fwd, flop_step=f_step,
               saved_bytes=sizes[0](n), workspace_bytes=sizes[1](n))
    for k in res:
        for what, fl in (('forward', f_fwd), ('step', f_step)):
            meds = [w['median_ms'] for w in res[k][what]]
            best = min(meds)
            out[f'{k}_{what}_ms'] = best
            out[f'{k}_{what}_ms_windows'] = [round(m, 4) for m in meds]
            if not (a.pose_grad and what == 'step' and k != 'no_pose_grad') and not (a.jacobian and k != 'plain'):  # flop_* count the plain call      # flop_step counts no pose gradient: no share for such a step
                out[f'{k}_{what}_mfma_peak_share'] = round(fl / (best * 1e-3) / PEAK_F32_MFMA, 4)
    if a.baseline:
        out['speedup_forward'] = round(out['torch_forward_ms'] / out['fused_forward_ms'], 3)
        out['speedup_step'] = round(out['torch_step_ms'] / out['fused_step_ms'], 3)
    if a.jacobian:
        out['jacobian_ratio_forward'] = round(out['fused_forward_ms'] / out['plain_forward_ms'], 3)
        out['jacobian_ratio_step'] = round(out['fused_step_ms'] / out['plain_step_ms'], 3)
    if a.pose_grad:
        out['pose_grad_cost_ms'] = round(out['fused_step_ms'] - out['no_pose_grad_step_ms'], 4)
        out['pose_grad_cost_ratio'] = round(out['fused_step_ms'] / out['no_pose_grad_step_ms'], 3)
    print(json.dumps(out))


if __name__ == '__main__':
    main()
