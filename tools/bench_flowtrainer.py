"""Time one step of the flow trainer: FlowTrainer.training_step + zero_grad / backward / FusedLAMB step, at the reference's
`--batch 3 --size 436` on SyntheticClip(frames, 436, 1024), with device events, after a warm-up, over windows of at least --seconds
(the window method of tools/bench_flownet.py); one JSON line.

    python tools/bench_flowtrainer.py [--net RBF] [--batch 3] [--height 436] [--width 1024]

Three paths run in alternating windows in one process:
    fused     the step as FlowTrainer runs it
    torch     the same step with the three operators of csrc/flowtrain.hip (end-point error, mask * (splat != 0)) replaced by their
              torch expressions (FlowTrainer.fused = False); flow2img is not part of a training step
    network   flow_fields forward + backward alone on the same grid, with a random upstream gradient: the share of the step that is
              the network
A progressive net runs under LinearControllerEarly(net, 5000): the controller reads the loss on every step, as in the reference.

    python tools/bench_flowtrainer.py --spatially-adaptive [--net PRBF] [--res 50]

times the step under StashedSpatialController(net, res) instead (training_step, backward, on_after_backward, optimizer step;
block_iterations is set beyond the run, so no window contains an update_progress), again in alternating windows:
    spatial_fused      the stash is the fused error_stash (csrc/flowtrain.hip)
    spatial_composed   the stash is its composed form (FlowTrainer.fused = False; the two other operators stay fused)
    linear             the same network's step under LinearControllerEarly, the baseline
    stash_fused / stash_composed   the stash alone, on the tensors of one step
and reports the bytes per pixel the fused stash moves, counted from its definition.

    python tools/bench_flowtrainer.py --loss-between 1 [--between-taus 1] [--between-back network] [--log]

adds the step with the in-between consistency loss next to the step without it, in the same alternating windows:
    between_fused      the loss through flowsynth.gather(.., flow_grad=True) (the backward kernels of csrc/flowgather.hip)
    between_composed   the loss through gather_composed(.., flow_grad=True) (FlowTrainer.fused = False; as `torch` above, the two
                       flowtrain operators are torch expressions too)
    between_network    flow_fields forward + backward alone at the stamps of one between term: what the extra evaluations cost
With --between-points N the loss is drawn at N random points a step -- flowsynth.gather_at, or gather_at_composed -- and
between_network is flow_at forward + backward at the N (under --between-back network 2 N) poses of one draw.
    python tools/bench_flowtrainer.py --loss-smooth-at 1 --smooth-points N [--log]
adds smooth_at_fused / smooth_at_composed, the step with the smoothness prior on the flow Jacobian at N sampled points.
The generator is reset before every window, so all windows draw the same times.  --log appends the line to
profiles/flowtrainer_bench.jsonl.
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

from bench_flownet import window  # noqa: E402
from sin_inn_amd import flowcaps  # noqa: E402


def main():
    ap = argparse.ArgumentParser(description=__doc__.split('\n')[0])
    ap.add_argument('--net', default='RBF', choices=flowcaps.names(cli=True))
    ap.add_argument('--frames', type=int, default=4)
    ap.add_argument('--batch', type=int, default=3)
    ap.add_argument('--height', type=int, default=436)
    ap.add_argument('--width', type=int, default=1024)
    ap.add_argument('--loss-ssim', type=float, default=0.0)
    ap.add_argument('--seconds', type=float, default=1.0)
    ap.add_argument('--warmup', type=int, default=3)
    ap.add_argument('--rounds', type=int, default=2)
    ap.add_argument('--spatially-adaptive', action='store_true', help='time the step under StashedSpatialController: fused and composed stash')
    ap.add_argument('--res', type=int, default=50, help='--spatially-adaptive: cells per axis of the mask grid')
    ap.add_argument('--loss-between', type=float, default=0.0, help='also time the step with the in-between loss of this weight')
    ap.add_argument('--between-taus', type=int, default=1)
    ap.add_argument('--between-back', default='network', choices=['network', 'reverse'])
    ap.add_argument('--between-points', type=int, metavar='N',
                    help='--loss-between: the loss at N random points a step (DESIGN 23) instead of --between-taus whole frames')
    ap.add_argument('--loss-smooth-at', type=float, default=0.0, help='also time the step with the smoothness prior on the flow Jacobian at '
                    'sampled points (DESIGN 24): smooth_at_fused / smooth_at_composed next to the step without it')
    ap.add_argument('--smooth-points', type=int, default=4096, metavar='N', help='--loss-smooth-at: points a step')
    ap.add_argument('--log', action='store_true', help='append the line to profiles/flowtrainer_bench.jsonl')
    a = ap.parse_args()
    from sin_inn_amd import flowdata, flownet, flowtrainer, progressive
    dev = torch.device('cuda', 0)
    if a.spatially_adaptive:
        return spatial(a, dev)
    torch.manual_seed(0)
    net = flownet.all_model_dict[a.net](flownet.ModelParams())
    if net.is_progressive:
        net = progressive.LinearControllerEarly(net, 5000, epsilon=1e-3)
    args = argparse.Namespace(lr=1e-4, loss_l1=1, loss_census=0.1, loss_ssim=a.loss_ssim, census_width=3, loss_smooth1=0.1,
                              edge_constant=150, edge_func='gauss', occl='wang', occl_thresh=0.7, net=net)
    model = flowtrainer.FlowTrainer(args).to(dev)
    opt = model.attach_optimizer()
    clip = flowdata.SyntheticClip(a.frames, a.height, a.width)
    assert a.batch <= len(clip)
    batch = [clip.video[:a.batch].to(dev), clip.video[1:a.batch + 1].to(dev), clip.T[:a.batch].to(dev),
             torch.tensor([clip.flow_scale] * a.batch, dtype=torch.float64).to(dev), clip.flow[:a.batch].to(dev)]
    up = torch.randn(a.batch, 4, a.height, a.width, device=dev)

    def step(fused):
        def run():
            model.fused = fused
            opt.zero_grad()
            model.training_step(batch, 0).backward()
            opt.step()
        return run

    def network():
        opt.zero_grad()
        f12, f21 = model(batch[0], batch[2], batch[3])
        torch.autograd.backward([f12, f21], [up[:, :2], up[:, 2:]])

    todo = {'fused': step(True), 'torch': step(False), 'network': network}
    if a.loss_between != 0:
        from sin_inn_amd import flowsynth
        dt = 2 / (a.frames - 1)
        torch.manual_seed(0)
        net2 = flownet.all_model_dict[a.net](flownet.ModelParams())
        if net2.is_progressive:
            net2 = progressive.LinearControllerEarly(net2, 5000, epsilon=1e-3)
        how = {'between_points': a.between_points} if a.between_points else {'between_taus': a.between_taus}
        args2 = argparse.Namespace(**{**vars(args), 'net': net2, 'loss_between': a.loss_between, 'between_back': a.between_back,
                                      'between_dt': dt, **how})
        model2 = flowtrainer.FlowTrainer(args2).to(dev)
        opt2 = model2.attach_optimizer()
        times_host = clip.T[:a.batch].tolist()
        state = model2.between_rng.getstate()
        stamps, _ = flowsynth.gather_slots(times_host, [0.5] * a.between_taus, dt, a.between_back)
        at = torch.tensor(stamps, dtype=torch.float32, device=dev)
        up2 = torch.randn(len(stamps), 4, a.height, a.width, device=dev)

        def between(fused):
            def run():
                model2.fused = fused
                model2._times_on_host = times_host           # what the trainer loop's on_before_batch_transfer keeps
                opt2.zero_grad()
                model2.training_step(batch, 0).backward()
                opt2.step()
            return run

        def points_network():
            opt2.zero_grad()
            for p, u in zip(poses, up_points):
                flownet.flow_at(model2.net, p, clip.flow_scale, planar=True).backward(u)

        if a.between_points:
            poses = model2.between_points_table(batch[2], a.batch, a.height, a.width)[4]
            up_points = [torch.randn(4, a.between_points, device=dev) for _ in poses]

        def between_network():
            if a.between_points:
                return points_network()
            opt2.zero_grad()
            per = max(1, flowtrainer.GRID_POINTS // (a.height * a.width))
            for i in range(0, len(stamps), per):
                f12, f21 = model2(batch[0], at[i:i + per], batch[3])
                torch.autograd.backward([f12, f21], [up2[i:i + per, :2], up2[i:i + per, 2:]])

        todo.update(between_fused=between(True), between_composed=between(False), between_network=between_network)
    if a.loss_smooth_at != 0:
        torch.manual_seed(0)
        net3 = flownet.all_model_dict[a.net](flownet.ModelParams())
        if net3.is_progressive:
            net3 = progressive.LinearControllerEarly(net3, 5000, epsilon=1e-3)
        args3 = argparse.Namespace(**{**vars(args), 'net': net3, 'loss_smooth_at': a.loss_smooth_at, 'smooth_points': a.smooth_points})
        model3 = flowtrainer.FlowTrainer(args3).to(dev)
        opt3 = model3.attach_optimizer()

        def smooth_at(fused):
            def run():
                model3.fused = fused
                opt3.zero_grad()
                model3.training_step(batch, 0).backward()
                opt3.step()
            return run
        todo.update(smooth_at_fused=smooth_at(True), smooth_at_composed=smooth_at(False))
    res = {k: [] for k in todo}
    for _ in range(a.rounds):
        for k, fn in todo.items():
            if a.loss_between != 0:
                model2.between_rng.setstate(state)
            res[k].append(window(fn, a.seconds, a.warmup))
    out = dict(net=a.net, batch=a.batch, height=a.height, width=a.width, loss_ssim=a.loss_ssim, points=a.batch * a.height * a.width)
    for k in res:
        meds = [w['median_ms'] for w in res[k]]
        out[f'{k}_ms'] = round(min(meds), 4)
        out[f'{k}_ms_windows'] = [round(m, 4) for m in meds]
    out['network_share'] = round(out['network_ms'] / out['fused_ms'], 3)
    out['fused_over_torch'] = round(out['fused_ms'] / out['torch_ms'], 4)
    if a.loss_between != 0:
        out.update(loss_between=a.loss_between, between_taus=a.between_taus, between_back=a.between_back, between_stamps=len(stamps))
        if a.between_points:
            del out['between_taus'], out['between_stamps']
            out.update(between_points=a.between_points, between_network_points=a.between_points * len(poses))
        out['between_extra_ms'] = round(out['between_fused_ms'] - out['fused_ms'], 4)
        out['between_network_share_of_extra'] = round(out['between_network_ms'] / out['between_extra_ms'], 3)
        out['between_fused_over_composed'] = round(out['between_fused_ms'] / out['between_composed_ms'], 4)
    if a.loss_smooth_at != 0:
        out.update(loss_smooth_at=a.loss_smooth_at, smooth_points=a.smooth_points)
        out['smooth_at_extra_ms'] = round(out['smooth_at_fused_ms'] - out['fused_ms'], 4)
        out['smooth_at_fused_over_composed'] = round(out['smooth_at_fused_ms'] / out['smooth_at_composed_ms'], 4)
    print(json.dumps(out))
    if a.log:
        with open(os.path.join(ROOT, 'profiles', 'flowtrainer_bench.jsonl'), 'a') as f:
            f.write(json.dumps(out) + '\n')


def spatial(a, dev):
    from sin_inn_amd import flowdata, flownet, flowtrainer, progressive
    name = a.net if a.net != 'RBF' else 'PRBF'
    clip = flowdata.SyntheticClip(a.frames, a.height, a.width)
    assert a.batch <= len(clip)
    batch = [clip.video[:a.batch].to(dev), clip.video[1:a.batch + 1].to(dev), clip.T[:a.batch].to(dev),
             torch.tensor([clip.flow_scale] * a.batch, dtype=torch.float64).to(dev), clip.flow[:a.batch].to(dev)]

    def trainer(controller):
        torch.manual_seed(0)
        net = flownet.all_model_dict[name](flownet.ModelParams()).to(dev)
        if controller == 'spatial':
            net = progressive.StashedSpatialController(net, a.res, block_iterations=1 << 30, epsilon=1e-3)
        else:
            net = progressive.LinearControllerEarly(net, 5000, epsilon=1e-3)
        args = argparse.Namespace(lr=1e-4, loss_l1=1, loss_census=0.1, loss_ssim=a.loss_ssim, census_width=3, loss_smooth1=0.1,
                                  edge_constant=150, edge_func='gauss', occl='wang', occl_thresh=0.7, net=net)
        model = flowtrainer.FlowTrainer(args).to(dev)
        return model, model.attach_optimizer()

    models = {'spatial': trainer('spatial'), 'linear': trainer('linear')}

    def step(which, fused):
        model, opt = models[which]

        def run():
            model.fused = fused
            opt.zero_grad()
            model.training_step(batch, 0).backward()
            model.on_after_backward()
            opt.step()
            model.fused = True
        return run

    # the stash alone, on the tensors of one step
    model, _ = models['spatial']
    model.training_step(batch, 0).backward()
    six, model._stash = model._stash, None
    net = model.net
    grid = net._last_grid
    logs = torch.zeros_like(net.log_buffer), torch.zeros_like(net.log_counter)
    ws = torch.empty(flowtrainer._lib.lib().sininn_flow_error_stash_workspace_floats(a.batch, a.height, a.width, a.res), device=dev)

    def stash_fused():
        flowtrainer.error_stash(*six, *grid, a.res, net.centre_scale_host(), *logs, workspace=ws)

    def stash_composed():
        flowtrainer.error_stash_composed(*six, *grid, net.cells, *logs)

    todo = {'spatial_fused': step('spatial', True), 'spatial_composed': step('spatial', False), 'linear': step('linear', True),
            'stash_fused': stash_fused, 'stash_composed': stash_composed}
    res = {k: [] for k in todo}
    for _ in range(a.rounds):
        for k, fn in todo.items():
            res[k].append(window(fn, a.seconds, a.warmup))
    points = a.batch * a.height * a.width
    channels = six[0].shape[1]
    # per pixel: two splats and two frames of C floats, two masks of their channel count, read once; plus the row sums R1 (res floats
    # per row and tile, written once and read once) and, per call, the logs (read and written) and R2 -- a few floats per cell
    per_pixel = 4 * (4 * channels + six[2].shape[1] + six[5].shape[1])
    per_call = 4 * (2 * a.batch * a.height * ((a.width + 1023) // 1024) * a.res + 2 * a.batch * a.res ** 2 + 4 * a.res ** 3)
    out = dict(mode='spatially-adaptive', net=name, res=a.res, batch=a.batch, height=a.height, width=a.width, loss_ssim=a.loss_ssim,
               points=points, stash_bytes_per_pixel=per_pixel, stash_bytes_per_call=points * per_pixel + per_call)
    for k in res:
        meds = [w['median_ms'] for w in res[k]]
        out[f'{k}_ms'] = round(min(meds), 4)
        out[f'{k}_ms_windows'] = [round(m, 4) for m in meds]
    out['stash_fused_over_composed'] = round(out['stash_fused_ms'] / out['stash_composed_ms'], 4)
    out['stash_fused_gb_per_s'] = round(out['stash_bytes_per_call'] / out['stash_fused_ms'] / 1e6, 1)
    out['spatial_over_linear'] = round(out['spatial_fused_ms'] / out['linear_ms'], 4)
    print(json.dumps(out))


if __name__ == '__main__':
    main()
