"""Time the frame synthesis (sin_inn_amd.flowsynth): the fused operator and, with --baseline, `flowsynth.composed` (the same
definition from the existing operators) in the same process, alternating windows; device events, windows of at least --seconds
after a warm-up; one JSON line per K, appended to profiles/flowsynth_bench.jsonl with --log.

    python tools/bench_flowsynth.py --height 436 --width 1024 --batch 3 --factor 8 [--baseline]

K = factor - 1 times per call (tau = j / factor), and K = 1 (tau = 1 / 2) beside it.  The inputs are a SyntheticClip pair and its
ground-truth flows (the backward flow: the negative of the forward one): smooth flows of a few pixels, what a fitted network gives.
`*_bytes_per_frame` count the HBM traffic of one output frame from the definition, not from counters.

    python tools/bench_flowsynth.py --quality [--baseline]

times `flowsynth.quality` (csrc/framequality.hip) against `flowsynth.quality_composed` on batch x 7 frames, float and
quantised mode, one line each.  `min_bytes` is both frames read once; `fused_tb_per_s` is that count over the fused time.

    python tools/bench_flowsynth.py --gather [--baseline]

times the gather synthesis (csrc/flowgather.hip) at K = 1 and K = factor - 1, one `flowgather` line each: the fused operator
in both launch shapes (`lane`: one lane per (b, k, y, x); `kloop`: a lane walks the K times of its pixel), and with --baseline
`flowsynth.gather_composed` and `flowsynth.synthesize` on the same frames, alternating.  The flows are the clip's ground truth
repeated over the slot table's time slices (the operator's time does not depend on their values beyond locality).  `min_bytes` counts
4 flow words, 2 C words of the two frames at the pixel and C written per output pixel-frame (`kloop`: the 2 C words once per pixel).
Then one `flowgather_interpolate` line per K: the whole `FlowTrainer.interpolate` call -- network evaluations included, an unfitted
--net under its controller -- for splat, gather/network and gather/reverse.

    python tools/bench_flowsynth.py --gather --visible [--baseline] [--build NAME]

times the occlusion-aware rule `flowsynth.gather(.., visible=)` against the plain call in alternating windows, one
`flowgather_visible` line per K with `visible_over_plain`, the number to report; with --baseline also `gather_composed(.., visible=)`.

    python tools/bench_flowsynth.py --gather-at N [--baseline]

times forward plus backward of the point form `flowsynth.gather_at(.., blend=(0, 1), flow_grad=True)` at N random points of
the batch, one `flowgather_at_grad` line for S = 2 and one for S = 1, with --baseline against the autograd of `gather_at_composed`.
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


def bytes_per_frame(k):
    """(fused, composed) fp32 bytes per pixel of one output frame, C = 3, counted from the definition, in words:
    fused     once per call 16 (per source frame: the frame 3, the gathered other frame 3, the flow 2); per frame 35 (the 8 accumulator
              planes zeroed 8, atomically added to 16 -- a read and a write --, read back 8; the output 3)
    composed  once per call 66 (per source frame: warp + metric 12, -20 * 2, exp twice 4, frame * exp 7, cat 8); per frame 148 (per
              source frame 37.5: t * flow 4, zero-fill 4, splat 14, the guard 4, the divide 7, the hole mask 4.5; the blend 73)"""
    return 4 * (16 / k + 35), 4 * (66 / k + 148)


def quality_lines(a, dev):
    from sin_inn_amd import flowdata, flowsynth
    k = 7
    yy, xx = torch.meshgrid(torch.arange(a.height, dtype=torch.float32), torch.arange(a.width, dtype=torch.float32), indexing='ij')
    target = torch.stack([flowdata.texture(xx - 0.37 * n, yy + 0.21 * n, 0) for n in range(a.batch * k)]).clamp(0, 1)
    pred = torch.stack([flowdata.texture(xx - 0.37 * n + 0.25, yy + 0.21 * n - 0.15, 0) for n in range(a.batch * k)]).clamp(0, 1)
    target, pred = (t.view(a.batch, k, 3, a.height, a.width).to(dev) for t in (target, pred))
    ws = torch.empty(flowsynth.quality_workspace_floats(a.batch * k, 3, a.height, a.width), device=dev)
    lines = []
    for quantize in (False, True):
        todo = {'fused': lambda: flowsynth.quality(pred, target, quantize=quantize, workspace=ws)}
        if a.baseline:
            todo['composed'] = lambda: flowsynth.quality_composed(pred, target, quantize=quantize)
        res = {name: [] for name in todo}
        for _ in range(a.rounds):
            for name, fn in todo.items():
                res[name].append(window(fn, a.seconds, a.warmup))
        min_bytes = 2 * 4 * pred.numel()
        line = dict(op='frame_quality', height=a.height, width=a.width, batch=a.batch, K=k, quantize=quantize, min_bytes=min_bytes,
                    workspace_bytes=ws.numel() * 4)
        for name in res:
            meds = [w['median_ms'] for w in res[name]]
            line[f'{name}_ms'] = round(min(meds), 4)
            line[f'{name}_ms_windows'] = [round(m, 4) for m in meds]
        line['fused_tb_per_s'] = round(min_bytes / (line['fused_ms'] * 1e-3) / 1e12, 3)
        if a.baseline:
            line['speedup'] = round(line['composed_ms'] / line['fused_ms'], 3)
            f, c = flowsynth.quality(pred, target, quantize=quantize), flowsynth.quality_composed(pred, target, quantize=quantize)
            line['max_abs_ssim_diff'] = float((f.ssim - c.ssim).abs().max())
            line['max_rel_mse_diff'] = float(((f.mse - c.mse).abs() / c.mse).max())
        lines.append(line)
    return lines


def _timed(todo, a):
    """name -> (best median ms, the medians of the alternating windows)"""
    res = {name: [] for name in todo}
    for _ in range(a.rounds):
        for name, fn in todo.items():
            res[name].append(window(fn, a.seconds, a.warmup)['median_ms'])
    return {name: (round(min(m), 4), [round(v, 4) for v in m]) for name, m in res.items()}


def gather_lines(a, dev):
    from sin_inn_amd import flowdata, flownet, flowsynth, flowtrainer, progressive
    clip = flowdata.SyntheticClip(a.batch + 1, a.height, a.width)
    i0, i1 = clip.video[:-1].contiguous().to(dev), clip.video[1:].contiguous().to(dev)
    f01 = clip.flow.contiguous().to(dev)
    f10 = (-clip.flow).contiguous().to(dev)
    dt = 2 / a.batch
    times = clip.T[:-1]
    torch.manual_seed(0)
    net = flownet.flow_model_dict[a.net](flownet.ModelParams())
    if getattr(net, 'is_progressive', False):
        net = progressive.LinearControllerEarly(net, 1000, epsilon=1e-3)
    args = argparse.Namespace(lr=1e-4, loss_l1=1, loss_census=0.1, loss_ssim=0.05, census_width=3, loss_smooth1=0.1, edge_constant=150,
                              edge_func='gauss', occl='wang', occl_thresh=0.7, net=net.to(dev))
    model = flowtrainer.FlowTrainer(args).to(dev)
    batch = [i0, i1, times.to(dev), clip.flow_scale]
    lines = []
    for k in sorted({1, a.factor - 1}):
        taus = [0.5] if k == 1 else [j / a.factor for j in range(1, a.factor)]
        tau_dev = torch.tensor(taus, dtype=torch.float32, device=dev)
        stamps, slots = flowsynth.gather_slots(times, taus, dt)
        per_b = len(stamps) // a.batch + 1
        flows = torch.cat([f01, f10], 1).repeat_interleave(per_b, 0)[:len(stamps)].contiguous()     # every slice a ground-truth pair
        table = flowsynth.upload_slots(slots, dev)
        out = torch.empty(a.batch, k, 3, a.height, a.width, device=dev)
        ws = torch.empty(flowsynth.workspace_floats(a.batch, k, 3, a.height, a.width), device=dev)
        todo = {'lane': lambda: flowsynth.gather(i0, i1, flows, table, tau_dev, out=out, k_loop=False),
                'kloop': lambda: flowsynth.gather(i0, i1, flows, table, tau_dev, out=out, k_loop=True)}
        if a.baseline:
            todo['composed'] = lambda: flowsynth.gather_composed(i0, i1, flows, slots, taus)
            todo['splat'] = lambda: flowsynth.synthesize(i0, i1, f01, f10, tau_dev, out=out, workspace=ws)
        pixels = a.batch * a.height * a.width
        line = dict(op='flowgather', height=a.height, width=a.width, batch=a.batch, K=k, slices=len(stamps),
                    min_bytes_lane=4 * pixels * k * (4 + 6 + 3), min_bytes_kloop=4 * pixels * (k * (4 + 3) + 6))
        for name, (best, meds) in _timed(todo, a).items():
            line[f'{name}_ms'], line[f'{name}_ms_windows'] = best, meds
        for name in ('lane', 'kloop'):
            line[f'{name}_tb_per_s'] = round(line[f'min_bytes_{name}'] / (line[f'{name}_ms'] * 1e-3) / 1e12, 3)
        if a.baseline:
            best = min(line['lane_ms'], line['kloop_ms'])
            line['composed_over_fused'] = round(line['composed_ms'] / best, 3)
            line['splat_over_gather'] = round(line['splat_ms'] / best, 3)
            line['max_abs_diff_composed'] = float((flowsynth.gather(i0, i1, flows, table, tau_dev)
                                                   - flowsynth.gather_composed(i0, i1, flows, slots, taus)).abs().max())
        print(json.dumps(line), flush=True)
        lines.append(line)
        calls = {'splat': lambda: model.interpolate(batch, taus),
                 'gather_network': lambda: model.interpolate(batch, taus, synthesis='gather', dt=dt),
                 'gather_reverse': lambda: model.interpolate(batch, taus, synthesis='gather', dt=dt, back='reverse')}
        line = dict(op='flowgather_interpolate', net=a.net, height=a.height, width=a.width, batch=a.batch, K=k,
                    stamps_splat=a.batch, stamps_gather_network=len(stamps), stamps_gather_reverse=a.batch * k)
        for name, (best, meds) in _timed(calls, a).items():
            line[f'{name}_ms'], line[f'{name}_ms_windows'] = best, meds
        print(json.dumps(line), flush=True)
        lines.append(line)
    return lines


def gather_visible_lines(a, dev):
    """the masked rule `gather(.., visible=)` against the plain call and (with --baseline) against `gather_composed(.., visible=)`
    (DESIGN 26), K = 1 and factor - 1, in alternating windows of one session.  The masks are hard 0 / 1 planes with a hidden band of
    width // 16 columns; min_bytes counts them as the 2 (4 taps, one cache line or two) planes more that a (b, k) lane reads."""
    from sin_inn_amd import flowdata, flowsynth
    clip = flowdata.SyntheticClip(a.batch + 1, a.height, a.width)
    i0, i1 = clip.video[:-1].contiguous().to(dev), clip.video[1:].contiguous().to(dev)
    f01, f10 = clip.flow.contiguous().to(dev), (-clip.flow).contiguous().to(dev)
    dt, times = 2 / a.batch, clip.T[:-1]
    m0 = torch.ones(a.batch, 1, a.height, a.width, device=dev)
    m1 = torch.ones(a.batch, 1, a.height, a.width, device=dev)
    m0[..., a.width // 4:a.width // 4 + a.width // 16] = 0
    m1[..., a.width // 2:a.width // 2 + a.width // 16] = 0
    lines = []
    for k in sorted({1, a.factor - 1}):
        taus = [0.5] if k == 1 else [j / a.factor for j in range(1, a.factor)]
        tau_dev = torch.tensor(taus, dtype=torch.float32, device=dev)
        stamps, slots = flowsynth.gather_slots(times, taus, dt)
        per_b = len(stamps) // a.batch + 1
        flows = torch.cat([f01, f10], 1).repeat_interleave(per_b, 0)[:len(stamps)].contiguous()
        table = flowsynth.upload_slots(slots, dev)
        out = torch.empty(a.batch, k, 3, a.height, a.width, device=dev)
        todo = {'plain': lambda: flowsynth.gather(i0, i1, flows, table, tau_dev, out=out),
                'visible': lambda: flowsynth.gather(i0, i1, flows, table, tau_dev, out=out, visible=(m0, m1))}
        if a.baseline:
            todo['composed'] = lambda: flowsynth.gather_composed(i0, i1, flows, slots, taus, visible=(m0, m1))
        pixels = a.batch * a.height * a.width
        line = dict(op='flowgather_visible', height=a.height, width=a.width, batch=a.batch, K=k, slices=len(stamps),
                    min_bytes_plain=4 * pixels * k * (4 + 6 + 3), min_bytes_visible=4 * pixels * k * (4 + 6 + 3 + 2))
        for name, (best, meds) in _timed(todo, a).items():
            line[f'{name}_ms'], line[f'{name}_ms_windows'] = best, meds
        line['visible_over_plain'] = round(line['visible_ms'] / line['plain_ms'], 3)
        line['visible_tb_per_s'] = round(line['min_bytes_visible'] / (line['visible_ms'] * 1e-3) / 1e12, 3)
        if a.baseline:
            line['composed_over_fused'] = round(line['composed_ms'] / line['visible_ms'], 3)
            line['max_abs_diff_composed'] = float((flowsynth.gather(i0, i1, flows, table, tau_dev, visible=(m0, m1))
                                                   - flowsynth.gather_composed(i0, i1, flows, slots, taus, visible=(m0, m1))).abs().max())
        line['build'] = a.build
        print(json.dumps(line), flush=True)
        lines.append(line)
    return lines


def gather_grad_lines(a, dev):
    """forward plus backward of gather(.., flow_grad=True) against the autograd of gather_composed on the device, K = 1
    and factor - 1, on the regular table of gather_slots (reverse rows for the clip's first pair: the two-launch backward path)"""
    from sin_inn_amd import flowdata, flowsynth
    clip = flowdata.SyntheticClip(a.batch + 1, a.height, a.width)
    i0, i1 = clip.video[:-1].contiguous().to(dev), clip.video[1:].contiguous().to(dev)
    f01, f10 = clip.flow.contiguous().to(dev), (-clip.flow).contiguous().to(dev)
    dt, times = 2 / a.batch, clip.T[:-1]
    lines = []
    for k in sorted({1, a.factor - 1}):
        taus = [0.5] if k == 1 else [j / a.factor for j in range(1, a.factor)]
        stamps, slots = flowsynth.gather_slots(times, taus, dt)
        per_b = len(stamps) // a.batch + 1
        flows = torch.cat([f01, f10], 1).repeat_interleave(per_b, 0)[:len(stamps)].contiguous().requires_grad_(True)
        g = torch.randn(a.batch, k, 3, a.height, a.width, device=dev)

        def step(fn):
            flows.grad = None
            fn(i0, i1, flows, slots, taus, flow_grad=True).backward(g)
            return flows.grad

        todo = {'fused': lambda: step(flowsynth.gather)}
        if a.baseline:
            todo['composed'] = lambda: step(flowsynth.gather_composed)
        pixels = a.batch * a.height * a.width
        # words per pixel-frame, C = 3: forward 13; backward flows 4, taps 6, I(p) 6, g 3, the row buffer written 4 and
        # read 4; and d flows written once, 4 words per pixel of every slice
        min_bytes = 4 * pixels * k * (13 + 27) + 4 * 4 * len(stamps) * a.height * a.width
        line = dict(op='flowgather_grad', height=a.height, width=a.width, batch=a.batch, K=k, slices=len(stamps), min_bytes=min_bytes,
                    min_bytes_backward=min_bytes - 4 * pixels * k * 13)
        for name, (best, meds) in _timed(todo, a).items():
            line[f'{name}_ms'], line[f'{name}_ms_windows'] = best, meds
        line['fused_tb_per_s'] = round(min_bytes / (line['fused_ms'] * 1e-3) / 1e12, 3)       # forward plus backward bytes over their time
        if a.baseline:
            line['composed_over_fused'] = round(line['composed_ms'] / line['fused_ms'], 3)
            line['max_abs_diff_composed'] = float((step(flowsynth.gather).clone() - step(flowsynth.gather_composed)).abs().max())
        print(json.dumps(line), flush=True)
        lines.append(line)
    return lines


def gather_at_lines(a, dev):
    """forward plus backward of gather_at(.., blend=(0, 1), flow_grad=True) at N random points against the autograd of
    gather_at_composed on the device: S = 2 with the first pair's points reversed, and S = 1.  min_bytes, C = 3, per
    point: forward pix 2, pair, tau, flows 4, taps 2 x 4 x 3 x 2 (q and p), out 2 x 3 written; backward the same reads, g 6 read, the
    column's 4 S words written."""
    from sin_inn_amd import flowdata, flowsynth
    clip = flowdata.SyntheticClip(a.batch + 1, a.height, a.width)
    i0, i1 = clip.video[:-1].contiguous().to(dev), clip.video[1:].contiguous().to(dev)
    n = a.gather_at
    gen = torch.Generator(device=dev).manual_seed(0)
    pair = torch.randint(0, a.batch, (n,), generator=gen, device=dev, dtype=torch.int32)
    u = torch.rand(3, n, generator=gen, device=dev)
    tau, pix = u[0].contiguous(), torch.stack((u[1] * (a.height - 1), u[2] * (a.width - 1)), 1)
    at = pair.long() * a.height * a.width + pix[:, 0].round().long() * a.width + pix[:, 1].round().long()
    truth = torch.cat([clip.flow, -clip.flow], 1).to(dev).permute(1, 0, 2, 3).reshape(4, -1)[:, at]       # the clip's flows at the points
    lines = []
    for s in (2, 1):
        flows = torch.stack([truth] * s).contiguous().requires_grad_(True)
        rev = (pair == 0) if s == 2 else None
        g = torch.randn(2, n, 3, device=dev)

        def step(fn):
            flows.grad = None
            fn(i0, i1, flows, pix, pair, tau, rev, blend=(0.0, 1.0), flow_grad=True).backward(g)
            return flows.grad

        todo = {'fused': lambda: step(flowsynth.gather_at)}
        if a.baseline:
            todo['composed'] = lambda: step(flowsynth.gather_at_composed)
        reads = 2 + 1 + 1 + 4 + 48
        min_bytes = 4 * n * ((reads + 6) + (reads + 6 + 4 * s))
        line = dict(op='flowgather_at_grad', height=a.height, width=a.width, batch=a.batch, N=n, S=s, R=2, min_bytes=min_bytes)
        for name, (best, meds) in _timed(todo, a).items():
            line[f'{name}_ms'], line[f'{name}_ms_windows'] = best, meds
        line['fused_tb_per_s'] = round(min_bytes / (line['fused_ms'] * 1e-3) / 1e12, 3)
        if a.baseline:
            line['composed_over_fused'] = round(line['composed_ms'] / line['fused_ms'], 3)
            line['max_abs_diff_composed'] = float((step(flowsynth.gather_at).clone() - step(flowsynth.gather_at_composed)).abs().max())
        print(json.dumps(line), flush=True)
        lines.append(line)
    return lines


def main():
    from sin_inn_amd import flowdata, flowsynth
    ap = argparse.ArgumentParser(description=__doc__.split('\n')[0])
    ap.add_argument('--height', type=int, default=436)
    ap.add_argument('--width', type=int, default=1024)
    ap.add_argument('--batch', type=int, default=3)
    ap.add_argument('--factor', type=int, default=8)
    ap.add_argument('--seconds', type=float, default=1.0)
    ap.add_argument('--warmup', type=int, default=5)
    ap.add_argument('--rounds', type=int, default=3, help='alternations of the fused and the composed windows')
    ap.add_argument('--baseline', action='store_true')
    ap.add_argument('--log', action='store_true', help='append the lines to profiles/flowsynth_bench.jsonl')
    ap.add_argument('--quality', action='store_true', help='time flowsynth.quality (and with --baseline quality_composed) instead')
    ap.add_argument('--gather', action='store_true', help='time flowsynth.gather and the whole interpolate call instead (DESIGN 19)')
    ap.add_argument('--gather-grad', action='store_true',
                    help='time forward plus backward of flowsynth.gather(.., flow_grad=True) (and with --baseline the autograd of gather_composed) instead (DESIGN 22)')
    ap.add_argument('--gather-at', type=int, metavar='N',
                    help='time forward plus backward of flowsynth.gather_at at N points (and with --baseline the autograd of gather_at_composed) instead (DESIGN 23)')
    ap.add_argument('--visible', action='store_true',
                    help='--gather: time the masked rule gather(.., visible=) against the plain call (and with --baseline gather_composed(.., visible=)) instead (DESIGN 26)')
    ap.add_argument('--build', default='tree', help='--visible: what the `build` field of the lines says')
    ap.add_argument('--net', default='PRBF', help='--gather: the network of the whole-call lines')
    a = ap.parse_args()
    assert 2 <= a.factor <= 65
    dev = torch.device('cuda', 0)
    if a.quality or a.gather or a.gather_grad or a.gather_at:
        lines = (gather_at_lines(a, dev) if a.gather_at else gather_grad_lines(a, dev) if a.gather_grad else gather_visible_lines(a, dev)
                 if a.gather and a.visible else gather_lines(a, dev) if a.gather else quality_lines(a, dev))
        for line in ([] if a.gather or a.gather_grad or a.gather_at else lines):   # the gather lines are printed as they are measured
            print(json.dumps(line))
        if a.log:
            with open(os.path.join(ROOT, 'profiles', 'flowsynth_bench.jsonl'), 'a') as f:
                for line in lines:
                    f.write(json.dumps(line) + '\n')
        return
    clip = flowdata.SyntheticClip(a.batch + 1, a.height, a.width)
    i0, i1 = clip.video[:-1].contiguous().to(dev), clip.video[1:].contiguous().to(dev)
    f01 = clip.flow.contiguous().to(dev)
    f10 = (-clip.flow).contiguous().to(dev)
    lines = []
    for k in sorted({1, a.factor - 1}):
        taus = [0.5] if k == 1 else [j / a.factor for j in range(1, a.factor)]
        tau_dev = torch.tensor(taus, dtype=torch.float32, device=dev)
        ws = torch.empty(flowsynth.workspace_floats(a.batch, k, 3, a.height, a.width), device=dev)
        out = torch.empty(a.batch, k, 3, a.height, a.width, device=dev)
        todo = {'fused': lambda: flowsynth.synthesize(i0, i1, f01, f10, tau_dev, out=out, workspace=ws)}
        if a.baseline:
            todo['composed'] = lambda: flowsynth.composed(i0, i1, f01, f10, taus)
        res = {name: [] for name in todo}
        for _ in range(a.rounds):
            for name, fn in todo.items():
                res[name].append(window(fn, a.seconds, a.warmup))
        fb, cb = bytes_per_frame(k)
        line = dict(op='flowsynth', height=a.height, width=a.width, batch=a.batch, K=k, workspace_bytes=ws.numel() * 4,
                    fused_bytes_per_pixel_frame=round(fb, 1), composed_bytes_per_pixel_frame=round(cb, 1))
        for name in res:
            meds = [w['median_ms'] for w in res[name]]
            line[f'{name}_ms'] = round(min(meds), 4)
            line[f'{name}_ms_windows'] = [round(m, 4) for m in meds]
        line['fused_ms_per_frame'] = round(line['fused_ms'] / k, 4)
        if a.baseline:
            line['speedup'] = round(line['composed_ms'] / line['fused_ms'], 3)
        print(json.dumps(line))
        lines.append(line)
    if a.log:
        os.makedirs(os.path.join(ROOT, 'profiles'), exist_ok=True)
        with open(os.path.join(ROOT, 'profiles', 'flowsynth_bench.jsonl'), 'a') as f:
            for line in lines:
                f.write(json.dumps(line) + '\n')


if __name__ == '__main__':
    main()
