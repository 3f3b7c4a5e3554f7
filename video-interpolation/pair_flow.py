"""Fit a flow network to ONE frame pair: the reference's video-interpolation/pair_flow.py as a command, on this project's kernels.

    python video-interpolation/pair_flow.py --input-video <sintel scene folder> --index 28
    python video-interpolation/pair_flow.py --synthetic 436 1024 --epochs 20
    python video-interpolation/pair_flow.py --synthetic 64 96 --net PFF --composed

What the reference's script fixes is fixed here (pair_flow.py:39-49): the network is built with ModelParams(domain_dim=2, std_rbf=50, std=50),
so its poses are (y, x) on the h x w grid of the pair, linspace(-1, 1, h) x linspace(-1, 1, w) (pair_flow.py:55-59); a progressive network
sits under LinearControllerEarly(net, epochs, epsilon=1e-3); the losses are L1 1, census 0.1 of width 3 and the bilateral smoothness 0.1 with
the `gauss` edge function at 150, under the `occlusion_wang` masks at 0.7 times the splats' coverage; the optimiser is FusedLAMB(lr=1e-3).
There are no notebook cells and no plots: every --log-every steps one line with l1 / census / smooth / EPE (EPE only where the pair has a
ground-truth flow).

  --input-video SCENE --index I   frames I, I + 1 of `sin_inn_amd.flowdata.Images(SCENE, --size)`
  --synthetic H W                 frames --index, --index + 1 of `SyntheticClip(max(--index + 2, 3), H, W)`, with its analytic flow
  --net                           a network with `pair` in the table of sin_inn_amd/flowcaps.py (default PRBF)
  --composed                      the same loop with the network evaluated by torch's own ops (tools/fit_flow.composed_flow_fields)

The network runs in the fused kernels: `flow_fields(net, None, h, w, scale)`, the two-coordinate call of sin_inn_amd.flownet.
"""
import argparse
import os
import sys
import time

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, 'tools')):
    if p not in sys.path:
        sys.path.insert(0, p)

from sin_inn_amd import flowcaps  # noqa: E402

NETWORKS = tuple(sorted(flowcaps.names('pair'), key=lambda name: flowcaps.TABLE[name].progressive))     # the plain ones first
PARAMS = dict(domain_dim=2, std_rbf=50, std=50)          # pair_flow.py:39
OCCL_THRESH, LR, EPSILON = 0.7, 1e-3, 1e-3


def load_pair(a):
    """(frame1, frame2 (1, 3, h, w), scale, gt (2, h, w) or None) on the CPU"""
    from sin_inn_amd import flowdata
    if a.synthetic:
        h, w = a.synthetic
        video = flowdata.SyntheticClip(max(a.index + 2, 3), h, w, seed=a.seed)
    else:
        video = flowdata.Images(a.input_video, a.size)
    item = video[a.index]
    return item[0][None], item[1][None], float(item[3]), (item[4] if len(item) == 5 else None)


def build_net(name, epochs, device, seed=0):
    """pair_flow.py:39-42"""
    from sin_inn_amd import flownet, progressive
    assert name in NETWORKS, f'--net: one of {NETWORKS}'
    torch.manual_seed(seed)
    net = flownet.flow_model_dict[name](flownet.ModelParams(**PARAMS))
    if net.is_progressive:
        net = progressive.LinearControllerEarly(net, epochs, epsilon=EPSILON)
        if net.block_iterations == 0:                          # 3 * epochs // (4 * 127): fewer than 170 epochs; the reference divides by zero
            net.block_iterations = 1                           # here such a short run opens one block per step, as main.py does
            net.progress_iterations = (net.encoding_dim - net.block_size) // net.block_size
    return net.to(device)


class PairLosses:
    """pair_flow.py:43-47 and 62-79: the masks, the two splats and the three loss terms of a step"""

    def __init__(self):
        from sin_inn_amd import flowloss as FL
        self.FL = FL
        self.l1, self.census = FL.L1Loss(1), FL.CensusLoss(0.1, max_distance=3)
        self.smooth1 = FL.BilateralSmooth(0.1, 'gauss', 150, 1)

    def __call__(self, frame1, frame2, flow12, flow21):
        """(l1, census, smooth, (mask1, mask2))"""
        from sin_inn_amd.functional import flow_warp_l1
        FL = self.FL
        mask1 = FL.occlusion_wang(flow12, flow21, OCCL_THRESH)
        mask2 = FL.occlusion_wang(flow21, flow12, OCCL_THRESH)
        _, metric = flow_warp_l1(frame1, flow21, frame2)
        softmax1 = FL.FunctionSoftsplat(frame2, flow21, -20 * metric, strType='softmax')
        mask1 = mask1 * (softmax1 != 0)
        _, metric = flow_warp_l1(frame2, flow12, frame1)
        softmax2 = FL.FunctionSoftsplat(frame1, flow12, -20 * metric, strType='softmax')
        mask2 = mask2 * (softmax2 != 0)
        l1_loss = self.l1(softmax1, frame1, mask1) + self.l1(softmax2, frame2, mask2)
        census_loss = self.census(softmax1, frame1, mask1) + self.census(softmax2, frame2, mask2)
        smooth_loss = self.smooth1(frame1, flow12) + self.smooth1(frame2, flow21)
        return l1_loss, census_loss, smooth_loss, (mask1, mask2)


def pair_flows(net, h, w, scale, composed=False):
    """(flow12, flow21), each (1, 2, h, w), contiguous: pair_flow.py:55-60"""
    if composed:
        from fit_flow import composed_flow_fields as fields
    else:
        from sin_inn_amd.flownet import flow_fields as fields
    flow12, flow21 = fields(net, None, h, w, scale)
    return flow12.contiguous(), flow21.contiguous()


def epe(flow12, gt):
    """pair_flow.py:86"""
    return ((flow12[0] - gt) ** 2).sum(dim=0).sqrt().mean()


def fit_pair(frame1, frame2, scale, gt=None, name='PRBF', epochs=1000, composed=False, seed=0, log=None, log_every=50, info=None):
    """the loop of pair_flow.py:52-88.  Returns one dict per step: loss, l1, census, smooth and (with gt) epe, floats, and `clock`, the
    host's time when the step had finished.  `info`: a dict
    that receives the network (the controller of a progressive one) as info['net'] and, as info['first'], the first step's flows and
    masks (detached)"""
    from sin_inn_amd import FusedLAMB
    device = frame1.device
    _, _, h, w = frame1.shape
    net = build_net(name, epochs, device, seed)
    if info is not None:
        info['net'] = net
    losses = PairLosses()
    opt = FusedLAMB(net.parameters(), lr=LR)
    history = []
    for epoch in range(epochs):
        opt.zero_grad()
        flow12, flow21 = pair_flows(net, h, w, scale, composed)
        l1_loss, census_loss, smooth_loss, masks = losses(frame1, frame2, flow12, flow21)
        loss = l1_loss + census_loss + smooth_loss
        loss.backward()
        opt.step()
        net.stash_iteration(loss.detach())
        rec = dict(loss=float(loss.detach()), l1=float(l1_loss.detach()), census=float(census_loss.detach()), smooth=float(smooth_loss.detach()))
        if gt is not None:
            with torch.no_grad():
                rec['epe'] = float(epe(flow12, gt))
        rec['clock'] = time.perf_counter()                     # after the floats above: the step's work has finished
        if info is not None and epoch == 0:
            info['first'] = dict(flow12=flow12.detach(), flow21=flow21.detach(), masks=tuple(m.detach() for m in masks))
        history.append(rec)
        if log and ((epoch + 1) % log_every == 0 or epoch == 0 or epoch + 1 == epochs):
            extra = f"  epe {rec['epe']:.4f}" if gt is not None else ''
            opened = f'  open {net.cur_block:3d} / {net.encoding_dim}' if net.is_progressive else ''
            log(f"step {epoch + 1:5d}  l1 {rec['l1']:.6f}  census {rec['census']:.6f}  smooth {rec['smooth']:.6f}{extra}{opened}")
    return history


def get_parser():
    ap = argparse.ArgumentParser(description=__doc__.split('\n')[0])
    ap.add_argument('--input-video', help='an Images scene folder (frame_0001.png ..)')
    ap.add_argument('--size', type=int, default=436, help='--input-video: the shorter side of the frames')
    ap.add_argument('--index', type=int, default=0, help='the pair is frames I, I + 1')
    ap.add_argument('--synthetic', nargs=2, type=int, metavar=('H', 'W'), help='a pair of a SyntheticClip of H x W instead of --input-video')
    ap.add_argument('--net', default='PRBF', choices=NETWORKS)
    ap.add_argument('--epochs', type=int, default=1000)
    ap.add_argument('--seed', type=int, default=0)
    ap.add_argument('--log-every', type=int, default=50, metavar='N')
    ap.add_argument('--composed', action='store_true', help='evaluate the network with torch ops instead of the fused kernels')
    return ap


def main(argv=None):
    ap = get_parser()
    a = ap.parse_args(argv)
    if bool(a.input_video) == bool(a.synthetic):
        ap.error('one of --input-video SCENE and --synthetic H W')
    frame1, frame2, scale, gt = load_pair(a)
    device = torch.device('cuda', 0)
    frame1, frame2 = frame1.to(device).contiguous(), frame2.to(device).contiguous()
    gt = gt.to(device) if gt is not None else None
    print(f"{a.net} {'composed' if a.composed else 'fused'}  pair {a.index}, {a.index + 1}  {frame1.shape[-2]} x {frame1.shape[-1]}  scale {scale:g}")
    history = fit_pair(frame1, frame2, scale, gt, a.net, a.epochs, a.composed, a.seed, log=print, log_every=a.log_every)
    print(f"loss: first {history[0]['loss']:.6f}  last {history[-1]['loss']:.6f}")
    steps = sorted(b['clock'] - c['clock'] for c, b in zip(history[4:], history[5:]))     # the first five steps warm up
    if steps:
        print(f'step: median {steps[len(steps) // 2] * 1e3:.2f} ms, min {steps[0] * 1e3:.2f}, max {steps[-1] * 1e3:.2f} over {len(steps)} steps '
              '(host clock, one synchronisation per step: the logged floats)')


if __name__ == '__main__':
    main()
