"""The flow trainer's step restated in plain torch (helper of tests/test_flowtrainer_host.py and tests/test_gpu_flowtrainer.py;
not collected).  Nothing here calls the library.

`flow2img_ref` is my_utils/flow_viz.py:6-77 for one frame, in torch on any device.  numpy (2.x promotion rules) evaluates the clip,
the radius, its maximum and the division by it on the fp32 array in fp32, and everything after `+ np.finfo(float).eps` in float64;
so does this.  tests/test_flowtrainer_host.py ties it to the reference's own outputs through tests/golden/golden_flowtrainer.npz.

`epe_ref`, `splat_mask_ref` and `step_losses_ref` are trainer.py:58, 64 and 50-74 in the dtype of their inputs: float64 they are the
reference of the GPU tests, float32 their unit of error (the method of tests/test_gpu_flownet.py).  `step_losses_ref` is composed
from oracle/flow_oracle.py.

`smooth_flows`, `grad_case`, `step_grads_ref` and the helpers after them serve tests/test_flowtrainer_grads_host.py and
tests/test_gpu_flowtrainer_grads.py: the inputs of their cases and the step's gradient with respect to the two flows under
torch.autograd.  They build the library's data sets and networks on the CPU and run none of its kernels.
"""
import math
import os

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
MISMATCH_CAP = 1e-4                 # at most 1 value in 10^4 may differ from a fixture image, and only by one level


def fixture():
    return np.load(os.path.join(ROOT, 'tests', 'golden', 'golden_flowtrainer.npz'))


F2I_CASES = ('random', 'clip50', 'zero', 'unknown', 'radial')


def color_wheel_ref():
    """flow_viz.py:80-127, written out segment by segment"""
    rows = []
    for i in range(15):
        rows.append((255, math.floor(255 * i / 15), 0))           # red -> yellow
    for i in range(6):
        rows.append((255 - math.floor(255 * i / 6), 255, 0))      # yellow -> green
    for i in range(4):
        rows.append((0, 255, math.floor(255 * i / 4)))            # green -> cyan
    for i in range(11):
        rows.append((0, 255 - math.floor(255 * i / 11), 255))     # cyan -> blue
    for i in range(13):
        rows.append((math.floor(255 * i / 13), 0, 255))           # blue -> magenta
    for i in range(6):
        rows.append((255, 0, 255 - math.floor(255 * i / 6)))      # magenta -> red
    return torch.tensor(rows, dtype=torch.float64)


def flow2img_ref(flow, clip=10):
    """(2, h, w) fp32 -> (3, h, w) uint8"""
    flow = flow.to(torch.float32)
    uv = torch.where(torch.isnan(flow), flow, flow.clamp(-clip, clip))
    u, v = uv[0].clone(), uv[1].clone()
    unknown = (u.abs() > 1e7) | (v.abs() > 1e7)
    u[unknown] = 0
    v[unknown] = 0
    rad = (u * u + v * v).sqrt()
    radmax = float('nan') if bool(torch.isnan(rad).any()) else float(rad.max())
    maxrad = torch.tensor(max(-1, radmax), dtype=torch.float32, device=flow.device)      # Python's max: max(-1, nan) is -1
    eps = 2.220446049250313e-16
    u = (u / maxrad).to(torch.float64) + eps
    v = (v / maxrad).to(torch.float64) + eps
    nan = torch.isnan(u) | torch.isnan(v)
    u = torch.where(nan, torch.zeros_like(u), u)
    v = torch.where(nan, torch.zeros_like(v), v)
    wheel = color_wheel_ref().to(flow.device)
    ncols = wheel.shape[0]
    rad = (u * u + v * v).sqrt()
    a = torch.atan2(-v, -u) / math.pi
    fk = (a + 1) / 2 * (ncols - 1) + 1
    k0 = torch.floor(fk).long()
    k1 = k0 + 1
    k1[k1 == ncols + 1] = 1
    f = fk - k0
    img = torch.zeros((3,) + tuple(u.shape), dtype=torch.uint8, device=flow.device)
    for i in range(3):
        col0 = wheel[k0 - 1, i] / 255
        col1 = wheel[k1 - 1, i] / 255
        col = (1 - f) * col0 + f * col1
        col = torch.where(rad <= 1, 1 - rad * (1 - col), col * 0.75)
        img[i] = torch.floor(255 * col * (1 - nan.to(torch.float64))).to(torch.uint8)
    img[:, unknown] = 0
    return img


def image_mismatch(got, want):
    """(number of differing values, largest difference in levels) of two uint8 images"""
    d = (torch.as_tensor(got).to(torch.int16) - torch.as_tensor(want).to(torch.int16)).abs()
    return int((d != 0).sum()), int(d.max()) if d.numel() else 0


def assert_image_close(got, want, what):
    """the fixture condition: at most 1 value in 10^4 differs, and only by one level"""
    count, worst = image_mismatch(got, want)
    total = torch.as_tensor(want).numel()
    print(f'{what}: {count} of {total} values differ, worst {worst} level(s)')
    assert tuple(torch.as_tensor(got).shape) == tuple(torch.as_tensor(want).shape), what
    assert count <= MISMATCH_CAP * total and worst <= 1, (what, count, total, worst)


def epe_ref(flow, gt):
    """trainer.py:58"""
    return torch.sum((flow - gt) ** 2, dim=1).sqrt().mean()


def splat_mask_ref(mask, splat):
    """trainer.py:64"""
    return mask * (splat != 0)


def _softmax_splat_ref(inp, flow, metric, detach=()):
    """FunctionSoftsplat(inp, flow, -20 metric, 'softmax').  `detach` cuts edges of the graph (the values stay): 'metric', the warp's L1
    metric into the splat; 'normaliser', the splatted last channel before the division.  Without a cut this is the oracle's own function."""
    from oracle import flow_oracle as FO
    if 'metric' in detach:
        metric = metric.detach()
    if 'normaliser' not in detach:
        return FO.function_softsplat(inp, flow, -20 * metric, 'softmax')
    e = (-20 * metric).exp()                                  # flow_oracle.function_softsplat, the softmax branch, with the one cut
    out = FO.softsplat_sum(torch.cat([inp * e, e], 1), flow)
    norm = out[:, -1:].detach()
    norm = torch.where(norm == 0.0, torch.ones_like(norm), norm)
    return out[:, :-1] / norm


def step_masks_ref(frame1, frame2, flow12, flow21, occl, thresh, detach=()):
    """trainer.py:50-68: (mask1, mask2, softmax1, softmax2) in the dtype of the inputs, on the CPU.  `detach`: see `_softmax_splat_ref`
    (only the gradient tests' power check passes one)."""
    from oracle import flow_oracle as FO, sininn_oracle as O
    if occl == 'wang':
        mask1, mask2 = FO.occlusion_wang(flow12, flow21, thresh), FO.occlusion_wang(flow21, flow12, thresh)
    elif occl == 'brox':
        mask1, mask2 = FO.occlusion_brox(flow12, flow21).to(frame1.dtype), FO.occlusion_brox(flow21, flow12).to(frame1.dtype)
    else:
        mask1 = mask2 = torch.ones(frame1.shape[0], 1, *frame1.shape[2:], dtype=frame1.dtype)
    warped2 = O.flow_warp(frame1, flow21)
    metric = (frame2 - warped2).abs().mean(1, True)
    softmax1 = _softmax_splat_ref(frame2, flow21, metric, detach)
    mask1 = splat_mask_ref(mask1, softmax1)
    warped1 = O.flow_warp(frame2, flow12)
    metric = (frame1 - warped1).abs().mean(1, True)
    softmax2 = _softmax_splat_ref(frame1, flow12, metric, detach)
    mask2 = splat_mask_ref(mask2, softmax2)
    return mask1, mask2, softmax1, softmax2


def step_losses_ref(frame1, frame2, flow12, flow21, args, masks=None, detach=()):
    """trainer.py:50-74: dict of l1, census, ssim, smooth, loss (0-d tensors of the inputs' dtype) and the masks used.  `masks`
    replaces the (mask1, mask2) this dtype would threshold itself (the losses are then compared on the same pixels).  `detach`: graph
    edges to cut, see `_softmax_splat_ref`."""
    from oracle import flow_oracle as FO
    mask1, mask2, softmax1, softmax2 = step_masks_ref(frame1, frame2, flow12, flow21, args.occl, args.occl_thresh, detach)
    if masks is not None:
        mask1, mask2 = (m.to(frame1.dtype) for m in masks)
    out = {
        'l1': FO.l1_loss(softmax1, frame1, mask1, args.loss_l1) + FO.l1_loss(softmax2, frame2, mask2, args.loss_l1),
        'census': FO.census_loss(softmax1, frame1, mask1, args.loss_census, args.census_width)
                  + FO.census_loss(softmax2, frame2, mask2, args.loss_census, args.census_width),
        'ssim': FO.ssim_loss(softmax1, frame1, mask1, args.loss_ssim) + FO.ssim_loss(softmax2, frame2, mask2, args.loss_ssim),
        'smooth': FO.bilateral_smooth(frame1, flow12, args.loss_smooth1, args.edge_func, args.edge_constant, 1)
                  + FO.bilateral_smooth(frame2, flow21, args.loss_smooth1, args.edge_func, args.edge_constant, 1),
    }
    out['loss'] = out['l1'] + out['census'] + out['ssim'] + out['smooth']
    return out, (mask1, mask2)


# ---- the step's gradient with respect to the flows (tests/test_flowtrainer_grads_host.py, tests/test_gpu_flowtrainer_grads.py) ----

GRAD_TERMS = ('l1', 'census', 'ssim', 'smooth', 'loss')
GRAD_ARGS = dict(lr=1e-4, loss_l1=1, loss_census=0.1, loss_ssim=0.05, census_width=3, loss_smooth1=0.1, edge_constant=150, edge_func='gauss',
                 occl='wang', occl_thresh=0.7, net=None)            # `_args` of tests/test_gpu_flowtrainer.py
# name -> (frame pairs, h, w, seed, what differs from GRAD_ARGS, px added to flow21[:, 0]).  (1, 37, 70) is the smallest shape that
# crosses a 32 x 8 splat tile and the 16 x 16 census / SSIM tiles in both directions with ragged edges; 'band' leaves target pixels
# that nothing lands on.
GRAD_CASES = {
    'wang 24x40': (2, 24, 40, 0, {}, 0.0),
    'wang 13x37': (2, 13, 37, 0, {}, 0.0),
    'brox 24x40': (2, 24, 40, 0, dict(occl='brox'), 0.0),
    'none 24x40': (2, 24, 40, 0, dict(occl=None), 0.0),
    'nossim 24x40': (2, 24, 40, 0, dict(loss_ssim=0), 0.0),
    'wang 1x37x70': (1, 37, 70, 0, {}, 0.0),
    'band 24x40': (2, 24, 40, 0, {}, 12.0),
}


def grad_args(**kw):
    import argparse
    return argparse.Namespace(**{**GRAD_ARGS, **kw})


def smooth_flows(clip, seed, pairs=None):
    """(flow12, flow21), fp32 (pairs, 2, h, w): the clip's ground truth (and its negative) plus half a pixel of smooth noise, a
    (pairs, 2, 4, 5) normal field from Generator(seed + 10) enlarged bicubically (align_corners) to the frame.  Smooth and close to the
    truth: the flows a trainer meets after its first epochs, and far from every threshold of the step."""
    n = clip.flow.shape[0] if pairs is None else pairs
    h, w = clip.flow.shape[-2:]
    g = torch.Generator().manual_seed(seed + 10)

    def up():
        return torch.nn.functional.interpolate(torch.randn(n, 2, 4, 5, generator=g), size=(h, w), mode='bicubic', align_corners=True)

    gt = clip.flow[:n]
    return (gt + 0.5 * up()).contiguous(), (-gt + 0.5 * up()).contiguous()


def grad_case(name):
    """(frame1, frame2, flow12, flow21, args) of GRAD_CASES[name]: fp32 CPU tensors and the trainer's namespace"""
    from sin_inn_amd import flowdata
    n, h, w, seed, kw, shift = GRAD_CASES[name]
    clip = flowdata.SyntheticClip(3, h, w, seed=seed)
    flow12, flow21 = smooth_flows(clip, seed, n)
    if shift:
        flow21 = flow21.clone()
        flow21[:, 0] += shift
    return clip.video[0:n].contiguous(), clip.video[1:n + 1].contiguous(), flow12, flow21, grad_args(**kw)


def step_grads_ref(frame1, frame2, flow12, flow21, args, masks, dtype, detach=()):
    """{term: (dflow12, dflow21)} of `step_losses_ref` evaluated in `dtype` on the given fp32 inputs (widened) and the given masks, for
    the terms of GRAD_TERMS whose weight is not zero ('loss': their sum).  `detach`: graph edges cut in the reference -- only the power
    check of the tests passes one."""
    frame1, frame2 = frame1.detach().to(dtype), frame2.detach().to(dtype)
    f12, f21 = (f.detach().to(dtype).clone().requires_grad_(True) for f in (flow12, flow21))
    out, _ = step_losses_ref(frame1, frame2, f12, f21, args, masks=masks, detach=detach)
    weights = dict(l1=args.loss_l1, census=args.loss_census, ssim=args.loss_ssim, smooth=args.loss_smooth1, loss=1)
    grads = {}
    for term in GRAD_TERMS:
        if weights[term] != 0:
            grads[term] = torch.autograd.grad(out[term], (f12, f21), retain_graph=True)
    return grads


def relmax(a, ref):
    """max |a - ref| / max |ref| in float64; a value that is not finite counts as an infinite error"""
    a, ref = a.detach().to(torch.float64).cpu(), ref.detach().to(torch.float64).cpu()
    err = (a - ref).abs()
    err = torch.where(torch.isfinite(a), err, torch.full_like(err, float('inf')))
    return float(err.max() / ref.abs().max())


def grad_units(ref32, ref64):
    """{(term, 'flow12' | 'flow21'): the fp32-torch unit, max |g32 - g64| / max |g64|}"""
    return {(t, f): relmax(ref32[t][i], ref64[t][i]) for t in ref64 for i, f in enumerate(('flow12', 'flow21'))}


def all_taps_outside(flow):
    """(n, h, w) bool: source pixels whose four splat taps fall outside the frame, whether x + flow is rounded to fp32 (the kernels)
    or not (float64).  A pixel on which the two disagree is left out."""
    n, _, h, w = flow.shape
    out = None
    for dtype in (torch.float32, torch.float64):
        ys, xs = torch.meshgrid(torch.arange(h, dtype=dtype), torch.arange(w, dtype=dtype), indexing='ij')
        nwx, nwy = torch.floor(xs[None] + flow[:, 0].to(dtype)), torch.floor(ys[None] + flow[:, 1].to(dtype))
        o = (nwx + 1 < 0) | (nwx >= w) | (nwy + 1 < 0) | (nwy >= h)
        out = o if out is None else out & o
    return out


STEP_NETS = ('RBF', 'PRBF', 'siren', 'MPFF')                   # the networks of the gradient tests' training_step cases
PAIR_NET = 'PRBF'                                               # and of the pair fit (two coordinates)


def step_net(name):
    """the network of a step case on the CPU, seeded; a progressive one under LinearControllerEarly(net, 1000, epsilon=1e-3)"""
    from sin_inn_amd import flownet, progressive
    torch.manual_seed(0)
    net = flownet.flow_model_dict[name](flownet.ModelParams())
    if getattr(net, 'is_progressive', False):
        net = progressive.LinearControllerEarly(net, 1000, epsilon=1e-3)
    return net


def step_batch():
    """SyntheticClip(3, 24, 40), batch 2: [frame1, frame2, times, scale, gt] as the trainer's loader collates them"""
    from sin_inn_amd import flowdata
    clip = flowdata.SyntheticClip(3, 24, 40, seed=0)
    return [clip.video[0:2], clip.video[1:3], clip.T[0:2], torch.tensor([clip.flow_scale] * 2, dtype=torch.float64), clip.flow[0:2]]


def pair_inputs():
    """(frame1, frame2, scale) of video-interpolation/pair_flow.py --synthetic 24 40"""
    from sin_inn_amd import flowdata
    item = flowdata.SyntheticClip(3, 24, 40, seed=0)[0]
    return item[0][None].contiguous(), item[1][None].contiguous(), float(item[3])


def pair_flow_module():
    """video-interpolation/pair_flow.py as a module, loaded from its file: its folder holds a main.py of its own and stays off sys.path"""
    import importlib.util
    spec = importlib.util.spec_from_file_location('pair_flow_cmd', os.path.join(ROOT, 'video-interpolation', 'pair_flow.py'))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def composed_flows(net, times, h, w, scale):
    """the flows of `net` from torch's own ops on the CPU (tools/fit_flow.composed_flow_fields): what the fused kernels compute, to fp32
    rounding -- the host file checks its conditions on them"""
    import sys
    tools = os.path.join(ROOT, 'tools')
    if tools not in sys.path:
        sys.path.insert(0, tools)
    from fit_flow import composed_flow_fields
    with torch.no_grad():
        flow12, flow21 = composed_flow_fields(net, times, h, w, scale)
    return flow12.contiguous(), flow21.contiguous()
