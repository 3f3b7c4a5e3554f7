"""The flow trainer's step restated in plain torch (helper of tests/test_flowtrainer_host.py and tests/test_gpu_flowtrainer.py;
not collected).  Nothing here calls the library.

`flow2img_ref` is my_utils/flow_viz.py:6-77 for one frame, in torch on any device.  numpy (2.x promotion rules) evaluates the clip,
the radius, its maximum and the division by it on the fp32 array in fp32, and everything after `+ np.finfo(float).eps` in float64;
so does this.  tests/test_flowtrainer_host.py ties it to the reference's own outputs through tests/golden/golden_flowtrainer.npz.

`epe_ref`, `splat_mask_ref` and `step_losses_ref` are trainer.py:58, 64 and 50-74 in the dtype of their inputs: float64 they are the
reference of the GPU tests, float32 their unit of error (the method of tests/test_gpu_flownet.py).  `step_losses_ref` is composed
from oracle/flow_oracle.py.
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


def step_masks_ref(frame1, frame2, flow12, flow21, occl, thresh):
    """trainer.py:50-68: (mask1, mask2, softmax1, softmax2) in the dtype of the inputs, on the CPU"""
    from oracle import flow_oracle as FO, sininn_oracle as O
    if occl == 'wang':
        mask1, mask2 = FO.occlusion_wang(flow12, flow21, thresh), FO.occlusion_wang(flow21, flow12, thresh)
    elif occl == 'brox':
        mask1, mask2 = FO.occlusion_brox(flow12, flow21).to(frame1.dtype), FO.occlusion_brox(flow21, flow12).to(frame1.dtype)
    else:
        mask1 = mask2 = torch.ones(frame1.shape[0], 1, *frame1.shape[2:], dtype=frame1.dtype)
    warped2 = O.flow_warp(frame1, flow21)
    metric = (frame2 - warped2).abs().mean(1, True)
    softmax1 = FO.function_softsplat(frame2, flow21, -20 * metric, 'softmax')
    mask1 = splat_mask_ref(mask1, softmax1)
    warped1 = O.flow_warp(frame2, flow12)
    metric = (frame1 - warped1).abs().mean(1, True)
    softmax2 = FO.function_softsplat(frame1, flow12, -20 * metric, 'softmax')
    mask2 = splat_mask_ref(mask2, softmax2)
    return mask1, mask2, softmax1, softmax2


def step_losses_ref(frame1, frame2, flow12, flow21, args, masks=None):
    """trainer.py:50-74: dict of l1, census, ssim, smooth, loss (0-d tensors of the inputs' dtype) and the masks used.  `masks`
    replaces the (mask1, mask2) this dtype would threshold itself (the losses are then compared on the same pixels)."""
    from oracle import flow_oracle as FO
    mask1, mask2, softmax1, softmax2 = step_masks_ref(frame1, frame2, flow12, flow21, args.occl, args.occl_thresh)
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
