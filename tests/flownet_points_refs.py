"""The flow-field networks restated on a POSE LIST (N, 3) in any dtype: what tests/test_gpu_flownet_points.py holds the points mode of the
kernels against (sin_inn_amd.flownet.flow_at, sininn_flownet_*_points / sininn_siren_*_points).  Built from tests/flownet_refs.py
(`layer1_input` takes poses already; the MLP part follows `restate`) and tests/siren_refs.py.  Outputs are planar, (4, N), the kernels'
own layout.  A plain module, no fixtures.
"""
import torch
import torch.nn.functional as nnf

from flownet_refs import layer1_input
from siren_refs import OMEGA


def grid_poses(times, ys, xs):
    """the reference's construction (trainer.py:40-43): meshgrid -> stack -> view(-1, 3), a contiguous (N, 3) tensor"""
    gt, gh, gw = torch.meshgrid(times, ys, xs, indexing='ij')
    return torch.stack((gt, gh, gw), dim=-1).view(-1, 3)


def restate_points(name, bufs, weights, poses, scale, dtype, mask=None, gates=None):
    """net(poses)^T * scale, (4, N), in `dtype` from the fp32 poses / buffers / weights (widened); the arguments of flownet_refs.restate
    with a pose list in place of the three axis vectors"""
    weights = [p.to(dtype) for p in weights]
    x = layer1_input(name, bufs, poses.to(dtype), mask)
    for l in range(3):
        pre = nnf.linear(x, weights[2 * l], weights[2 * l + 1])
        x = torch.relu(pre) if gates is None else pre * gates[l].to(dtype)
    return nnf.linear(x, weights[6], weights[7]).t() * scale


def siren_restate_points(weights, poses, scale, dtype, omega=OMEGA):
    """siren_refs.siren_restate on a pose list: (4, N)"""
    x = poses.to(dtype)
    w = [p.to(dtype) for p in weights]
    for l in range(4):
        x = torch.sin(omega * nnf.linear(x, w[2 * l], w[2 * l + 1]))
    return nnf.linear(x, w[8], w[9]).t() * scale


def reference_grads_points(name, bufs, weights, poses, scale, up, mask, gates):
    """flownet_refs.reference_grads on a pose list: {dtype: (flows, gradients of sum(flows * up) with respect to the weights and, where
    `bufs` is the frequency matrix F_eff itself (RFF / PRFF), with respect to it as the last entry)}, the kernel's own gates forced.
    name == 'siren': weights are the ten tensors of siren_refs.siren_tensors, bufs / mask / gates unused (no gates: the sine is smooth)"""
    out = {}
    for dtype in (torch.float64, torch.float32):
        w = [p.to(dtype).requires_grad_(True) for p in weights]
        leaves = list(w)
        if name == 'siren':
            flows = siren_restate_points(w, poses, scale, dtype)
        else:
            b = bufs
            if torch.is_tensor(bufs):
                b = bufs.to(dtype).requires_grad_(True)
                leaves.append(b)
            flows = restate_points(name, b, w, poses, scale, dtype, mask, gates)
        out[dtype] = (flows.detach(), torch.autograd.grad((flows * up.to(dtype)).sum(), leaves))
    return out
