"""The SIREN flow network restated with torch ops in any dtype: what tests/test_flownet_siren_golden.py ties to the reference's own
model.py through the fixture and what tests/test_gpu_flownet_siren.py holds the kernels against.

    u_l = omega (h_{l-1} W_l^T + b_l),  h_l = sin(u_l)   l = 1 .. 4,  h_0 = (t, y, x) of meshgrid(times, ys, xs)
    flows[t][c][y][x] = (h_4 W_5^T + b_5)[p][c] * scale
"""
import torch
import torch.nn.functional as nnf

OMEGA = 30.0


def siren_tensors(net, dev=None):
    """[W1, b1, .., W5, b5] of a SirenModel, detached (on `dev`)"""
    out = [p.detach() for lin in net.linears() for p in (lin.weight, lin.bias)]
    return [p.to(dev) for p in out] if dev is not None else out


def siren_restate(weights, times, ys, xs, scale, dtype, omega=OMEGA):
    """flows (t, 4, h, w) in `dtype` from the fp32 tensors the kernels receive, widened"""
    gt, gh, gw = torch.meshgrid(times.to(dtype), ys.to(dtype), xs.to(dtype), indexing='ij')
    x = torch.stack((gt, gh, gw), dim=-1).view(-1, 3)
    w = [p.to(dtype) for p in weights]
    for l in range(4):
        x = torch.sin(omega * nnf.linear(x, w[2 * l], w[2 * l + 1]))
    out = nnf.linear(x, w[8], w[9])
    return out.view(times.numel(), ys.numel(), xs.numel(), 4).permute(0, 3, 1, 2) * scale
