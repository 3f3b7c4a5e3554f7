"""The piecewise-linear encoding of MPFF (sin_inn_amd.flownet.PieceWiseEncoding, SININN_FLOWNET_PIECEWISE of csrc/flownet.hip) restated in
plain torch in any dtype, and what its tests share: tests/test_flownet_piecewise_golden.py ties the restatement to the reference's own
model.py through the fixture, tests/test_gpu_flownet_piecewise.py measures the kernels against it.  Importing this module adds the 'MPFF'
row to the tables of tests/flownet_refs.py (ENCODERS, PROGRESSIVE), so `restate`, `reference_grads`, flownet_points_refs.restate_points and
flownet_spatial_refs.restate_points serve this network as they serve the others.  A plain module, no fixtures.

The encoding has kinks (at every integer of u the slope of both features of a frequency changes sign) and, for u < 0, jumps (the
reference's fmod truncates: the value drops by 4 at every other negative integer).  Two evaluations of u that differ in the last bits
can stand on opposite sides of one, so the tests that look at a quantity that is discontinuous there name the (point, feature) pairs
whose float64 u lies within DELTA_ULPS fp32 ulps of max |u| of such an integer (`kink_delta`, `near_integer`), from the float64
reference alone, and bound how many there may be.
"""
import os

import numpy as np
import torch

import flownet_refs

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAME, SEED = 'MPFF', 1414
TIMES, GH, GW, SCALE, STRIDE = (0.0, 0.5), 20, 28, 3.0, 97
MAX_ITERATION, EPSILON, N_RAMP, N_MID = 1000, 1e-3, 98, 100
KEYS = [f'model.model.{i}.{s}' for i in (0, 2, 4, 6) for s in ('weight', 'bias')]
DELTA_ULPS = 8.0                                       # of max |u|, in units of 2^-24


def piecewise_arg(bufs, poses):
    """u = (x + 1) @ frequencies (model.py:638) in the dtype of `poses`: (N, 256)"""
    return torch.matmul(poses + 1, bufs['encode.frequencies'].to(poses))


def encode_piecewise(bufs, poses):
    """model.py:638-644 in the dtype of `poses`, from the fp32 buffer (widened): (N, 512), feature 2 f = tri(u_f), 2 f + 1 = tri(u_f + 1).
    torch.fmod truncates (the sign of the dividend).  Out of place, so that autograd with the poses as a leaf gives the derivative of
    the branch this dtype takes"""
    out = piecewise_arg(bufs, poses)
    out = torch.stack((out, out + 1), dim=2).view(poses.shape[0], -1)
    out = torch.fmod(out, 2) - 1
    return torch.where(out.lt(0), 2 * out + 1, 1 - 2 * out)


flownet_refs.ENCODERS[NAME] = encode_piecewise
if NAME not in flownet_refs.PROGRESSIVE:
    flownet_refs.PROGRESSIVE = flownet_refs.PROGRESSIVE + (NAME,)


def kink_delta(u64):
    """DELTA_ULPS fp32 ulps of the largest |u|: what two correct fp32 evaluations of u may differ by, with room"""
    return DELTA_ULPS * 2.0 ** -24 * float(u64.detach().abs().max())


def near_integer(u64, delta, negative_only=False):
    """(N, 256) bool: the float64 u within `delta` of an integer (`negative_only`: of an integer <= -1, where the value jumps)"""
    nearest = torch.round(u64)
    near = (u64 - nearest).abs() <= delta
    return near & (nearest <= -1) if negative_only else near


def layer1_gradient(bufs, weights, poses, scale, up, mask, gates):
    """G (N, 515) in float64: the gradient of sum(flows * up) with respect to the UNMASKED input of layer 1, (dh1 W1)_k mask_k, with the
    gates forced; flows planar (4, N).  Column 3 + k belongs to encoded feature k"""
    dt = torch.float64
    x = poses.detach().to(dt)
    inp = torch.cat((x, encode_piecewise(bufs, x)), dim=-1).requires_grad_(True)
    h = inp * mask.to(dt)[None, :]
    w = [p.detach().to(dt) for p in weights]
    for l in range(3):
        h = torch.nn.functional.linear(h, w[2 * l], w[2 * l + 1]) * gates[l].to(dt)
    flows = torch.nn.functional.linear(h, w[6], w[7]).t() * scale
    return torch.autograd.grad((flows * up.to(dt)).sum(), inp)[0]


def kink_allowance(bufs, G, near):
    """(N, 3) float64: sum over the near-kink features k of 4 |G_k| |F[d][f]|, f = k // 2: both features of a frequency whose u is near
    an integer may have their slope +-2 F[d][f] flipped, a change of 4 |F[d][f]| each.  `near`: (N, 256), per frequency"""
    F = bufs['encode.frequencies'].to(G).abs()                    # (3, 256)
    g = G[:, 3:].abs().view(G.shape[0], 256, 2).sum(2) * near.to(G)   # (N, 256)
    return 4.0 * g @ F.t()


def gold():
    return np.load(os.path.join(ROOT, 'tests', 'golden', 'golden_flownet_piecewise.npz'))


def build():
    from sin_inn_amd import flownet
    torch.manual_seed(SEED)
    return flownet.piecewise_model_dict[NAME](flownet.ModelParams())


def controller(net):
    from sin_inn_amd import progressive
    return progressive.LinearControllerEarly(net, MAX_ITERATION, epsilon=EPSILON)
