"""The restatement of the progressive flow-field networks under a PER-POINT mask (sin_inn_amd.progressive.StashedSpatialController) in
plain torch: the cells and weights of a point with the reference's fp32 expressions, the weighted sum of the eight grid rows and the
network in the dtype asked for.  tests/test_flownet_spatial_golden.py ties it to the reference's own progressive_controller.py through
the fixture, tests/test_gpu_flownet_spatial.py measures the kernels against it.  Uses the encoders of tests/flownet_refs.py.
"""
import torch

from flownet_refs import ENCODERS, poses_of

IDENTITY = (0.0, 0.0, 0.0, 1.0, 1.0, 1.0)


def cells(poses32, res, centre_scale=IDENTITY):
    """interpolate_ / flat_inds (progressive_controller.py:613-628, 655-660) on the CPU in fp32: (inds (N, 8) int64, alphas (N, 8)
    fp32), corner c taking index / weight number (c >> 2) & 1 of t, (c >> 1) & 1 of y, c & 1 of x; row = i_t + i_y res + i_x res^2"""
    x = poses32.detach().cpu().to(torch.float32)
    cs = torch.tensor(centre_scale, dtype=torch.float32).view(2, 1, 3)
    x = (x - cs[0]) * cs[1]
    x_ = ((x + 1) / 2) * max(res - 2, 1) + .5
    lo, hi = torch.floor(x_), torch.ceil(x_ + 1e-6)
    a = (hi - x_, x_ - lo)
    i = (lo, hi)
    inds, alphas = [], []
    for c in range(8):
        sel = ((c >> 2) & 1, (c >> 1) & 1, c & 1)
        ind, alpha = 0, 1
        for d in range(3):
            ind = ind + i[sel[d]][:, d] * res ** d
            alpha = alpha * a[sel[d]][:, d]
        inds.append(ind.long())
        alphas.append(alpha)
    return torch.stack(inds, 1), torch.stack(alphas, 1)


def interp_mask(grid, res, poses32, dtype=torch.float64, centre_scale=IDENTITY, chunk=4096):
    """m (N, 515) in `dtype` on the device of `grid`: sum over the eight corners of alpha * grid[row], indices and alphas from `cells`
    (fp32, exact in any wider dtype)"""
    inds, alphas = cells(poses32, res, centre_scale)
    inds, alphas = inds.to(grid.device), alphas.to(grid.device, dtype)
    out = []
    for s in range(0, inds.shape[0], chunk):
        rows = grid[inds[s:s + chunk]].to(dtype)
        out.append((rows * alphas[s:s + chunk, :, None]).sum(1))
    return torch.cat(out)


def restate_points(name, bufs, weights, poses, dtype, mask_pp, gates=None):
    """the network at a list of points (N, 3) under a per-point mask (N, 515), in `dtype`: (N, 4)"""
    poses = poses.to(dtype)
    weights = [p.to(dtype) for p in weights]
    x = torch.cat((poses, ENCODERS[name](bufs, poses)), dim=-1) * mask_pp.to(dtype)
    for l in range(3):
        pre = torch.nn.functional.linear(x, weights[2 * l], weights[2 * l + 1])
        x = torch.relu(pre) if gates is None else pre * gates[l].to(dtype)
    return torch.nn.functional.linear(x, weights[6], weights[7])


def restate_spatial(name, bufs, weights, times, ys, xs, scale, dtype, mask_pp, gates=None):
    """FlowTrainer.forward on the (times, ys, xs) grid under a per-point mask (t h w, 515): flows (t, 4, h, w) in `dtype`"""
    t, h, w = times.numel(), ys.numel(), xs.numel()
    out = restate_points(name, bufs, weights, poses_of(times, ys, xs, dtype), dtype, mask_pp, gates)
    return out.view(t, h, w, 4).permute(0, 3, 1, 2) * scale
