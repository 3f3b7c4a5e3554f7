"""Float64 references for the coordinate gradient of the flow networks (tests/test_gpu_flownet_posegrad.py,
tests/test_gpu_flownet_posegrad_sweep.py): autograd through the restatements of tests/flownet_points_refs.py with the POSES as a leaf, the
points the radial-basis grid excludes, and the check of g_poses per coordinate column.  A plain module, no fixtures.
"""
import torch

from flownet_points_refs import restate_points, siren_restate_points

WRAP_TOL = 1e-6


def reference_pose_grads(name, bufs, weights, poses, scale, up, mask=None, gates=None, with_enc=False):
    """{dtype: (g_poses (N, 3)[, gF (3, 256)])}: the gradient of sum(flows * up) with respect to the poses (and, `with_enc`, to the
    frequency matrix `bufs`) of restate_points / siren_restate_points in float64 and in fp32, from the fp32 poses (widened), `gates`
    forced.  name == 'siren': weights are siren_refs.siren_tensors', bufs / mask / gates unused"""
    out = {}
    for dtype in (torch.float64, torch.float32):
        x = poses.detach().to(dtype).requires_grad_(True)
        leaves, b = [x], bufs
        if with_enc:
            b = bufs.to(dtype).requires_grad_(True)
            leaves.append(b)
        if name == 'siren':
            flows = siren_restate_points(weights, x, scale, dtype)
        else:
            flows = restate_points(name, b, weights, x, scale, dtype, mask, gates)
        out[dtype] = torch.autograd.grad((flows * up.to(dtype)).sum(), leaves)
    return out


def rbfg_near_wrap(bufs, poses, tol=WRAP_TOL, chunk=4096):
    """(N,) bool: points with a float64 operand of the grid encoding's remainder, x_d + offset (+ 1 / sigma), within `tol` absolute of a
    multiple of the period 2 / sigma, for any feature and coordinate: there d (x mod p) / d x jumps, and fp32 and float64 may stand on
    opposite sides.  `chunk` points at a time: the operands are (chunk, 256, 2, 3) float64"""
    x = poses.detach().to(torch.float64)
    offsets, sigma = bufs['encode.offsets'].to(x), bufs['encode.sigma'].to(x)
    period = (2 / sigma)[None, :, None, None]
    out = []
    for s in range(0, x.shape[0], chunk):
        x_a = x[s:s + chunk, None, :] + offsets[None, :]
        ops = torch.stack((x_a, x_a + (1 / sigma[None, :, None])), dim=2)
        r = ops % period
        out.append(((r < tol) | (period - r < tol)).flatten(1).any(1))
    return torch.cat(out) if out else torch.zeros(0, dtype=torch.bool, device=x.device)


def reference_all_grads(flows_of, weights, poses, up, enc=None):
    """{dtype: the gradients of sum(flows * up) with respect to the weights, (`enc` given) the frequency matrix, and the poses, in that
    order} for flows (4, N) = flows_of(w, enc, x, dtype), a restatement with the mask and the gates bound, in float64 and in fp32 from
    the fp32 tensors (widened): ONE autograd pass gives the parameter gradients and g_poses of the same call"""
    out = {}
    for dtype in (torch.float64, torch.float32):
        w = [p.detach().to(dtype).requires_grad_(True) for p in weights]
        e = [] if enc is None else [enc.detach().to(dtype).requires_grad_(True)]
        x = poses.detach().to(dtype).requires_grad_(True)
        flows = flows_of(w, e[0] if e else None, x, dtype)
        out[dtype] = torch.autograd.grad((flows * up.to(dtype)).sum(), w + e + [x])
    return out


def check_whole_and_columns(check, tag, got, r64, r32, keep=None):
    """`check(tag, got, r64, r32)` on g_poses (N, 3) as a whole and on each coordinate column alone, each relative to its own max |ref| and
    with its own unit: a column whose gradient is smaller than the largest one does not hide behind it.  `keep`: the rows compared"""
    if keep is not None:
        got, r64, r32 = got[keep], r64[keep], r32[keep]
    check(tag, got, r64, r32)
    for d, axis in enumerate('tyx'):
        check(f'{tag} column {axis}', got[:, d], r64[:, d], r32[:, d])


def chained(query, poses):
    """flow at p' = p + (0, flow[..., 0], flow[..., 1]) for `query`: (N, 3) -> (N, 4): the forward flow of p, followed"""
    first = query(poses)
    moved = poses + torch.cat((torch.zeros_like(first[:, :1]), first[:, :2]), dim=1)
    return query(moved)
