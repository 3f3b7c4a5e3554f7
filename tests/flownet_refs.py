"""The float64 restatement of the twelve flow-field networks (sin_inn_amd/flownet.py) in plain torch, once: the five
tests/test_flownet*_golden.py tie it to the reference's own model.py through their fixtures, the six tests/test_gpu_flownet*.py measure
the kernels against it.  One encoder per encoding, one `restate` for every network; a new encoding adds an encoder and a row of ENCODERS.
Also the helpers the GPU files share (NaN-filled buffers, exact-zero checks, reference gradients).  A plain module, no fixtures.
"""
import numpy as np
import torch

PROGRESSIVE = ('PRBF', 'PFF', 'PUFF', 'PRFF', 'PRBFG', 'PPE')


def poses_of(times, ys, xs, dtype):
    gt, gh, gw = torch.meshgrid(times.to(dtype), ys.to(dtype), xs.to(dtype), indexing='ij')
    return torch.stack((gt, gh, gw), dim=-1).view(-1, 3)


def encode_rbf(bufs, poses):
    """model.py:349-356, in the dtype of `poses`"""
    centres, sigma = bufs['encode.centres'].to(poses), bufs['encode.sigma'].to(poses)
    out = (poses[:, None, :] - centres[None, :, :]).pow(2).sum(2)
    return torch.exp(-(out * sigma[None, :] ** 2))


def encode_fourier(bufs, poses):
    """model.py:230-238, in the dtype of `poses`.  bufs: the buffers of FFN / UFF, or the matrix (3, 256) itself: F_eff
    (model.py:273-278) of the learnable RFF / PRFF, an autograd leaf if its gradient is wanted"""
    freq = (bufs if torch.is_tensor(bufs) else bufs['encode.frequencies']).to(poses)
    out = torch.matmul(poses * 2 * np.pi, freq)
    return torch.stack((torch.sin(out), torch.cos(out)), dim=2).view(poses.shape[0], -1)


def encode_grid(bufs, poses):
    """model.py:375-387 in the dtype of `poses`, from the fp32 buffers (widened): (N, 512), feature 2 j = e(xa), 2 j + 1 = e(xb)"""
    offsets, sigma = bufs['encode.offsets'].to(poses), bufs['encode.sigma'].to(poses)
    x_a = poses[:, None, :] + offsets[None, :]
    x_b = x_a + (1 / sigma[None, :, None])
    out = torch.stack((x_a, x_b), dim=2)
    out = (out % (2 / sigma[None, :, None, None])) * 2 - (2 / sigma[None, :, None, None])
    out = out.pow(2).sum(3)
    out = out * sigma[None, :, None] ** 2
    out = out.view(-1, 2 * sigma.numel())
    return torch.exp(-out) * 2 - 1


def encode_pe(bufs, poses):
    """model.py:331-332 as a formula, in the dtype of `poses`, from the fp32 buffer (widened): (N, 24), feature 6 f + d =
    cos(freqs[f] x_d), 6 f + 3 + d = sin(freqs[f] x_d).  No einsum: one product per element, for every N."""
    freqs = bufs['encode.freqs'].to(poses)
    arg = freqs[None, :, None] * poses[:, None, :]
    return torch.cat((torch.cos(arg), torch.sin(arg)), dim=2).reshape(poses.shape[0], -1)


ENCODERS = {'RBF': encode_rbf, 'FFN': encode_fourier, 'UFF': encode_fourier, 'RFF': encode_fourier, 'RBFG': encode_grid, 'PE': encode_pe,
            'PRBF': encode_rbf, 'PFF': encode_fourier, 'PUFF': encode_fourier, 'PRFF': encode_fourier, 'PRBFG': encode_grid, 'PPE': encode_pe}


def layer1_input(name, bufs, poses, mask):
    """what layer 1 reads: the encoding, or (progressive, model.py:532-535) cat((poses, encoding)) * mask; mask None: the bare
    network, no mask applied"""
    x = ENCODERS[name](bufs, poses)
    if name not in PROGRESSIVE:
        assert mask is None
        return x
    x = torch.cat((poses, x), dim=-1)
    return x if mask is None else x * mask.to(poses)[None, :]


def restate(name, bufs, weights, times, ys, xs, scale, dtype, mask=None, gates=None):
    """FlowTrainer.forward (trainer.py:37-45) in plain torch in `dtype`, from fp32 axis vectors / buffers / weights (widened).
    bufs: the network's `encode.*` state (RFF / PRFF: the matrix F_eff, see encode_fourier); weights: [W1, b1, .., W4, b4] (autograd
    leaves of `dtype` if gradients are wanted); mask: the 515 (PPE: 27) values of a progressive network; gates: None (ReLU) or three
    bool (N, 256) tensors that REPLACE the ReLU decision: h = pre * gate.  Returns flows (t, 4, h, w)."""
    t, h, w = times.numel(), ys.numel(), xs.numel()
    weights = [p.to(dtype) for p in weights]
    x = layer1_input(name, bufs, poses_of(times, ys, xs, dtype), mask)
    for l in range(3):
        pre = torch.nn.functional.linear(x, weights[2 * l], weights[2 * l + 1])
        x = torch.relu(pre) if gates is None else pre * gates[l].to(dtype)
    out = torch.nn.functional.linear(x, weights[6], weights[7])
    return out.view(t, h, w, 4).permute(0, 3, 1, 2) * scale


def own_gates(name, bufs, w64, times, ys, xs, mask=None):
    """the ReLU decisions of the float64 network itself"""
    with torch.no_grad():
        x = layer1_input(name, bufs, poses_of(times, ys, xs, torch.float64), mask)
        gates = []
        for l in range(3):
            x = torch.relu(torch.nn.functional.linear(x, w64[2 * l], w64[2 * l + 1]))
            gates.append(x > 0)
    return gates


def net_tensors(net, device='cpu'):
    """(the `encode.*` entries of the state dict, [W1, b1, .., W4, b4]) detached on `device`"""
    bufs = {k: v.detach().to(device) for k, v in net.state_dict().items() if k.startswith('encode.')}
    weights = [p.detach().to(device) for lin in net.linears() for p in (lin.weight, lin.bias)]
    return bufs, weights


# ---- shared by the GPU files ----
def nan_saved(n, dev):
    from sin_inn_amd import _lib
    nbytes = _lib.lib().sininn_flownet_saved_bytes(n)
    return torch.full((3, nbytes // (3 * 256 * 4), 256), float('nan'), device=dev)


def nan_workspace(n, dev):
    from sin_inn_amd import _lib
    return torch.full((_lib.lib().sininn_flownet_workspace_bytes(n) // 4,), float('nan'), device=dev)


def nan_buffers(n, dev):
    """(saved, workspace, the frequency gradient's workspace), all NaN"""
    from sin_inn_amd import _lib
    a = _lib.FlowNetArgs()
    a.encoding = 1
    ews = torch.full((_lib.lib().sininn_flownet_encgrad_workspace_bytes(a) // 4,), float('nan'), device=dev)
    assert ews.numel() >= 512 * 256 + 512 * 768
    return nan_saved(n, dev), nan_workspace(n, dev), ews


def is_plus_zero(t):
    return bool((t == 0.0).all()) and not bool(torch.signbit(t).any())


def closed_frequencies(hmask):
    """frequencies whose sin and cos are both closed by a 515-value mask"""
    return (hmask[3::2] == 0) & (hmask[4::2] == 0)


def reference_grads(name, bufs, weights, times, ys, xs, scale, up, mask, gates):
    """{dtype: gradients of sum(flows * up) with respect to the weights} of `restate` in float64 and in fp32"""
    out = {}
    for dtype in (torch.float64, torch.float32):
        w = [p.to(dtype).requires_grad_(True) for p in weights]
        flows = restate(name, bufs, w, times, ys, xs, scale, dtype, mask, gates)
        out[dtype] = torch.autograd.grad((flows * up.to(dtype)).sum(), w)
    return out
