"""float64 references of the conv engine, one image and one tap at a time (no unfold over the batch: GBs at production sizes).
Plain helpers shared by the size tests (tests/test_gpu_bf16_tiles.py, tests/test_gpu_conv_fp32_sizes.py); tensors are pixel-major
[B,H,W,C] of any dtype, the result is float64 on the device of the first operand."""
import torch
import torch.nn.functional as F


def ref_conv(x, w, b=None):
    """x [B,H,W,C] (any dtype), w [N,C,k,k] -> float64 [B,H,W,N]; zero padding k // 2"""
    B, H, W, Cn = x.shape
    n, _, k, _ = w.shape
    p = k // 2
    w = w.double()
    out = torch.zeros(B, H, W, n, dtype=torch.float64, device=x.device)
    for i in range(B):
        xp = F.pad(x[i].double(), (0, 0, p, p, p, p))
        acc = out[i].view(H * W, n)
        for ky in range(k):
            for kx in range(k):
                acc += xp[ky:ky + H, kx:kx + W].reshape(H * W, Cn) @ w[:, :, ky, kx].t()
    if b is not None:
        out += b.double()
    return out


def ref_dgrad(g, w):
    """data gradient of ref_conv: g [B,H,W,N], w [N,C,k,k] -> float64 [B,H,W,C]"""
    B, H, W, n = g.shape
    _, Cn, k, _ = w.shape
    p = k // 2
    w = w.double()
    out = torch.zeros(B, H, W, Cn, dtype=torch.float64, device=g.device)
    for i in range(B):
        gp = F.pad(g[i].double(), (0, 0, p, p, p, p))
        acc = out[i].view(H * W, Cn)
        for ky in range(k):
            for kx in range(k):
                acc += gp[2 * p - ky:2 * p - ky + H, 2 * p - kx:2 * p - kx + W].reshape(H * W, n) @ w[:, :, ky, kx]
    return out


def ref_wgrad(x, g, k):
    """weight gradient of ref_conv: x [B,H,W,C], g [B,H,W,N] -> float64 [N,C,k,k]"""
    B, H, W, Cn = x.shape
    n = g.shape[3]
    p = k // 2
    gw = torch.zeros(n, Cn, k, k, dtype=torch.float64, device=x.device)
    for i in range(B):
        xp = F.pad(x[i].double(), (0, 0, p, p, p, p))
        gi = g[i].double().reshape(H * W, n).t()
        for ky in range(k):
            for kx in range(k):
                gw[:, :, ky, kx] += gi @ xp[ky:ky + H, kx:kx + W].reshape(H * W, Cn)
    return gw
