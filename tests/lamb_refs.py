"""LAMB restated in plain torch (helper of tests/test_lamb_host.py and tests/test_gpu_lamb.py; not collected).

`lamb_step_ref` is the formula block of include/sininn.h (apex/optimizers/fused_lamb.py with multi_tensor_lamb stages 1 and 2), per
tensor, in the dtype asked for.  It never calls the library.  In float64 it is the reference of the GPU tests, in float32 their unit of
error (the method of tests/test_gpu_flownet.py).
"""
import torch

DEFAULTS = dict(lr=1e-3, bias_correction=True, betas=(0.9, 0.999), eps=1e-6, weight_decay=0.01, adam_w_mode=True,
                grad_averaging=True, max_grad_norm=1.0, use_nvlamb=False)


def lamb_grad_sq(g, offsets, grad_scale, dtype):
    """sum over the tensors of one flat gradient buffer of (grad_scale * g)^2, a 0-d tensor of `dtype`; offsets = [(begin, numel)]"""
    total = torch.zeros((), dtype=dtype, device=g.device)
    for b, k in offsets:
        total = total + (g[b:b + k].to(dtype) * grad_scale).pow(2).sum()
    return total


def lamb_step_ref(p, g, m, v, offsets, hyper, step, grad_scale, dtype, global_sq=None):
    """One LAMB step on flat buffers p, g, m, v (any float dtype; widened / narrowed to `dtype` first; not modified).
    offsets: [(begin, numel)] per tensor; hyper: the keys of DEFAULTS (missing ones take the default); step counts from 1.
    global_sq: the sum of (grad_scale * g)^2 over ALL param groups when there are several (default: this buffer's own).
    Returns dict(p, m, v: new flat buffers of `dtype`, padding as it was; ratios: [n_tensors]; G: the global gradient norm)."""
    h = dict(DEFAULTS, **hyper)
    beta1, beta2 = h['betas']
    lr, eps, wd, mgn = h['lr'], h['eps'], h['weight_decay'], h['max_grad_norm']
    p, g, m, v = (t.detach().to(dtype).clone() for t in (p, g, m, v))
    sq = lamb_grad_sq(g, offsets, grad_scale, dtype) if global_sq is None else global_sq.to(dtype)
    G = sq.sqrt()
    clip = torch.where(G > mgn, G / mgn, torch.ones_like(G)) if mgn > 0 else torch.ones_like(G)
    bc1 = 1.0 - beta1 ** step if h['bias_correction'] else 1.0
    bc2 = 1.0 - beta2 ** step if h['bias_correction'] else 1.0
    beta3 = 1.0 - beta1 if h['grad_averaging'] else 1.0
    ratios = []
    for b, k in offsets:
        pt, mt, vt = p[b:b + k], m[b:b + k], v[b:b + k]
        sg = g[b:b + k] * grad_scale / clip
        if not h['adam_w_mode']:
            sg = sg + wd * pt
        mt.copy_(beta1 * mt + beta3 * sg)
        vt.copy_(beta2 * vt + (1.0 - beta2) * sg * sg)
        u = (mt / bc1) / ((vt / bc2).sqrt() + eps)
        if h['adam_w_mode']:
            u = u + wd * pt
        pn, un = pt.pow(2).sum().sqrt(), u.pow(2).sum().sqrt()
        lr_t = torch.full((), lr, dtype=dtype, device=p.device)
        if (h['use_nvlamb'] or wd != 0) and float(pn) != 0 and float(un) != 0:
            ratio = lr_t * (pn / un)
        else:
            ratio = lr_t
        pt.sub_(ratio * u)
        ratios.append(ratio)
    return dict(p=p, m=m, v=v, ratios=torch.stack(ratios), G=G)
