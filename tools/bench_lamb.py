"""Time one optimiser step of FusedLAMB, of FusedAdam and of a LAMB composed from torch's own GPU ops (torch._foreach_* and
torch.linalg.vector_norm on the same tensors, no host read-back) in ONE process, with device events, after a warm-up, in windows of at
least --seconds, the three paths alternating --rounds times.  One JSON line per window, then one summary line per parameter set.

    python tools/bench_lamb.py [--sets RBF SRF] [--seconds 1.0] [--rounds 3] > profiles/lamb_bench.jsonl

Parameter sets: RBF = flownet.RbfModel (8 tensors, 0.26 M elements: the flow trainer's network), SRF = the SRFlow model of BASELINE
configs[1] (256 x 256, 4 coupling blocks per level, LR window 10; about 3.7 M elements).  The gradients are seeded normal values scaled
so that the clip is active; every path steps on its own copy of the parameters.  A step is what the training loop calls: step() of the
optimiser, host side included.  `spread` in the summary is (max - min) / min over the window medians of one path.
"""
import argparse
import json
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, 'tools')):
    if p not in sys.path:
        sys.path.insert(0, p)

from bench_flownet import window  # noqa: E402


class TorchLAMB:
    """apex FusedLAMB's defaults (include/sininn.h has the formulas) from torch's multi-tensor ops; nothing is read back"""

    def __init__(self, params, lr=1e-3, betas=(0.9, 0.999), eps=1e-6, weight_decay=0.01, max_grad_norm=1.0):
        self.ps = [p.detach() for p in params]
        self.gs = [torch.zeros_like(p) for p in self.ps]
        self.ms = [torch.zeros_like(p) for p in self.ps]
        self.vs = [torch.zeros_like(p) for p in self.ps]
        self.lr, self.betas, self.eps, self.wd, self.mgn, self.t = lr, betas, eps, weight_decay, max_grad_norm, 0
        self.lr_t = torch.full((), lr, device=self.ps[0].device, dtype=self.ps[0].dtype)

    @torch.no_grad()
    def step(self):
        self.t += 1
        b1, b2 = self.betas
        bc1, bc2 = 1 - b1 ** self.t, 1 - b2 ** self.t
        G = torch.linalg.vector_norm(torch.stack(torch._foreach_norm(self.gs)))
        clip = torch.clamp(G / self.mgn, min=1.0)
        sg = torch._foreach_div(self.gs, clip)
        torch._foreach_mul_(self.ms, b1)
        torch._foreach_add_(self.ms, sg, alpha=1 - b1)
        torch._foreach_mul_(self.vs, b2)
        torch._foreach_addcmul_(self.vs, sg, sg, value=1 - b2)
        den = torch._foreach_div(self.vs, bc2)
        torch._foreach_sqrt_(den)
        torch._foreach_add_(den, self.eps)
        u = torch._foreach_div(self.ms, bc1)
        torch._foreach_div_(u, den)
        torch._foreach_add_(u, self.ps, alpha=self.wd)
        pn, un = torch.stack(torch._foreach_norm(self.ps)), torch.stack(torch._foreach_norm(u))
        ratio = torch.where((pn != 0) & (un != 0), self.lr_t * (pn / un), self.lr_t)
        torch._foreach_mul_(u, ratio.unbind())
        torch._foreach_sub_(self.ps, u)


def parameter_set(name, dev):
    torch.manual_seed(0)
    if name == 'RBF':
        from sin_inn_amd import flownet
        mod = flownet.RbfModel(flownet.ModelParams())
    else:
        import lit_wrapper
        from bench import make_opt
        mod = lit_wrapper.SingleVideoINN(3, 256, 256, make_opt(4, 10))
    return [p.detach().clone().to(dev) for p in mod.parameters() if p.requires_grad]


def main():
    ap = argparse.ArgumentParser(description=__doc__.split('\n')[0])
    ap.add_argument('--sets', nargs='+', default=['RBF', 'SRF'], choices=['RBF', 'SRF'])
    ap.add_argument('--seconds', type=float, default=1.0)
    ap.add_argument('--warmup', type=int, default=20)
    ap.add_argument('--rounds', type=int, default=3)
    a = ap.parse_args()
    assert torch.cuda.is_available(), 'bench_lamb.py measures on the GPU; there is no CPU path'
    from sin_inn_amd import FusedAdam, FusedLAMB
    dev = torch.device('cuda', 0)
    for name in a.sets:
        shapes = parameter_set(name, dev)
        n = sum(p.numel() for p in shapes)
        gen = torch.Generator().manual_seed(1)
        grads = [(torch.randn(p.shape, generator=gen) * (2.0 / n ** 0.5)).to(dev) for p in shapes]      # |g| about 2: the clip is active

        def clones():
            return [torch.nn.Parameter(p.clone()) for p in shapes]
        lamb, adam, composed = FusedLAMB(clones(), lr=1e-4), FusedAdam(clones(), lr=1e-4), TorchLAMB(clones(), lr=1e-4)
        for opt in (lamb, adam):
            for p, g in zip(opt._flat[0]['params'], grads):
                p.grad.copy_(g)
        for dst, g in zip(composed.gs, grads):
            dst.copy_(g)
        paths = {'fused_lamb': lamb.step, 'fused_adam': adam.step, 'torch_lamb': composed.step}
        meds = {k: [] for k in paths}
        for rnd in range(a.rounds):
            for k, fn in paths.items():
                w = window(fn, a.seconds, a.warmup)
                meds[k].append(w['median_ms'])
                print(json.dumps(dict(set=name, tensors=len(shapes), elements=n, path=k, round=rnd, **{q: round(x, 5) if isinstance(x, float) else x
                                                                                                     for q, x in w.items()})), flush=True)
        best = {k: min(v) for k, v in meds.items()}
        print(json.dumps(dict(set=name, tensors=len(shapes), elements=n, summary=True,
                              **{f'{k}_ms': round(x, 5) for k, x in best.items()},
                              **{f'{k}_spread': round((max(v) - min(v)) / min(v), 4) for k, v in meds.items()},
                              lamb_speedup_over_torch=round(best['torch_lamb'] / best['fused_lamb'], 3),
                              lamb_minus_adam_ms=round(best['fused_lamb'] - best['fused_adam'], 5))), flush=True)


if __name__ == '__main__':
    main()
