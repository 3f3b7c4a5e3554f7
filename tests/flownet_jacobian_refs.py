"""The float64 reference of the flow Jacobian (flow_at(.., jacobian=), flow_jacobian_composed), and the budget rule its tests
share.  A plain module, no fixtures.

The reference is tests/flownet_points_refs.restate_points with the ReLU gates FORCED (h = pre * gate): with the gates fixed the network is
smooth in the poses (RBF and Fourier encodings), jac is torch.autograd.grad of each output channel with respect to the poses
(create_graph=True), and the parameter gradients are those of sum(up * flows) + sum(upj * jac), a double backward.  The same restatement in
fp32 gives the unit.  Budget (the project's standing rule, tests/test_gpu_flownet_posegrad.py): error <= MULT x the fp32-torch unit, both
max-norms relative to the max-norm of the float64 value; applied to jac as a whole, per direction, per channel pair and per parameter gradient,
so that a small column does not hide behind a large one.  No element is excluded.
"""
import torch

from flownet_points_refs import restate_points

F64, F32 = torch.float64, torch.float32
MULT = 4.0
CHUNK = 8192                                            # points per chunk of the double backward: (N, 512, 3) intermediates in float64


def relmax(a, ref):
    """max |a - ref| / max |ref| in float64; a non-finite entry of `a` is an infinite error"""
    a, ref = a.detach().to(F64), ref.detach().to(F64)
    err = (a - ref).abs()
    err = torch.where(torch.isfinite(a), err, torch.full_like(err, float('inf')))
    return float(err.max() / ref.abs().max().clamp_min(1e-300))


def reference(name, bufs, weights, poses, scale, dirs, up, upj, mask, gates):
    """{dtype: (flows (4, N), jac (|D|, 4, N), [gW1, gb1, .., gW4, gb4])} in float64 and fp32.  `dirs`: ascending indices into (t, y, x);
    `up` (4, N), `upj` (|D|, 4, N): the upstream gradients; `gates`: three bool (N, 256) tensors, the decisions the code under test took.
    Evaluated in chunks of points: every output is a sum over points or belongs to one"""
    out = {}
    n = poses.shape[0]
    for dtype in (F64, F32):
        w = [p.to(dtype).requires_grad_(True) for p in weights]
        flows_all, jac_all, grads = [], [], None
        for lo in range(0, n, CHUNK):
            hi = min(n, lo + CHUNK)
            x = poses[lo:hi].to(dtype).requires_grad_(True)
            flows = restate_points(name, bufs, w, x, scale, dtype, mask, [g[lo:hi] for g in gates])
            rows = [torch.autograd.grad(flows[c].sum(), x, create_graph=True)[0] for c in range(4)]            # each (n, 3)
            jac = torch.stack([torch.stack([rows[c][:, d] for c in range(4)]) for d in dirs])                  # (|D|, 4, n)
            loss = (flows * up[:, lo:hi].to(dtype)).sum() + (jac * upj[:, :, lo:hi].to(dtype)).sum()
            g = torch.autograd.grad(loss, w)
            grads = list(g) if grads is None else [a + b for a, b in zip(grads, g)]
            flows_all.append(flows.detach())
            jac_all.append(jac.detach())
        out[dtype] = (torch.cat(flows_all, 1), torch.cat(jac_all, 2), grads)
    return out


def check(name, got, ref64, ref32, worst=None):
    """error of `got` against MULT x the fp32-torch unit; prints ratio(error / budget) and keeps the worst in `worst`"""
    unit = relmax(ref32, ref64)
    budget = MULT * unit
    err = relmax(got, ref64)
    ratio = err / budget if budget > 0 else (0.0 if err == 0 else float('inf'))      # an exactly zero reference (a closed mask): exact zeros asked
    print(f'ratio({name}) = {ratio:.3g}   [err {err:.3g}, fp32-torch unit {unit:.3g}, budget {budget:.3g}]')
    if worst is not None:
        worst.append((ratio, name))
    assert err <= budget, (name, err, budget)
    return ratio


def jac_views(dirs, jac):
    """(label, slice function) for jac (|D|, 4, N) as a whole, per direction and per channel pair of a direction"""
    views = [('jac', lambda j: j)]
    for i, d in enumerate(dirs):
        views.append((f'jac[{"tyx"[d]}]', lambda j, i=i: j[i]))
        views.append((f'jac[{"tyx"[d]}][0:2]', lambda j, i=i: j[i, 0:2]))
        views.append((f'jac[{"tyx"[d]}][2:4]', lambda j, i=i: j[i, 2:4]))
    return views


def check_all(label, dirs, flows, jac, grads, ref, worst=None):
    """the whole rule: flows, every view of jac, every parameter gradient.  `grads` may be None (a forward-only comparison)"""
    check(f'{label} flows', flows, ref[F64][0], ref[F32][0], worst)
    for nm, view in jac_views(dirs, jac):
        check(f'{label} {nm}', view(jac), view(ref[F64][1]), view(ref[F32][1]), worst)
    if grads is not None:
        names = [f'g{k}{l}' for l in range(1, 5) for k in ('W', 'b')]
        for nm, g, r64, r32 in zip(names, grads, ref[F64][2], ref[F32][2]):
            check(f'{label} {nm}', g, r64, r32, worst)


def exceeds(dirs, jac, grads, ref):
    """True if any view of jac or any parameter gradient is over its budget: what a seeded defect must do"""
    for _, view in jac_views(dirs, jac):
        if relmax(view(jac), view(ref[F64][1])) > MULT * relmax(view(ref[F32][1]), view(ref[F64][1])):
            return True
    for g, r64, r32 in zip(grads, ref[F64][2], ref[F32][2]):
        if relmax(g, r64) > MULT * relmax(r32, r64):
            return True
    return False
