"""Per-element references, budgets and cases for the SIREN flow-network kernels (csrc/siren.hip): what tests/test_siren_elements_host.py
establishes on the CPU and tests/test_gpu_siren_elements.py applies to the kernels.  A plain module, no fixtures; everything
runs on the device of the tensors it is given.  The method, `U`, `MULT`, `EXACT_LIMIT`, `element_ratio`, `Points` and the source readers
are those of tests/flownet_element_refs.py.

`Plan` / `views`: the launch plan and the layout of `saved` and the workspace, from constants read from the sources.
Part A1, the backward pass on exact integers: `integer_inputs` (phases 0, omega 1, weights and dflows in {-1, 0, 1}, quarter-integer
coordinates from `quarter_points`), `integer_ref` the chain in float64 with the largest sum |terms| of every output and intermediate.
Part A2, the backward pass stage by stage: `backward_stages` evaluates each stage in float64 from the inputs the kernel itself used for it
(the caller's `saved`, the kernel's own `dz` and `hin` in the workspace) with a single-stage budget.
Part B, the forward pass stage by stage: `forward_stages`, from the kernel's own `saved`.
"""
import os
import re
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import flownet_element_refs as E  # noqa: E402
from flownet_element_refs import EXACT_LIMIT, F64, HID, MULT, U, Points, _const, _source, element_ratio, relmax, relmax_budget  # noqa: E402,F401

SINES, IN_DIM, OUT = 4, 3, 4
SCALE_A1, SCALE = 1.0, 3.0          # part A1 (dout = dflows); parts A2 and B
PHASE_RANGE = 512.0                 # regime (b): phases uniform in [-512, 512] rad
GRAD_NAMES = [f'g{k}{l}' for l in (1, 2, 3, 4, 5) for k in ('W', 'b')]
TIMES3 = (0.0, 0.25, 1.0)
# ---- the cases: name -> ('grid', times, h, w) or ('list', N) ----
SHAPES = {'one': ('grid', (0.5,), 1, 1), 'few': ('list', 171), 'ragged': ('grid', TIMES3, 13, 37), 'past_cap': ('grid', TIMES3, 109, 118),
          'past_cap_list': ('list', 3 * 109 * 118)}
POSE_GRAD = ('few', 'past_cap_list')


# ---- constants of the kernels, read from the sources with the line that applies each ----
def kernel_constants():
    tile, src = _source('flownet_tile.h'), _source('siren.hip')
    c = {'P': int(_const(tile, 'FN_P')), 'CHAIN_CAP': int(_const(tile, 'FN_CHAIN_MAX_BLOCKS')), 'HID': int(_const(tile, 'FN_HID')),
         'OUT': int(_const(tile, 'FN_OUT')), 'SINES': int(_const(src, 'SR_SINES')), 'IN': int(_const(src, 'SR_IN'))}
    for line, text in (('constexpr int SR_PART_GB1 = FN_HID * SR_IN, SR_PART_GW5 = SR_PART_GB1 + FN_HID, SR_PART_GB5 = SR_PART_GW5 + FN_OUT * FN_HID;', src),
                       ('constexpr int SR_PART = SR_PART_GB5 + 2 * FN_OUT;', src),
                       ('return ntiles < FN_CHAIN_MAX_BLOCKS ? ntiles : FN_CHAIN_MAX_BLOCKS;', tile),
                       ('hipLaunchKernelGGL(siren_fwd_kernel, dim3(chain_blocks(q.ntiles)), dim3(FN_NTHR), SR_LDS, st, q);', src),
                       ('const int cb = chain_blocks(q.ntiles);', src),
                       ('hipLaunchKernelGGL(siren_bwd_chain_kernel<true>, dim3(cb), dim3(FN_NTHR), SR_LDS, st, q);', src),
                       ('hipLaunchKernelGGL(siren_bwd_chain_kernel<false>, dim3(cb), dim3(FN_NTHR), SR_LDS, st, static_cast<const SirenDev&>(q));', src),
                       ('float* const out = q.part + (size_t)blockIdx.x * SR_PART;', src),
                       ('const size_t lstride = (size_t)q.ntiles * FN_P * FN_HID;', src),
                       ('float* const ws = static_cast<float*>(a->workspace);', src),
                       ('q.dz = ws;', src), ('q.hin = ws + (SR_SINES - 1) * lstride;', src),
                       ('float* const wt = ws + 2 * (SR_SINES - 1) * lstride;', src),
                       ('q.part = wt + (size_t)(SR_SINES - 1) * FN_HID * FN_HID;', src),
                       ('return (size_t)SR_SINES * (size_t)((n + FN_P - 1) / FN_P) * FN_P * FN_HID * sizeof(float);', src),
                       ('hidden_wgrad_launch(q.ntiles, q.dz + (l - 1) * lstride, q.hin + (l - 1) * lstride, q.part, a->gw[l], a->gb[l], st)', src)):
        assert line in text, line
    assert re.search(r'float\* saved; +// \[4\]\[ntiles \* 64\]\[256\]: the phases u_1 \.\. u_4', src)
    # both kernels walk the tiles with the same grid-stride loop
    assert src.count('for (int tile = blockIdx.x; tile < q.ntiles; tile += gridDim.x)') == 2
    c['PART_GB1'] = c['HID'] * c['IN']
    c['PART_GW5'] = c['PART_GB1'] + c['HID']
    c['PART_GB5'] = c['PART_GW5'] + c['OUT'] * c['HID']
    c['PART'] = c['PART_GB5'] + 2 * c['OUT']      # gb5 as (hi, lo) pairs
    return c


class Plan(E.Plan):
    """the launches of one SIREN call at N points: the forward and the chain kernel grid-stride over 64-point tiles with `chain_blocks`
    blocks; the hidden weight gradients (hidden_wgrad_launch of flownet.hip) split the tiles over `hidden_chunks`.  `lstride`: floats per
    layer of `saved`, `dz`, `hin`; `ws_floats`: the workspace up to the partial sums"""

    def __init__(self, n):
        c = kernel_constants()
        assert (c['P'], c['HID'], c['OUT'], c['SINES'], c['IN']) == (E.kernel_constants()['P'], HID, OUT, SINES, IN_DIM)
        super().__init__(n)
        self.lstride = self.npad * HID
        self.ws_floats = 2 * (SINES - 1) * self.lstride + (SINES - 1) * HID * HID
        self.chain_terms = self.p * self.chain_walk[1] + self.chain_blocks + 2      # a chain block's sum, its partials, product and store
        self.hidden_terms = self.p * self.hidden_walk[1] + self.hidden_chunks + 2   # a chunk's sum, its partials, product and store


def views(ws, saved, ntiles):
    """(dz (3, Npad, 256): dz_2 .. dz_4; hin (3, Npad, 256): h_1 .. h_3; wt (3, 256, 256): W2^T, W3^T, W4^T; saved (4, Npad, 256): u_1 ..
    u_4) as views of a flat workspace and a flat `saved`"""
    p = kernel_constants()['P']
    npad = ntiles * p
    ls = npad * HID
    nl = SINES - 1
    assert ws.numel() >= 2 * nl * ls + nl * HID * HID and saved.numel() == SINES * ls
    return (ws[:nl * ls].view(nl, npad, HID), ws[nl * ls:2 * nl * ls].view(nl, npad, HID),
            ws[2 * nl * ls:2 * nl * ls + nl * HID * HID].view(nl, HID, HID), saved.view(SINES, npad, HID))


# ---- points ----
def quarter_points(shape, dev='cpu'):
    """the points of a shape with every coordinate a multiple of 1/4 in [-1, 1] (part A1): grid axes ((arange(h) % 9) - 4) / 4, the times
    as they are; a pose list of seeded multiples"""
    pts = Points(shape, dev)
    if pts.grid is not None:
        _, times, h, w = shape
        assert all(float(t) * 4 == int(float(t) * 4) and abs(t) <= 1 for t in times)
        pts.ys, pts.xs = (((torch.arange(h) % 9) - 4) / 4.0).to(dev), (((torch.arange(w) % 9) - 4) / 4.0).to(dev)
    else:
        g = torch.Generator().manual_seed(4 + pts.n)
        pts.list = (torch.randint(-4, 5, (pts.n, 3), generator=g) / 4.0).to(dev).contiguous()
    return pts


def build():
    from test_flownet_siren_golden import build as b
    return b()


# ---- part A1: the backward pass on exact integers ----
W_DENSITY = 1.0 / 32                # of W2 .. W4: 8 entries per row on average; the host test establishes the precondition with it


def integer_inputs(n, seed=2025):
    """W1 (256, 3), W5 (4, 256) and dflows (4, n) in {-1, 0, 1}; W2 .. W4 sparse in {-1, 0, 1}; the last point's dflows are (1, -1, 1, -1),
    so that a pad row that took the clamped point's dout would show.  The phases are all 0 and omega is 1.  fp32, CPU"""
    g = torch.Generator().manual_seed(seed + n)
    inp = {'W1': torch.randint(-1, 2, (HID, IN_DIM), generator=g).float()}
    for k in ('W2', 'W3', 'W4'):
        r = torch.rand(HID, HID, generator=g)
        inp[k] = torch.where(r < W_DENSITY / 2, -1.0, torch.where(r < W_DENSITY, 1.0, 0.0))
    inp['W5'] = torch.randint(-1, 2, (OUT, HID), generator=g).float()
    inp['dflows'] = torch.randint(-1, 2, (OUT, n), generator=g).float()
    inp['dflows'][:, n - 1] = torch.tensor([1.0, -1.0, 1.0, -1.0])
    return inp


def integer_ref(inp, coords):
    """the chain at phase 0 and omega 1 in float64: dz_4 = dout W5, dz_l = dz_{l+1} W_{l+1}.  coords (n, 3) float64.  Returns (grads by
    name: gb1 .. gb5, gW1; dz: [dz_1 .. dz_4] (n, 256); g_poses (n, 3); worst: the largest sum |terms| of every output element and every
    intermediate dz element, that of gW1 in units of 1/4)"""
    w = {k: inp[k].to(F64) for k in ('W1', 'W2', 'W3', 'W4', 'W5')}
    dout = inp['dflows'].to(F64).t() * SCALE_A1
    dz4 = dout @ w['W5']
    dz3 = dz4 @ w['W4']
    dz2 = dz3 @ w['W3']
    dz1 = dz2 @ w['W2']
    dz = [dz1, dz2, dz3, dz4]
    grads = {f'gb{l + 1}': dz[l].sum(0) for l in range(4)}
    grads['gb5'] = dout.sum(0)
    grads['gW1'] = dz1.t() @ coords
    g_poses = dz1 @ w['W1']
    worst = {'dz4': dout.abs() @ w['W5'].abs(), 'dz3': dz4.abs() @ w['W4'].abs(), 'dz2': dz3.abs() @ w['W3'].abs(),
             'dz1': dz2.abs() @ w['W2'].abs(), 'gb5': dout.abs().sum(0), 'gW1': 4 * (dz1.abs().t() @ coords.abs()),
             'g_poses': dz1.abs() @ w['W1'].abs()}
    worst.update({f'gb{l + 1}': dz[l].abs().sum(0) for l in range(4)})
    return grads, dz, g_poses, {k: float(v.max()) for k, v in worst.items()}


# ---- the sine and cosine allowance: torch's own fp32 functions against float64 on the same phases, never below 2 u ----
def trig_delta(phases):
    """(d_sin, d_cos) of a tensor of fp32 phases"""
    p64 = phases.to(F64)
    d_sin = max(2 * U, float((torch.sin(phases).to(F64) - torch.sin(p64)).abs().max()))
    d_cos = max(2 * U, float((torch.cos(phases).to(F64) - torch.cos(p64)).abs().max()))
    return d_sin, d_cos


def synthetic_phases(npad, seed=512):
    """regime (b): `saved` (4, npad, 256) uniform in [-512, 512] rad, pad rows included.  fp32, CPU"""
    g = torch.Generator().manual_seed(seed + npad)
    return (torch.rand(SINES, npad, HID, generator=g) * 2 - 1) * PHASE_RANGE


def upstream(n, seed=11):
    """dflows (4, n), standard normal.  fp32, CPU"""
    return torch.randn(OUT, n, generator=torch.Generator().manual_seed(seed))


# ---- part A2: the backward pass stage by stage ----
def dz_stage(dz_next, w, phase, omega, d_cos, terms=HID):
    """dz = omega (dz_next W) cos(phase) in float64 and its single-stage budget (terms + 3) u omega (|dz_next| |W|) |cos| + MULT d_cos
    omega |dz_next W|: the sum, then the roundings of omega, of the cosine's product and of the store (layer 4: of dout = dflows scale)"""
    co = torch.cos(phase)
    lin = dz_next @ w
    return omega * lin * co, (terms + 3) * U * omega * (dz_next.abs() @ w.abs()) * co.abs() + MULT * d_cos * omega * lin.abs()


def backward_stages(weights, pts, omega, scale, dflows, saved, dz, hin, grads, plan, g_poses=None):
    """{stage: (got, ref, budget)} of one backward call.  weights: [W1, b1, .., W5, b5] fp32; dflows (4, N) fp32; saved (4, Npad, 256) the
    phases the call was given; dz, hin (3, Npad, 256) the kernel's own, read back from the workspace; grads: the ten gradients.  Each stage
    in float64 from the inputs the kernel itself used for it.  dz_1 is not stored: gW1, gb1 and g_poses are two stages, the dz bound on
    dz_1 (from the kernel's dz_2) carried linearly through |coord|, 1 or |W1|, plus the output's own summation term"""
    n = pts.n
    w = [p.to(F64) for p in weights]
    g = dict(zip(GRAD_NAMES, grads))
    u = [saved[l, :n].to(F64) for l in range(SINES)]
    trig = [trig_delta(saved[l, :n]) for l in range(SINES)]
    dout = (dflows * scale).to(F64).t()                  # the fp32 product, as the kernel forms it: (N, 4)
    own_dz = [None] + [dz[l, :n].to(F64) for l in range(3)]   # own_dz[l] = dz_{l+1}, l = 1 .. 3
    own_h = [hin[l, :n].to(F64) for l in range(3)]            # own_h[l] = h_{l+1}
    out = {}
    for l in range(3):
        out[f'hin{l}'] = (hin[l, :n], torch.sin(u[l]), MULT * trig[l][0])
    ref, budget = dz_stage(dout, w[8], u[3], omega, trig[3][1], terms=OUT)
    out['dz4'] = (dz[2, :n], ref, budget)
    for l in (3, 2):                                     # dz_l from the kernel's own dz_{l+1}, W_{l+1}, the phases u_l
        ref, budget = dz_stage(own_dz[l], w[2 * l], u[l - 1], omega, trig[l - 1][1])
        out[f'dz{l}'] = (dz[l - 2, :n], ref, budget)
    for l in (2, 3, 4):                                  # gW_l = dz_l^T h_{l-1}, gb_l = sum_p dz_l
        d, h = own_dz[l - 1], own_h[l - 2]
        out[f'gW{l}'] = (g[f'gW{l}'], d.t() @ h, plan.hidden_terms * U * (d.abs().t() @ h.abs()))
        out[f'gb{l}'] = (g[f'gb{l}'], d.sum(0), plan.hidden_terms * U * d.abs().sum(0))
    s4 = torch.sin(u[3])
    out['gW5'] = (g['gW5'], dout.t() @ s4, plan.chain_terms * U * (dout.abs().t() @ s4.abs()) + MULT * trig[3][0] * dout.abs().sum(0)[:, None])
    tot = dout.sum(0)
    out['gb5'] = (g['gb5'], tot, 2 * U * tot.abs() + U * U * n * dout.abs().sum(0))
    dz1, b1 = dz_stage(own_dz[1], w[2], u[0], omega, trig[0][1])
    c = pts.poses(F64)
    out['gW1'] = (g['gW1'], dz1.t() @ c, b1.t() @ c.abs() + plan.chain_terms * U * (dz1.abs().t() @ c.abs()))
    out['gb1'] = (g['gb1'], dz1.sum(0), b1.sum(0) + plan.chain_terms * U * dz1.abs().sum(0))
    if g_poses is not None:
        out['g_poses'] = (g_poses, dz1 @ w[0], b1 @ w[0].abs() + (HID + 2) * U * (dz1.abs() @ w[0].abs()))
    return out


def fp32_backward(weights, pts, omega, scale, dflows, saved):
    """the fp32 torch restatement of one backward call with every intermediate kept: (dz (3, N, 256), hin (3, N, 256), the ten gradients,
    g_poses), torch's own sin / cos and summation order; gb5 in double, rounded once, as the kernels sum it"""
    n = pts.n
    u = saved[:, :n]
    dout = (dflows * scale).t()
    d = [None] * 5
    d[4] = omega * (dout @ weights[8]) * torch.cos(u[3])
    for l in (3, 2, 1):
        d[l] = omega * (d[l + 1] @ weights[2 * l]) * torch.cos(u[l - 1])
    h = [None] + [torch.sin(u[l]) for l in range(SINES)]
    c = pts.poses(torch.float32)
    grads = [d[1].t() @ c, d[1].sum(0)]
    for l in (2, 3, 4):
        grads += [d[l].t() @ h[l - 1], d[l].sum(0)]
    grads += [dout.t() @ h[4], dout.to(F64).sum(0).float()]
    return torch.stack(d[2:]), torch.stack(h[1:4]), grads, d[1] @ weights[0]


# ---- part B: the forward pass, layer by layer from the kernel's own `saved` ----
def forward_stages(weights, pts, omega, scale, saved, flows):
    """{stage: (got, ref, budget)} for u_1 .. u_4 (rows below N of `saved`) and flows (N, 4): each stage in float64 from the inputs the
    kernel itself used for it.  saved (4, Npad, 256) and flows (4, N) are the kernel's"""
    n = pts.n
    w = [p.to(F64) for p in weights]
    c = pts.poses(F64)
    out = {'u1': (saved[0, :n], omega * (c @ w[0].t() + w[1]), (IN_DIM + 3) * U * omega * (c.abs() @ w[0].abs().t() + w[1].abs()))}
    for l in (2, 3, 4):
        d_sin, _ = trig_delta(saved[l - 2, :n])
        h = torch.sin(saved[l - 2, :n].to(F64))
        wl, bl = w[2 * l - 2], w[2 * l - 1]
        budget = (HID + 3) * U * omega * (h.abs() @ wl.abs().t() + bl.abs()) + MULT * d_sin * omega * wl.abs().sum(1)[None, :]
        out[f'u{l}'] = (saved[l - 1, :n], omega * (h @ wl.t() + bl), budget)
    d_sin, _ = trig_delta(saved[3, :n])
    h = torch.sin(saved[3, :n].to(F64))
    budget = (HID + 3) * U * (h.abs() @ w[8].abs().t() + w[9].abs()) * scale + MULT * d_sin * scale * w[8].abs().sum(1)[None, :]
    out['flows'] = (flows.t(), (h @ w[8].t() + w[9]) * scale, budget)
    return out


def fp32_forward(weights, pts, omega, scale):
    """the fp32 torch restatement with every layer kept: (saved (4, N, 256) phases, flows (4, N))"""
    x = pts.poses(torch.float32)
    saved = []
    for l in range(SINES):
        saved.append(omega * torch.nn.functional.linear(x, weights[2 * l], weights[2 * l + 1]))
        x = torch.sin(saved[-1])
    return torch.stack(saved), (torch.nn.functional.linear(x, weights[8], weights[9]) * scale).t().contiguous()


def resolved_sine_error(weights, omega, scale, saved, n):
    """the smallest uniform sine error (the same sign pattern as the weights, the worst case) that the forward stage budgets resolve:
    min over stages and elements of budget / (omega sum_k |W[j][k]|).  An error below this passes part B"""
    w = [p.to(F64) for p in weights]
    best = float('inf')
    for l in (2, 3, 4, 5):
        d_sin, _ = trig_delta(saved[l - 2, :n])
        h = torch.sin(saved[l - 2, :n].to(F64))
        wl, bl = w[2 * l - 2], w[2 * l - 1]
        amp = wl.abs().sum(1)[None, :]
        best = min(best, float(((HID + 3) * U * (h.abs() @ wl.abs().t() + bl.abs()) / amp + MULT * d_sin).min()))
    return best


def scaled_first_layer(weights, factor=8.0):
    """the weights with W1 and b1 x 8: layer-1 phases of some hundreds of radians, as after training"""
    return [weights[0] * factor, weights[1] * factor] + list(weights[2:])
