"""Per-element references, budgets and cases for the flow-field network kernels (csrc/flownet.hip): what
tests/test_flownet_elements_host.py establishes on the CPU and tests/test_gpu_flownet_elements.py applies to the kernels.
A plain module, no fixtures; everything runs on the device of the tensors it is given.

Part A, the backward pass on exact integers: `integer_inputs` makes a synthetic `saved` in {0, 1, 2} (pad rows 3), sparse W2 / W3 and a
W4 in {-1, 0, 1}, dflows in {-1, 0, 1}; `backward_ref` is the chain in float64 with the gates `saved > 0` and the largest sum |terms| of any
output element or intermediate dh; `gw1_ref` is gW1 = dh1^T x in float64 with its per-element budget.
Part B, the forward pass stage by stage: `forward_stages` evaluates each layer in float64 from the inputs the kernel itself used for it
(the kernel's own `saved`) with a single-stage budget.
`Plan` rebuilds the launch plan (tiles, chain blocks, chunks and how many tiles each walks) from constants read from the sources.
"""
import os
import re
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from flownet_refs import ENCODERS, PROGRESSIVE, layer1_input, poses_of  # noqa: E402

F64 = torch.float64
U = 2.0 ** -24                      # unit roundoff of fp32
MULT, CEIL = 4.0, 1e-4              # the factor and the ceiling of every flownet test (tests/test_gpu_flownet.py)
EXACT_LIMIT = 2.0 ** 23             # sum |terms| below this: every partial sum is an integer below 2^24, exact in fp32 in any order
SCALE_A, SCALE_B = 2.0, 3.0
NETS = ('RBF', 'FFN', 'RBFG', 'PE', 'PRBF', 'PPE')
HID = 256
GRAD_NAMES = [f'g{k}{l}' for l in (1, 2, 3, 4) for k in ('W', 'b')]
EXACT_NAMES = ('gb1', 'gW2', 'gb2', 'gW3', 'gb3', 'gW4', 'gb4')

# ---- the cases: name -> ('grid', times, h, w) or ('list', N) ----
A_SHAPES = {'one': ('grid', (0.5,), 1, 1), 'few': ('list', 171), 'past_caps': ('grid', (0.0, 0.25, 1.0), 113, 200)}
B_SHAPES = {'one': ('grid', (0.5,), 1, 1), 'ragged': ('grid', (0.0, 0.25, 1.0), 13, 37), 'past_cap': ('grid', (0.0, 0.25, 1.0), 151, 290)}
B_PAST_CAP_NETS = ('RBF', 'PRBF')   # the cap is a property of the launch, not of the encoding


# ---- constants of the kernels, read from the sources with the line that applies each ----
def _source(name):
    with open(os.path.join(ROOT, 'sin-inn_amd', 'csrc', name)) as f:
        return f.read()


def _const(text, name):
    m = re.search(rf'constexpr int {name} = ([^;]+);', text)
    assert m, name
    return m.group(1).strip()


def kernel_constants():
    tile, src = _source('flownet_tile.h'), _source('flownet.hip')
    c = {'P': int(_const(tile, 'FN_P')), 'CHAIN_CAP': int(_const(tile, 'FN_CHAIN_MAX_BLOCKS')), 'FWD_CAP': int(_const(src, 'FN_FWD_MAX_BLOCKS')),
         'WT': int(_const(src, 'FN_WT'))}
    assert _const(src, 'FN_CHUNK_ELEMS') == '1 << 15'
    c['CHUNK_ELEMS'] = 1 << 15
    for line, text in (('q.ntiles = (q.N + FN_P - 1) / FN_P;', tile),
                       ('return ntiles < FN_CHAIN_MAX_BLOCKS ? ntiles : FN_CHAIN_MAX_BLOCKS;', tile),
                       ('const int blocks = q.ntiles < FN_FWD_MAX_BLOCKS ? q.ntiles : FN_FWD_MAX_BLOCKS;', src),
                       ('for (int tile = blockIdx.x; tile < q.ntiles; tile += gridDim.x)', src),
                       ('const int want = FN_CHUNK_ELEMS / kf;', src), ('return ntiles < want ? ntiles : want;', src),
                       ('for (int tile = chunk; tile < q.ntiles; tile += nchunks)', src),
                       ('static constexpr bool NARROW = KW < FN_WT;', src), ('static constexpr int KT = NARROW ? KW : FN_WT;', src),
                       ('static constexpr int CHUNK_KF = FN_WT * (KW / KT);', src),
                       ('const int nc = wgrad_chunks(ntiles, Hidden::CHUNK_KF);', src), ('const int nc = wgrad_chunks(q.ntiles, E::CHUNK_KF);', src),
                       ('using Hidden = LayerInput<FN_HID, FN_HID>;', src),
                       ('struct Enc<SININN_FLOWNET_RBF> : LayerInput<512, 512, true>', src),
                       ('struct Enc<SININN_FLOWNET_FOURIER> : LayerInput<512, 512, false, true>', src),
                       ('struct Enc<SININN_FLOWNET_RBFG> : LayerInput<512, 512, true>', src),
                       ('struct Enc<SININN_FLOWNET_PE> : LayerInput<24, 32>', src)):
        assert line in text, line
    return c


KW = {'RBF': 512, 'FFN': 512, 'RBFG': 512, 'PRBF': 512, 'PE': 32, 'PPE': 32}    # the padded K width of layer 1 (the Enc<> rows above)


def _walks(ntiles, stride):
    counts = [len(range(b, ntiles, stride)) for b in range(stride)]
    return min(counts), max(counts)


class Plan:
    """the launches of one call at N points: 64-point tiles; forward and chain blocks grid-stride over them; the weight-gradient kernels
    split them over chunks, chunk c walks tiles c, c + chunks, ..  `*_walk`: (fewest, most) tiles any block / chunk walks"""

    def __init__(self, n, name=None):
        c = kernel_constants()
        self.p = c['P']
        self.n, self.ntiles = n, (n + c['P'] - 1) // c['P']
        self.npad = self.ntiles * c['P']
        self.fwd_blocks, self.chain_blocks = min(self.ntiles, c['FWD_CAP']), min(self.ntiles, c['CHAIN_CAP'])

        def chunks(kw):
            kt = kw if kw < c['WT'] else c['WT']
            return min(self.ntiles, c['CHUNK_ELEMS'] // (c['WT'] * (kw // kt)))
        self.hidden_chunks = chunks(HID)
        self.l1_chunks = chunks(KW[name]) if name else None
        self.fwd_walk, self.chain_walk = _walks(self.ntiles, self.fwd_blocks), _walks(self.ntiles, self.chain_blocks)
        self.hidden_walk = _walks(self.ntiles, self.hidden_chunks)
        self.l1_walk = _walks(self.ntiles, self.l1_chunks) if name else None

    def chunk_rows(self, chunk, nchunks):
        """the point rows (below N) of the tiles a chunk walks"""
        rows = torch.cat([torch.arange(t * self.p, min((t + 1) * self.p, self.n)) for t in range(chunk, self.ntiles, nchunks)])
        return rows


# ---- networks, masks, points ----
def build(name):
    """the network of a name as the golden tests build it (their seeds)"""
    if name in ('RBF', 'FFN'):
        from test_flownet_golden import build as b
    elif name == 'PRBF':
        from test_flownet_progressive_golden import build as b
    elif name == 'RBFG':
        from test_flownet_grid_golden import build as b
    else:
        from test_flownet_pe_golden import build as b
    return b(name)


def ramp(name):
    """(the fixture's `mask_ramp` on the host, the k_active a controller would pass) of a progressive network, else (None, None)"""
    from sin_inn_amd import flownet
    if name not in PROGRESSIVE:
        return None, None
    fixture = {'PRBF': 'golden_flownet_progressive.npz', 'PPE': 'golden_flownet_pe.npz'}[name]
    host = torch.from_numpy(np.load(os.path.join(ROOT, 'tests', 'golden', fixture))['mask_ramp']).clone()
    k = flownet.last_open(host)
    assert host.shape == ({'PRBF': 515, 'PPE': 27}[name],) and 3 < k < host.numel() and 0.0 < float(host[k - 1]) < 1.0
    return host, k


class Points:
    """the points of a case on a device: a grid (times, ys, xs) or a pose list (N, 3), fp32 as the kernels receive them"""

    def __init__(self, shape, dev='cpu'):
        if shape[0] == 'grid':
            _, times, h, w = shape
            self.times, self.ys, self.xs = torch.tensor(times).to(dev), torch.linspace(-1, 1, h).to(dev), torch.linspace(-1, 1, w).to(dev)
            self.grid, self.list = (len(times), h, w), None
            self.n = len(times) * h * w
        else:
            # ('list', N): N seeded points of [-1, 1]^3; ('list', N, first): the rows first .. first + N - 1 of the list of 171
            n = 171 if len(shape) > 2 else shape[1]
            first = shape[2] if len(shape) > 2 else 0
            every = torch.rand(n, 3, generator=torch.Generator().manual_seed(171)) * 2 - 1
            self.n = shape[1]
            self.list = every[first:first + self.n].to(dev).contiguous()
            self.grid = None

    def poses(self, dtype):
        return self.list.to(dtype) if self.grid is None else poses_of(self.times, self.ys, self.xs, dtype)

    def planar(self, flows):
        """flows / dflows of a call as (4, N)"""
        return flows if self.grid is None else flows.permute(1, 0, 2, 3).reshape(4, -1)

    def shaped(self, planar):
        """(4, N) as the call takes dflows"""
        if self.grid is None:
            return planar
        t, h, w = self.grid
        return planar.view(4, t, h, w).permute(1, 0, 2, 3).contiguous()


def layer1_in(name, bufs, pts, mask, dtype, rows=1 << 14):
    """`layer1_input` of tests/flownet_refs.py at the points of a case, in blocks of rows (the RBF encoder holds N x 512 x 3 values)"""
    poses = pts.poses(dtype)
    return torch.cat([layer1_input(name, bufs, poses[i:i + rows], mask) for i in range(0, poses.shape[0], rows)])


def feature_delta(x32, x64):
    """per feature: max(2 u, the largest deviation of the fp32 torch encoding from float64 over the case's points)"""
    return (x32.to(F64) - x64).abs().amax(0).clamp_min(2 * U)


# ---- part A: the backward pass on exact integers ----
W_DENSITY = 1.0 / 16                # of W2 / W3: 16 entries per row on average; the host test establishes the precondition with it


def integer_inputs(n, npad, seed=2024):
    """saved (3, npad, 256) in {0, 1, 2}, half of it zero, rows from n on 3; W2, W3 sparse in {-1, 0, 1}; W4 (4, 256) and dflows (4, n) in
    {-1, 0, 1}; the last point's dflows are (1, -1, 1, -1), so that a pad row that took the clamped point's dout would show.  fp32, CPU"""
    g = torch.Generator().manual_seed(seed + n)
    saved = torch.tensor([0.0, 0.0, 1.0, 2.0])[torch.randint(0, 4, (3, npad, HID), generator=g)]
    saved[:, n:] = 3.0
    ws = []
    for _ in range(2):
        r = torch.rand(HID, HID, generator=g)
        ws.append(torch.where(r < W_DENSITY / 2, -1.0, torch.where(r < W_DENSITY, 1.0, 0.0)))
    w4 = torch.randint(-1, 2, (4, HID), generator=g).float()
    dflows = torch.randint(-1, 2, (4, n), generator=g).float()
    dflows[:, n - 1] = torch.tensor([1.0, -1.0, 1.0, -1.0])
    return {'saved': saved, 'W2': ws[0], 'W3': ws[1], 'W4': w4, 'dflows': dflows}


def backward_ref(inp, n, scale=SCALE_A):
    """the chain in float64 with gates `saved > 0`, rows below n only.  Returns (grads: the seven exact gradients by name; dh: [dh1, dh2,
    dh3] (n, 256); dout (n, 4); worst: the largest sum |terms| over every output element and every intermediate dh element)"""
    s = inp['saved'][:, :n].to(F64)
    w2, w3, w4 = (inp[k].to(F64) for k in ('W2', 'W3', 'W4'))
    dout = inp['dflows'].to(F64).t() * scale
    dh3 = (dout @ w4) * (s[2] > 0)
    dh2 = (dh3 @ w3) * (s[1] > 0)
    dh1 = (dh2 @ w2) * (s[0] > 0)
    grads = {'gW4': dout.t() @ s[2], 'gb4': dout.sum(0), 'gW3': dh3.t() @ s[1], 'gb3': dh3.sum(0), 'gW2': dh2.t() @ s[0], 'gb2': dh2.sum(0),
             'gb1': dh1.sum(0)}
    worst = {'dh3': dout.abs() @ w4.abs(), 'dh2': dh3.abs() @ w3.abs(), 'dh1': dh2.abs() @ w2.abs(),
             'gW4': dout.abs().t() @ s[2], 'gb4': dout.abs().sum(0), 'gW3': dh3.abs().t() @ s[1], 'gb3': dh3.abs().sum(0),
             'gW2': dh2.abs().t() @ s[0], 'gb2': dh2.abs().sum(0), 'gb1': dh1.abs().sum(0)}
    return grads, [dh1, dh2, dh3], dout, {k: float(v.max()) for k, v in worst.items()}


def gw1_ref(name, bufs, pts, mask, dh1, plan):
    """gW1 = dh1^T x in float64 and its per-element budget (chain + partials + c) u S + MULT D: x the layer-1 input in
    float64, S = |dh1|^T |x|, D = sum_p |dh1[p][j]| delta_k; chain = 64 x the most tiles a chunk walks, partials = the chunks; c = 2, and 3
    for a progressive network (the folded mask).  Returns (ref, budget, S)"""
    x64 = layer1_in(name, bufs, pts, mask, F64)
    delta = feature_delta(layer1_in(name, bufs, pts, mask, torch.float32), x64)
    ref = dh1.t() @ x64
    big_s = dh1.abs().t() @ x64.abs()
    big_d = dh1.abs().sum(0)[:, None] * delta[None, :]
    c = 3 if name in PROGRESSIVE else 2
    terms = plan.p * plan.l1_walk[1] + plan.l1_chunks + c
    return ref, terms * U * big_s + MULT * big_d, big_s


def closed_columns(mask, k_active):
    """columns of a progressive gW1 that are an exact +0: the mask is zero there or the column lies beyond k_active"""
    closed = mask == 0
    closed[k_active:] = True
    return closed


# ---- part B: the forward pass, layer by layer from the kernel's own `saved` ----
def forward_stages(name, bufs, weights, pts, mask, saved, flows, scale=SCALE_B):
    """{stage: (got, ref, budget)} for saved[0], saved[1], saved[2] (rows below N) and flows (N, 4): each stage in float64 from the inputs
    the kernel itself used for it, with its single-stage budget.  weights: [W1, b1, .., W4, b4] fp32; mask: the host values moved to the
    device, or None; saved (3, Npad, 256) and flows (4, N) are the kernel's"""
    n = pts.n
    w = [p.to(F64) for p in weights]
    out = {}
    # layer 1: x in float64; progressive: x (W1 m)^T, the mask folded into the weights as the pack kernel folds it
    x64 = layer1_in(name, bufs, pts, None, F64)
    delta = feature_delta(layer1_in(name, bufs, pts, None, torch.float32), x64)
    w1 = w[0] if mask is None else w[0] * mask.to(F64)[None, :]
    live = x64.shape[1] if mask is None else int((mask != 0).sum())
    c = 2 if mask is None else 3
    ref = torch.relu(x64 @ w1.t() + w[1])
    budget = (live + c) * U * (x64.abs() @ w1.abs().t() + w[1].abs()) + MULT * (delta[None, :] @ w1.abs().t())
    out['saved0'] = (saved[0, :n], ref, budget)
    for l in (1, 2):
        a = saved[l - 1, :n].to(F64)
        ref = torch.relu(a @ w[2 * l].t() + w[2 * l + 1])
        budget = (HID + 2) * U * (a @ w[2 * l].abs().t() + w[2 * l + 1].abs())
        out[f'saved{l}'] = (saved[l, :n], ref, budget)
    a = saved[2, :n].to(F64)
    ref = (a @ w[6].t() + w[7]) * scale
    budget = (HID + 3) * U * (a @ w[6].abs().t() + w[7].abs()) * scale
    out['flows'] = (flows.t(), ref, budget)
    return out


def fp32_forward(name, bufs, weights, pts, mask, scale=SCALE_B):
    """the fp32 torch restatement with every layer kept: (saved (3, N, 256), flows (4, N)), torch's own sin / exp and summation order"""
    x = layer1_in(name, bufs, pts, mask, torch.float32)
    saved = []
    for l in range(3):
        x = torch.relu(torch.nn.functional.linear(x, weights[2 * l], weights[2 * l + 1]))
        saved.append(x)
    return torch.stack(saved), (torch.nn.functional.linear(x, weights[6], weights[7]) * scale).t().contiguous()


# ---- the comparisons ----
def element_ratio(got, ref, budget):
    """max over elements of |got - ref| / budget; 0 where both are 0, inf where the error exceeds a zero budget or `got` is not finite"""
    err = (got.to(F64) - ref).abs()
    err = torch.where(torch.isfinite(got), err, torch.full_like(err, float('inf')))
    ratio = torch.where(err == 0, torch.zeros_like(err), err / budget)
    return float(ratio.max())


def relmax(a, ref):
    """the yardstick of the other flownet tests: max |a - ref| / max |ref| over the whole tensor"""
    a, ref = a.detach().to(F64), ref.detach().to(F64)
    err = (a - ref).abs()
    err = torch.where(torch.isfinite(a), err, torch.full_like(err, float('inf')))
    return float(err.max() / ref.abs().max())


def relmax_budget(ref32, ref64):
    """min(MULT x the fp32-torch unit, CEIL), the budget of the other flownet tests"""
    return min(MULT * relmax(ref32, ref64), CEIL)
