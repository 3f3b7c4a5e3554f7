"""GPU: the flow-loss kernels of csrc/flowloss.hip at the bench shape (4 x 512 x 512), at ragged shapes and on smooth flows, against
float64.

tests/test_gpu_flow.py compares these kernels with fp32 references on fixtures of at most 64 x 64 pixels and `randn` flows, at 1e-3 ..
1e-4 of the max-norm.  Here every operator runs where its launch plan has many tiles per accumulator slot, several trips per thread,
partial tiles in both directions, and -- for the splat -- flows that are locally smooth, which is the only regime in which the lane
merges of splat_fwd_kernel do any work.

Method (that of tests/test_gpu_elementwise_sizes.py):
  * the reference is float64 torch of the same operation, evaluated on the GPU, from the fp32 inputs the kernel received, widened.  The
    float64 restatements live in this file because the budgets need their per-element pieces (sums of |terms|, derivatives);
    test_references_are_the_oracle ties each of them to oracle/flow_oracle.py, run in float64 on the CPU, value and autograd gradients.
    A later stage starts from what the earlier kernel wrote (sum(mask) handed from forward to backward, the scalar formed from `acc`,
    occlusion_brox from the warp kernel's output);
  * budgets, U = 2^-24, each derived next to its reference:
      - a sum accumulated in an unknown order: depth * U * sum|terms|, depth = roundings on the longest path;
      - the splat coordinate x + flow is rounded to fp32 (half an ulp of the coordinate, 2^-16 at x >= 256): that rounding times the
        float64 derivative of the output with respect to the coordinate;
      - census and SSIM (rsqrtf, __frcp_rn, E[x^2] - E[x]^2 in fp32) are not derivable from U alone.  Their unit is measured on the
        REFERENCE: the same formula evaluated in fp32 torch on the same inputs, against float64; per element the unit is the worst
        such deviation, for a sum it is the sum of the deviations.  The kernel is allowed MULT = 4 units: a factor 2 because it is a
        second, independent evaluation order of the (2 md + 1)^2 window (gather instead of autograd's scatter, rsqrt instead of sqrt +
        divide, reciprocal + multiply instead of divide, FMA contraction), each of which can at most double a per-term bound, and a
        factor 2 because the unit is the maximum of one sample of roundings and the kernel draws another;
  * every case recomputes its launch plan from the kernel's formulas and asserts what it claims to exercise;
  * discontinuities are excluded by a condition on the inputs, with an asserted cap on the excluded share.

Measured on an MI355X (worst error / budget; see the `ratio(...)` lines of a run with -s):
  splat (summation; softmax / average / linear payloads; the occlusion_wang range map): out 1.00, gin 1.00, gflow 1.00, normalised
    quotient 0.98.  These sit at 1 because the budget is dominated by the coordinate term and that term is attained: somewhere among a
    million pixels x + flow rounds by almost exactly half an ulp (2^-16 at x >= 256, errors of 2e-5 .. 6e-5 in out); the same figures
    come out of the fp32 CPU oracle in place of the kernel.  gflow excluded 0.04 .. 0.05 % (cap 0.2 %), wang mask undecided <= 0.006 %
    (cap 0.01 %), brox 0 %, tiny non-zero norm <= 0.0001 %.
  census: sum 0.041, scalar 0.33, g1 / g2 0.40.  Units: sum of deviations 1e-6 of the sum; per-element gradient 7.8e-9 .. 1.7e-6,
    i.e. 0.7e-4 .. 2.1e-4 of max |g|.  Most gradient ratios are 0.25 = 1 / MULT: kernel and fp32 reference share their worst error.
  SSIM: sum 0.017, scalar 0.28, g1 / g2 0.27.  Units: sum 1.5e-5 .. 2e-5 of the sum; gradient 6.5e-13 .. 8.5e-10, 0.2e-6 .. 2e-6 of max |g|.
  masked L1: sum 0.0074, scalar 0.084, gradients 0.18 (0.35 through the module).  Smoothness: sums 0.015, scalar 0.17, gflow 0.77.
  54 tests, 12 s.
Mutations of a scratch copy of the kernel, each failing (worst ratio): take_v without rse 1.4e6 (every splat and wang case); window
flush without its last row 4.7e5 and a far south-east tap not written 9e5 (smooth9 and randn3 cases; smooth2 never gets there, as its
plan asserts); census left halo column dropped on the last tile column 7e3 (g1 / g2); slot 63 left out of the finish, the SSIM border
mask sum stopping at y0 + 16 (only 18 x 35, where the last tile row is full) and masked_l1_fwd taking a single trip (only 512 x 512):
all three by the exact sum(mask); smooth_bwd without stencil point j = order 9.7e5.
Bug found: softsplat_bwd_kernel lacked the forward's |target| < 1e9 guard.  A flow of +inf or beyond 2^31 made it read gout out of
bounds (illegal memory access on the MI355X), -inf and NaN gave NaN gradients; see the comment in the kernel.  Fixed there.
"""
import os

import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

U = 2.0 ** -24
F64 = torch.float64
MULT = 4.0                                  # units of the fp32-reference deviation allowed to census / SSIM (module docstring)

SP_TX, SP_TY, SP_R, SP_CC = 32, 8, 8, 4     # csrc/flowloss.hip: splat tile, window margin, channels per LDS pass
CT = 16                                     # census / SSIM tile
SLOTS, ACC_FLOATS = 64, 130                 # CENSUS_SLOTS, SININN_CENSUS_ACC_FLOATS
BIG = (4, 512, 512)                         # tools/bench_flowloss.py


@pytest.fixture(scope='module')
def dev():
    import sin_inn_amd  # noqa: F401
    assert torch.cuda.is_available(), 'GPU tests need a GPU'
    return torch.device('cuda', 0)


def FL():
    from sin_inn_amd import flowloss
    return flowloss


def call(name, *args):
    from sin_inn_amd import _lib
    from sin_inn_amd.ops import _stream
    _lib.check(getattr(_lib.lib(), name)(*args, _stream()))


def P(t):
    from sin_inn_amd.ops import ptr
    return ptr(t)


def ratio(name, got, ref, budget, exempt=None):
    """worst |got - ref| / budget over the tensor; prints it; NaN / inf in `got` count as infinite"""
    got, ref = got.detach().to(F64), ref.detach().to(F64)
    err = (got - ref).abs()
    err = torch.where(torch.isfinite(got), err, torch.full_like(err, float('inf')))
    r = err / torch.as_tensor(budget, dtype=F64, device=err.device).expand_as(err).clamp_min(1e-300)
    r = torch.where(err == 0, torch.zeros_like(r), r)
    if exempt is not None:
        r = torch.where(exempt.expand_as(r), torch.zeros_like(r), r)
    worst = float(r.max())
    print(f'ratio({name}) = {worst:.3g}   [max err {float(err.max()):.3g}, max |ref| {float(ref.abs().max()):.3g}]')
    return worst


# =================================================================================================================================
# inputs
# =================================================================================================================================
def cpu_gen(seed):
    return torch.Generator().manual_seed(seed)


def make_flow(kind, b, h, w, seed, dev):
    """smooth2 / smooth9: bicubic upsampling of a normal field with one node per 64 pixels (8 x 8 at 512 x 512), amplitude 2 / 9: what a
    trained flow looks like.  Amplitude 9, not the 6 first thought of: at 6 only 5 % of the pixels have a tap outside their block's window
    (23 % have a component beyond 8 pixels, but the tile's own extent keeps most of those inside); at 9 it is 17 .. 21 % with 68 .. 75 %
    of the pairs still merging (measured on the CPU for seeds 11 .. 41, both shapes).
    randn3: independent per pixel (the control: what tests/test_gpu_flow.py uses)"""
    g = cpu_gen(seed)
    if kind == 'randn3':
        f = torch.randn(b, 2, h, w, generator=g) * 3
    else:
        amp = {'smooth2': 2.0, 'smooth9': 9.0}[kind]
        nodes = torch.randn(b, 2, -(-h // 64), -(-w // 64), generator=g)
        f = F.interpolate(nodes, size=(h, w), mode='bicubic', align_corners=False) * amp
    return f.to(dev).contiguous()


BAD_VALUES = (float('nan'), float('inf'), float('-inf'), 3e9, -2e9, float('nan'))
BAD_PIXELS = ((0, 0, 100, 100), (0, 1, 100, 131), (1, 0, 7, 31), (1, 1, 201, 300), (2, 0, 50, 64), (2, 1, 151, 33))


def plant_bad(flow):
    """NaN, +-inf and |flow| > 1e9 at six pixels (tile corners, tile interiors, odd and even rows: both sides of every merge)"""
    flow = flow.clone()
    for (b, k, y, x), v in zip(BAD_PIXELS, BAD_VALUES):
        flow[b, k, y, x] = v
    return flow


def make_images(b, c, h, w, seed, dev):
    g = cpu_gen(seed)
    im = torch.rand(b, c, h, w, generator=g)
    warped = (im + 0.05 * torch.randn(b, c, h, w, generator=g)).clamp(0, 1)
    return im.to(dev).contiguous(), warped.to(dev).contiguous()


def make_mask(b, mc, h, w, seed, dev):
    """0 / 1, about 20 % zeros, and one all-zero 16 x 16 tile (where H and W allow it)"""
    m = (torch.rand(b, mc, h, w, generator=cpu_gen(seed)) > 0.2).float()
    if h >= 48 and w >= 80:
        m[0, :, 32:48, 64:80] = 0
    return m.to(dev).contiguous()


# =================================================================================================================================
# A. splat: plan, float64 reference with its pieces
# =================================================================================================================================
def splat_plan(flow):
    """what splat_fwd_kernel does with this flow, from the fp32 x + flow exactly as the kernel forms it.  Shares are of the pixel pairs
    that can merge at all: horizontally (x, x + 1) inside one 32-pixel tile row, vertically (y, y + 1) with y even (the two rows of a
    wave; tiles start at multiples of 8)."""
    b, _, h, w = flow.shape
    dev = flow.device
    X, Y = torch.arange(w, device=dev), torch.arange(h, device=dev)
    ox = X.to(torch.float32)[None, None, :] + flow[:, 0]
    oy = Y.to(torch.float32)[None, :, None] + flow[:, 1]
    ok = (ox == ox) & (oy == oy) & (ox.abs() < 1e9) & (oy.abs() < 1e9)
    nwx = torch.where(ok, ox.floor(), torch.zeros_like(ox)).to(torch.int64)
    nwy = torch.where(ok, oy.floor(), torch.zeros_like(oy)).to(torch.int64)
    eh = (((X % SP_TX) != SP_TX - 1) & (X + 1 < w))[:-1]
    ev = ((Y % 2 == 0) & (Y + 1 < h))[:-1]
    gh = ok[:, :, :-1] & ok[:, :, 1:] & (nwx[:, :, 1:] == nwx[:, :, :-1] + 1) & (nwy[:, :, 1:] == nwy[:, :, :-1]) & eh
    gv = ok[:, :-1] & ok[:, 1:] & (nwx[:, 1:] == nwx[:, :-1]) & (nwy[:, 1:] == nwy[:, :-1] + 1) & ev[:, None]
    x0, y0 = (X // SP_TX * SP_TX)[None, None, :], (Y // SP_TY * SP_TY)[None, :, None]
    far = torch.zeros_like(ok)
    oob = torch.zeros_like(ok)
    for dx, dy in ((0, 0), (1, 0), (0, 1), (1, 1)):
        tx, ty = nwx + dx, nwy + dy
        valid = (tx >= 0) & (tx < w) & (ty >= 0) & (ty < h)
        inwin = (tx >= x0 - SP_R) & (tx < x0 + SP_TX + SP_R) & (ty >= y0 - SP_R) & (ty < y0 + SP_TY + SP_R)
        far |= ok & valid & ~inwin
        oob |= ok & ~valid
    n = b * h * w
    return dict(tiles=b * -(-h // SP_TY) * -(-w // SP_TX), tiles_x=-(-w // SP_TX), tiles_y=-(-h // SP_TY),
                give_h=float(gh.sum()) / (b * h * int(eh.sum())), give_v=float(gv.sum()) / (b * w * int(ev.sum())),
                far=float(far.sum()) / n, oob=float(oob.sum()) / n, skipped=int((~ok).sum()),
                left=int((ok & (nwx < 0)).sum()), right=int((ok & (nwx + 1 >= w)).sum()),
                top=int((ok & (nwy < 0)).sum()), bottom=int((ok & (nwy + 1 >= h)).sum()),
                partial_x=w % SP_TX != 0, partial_y=h % SP_TY != 0)


def assert_flow_kind(kind, plan):
    """the regime each flow kind exists for (bounds of the issue: well clear of 94 / 82 %, 23 % and 0.9 % measured on the CPU)"""
    print(f'plan({kind}) = ' + ', '.join(f'{k} {v:.4g}' if isinstance(v, float) else f'{k} {v}' for k, v in plan.items()))
    if kind == 'smooth2':
        assert plan['give_h'] > 0.8 and plan['give_v'] > 0.8 and plan['far'] == 0, plan
    elif kind == 'smooth9':
        assert plan['give_h'] > 0.6 and plan['give_v'] > 0.6 and plan['far'] > 0.1, plan
        assert min(plan['left'], plan['right'], plan['top'], plan['bottom']) > 0, 'flows must leave the image at all four borders'
    else:
        assert plan['give_h'] < 0.05 and plan['give_v'] < 0.05, plan


def taps64(flow):
    """float64 taps of every source pixel from the widened fp32 flow: per tap (nw, ne, sw, se) the target index, its validity, the
    bilinear weight and d weight / d(ox, oy); plus dx, dy = half an ulp of the fp32 coordinate the kernel works with, and `near` =
    pixels whose fp32 coordinate is within 1e-4 of an integer (where d out / d flow jumps).  Pixels the kernel skips (NaN, +-inf,
    |target| >= 1e9) have no valid tap."""
    b, _, h, w = flow.shape
    dev = flow.device
    xs32 = torch.arange(w, device=dev, dtype=torch.float32)[None, None, :]
    ys32 = torch.arange(h, device=dev, dtype=torch.float32)[None, :, None]
    ox32, oy32 = xs32 + flow[:, 0], ys32 + flow[:, 1]
    ok = torch.isfinite(ox32) & torch.isfinite(oy32) & (ox32.abs() < 1e9) & (oy32.abs() < 1e9)
    ox32, oy32 = torch.where(ok, ox32, torch.zeros_like(ox32)), torch.where(ok, oy32, torch.zeros_like(oy32))
    f = torch.where(ok[:, None], flow, torch.zeros_like(flow)).to(F64)
    ox, oy = xs32.to(F64) + f[:, 0], ys32.to(F64) + f[:, 1]
    nwx, nwy = ox.floor(), oy.floor()
    fx, fy = ox - nwx, oy - nwy
    inf = torch.full_like(ox32, float('inf'))

    def half_ulp(v):
        return (torch.nextafter(v.abs(), inf) - v.abs()).to(F64) / 2

    def flat(t):
        return t.reshape(b, 1, h * w)

    near = ((ox32 - ox32.round()).abs() < 1e-4) | ((oy32 - oy32.round()).abs() < 1e-4)
    taps = []
    for dx_, dy_ in ((0, 0), (1, 0), (0, 1), (1, 1)):
        tx, ty = nwx + dx_, nwy + dy_
        wx, dwx = (fx, 1.0) if dx_ else (1 - fx, -1.0)
        wy, dwy = (fy, 1.0) if dy_ else (1 - fy, -1.0)
        valid = (ok & (tx >= 0) & (tx < w) & (ty >= 0) & (ty < h)).to(F64)
        idx = (ty.clamp(0, h - 1) * w + tx.clamp(0, w - 1)).long()
        taps.append(dict(idx=flat(idx), valid=flat(valid), w=flat(wx * wy), dwdx=flat(dwx * wy), dwdy=flat(dwy * wx)))
    return dict(taps=taps, dx=flat(torch.where(ok, half_ulp(ox32), torch.zeros_like(ox))),
                dy=flat(torch.where(ok, half_ulp(oy32), torch.zeros_like(oy))), near=near, ok=ok, shape=(b, h, w))


def scatter64(src, T, weight):
    """out[b, c, target] += src[b, c, p] * weight(tap)[b, 1, p] over the valid taps"""
    b, h, w = T['shape']
    out = torch.zeros(b, src.shape[1], h * w, dtype=F64, device=src.device)
    for t in T['taps']:
        out.scatter_add_(2, t['idx'].expand(-1, src.shape[1], -1), src * (weight(t) * t['valid']))
    return out


def splat_ref(inp, T):
    """float64 summation splat and its budget per output element.
    Terms in[p] * w_tap: w = (1 - fx)(1 - fy) is one rounding (the two factors are exact differences of the fp32 coordinate and an
    integer), the product with in[p] a second.  Additions into one element: every term that lands there (lane merge, LDS atomic or
    global atomic: one addition each) and one flush of every block's window that holds some of them, at most one per term:
    2 cnt additions, each U * |partial sum| <= U * S.  Budget = (2 + 2 cnt) U S  +  coordinate rounding: in float64 out is
    sum in[p] w_tap(ox, oy), so |d out| <= sum |in[p]| (|dw/dox| dx + |dw/doy| dy)."""
    b, h, w = T['shape']
    src = inp.to(F64).reshape(b, inp.shape[1], h * w)
    ref = scatter64(src, T, lambda t: t['w'])
    S = scatter64(src.abs(), T, lambda t: t['w'])
    cnt = scatter64(torch.ones(b, 1, h * w, dtype=F64, device=inp.device), T, lambda t: (t['w'] > 0).to(F64))
    E = scatter64(src.abs(), T, lambda t: t['dwdx'].abs() * T['dx'] + t['dwdy'].abs() * T['dy'])
    budget = (2 + 2 * cnt) * U * S + E
    shape = (b, inp.shape[1], h, w)
    return ref.reshape(shape), budget.reshape(shape)


def splat_bwd_ref(inp, gout, T):
    """float64 gin, gflow of the summation splat (closed form; test_references_are_the_oracle checks it against autograd of the oracle).
      gin[c]  = sum_t g_t w_t            4 products (weight 1 rounding, product 1) and 3 additions: 5 U sum |g_t| w_t,
                                         coordinate: sum |g_t| (|dw_t/dox| dx + |dw_t/doy| dy)
      gfx     = sum_c in[c] sum_t g_t dw_t/dox = sum_c in[c] ((g_ne - g_nw)(1 - fy) + (g_se - g_sw) fy): difference, 1 - fy, product,
                addition, product with in[c]: 5 roundings, then C additions: (5 + C) U sum_c |in[c]| sum_t |g_t| |dw_t/dox|;
                it does not depend on ox inside a cell, and d gfx / d oy = sum_c in[c] (g_nw - g_ne - g_sw + g_se)   (gfy likewise)"""
    b, h, w = T['shape']
    c = inp.shape[1]
    src, g = inp.to(F64).reshape(b, c, h * w), gout.to(F64).reshape(b, c, h * w)
    gt = [g.gather(2, t['idx'].expand(-1, c, -1)) * t['valid'] for t in T['taps']]
    taps = T['taps']
    gin = sum(q * t['w'] for q, t in zip(gt, taps))
    gin_b = 5 * U * sum(q.abs() * t['w'] for q, t in zip(gt, taps)) + \
        sum(q.abs() * (t['dwdx'].abs() * T['dx'] + t['dwdy'].abs() * T['dy']) for q, t in zip(gt, taps))
    cross = (gt[0] - gt[1] - gt[2] + gt[3]).abs()
    gfx = (src * sum(q * t['dwdx'] for q, t in zip(gt, taps))).sum(1)
    gfy = (src * sum(q * t['dwdy'] for q, t in zip(gt, taps))).sum(1)
    gfx_b = (5 + c) * U * (src.abs() * sum(q.abs() * t['dwdx'].abs() for q, t in zip(gt, taps))).sum(1) + \
        T['dy'][:, 0] * (src.abs() * cross).sum(1)
    gfy_b = (5 + c) * U * (src.abs() * sum(q.abs() * t['dwdy'].abs() for q, t in zip(gt, taps))).sum(1) + \
        T['dx'][:, 0] * (src.abs() * cross).sum(1)
    return (gin.reshape(b, c, h, w), gin_b.reshape(b, c, h, w),
            torch.stack((gfx, gfy), 1).reshape(b, 2, h, w), torch.stack((gfx_b, gfy_b), 1).reshape(b, 2, h, w))


SPLAT_CASES = [('smooth2', (4, 3, 512, 512), False), ('smooth9', (4, 4, 512, 512), False), ('randn3', (4, 3, 512, 512), False),
               ('smooth2', (3, 5, 203, 317), False), ('smooth9', (3, 5, 203, 317), False), ('randn3', (3, 5, 203, 317), False),
               ('smooth2', (3, 5, 203, 317), True), ('smooth9', (4, 3, 512, 512), True)]


@pytest.mark.parametrize('kind,shape,bad', SPLAT_CASES, ids=[f'{k}-{"x".join(map(str, s))}{"-nonfinite" if bad else ""}'
                                                              for k, s, bad in SPLAT_CASES])
def test_splat_forward_and_gradients(dev, kind, shape, bad):
    """summation splat: forward element-wise, gin and gflow element-wise, the gin-only and gflow-only launches.
    bad: six planted pixels with NaN, +-inf and |flow| > 1e9: the forward skips them, both gradients are exactly 0 there, and their
    neighbours (which would have merged with them) are compared like every other pixel.  Every load and store of such a pixel is
    behind its validity flags in both kernels (forward: `any`; backward: `skip` clears the four flags)."""
    b, c, h, w = shape
    flow = make_flow(kind, b, h, w, 11, dev)
    if bad:
        flow = plant_bad(flow)
    g = cpu_gen(12)
    inp = (torch.rand(b, c, h, w, generator=g) - 0.3).to(dev)
    gout = torch.randn(b, c, h, w, generator=g).to(dev)
    plan = splat_plan(flow)
    assert_flow_kind(kind, plan)
    assert plan['skipped'] == (len(BAD_PIXELS) if bad else 0)
    if shape[2:] == BIG[1:]:
        assert plan['tiles'] == 4096 and plan['tiles_x'] > 1 and plan['tiles_y'] > 1
    else:
        assert plan['partial_x'] and plan['partial_y'] and c % SP_CC != 0 and c > SP_CC, 'partial tiles and a short second channel pass'
    T = taps64(flow)
    excl = T['near'][:, None]
    share = float(T['near'].double().mean())
    print(f'excluded from gflow (coordinate within 1e-4 of an integer): {100 * share:.4f} %')
    assert share < 0.002

    ref, budget = splat_ref(inp, T)
    gin_r, gin_b, gfl_r, gfl_b = splat_bwd_ref(inp, gout, T)
    fs = FL()._FunctionSoftsplat
    x, f = inp.clone().requires_grad_(True), flow.clone().requires_grad_(True)
    out = fs.apply(x, f)
    gin, gflow = torch.autograd.grad(out, [x, f], gout)
    torch.cuda.synchronize()
    worst = [ratio('splat out', out, ref, budget), ratio('splat gin', gin, gin_r, gin_b),
             ratio('splat gflow', gflow, gfl_r, gfl_b, exempt=excl)]
    # null-pointer variants of the backward launch
    x1 = inp.clone().requires_grad_(True)
    gin1, = torch.autograd.grad(fs.apply(x1, flow), [x1], gout)
    f1 = flow.clone().requires_grad_(True)
    gflow1, = torch.autograd.grad(fs.apply(inp, f1), [f1], gout)
    assert torch.equal(gin1, gin) and torch.equal(torch.nan_to_num(gflow1), torch.nan_to_num(gflow)), 'gin-only / gflow-only differ'
    if bad:
        for (bb, _, y, x_), _ in zip(BAD_PIXELS, BAD_VALUES):
            assert bool((gin[bb, :, y, x_] == 0).all()) and bool((gflow[bb, :, y, x_] == 0).all()), (bb, y, x_)
    assert max(worst) <= 1, worst


@pytest.mark.parametrize('kind', ['smooth2', 'smooth9', 'randn3'])
@pytest.mark.parametrize('mode', ['softmax', 'average', 'linear'])
def test_normalised_splat(dev, kind, mode):
    """softmax / average / linear splat at 4 x 3 x 512 x 512 (payload 4 channels == SP_CC, the bench shape) and 3 x 5 x 203 x 317
    (6 channels: a full and a short LDS pass).  The payload (input * weight, weight) is formed by torch; the kernel's raw output is
    compared channel by channel, the norm channel included.  The quotient num / norm is compared where the reference norm exceeds twice
    its own budget, with |d| <= (B_num + |out| B_norm) / (norm - B_norm) + U |out| (the division's amplification is in the budget).
    Where the reference norm is below that, out jumps between num / norm and 0 (norm == 0 -> divide by 1) under a perturbation of the
    size of the budget, so those elements are only required to be finite; their share is capped at 0.01 %.  The kernel's `norm == 0`
    must equal the reference's outside that set, and out must be exactly 0 wherever the kernel's norm is 0."""
    for b, c, h, w in ((4, 3, 512, 512), (3, 5, 203, 317)):
        flow = make_flow(kind, b, h, w, 21, dev)
        g = cpu_gen(22)
        inp = torch.rand(b, c, h, w, generator=g).to(dev)
        metric = (torch.randn(b, 1, h, w, generator=g) * (0.5 if mode == 'softmax' else 1.0)).to(dev)
        if mode == 'linear':
            metric = metric.abs() + 0.05
        assert_flow_kind(kind, splat_plan(flow))
        payload = {'average': lambda: torch.cat([inp, torch.ones_like(metric)], 1),
                   'linear': lambda: torch.cat([inp * metric, metric], 1),
                   'softmax': lambda: torch.cat([inp * metric.exp(), metric.exp()], 1)}[mode]().contiguous()
        T = taps64(flow)
        ref, budget = splat_ref(payload, T)
        raw = FL()._FunctionSoftsplat.apply(payload, flow)
        out = FL().FunctionSoftsplat(inp, flow, None if mode == 'average' else metric, mode)
        torch.cuda.synchronize()
        norm, nb = ref[:, -1:], budget[:, -1:]
        zero_r = norm == 0
        tiny = (norm <= 2 * nb) & ~zero_r
        share = float(tiny.double().mean())
        print(f'{mode} {kind} {h}x{w}: norm == 0 at {100 * float(zero_r.double().mean()):.3f} %, tiny non-zero norm at {100 * share:.5f} %')
        assert share < 1e-4
        assert bool(((raw[:, -1:] == 0) == zero_r)[~tiny].all()), 'norm == 0 differs from the reference'
        assert bool((out[(raw[:, -1:] == 0).expand_as(out)] == 0).all())
        assert bool(torch.isfinite(out).all())
        q = ref[:, :-1] / torch.where(zero_r, torch.ones_like(norm), norm)
        qb = (budget[:, :-1] + q.abs() * nb) / (norm - nb).clamp_min(1e-300) + U * q.abs()
        qb = torch.where(zero_r, budget[:, :-1], qb)
        worst = [ratio(f'{mode} raw', raw, ref, budget), ratio(f'{mode} out', out, q, qb, exempt=tiny)]
        assert max(worst) <= 1, worst


@pytest.mark.parametrize('kind,shape,bad', [('smooth2', (4, 512, 512), False), ('smooth9', (4, 512, 512), False),
                                            ('randn3', (4, 512, 512), False), ('smooth9', (3, 203, 317), False),
                                            ('smooth2', (3, 203, 317), True)],
                         ids=['smooth2-512', 'smooth9-512', 'randn3-512', 'smooth9-203x317', 'smooth2-203x317-nonfinite'])
def test_occlusion_wang_map_and_mask(dev, kind, shape, bad):
    """the range map (splat of a constant 1) element-wise, and the mask: it must equal `map_f64 > thresh` except where
    |map_f64 - thresh| is inside the map's own budget (cap 0.01 % of the pixels).  The mask has no end-to-end float64 bound beyond that:
    it is a threshold of an fp32 sum.  (occlusion_wang has no gradient in this project: the trainer detaches it.)"""
    b, h, w = shape
    flow = make_flow(kind, b, h, w, 31, dev)
    if bad:
        flow = plant_bad(flow)
    plan = splat_plan(flow)
    assert_flow_kind(kind, plan)
    assert plan['tiles'] == (4096 if shape == BIG else b * 26 * 10)
    T = taps64(flow)
    ref, budget = splat_ref(torch.ones(b, 1, h, w, device=dev), T)
    corr = FL().get_corresponding_map(flow)
    thresh = 0.7
    mask = FL().occlusion_wang(None, flow, thresh)
    torch.cuda.synchronize()
    unsure = (ref - thresh).abs() <= budget
    share = float(unsure.double().mean())
    print(f'wang mask undecided at {100 * share:.5f} % of the pixels')
    assert share < 1e-4
    assert bool(((mask == 1) == (ref > thresh))[~unsure].all()), 'mask differs from map_f64 > thresh outside the budget'
    assert bool(((mask == 0) | (mask == 1)).all())
    assert ratio('wang map', corr, ref, budget) <= 1


def test_occlusion_brox_pre_threshold(dev):
    """occlusion_brox on its pre-threshold quantity q = |fw + w|^2 - (0.01 (|fw|^2 + |w|^2) + 0.5), w = the warp kernel's own output
    (tests/test_gpu_elementwise_sizes.py bounds the warp).  fp32 roundings: each of the two sums of squares has a sum (1), a square
    (1) per component and additions (2): 4 U sq_sum + (4 + 1) U 0.01 sum_sq + U 0.5, rounded up to 6 U (sq_sum + 0.01 sum_sq + 0.5).
    The mask must equal q >= 0 wherever |q| exceeds that; cap 0.01 %."""
    from sin_inn_amd.functional import flow_warp_l1
    for b, h, w in (BIG, (3, 203, 317)):
        fw = make_flow('smooth9', b, h, w, 41, dev)
        bw = (-fw + 0.6 * torch.randn(b, 2, h, w, generator=cpu_gen(42)).to(dev)).contiguous()
        assert b * h * w > 256, 'more than one block'
        mask = FL().occlusion_brox(fw, bw, None)
        wbw = flow_warp_l1(bw, fw)[0].to(F64)
        f = fw.to(F64)
        sq_sum, sum_sq = ((f + wbw) ** 2).sum(1, keepdim=True), (f ** 2 + wbw ** 2).sum(1, keepdim=True)
        q = sq_sum - (0.01 * sum_sq + 0.5)
        budget = 6 * U * (sq_sum + 0.01 * sum_sq + 0.5)
        unsure = q.abs() <= budget
        share, ones = float(unsure.double().mean()), float((q >= 0).double().mean())
        print(f'brox {h}x{w}: mask true at {100 * ones:.1f} %, undecided at {100 * share:.5f} %')
        assert 0.1 < ones < 0.9, 'both outcomes must be common'
        assert share < 1e-4
        assert mask.dtype == torch.bool and bool((mask == (q >= 0))[~unsure].all())


# =================================================================================================================================
# B. reductions: census, masked L1, SSIM, bilateral smoothness
# =================================================================================================================================
def slot_depth(blocks, per_thread, threads=256):
    """roundings on the longest path of one of the two sums: the thread's own additions, the wave sum (6), the waves of the block, the
    atomics that land in one of the 64 slots, the 64-lane finish (6)"""
    return per_thread + 6 + threads // 64 + -(-blocks // SLOTS) + 6


def census_d(im1, im2, mask, md):
    """per-pixel census distance times the inner-region mask, [B,H,W], in the dtype of the inputs (loss.py:30-72)"""
    b, _, h, w = im1.shape

    def grey(im):
        x = im * mask
        return (x[:, 0] * 0.2989 + x[:, 1] * 0.5870 + x[:, 2] * 0.1140) * 255

    g1, g2 = grey(im1), grey(im2)
    p1, p2 = F.pad(g1, (md, md, md, md)), F.pad(g2, (md, md, md, md))
    n = 2 * md + 1
    tot = torch.zeros_like(g1)
    for oy in range(n):
        for ox in range(n):
            a, c = p1[:, oy:oy + h, ox:ox + w] - g1, p2[:, oy:oy + h, ox:ox + w] - g2
            q = (a / torch.sqrt(0.81 + a * a) - c / torch.sqrt(0.81 + c * c)) ** 2
            tot = tot + q / (0.1 + q)
    valid = torch.zeros_like(g1)
    valid[:, md:h - md, md:w - md] = 1
    return tot / (n * n) * valid


def ssim_d(x, y, mask, md):
    """per-window clamp((1 - SSIM) / 2, 0, 1), [B,C,H-2md,W-2md] (loss.py:75-103)"""
    x, y = x * mask, y * mask

    def pool(t):
        return F.avg_pool2d(t, 2 * md + 1, 1, 0)

    c1, c2 = 0.01 ** 2, 0.03 ** 2
    mx, my = pool(x), pool(y)
    sx, sy, sxy = pool(x * x) - mx ** 2, pool(y * y) - my ** 2, pool(x * y) - mx * my
    s = (2 * mx * my + c1) * (2 * sxy + c2) / ((mx ** 2 + my ** 2 + c1) * (sx + sy + c2))
    return torch.clamp((1 - s) / 2, 0, 1)


def measured_sum_and_grads(fn, im1, im2, mask, coef64):
    """fn(im1, im2, mask) -> per-element distances.  Returns the float64 sum and gradients of coef64 * sum, and the UNITS measured on the
    reference itself: the same formula in fp32 torch against float64 -- for the sum the sum of the per-element deviations, for each
    gradient the worst per-element deviation."""
    a64, b64 = im1.to(F64).requires_grad_(True), im2.to(F64).requires_grad_(True)
    d64 = fn(a64, b64, mask.to(F64))
    g64 = torch.autograd.grad(d64.sum() * coef64, [a64, b64])
    a32, b32 = im1.clone().requires_grad_(True), im2.clone().requires_grad_(True)
    d32 = fn(a32, b32, mask)
    g32 = torch.autograd.grad(d32.sum() * float(coef64), [a32, b32])
    unit_sum = float((d32.detach().to(F64) - d64.detach()).abs().sum())
    unit_g = [float((p.to(F64) - q).abs().max()) for p, q in zip(g32, g64)]
    return d64.detach(), g64, unit_sum, unit_g


def check_window_loss(name, dev, entry, fn, shape, mc, md, weight, gscale, blocks_fwd, win_scale):
    """common body of the census and SSIM cases.  `entry` = C entry point name, fn = float64 / fp32 reference of the per-element
    distance, win_scale = (number the finish kernel multiplies acc[0] / acc[1] with) / weight."""
    b, c, h, w = shape
    im1, im2 = make_images(b, c, h, w, 51, dev)
    mask = make_mask(b, mc, h, w, 52, dev)
    acc, out = torch.zeros(ACC_FLOATS, device=dev), torch.empty(1, device=dev)
    extra = (b, c, h, w) if entry == 'sininn_ssim' else (b, h, w)
    call(entry, P(im1), P(im2), P(mask), mc, *extra, md, weight, P(acc), P(out))
    msum = mask.to(F64).sum()
    assert float(msum) < 2 ** 24 and float(acc[1]) == float(msum), f'sum(mask): kernel {float(acc[1])}, exact {float(msum)}'
    assert float(acc[3::2].to(F64).sum()) == float(msum), 'the slots of sum(mask) add up to it'
    if blocks_fwd >= SLOTS:
        assert bool((acc[3::2] > 0).all()), 'every slot holds part of sum(mask)'
    gs = torch.tensor([gscale], device=dev)
    coef64 = float(gs.to(F64)) * weight * win_scale / float(acc[1])
    d64, g64, unit_sum, unit_g = measured_sum_and_grads(lambda p, q, m: fn(p, q, m, md), im1, im2, mask, coef64)
    sum_budget = MULT * unit_sum + slot_depth(blocks_fwd, 0) * U * float(d64.sum())
    print(f'{name}: unit(sum) {unit_sum:.3g} over sum {float(d64.sum()):.6g}; unit(g1) {unit_g[0]:.3g}, unit(g2) {unit_g[1]:.3g}, '
          f'max |g| {float(g64[0].abs().max()):.3g}')
    worst = [ratio(f'{name} sum', acc[0], d64.sum(), sum_budget)]
    # the scalar, from the kernel's own sums: scale (2 roundings on the host), product, quotient
    worst.append(ratio(f'{name} out', out[0], weight * win_scale * acc[0].to(F64) / acc[1].to(F64), 5 * U * out[0].to(F64).abs()))
    g1, g2 = torch.empty_like(im1), torch.empty_like(im2)
    call(entry + '_bwd', P(im1), P(im2), P(mask), mc, *extra, md, weight, P(acc), P(gs), P(g1), P(g2))
    worst += [ratio(f'{name} g1', g1, g64[0], MULT * unit_g[0]), ratio(f'{name} g2', g2, g64[1], MULT * unit_g[1])]
    # g1-only / g2-only launches write the same values
    o1, o2 = torch.empty_like(im1), torch.empty_like(im2)
    call(entry + '_bwd', P(im1), P(im2), P(mask), mc, *extra, md, weight, P(acc), P(gs), P(o1), None)
    call(entry + '_bwd', P(im1), P(im2), P(mask), mc, *extra, md, weight, P(acc), P(gs), None, P(o2))
    assert torch.equal(o1, g1) and torch.equal(o2, g2)
    assert bool((g1[(mask == 0).expand_as(g1)] == 0).all()) and bool((g2[(mask == 0).expand_as(g2)] == 0).all())
    return worst


CENSUS_CASES = [((4, 3, 512, 512), 1, 3), ((4, 3, 512, 512), 3, 2), ((3, 3, 203, 317), 3, 1), ((3, 3, 203, 317), 1, 4),
                ((3, 3, 203, 317), 1, 3), ((2, 3, 9, 45), 1, 1), ((2, 3, 9, 45), 3, 2), ((2, 3, 9, 45), 1, 3), ((2, 3, 9, 45), 3, 4),
                ((2, 3, 45, 11), 1, 4), ((2, 3, 45, 11), 3, 2)]


@pytest.mark.parametrize('shape,mc,md', CENSUS_CASES, ids=[f'{"x".join(map(str, s))}-mc{mc}-md{md}' for s, mc, md in CENSUS_CASES])
def test_census(dev, shape, mc, md):
    """census loss: sum of distances, exact sum(mask), the scalar, g1 / g2 with a non-unit gscale.  9 x 45 and 45 x 11: one tile row /
    column in which every pixel is border for md 4 but one line (H - 2 md = 1) and the `inner` test decides everything."""
    b, _, h, w = shape
    tiles = b * -(-h // CT) * -(-w // CT)
    if shape[2:] == BIG[1:]:
        assert tiles == 4096 and tiles // SLOTS == 64
    else:
        assert h % CT and w % CT and (min(h, w) > 16 or 2 * md < min(h, w) <= 16)
    worst = check_window_loss(f'census md{md}', dev, 'sininn_census', census_d, shape, mc, md, 0.7, 1.75, tiles, float(mc))
    assert max(worst) <= 1, worst


SSIM_CASES = [((4, 3, 512, 512), 1, 1), ((4, 3, 512, 512), 3, 2), ((3, 3, 203, 317), 3, 1), ((3, 3, 203, 317), 1, 2),
              ((2, 3, 7, 45), 1, 1), ((2, 3, 7, 45), 3, 2), ((2, 3, 45, 16), 3, 1), ((2, 3, 45, 16), 1, 2), ((2, 2, 18, 35), 2, 1)]


@pytest.mark.parametrize('shape,mc,md', SSIM_CASES, ids=[f'{"x".join(map(str, s))}-mc{mc}-md{md}' for s, mc, md in SSIM_CASES])
def test_ssim(dev, shape, mc, md):
    """SSIM loss.  Forward tiles cover the (H - 2 md) x (W - 2 md) windows; the last tile row / column also sums the mask over the 2 md
    border pixels.  7 x 45 and 45 x 16: a single tile in one direction that is mostly border; 18 x 35 with md 1: H - 2 md == 16, so
    the only tile row is full AND takes the border."""
    b, c, h, w = shape
    ho, wo = h - 2 * md, w - 2 * md
    tiles_f = b * c * -(-ho // CT) * -(-wo // CT)
    if shape[2:] == BIG[1:]:
        assert tiles_f == 12288 and tiles_f // SLOTS == 192
    else:
        assert (ho % CT or wo % CT) and (min(h, w) > 16 or 2 * md < min(h, w) <= 16)
    win_scale = (b * mc * h * w) / (b * c * ho * wo)
    worst = check_window_loss(f'ssim md{md}', dev, 'sininn_ssim', ssim_d, shape, mc, md, 0.9, 0.6, tiles_f, win_scale)
    assert max(worst) <= 1, worst


L1_CASES = [((4, 3, 512, 512), 1), ((4, 3, 512, 512), 3), ((3, 5, 203, 317), 1), ((3, 5, 203, 317), 5)]


@pytest.mark.parametrize('shape,mc', L1_CASES, ids=[f'{"x".join(map(str, s))}-mc{mc}' for s, mc in L1_CASES])
def test_masked_l1(dev, shape, mc):
    """masked L1.  Forward terms |a m - b m|: with a 0 / 1 mask the products are exact, the difference is one rounding; the thread adds
    C terms per trip, then the slot path: budget (1 + depth) U sum|terms|.  Backward: sign(a m - b m) m coef is exact up to coef =
    gscale * (weight MC / C) / sum(mask): 2 roundings on the host, product, quotient, product with m: 5 U |g|.  The sign is exact (the
    float64 difference of exact products has the sign of the fp32 one), so pixels with a == b and pixels with mask 0 must give exactly 0
    (torch's sign(0))."""
    b, c, h, w = shape
    im1, im2 = make_images(b, c, h, w, 61, dev)
    mask = make_mask(b, mc, h, w, 62, dev)
    same = torch.rand(b, c, h, w, generator=cpu_gen(63)).to(dev) < 0.01
    im2 = torch.where(same, im1, im2).contiguous()
    same = im1 == im2                                  # the clamp of the warped image makes a few more
    total = b * h * w
    blocks = min(-(-total // 256), 1024)
    trips = -(-total // (blocks * 256))
    blocks_b = min(-(-total * c // 256), 8192)
    trips_b = -(-total * c // (blocks_b * 256))
    print(f'masked_l1 plan: fwd {blocks} blocks x {trips} trips, bwd {blocks_b} blocks x {trips_b} trips')
    if shape[2:] == BIG[1:]:
        assert blocks == 1024 and trips == 4 and blocks // SLOTS == 16 and blocks_b == 8192 and trips_b == 2
    else:
        assert total % 256 != 0, 'a partial last block'
    weight, gscale = 0.8, 1.3
    acc, out = torch.zeros(ACC_FLOATS, device=dev), torch.empty(1, device=dev)
    call('sininn_masked_l1', P(im1), P(im2), P(mask), mc, b, c, h, w, weight, P(acc), P(out))
    m64 = mask.to(F64)
    msum = m64.sum()
    assert float(acc[1]) == float(msum), f'sum(mask): kernel {float(acc[1])}, exact {float(msum)}'
    diff = im1.to(F64) * m64 - im2.to(F64) * m64
    s = diff.abs().sum()
    worst = [ratio('l1 sum', acc[0], s, (1 + slot_depth(blocks, trips * c)) * U * s)]
    worst.append(ratio('l1 out', out[0], weight * mc / c * acc[0].to(F64) / acc[1].to(F64), 5 * U * out[0].to(F64).abs()))
    gs = torch.tensor([gscale], device=dev)
    g1, g2 = torch.empty_like(im1), torch.empty_like(im2)
    call('sininn_masked_l1_bwd', P(im1), P(im2), P(mask), mc, b, c, h, w, weight, P(acc), P(gs), P(g1), P(g2))
    gref = torch.sign(diff) * m64 * (float(gs.to(F64)) * weight * mc / c / float(acc[1]))
    worst += [ratio('l1 g1', g1, gref, 5 * U * gref.abs()), ratio('l1 g2', g2, -gref, 5 * U * gref.abs())]
    zero = same | (mask == 0).expand_as(same)
    assert float(same.double().mean()) > 0.005 and float(zero.double().mean()) > 0.2
    assert bool((g1[zero] == 0).all()) and bool((g2[zero] == 0).all()) and bool((g1[~zero] != 0).all())
    o1, o2 = torch.empty_like(im1), torch.empty_like(im2)
    call('sininn_masked_l1_bwd', P(im1), P(im2), P(mask), mc, b, c, h, w, weight, P(acc), P(gs), P(o1), None)
    call('sininn_masked_l1_bwd', P(im1), P(im2), P(mask), mc, b, c, h, w, weight, P(acc), P(gs), None, P(o2))
    assert torch.equal(o1, g1) and torch.equal(o2, g2)
    assert max(worst) <= 1, worst


def smooth_terms(img, flow, abs_fun, k, order):
    """float64 pieces of BilateralSmooth per anchor and direction (0: along H, 1: along W): weight w, its exponent m, the flow
    differences u [B,2,..] and the magnitudes that bound their fp32 rounding (loss.py:106-132)"""
    out = []
    for d in (2, 3):
        n = img.shape[d]

        def sl(t, a, e):
            return t.narrow(d, a, e - a)

        di = k * (sl(img, order, n) - sl(img, 0, n - order))
        m = (di.abs() if abs_fun == 'exp' else di ** 2).mean(1, keepdim=True)
        if order == 1:
            u = sl(flow, 1, n) - sl(flow, 0, n - 1)
            mag = u.abs()                                                   # one difference: U |u|
        else:
            d1, d0 = sl(flow, 2, n) - sl(flow, 1, n - 1), sl(flow, 1, n - 1) - sl(flow, 0, n - 2)
            u = d1 - d0
            mag = d1.abs() + d0.abs() + u.abs()                             # three differences
        out.append(dict(w=torch.exp(-m), m=m, u=u, du=U * mag.detach()))
    return out


SMOOTH_CASES = [(BIG, 'exp', 1), (BIG, 'gauss', 2), ((3, 203, 317), 'exp', 2), ((3, 203, 317), 'gauss', 1), ((9, 512, 512), 'exp', 2)]


@pytest.mark.parametrize('shape,abs_fun,order', SMOOTH_CASES, ids=[f'{"x".join(map(str, s))}-{f}-o{o}' for s, f, o in SMOOTH_CASES])
def test_bilateral_smooth(dev, shape, abs_fun, order):
    """edge-aware smoothness, C = 3, on a smooth flow plus a little noise (so that u spans both sides of the 1e-3 knee of robust()).
    Per anchor term T = w (t_0 + t_1), t = sqrt(u^2 + 1e-6):
      du  = fp32 rounding of the flow differences (smooth_terms);       dt <= du + 2 U t   (|dt/du| <= 1; square, sum, sqrt)
      m   = mean_c f(k dimg): difference, product, f, C additions, the division: (C + 4) U m;   dw = w (dm + 3 U)   (expf: 2 ulp)
      dT  = w (dt_0 + dt_1) + dw (t_0 + t_1) + 2 U T;        the sum adds depth * U * sum T (one term per trip, then the slot path).
    The scalar out = a ch + m cw from the kernel's own sums: ch, cw are 4 host roundings, two products and a sum: 8 U (|a ch| + |m cw|).
    Gradient, per pixel a sum of 2 (order + 1) terms coef w rho tap, rho = u / sqrt(u^2 + 1e-6), |d rho / du| = 1e-6 / (u^2 + 1e-6)^1.5:
      d term = |coef tap| (w (du |d rho/du| + 3 U |rho|) + dw |rho|) + 7 U |term|   (coef: gscale * ch, ch 4 host roundings; products),
      plus 2 (order + 1) U sum|terms| for the additions.  9 x 512 x 512 exists because smooth_bwd (8192 blocks) takes its second trip
      only above 2 M pixels."""
    b, h, w = shape
    c, k, weight, gscale = 3, 50.0 if abs_fun == 'gauss' else 10.0, 1.1, 0.7
    img, _ = make_images(b, c, h, w, 71, dev)
    # a smoother guide image: weights w spread over (0, 1) instead of underflowing
    img = F.avg_pool2d(img, 9, 1, 4).contiguous() if abs_fun == 'gauss' else (0.1 * img + 0.5).contiguous()
    flow = (make_flow('smooth2', b, h, w, 72, dev) + 2e-3 * torch.randn(b, 2, h, w, generator=cpu_gen(73)).to(dev)).contiguous()
    total = b * h * w
    blocks, blocks_b = min(-(-total // 256), 1024), min(-(-total // 256), 8192)
    trips, trips_b = -(-total // (blocks * 256)), -(-total // (blocks_b * 256))
    print(f'smooth plan: fwd {blocks} blocks x {trips} trips, bwd {blocks_b} blocks x {trips_b} trips')
    if shape == BIG:
        assert blocks == 1024 and trips == 4 and blocks // SLOTS == 16
    elif b == 9:
        assert blocks_b == 8192 and trips_b == 2 and trips == 9
    else:
        assert total % 256 != 0
    acc, out = torch.zeros(ACC_FLOATS, device=dev), torch.empty(1, device=dev)
    call('sininn_bilateral_smooth', P(img), P(flow), b, c, h, w, order, int(abs_fun == 'gauss'), k, weight, P(acc), P(out))
    f64 = flow.to(F64).requires_grad_(True)
    terms = smooth_terms(img.to(F64), f64, abs_fun, k, order)
    ch = 0.5 * weight / (b * 2.0 * (h - order) * w)
    cw = 0.5 * weight / (b * 2.0 * h * (w - order))
    worst, sums = [], []
    for i, t in enumerate(terms):
        rob = torch.sqrt(t['u'] ** 2 + 1e-6)
        T = (t['w'] * rob).sum(1)
        s = T.sum()
        sums.append(s)
        rob, T = rob.detach(), T.detach()
        dt = (t['du'] + 2 * U * rob).sum(1)
        dw = t['w'] * ((c + 4) * U * t['m'] + 3 * U)
        dT = t['w'][:, 0] * dt + dw[:, 0] * rob.sum(1) + 2 * U * T
        worst.append(ratio(f'smooth sum[{i}]', acc[i], s.detach(), float(dT.sum() + slot_depth(blocks, trips) * U * s.detach())))
        print(f'   weights of direction {i}: mean {float(t["w"].mean()):.3g}, min {float(t["w"].min()):.3g}; '
              f'|u| < 1e-3 at {100 * float((t["u"].abs() < 1e-3).double().mean()):.1f} %')
        assert float(t['w'].mean()) > 0.05
    a, m = acc[0].to(F64), acc[1].to(F64)
    worst.append(ratio('smooth out', out[0], a * ch + m * cw, 8 * U * (a * ch + m * cw)))
    gs = torch.tensor([gscale], device=dev)
    gflow = torch.empty_like(flow)
    call('sininn_bilateral_smooth_bwd', P(img), P(flow), b, c, h, w, order, int(abs_fun == 'gauss'), k, weight, P(gs), P(gflow))
    g = float(gs.to(F64))
    gref, = torch.autograd.grad(g * (sums[0] * ch + sums[1] * cw), [f64])
    # the budget, scattered to the pixels with the same stencil: every |term| and d term of an anchor lands on its order + 1 points
    budget = torch.zeros(b, 2, h, w, dtype=F64, device=dev)
    for (d, coef), t in zip(((2, g * ch), (3, g * cw)), terms):
        u, wgt = t['u'].detach(), t['w']
        rho, drho = u / torch.sqrt(u ** 2 + 1e-6), 1e-6 / (u ** 2 + 1e-6) ** 1.5
        dw = wgt * ((c + 4) * U * t['m'] + 3 * U)
        term = abs(coef) * wgt * rho.abs()
        dterm = abs(coef) * (wgt * (t['du'] * drho + 3 * U * rho.abs()) + dw * rho.abs()) + 7 * U * term
        per_anchor = dterm + 2 * (order + 1) * U * term
        n = budget.shape[d]
        for j, tap in enumerate((1, 1) if order == 1 else (1, 2, 1)):
            budget.narrow(d, j, n - order).add_(tap * per_anchor)
    worst.append(ratio('smooth gflow', gflow, gref, budget))
    assert max(worst) <= 1, worst


# =================================================================================================================================
# C. the module entry points (autograd wrappers, scalar placeholder mask) and the references themselves
# =================================================================================================================================
def test_loss_modules_with_placeholder_mask(dev):
    """CensusLoss / L1Loss / SSIMLoss through their autograd wrappers with the trainer's scalar placeholder mask `torch.ones(2)[i]`,
    at 3 x 3 x 203 x 317: value and both gradients against float64 with an all-ones mask; budgets as in the operator tests (census,
    SSIM: MULT measured units, plus 40 U of the value for the slot path and the scalar; L1: derived)."""
    b, c, h, w = 3, 3, 203, 317
    im1, im2 = make_images(b, c, h, w, 81, dev)
    ones = torch.ones(b, 1, h, w, device=dev)
    place = torch.ones(2, device=dev)[1]
    worst = []
    for name, module, fn, scale in (('census', FL().CensusLoss(0.7, 3), lambda p, q, m: census_d(p, q, m, 3), 1.0 / (b * h * w)),
                                    ('ssim', FL().SSIMLoss(0.7, 2), lambda p, q, m: ssim_d(p, q, m, 2),
                                     1.0 / (b * c * (h - 4) * (w - 4)))):
        a, bb = im1.clone().requires_grad_(True), im2.clone().requires_grad_(True)
        loss = module(a, bb, place)
        g1, g2 = torch.autograd.grad(loss * 1.5, [a, bb])
        d64, g64, unit_sum, unit_g = measured_sum_and_grads(fn, im1, im2, ones, 1.5 * 0.7 * scale)
        ref = 0.7 * scale * d64.sum()
        worst += [ratio(f'{name} module loss', loss, ref, 0.7 * scale * MULT * unit_sum + 40 * U * ref),
                  ratio(f'{name} module g1', g1, g64[0], MULT * unit_g[0]), ratio(f'{name} module g2', g2, g64[1], MULT * unit_g[1])]
    a, bb = im1.clone().requires_grad_(True), im2.clone().requires_grad_(True)
    loss = FL().L1Loss(0.8)(a, bb, place)
    g1, g2 = torch.autograd.grad(loss * 1.5, [a, bb])
    diff = im1.to(F64) - im2.to(F64)
    ref = 0.8 * diff.abs().mean()
    total = b * h * w
    blocks = min(-(-total // 256), 1024)
    gref = 1.5 * 0.8 * torch.sign(diff) / diff.numel()
    worst += [ratio('l1 module loss', loss, ref, (6 + slot_depth(blocks, -(-total // (blocks * 256)) * c)) * U * ref),
              ratio('l1 module g1', g1, gref, 6 * U * gref.abs()), ratio('l1 module g2', g2, -gref, 6 * U * gref.abs())]
    assert max(worst) <= 1, worst


def test_references_are_the_oracle():
    """the float64 restatements of this file against oracle/flow_oracle.py in float64 on the CPU, value and autograd gradients, at a
    ragged shape: 1e-12 relative (both are float64; only the order of the additions differs)."""
    from oracle import flow_oracle as O
    cpu = torch.device('cpu')
    b, c, h, w = 2, 3, 37, 53

    def close(p, q, what):
        return float((p - q).abs().max()) <= 1e-12 * max(1.0, float(q.abs().max())), what

    checks = []
    for kind in ('smooth9', 'randn3'):
        flow = make_flow(kind, b, h, w, 91, cpu)
        g = cpu_gen(92)
        inp, gout = torch.rand(b, c, h, w, generator=g) - 0.3, torch.randn(b, c, h, w, generator=g)
        T = taps64(flow)
        ref, _ = splat_ref(inp, T)
        gin_r, _, gfl_r, _ = splat_bwd_ref(inp, gout, T)
        x, f = inp.to(F64).requires_grad_(True), flow.to(F64).requires_grad_(True)
        out = O.function_softsplat(x, f, None, 'summation')
        gin, gfl = torch.autograd.grad(out, [x, f], gout.to(F64))
        near = T['near'][:, None].expand_as(gfl)
        checks += [close(ref, out.detach(), 'splat'), close(gin_r, gin, 'gin'), close(gfl_r[~near], gfl[~near], 'gflow')]
        one, _ = splat_ref(torch.ones(b, 1, h, w), T)
        ys, xs = torch.meshgrid(torch.arange(h, dtype=F64), torch.arange(w, dtype=F64), indexing='ij')
        checks.append(close(one, O.get_corresponding_map(torch.stack([xs, ys])[None] + flow.to(F64)), 'range map'))
    im1, im2 = make_images(b, c, h, w, 93, cpu)
    for mc in (1, 3):
        mask = make_mask(b, mc, h, w, 94, cpu).to(F64)
        for name, mine, theirs in (
                ('census', lambda p, q: census_d(p, q, mask, 2).sum() / (b * h * w) / mask.sum() * mask.numel() * 0.7,
                 lambda p, q: O.census_loss(p, q, mask, 0.7, 2)),
                ('ssim', lambda p, q: ssim_d(p, q, mask, 1).mean() / mask.sum() * mask.numel() * 0.7,
                 lambda p, q: O.ssim_loss(p, q, mask, 0.7, 1))):
            res = []
            for fn in (mine, theirs):
                p, q = im1.to(F64).requires_grad_(True), im2.to(F64).requires_grad_(True)
                v = fn(p, q)
                res.append((v.detach(),) + torch.autograd.grad(v, [p, q]))
            checks += [close(m, t, f'{name} mc{mc} [{i}]') for i, (m, t) in enumerate(zip(*res))]
    flow = make_flow('smooth2', b, h, w, 95, cpu).to(F64)
    for abs_fun, k, order in (('exp', 10.0, 1), ('gauss', 3.0, 2)):
        f = flow.clone().requires_grad_(True)
        terms = smooth_terms(im1.to(F64), f, abs_fun, k, order)
        mine = 0.5 * 1.1 * sum((t['w'] * torch.sqrt(t['u'] ** 2 + 1e-6)).mean() for t in terms)
        f2 = flow.clone().requires_grad_(True)
        theirs = O.bilateral_smooth(im1.to(F64), f2, 1.1, abs_fun, k, order)
        checks += [close(mine.detach(), theirs.detach(), 'smooth'),
                   close(torch.autograd.grad(mine, [f])[0], torch.autograd.grad(theirs, [f2])[0], 'smooth gflow')]
    bad = [what for ok, what in checks if not ok]
    assert not bad, bad
