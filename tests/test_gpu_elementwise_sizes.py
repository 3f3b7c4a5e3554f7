"""GPU: the loss, warp and optimiser kernels of csrc/elementwise.hip at production sizes, against float64.

The stand-alone tests of these kernels (tests/test_gpu_kernels.py, tests/test_gpu_flow.py) run shapes where ONE block does all the
work and compare with an fp32 reference at 1e-3 .. 1e-4 of the max-norm.  Here they run at the sizes of BASELINE configs[1]
(batch 16, 256x256) and configs[3] (batch 16, 512x512), where grid-stride loops take several trips, partial sums land in several
slots / blocks, the tiled flow-warp backward leaves its LDS window and Adam's float4 body is followed by a scalar tail.

Method (that of tests/test_gpu_bf16_tiles.py):
  * the reference is plain float64 torch of the same operation, evaluated on the GPU in float64; it never calls the kernel under
    test.  A later stage is compared with float64 applied to what the EARLIER KERNEL wrote (MMD: Grams -> coefficients ->
    gradients; flow warp: the L1 sign is taken from the staged `warped`), so no stage hides behind the conditioning of another;
  * every budget is derived per element next to the reference, with U = 2^-24 (fp32 unit roundoff):
      - a sum: depth * U * sum|terms|, depth = roundings on the longest path through the kernel's own summation tree;
      - a value that depends on an fp32 coordinate or distance with rounding error delta: |d value / d coordinate| * delta,
        both evaluated in float64 (the warps: a pixel coordinate of magnitude W carries ~6 U W; MMD: the distance
        r_i + r_j - 2 g_ij carries 2 U (|r_i| + |r_j| + 2 |g_ij|));
      - element-wise results: (number of roundings) * U relative;
    each test prints its worst error / budget ratio (`ratio(...)` lines, run with -s) and asserts it is <= 1;
  * every case recomputes the launch plan from the kernel's formulas and asserts the property it exists for."""
import os
import re
import sys

import numpy as np
import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, 'tests'))

U = 2.0 ** -24
F64 = torch.float64
BF = torch.bfloat16


@pytest.fixture(scope='module')
def dev():
    import sin_inn_amd  # noqa: F401
    assert torch.cuda.is_available(), 'GPU tests need a GPU'
    return torch.device('cuda', 0)


def gen(seed):
    return torch.Generator(device='cuda').manual_seed(seed)


def ratio(name, got, ref, budget, exempt=None):
    """worst |got - ref| / budget over the tensor; prints it; NaN / inf in `got` count as infinite"""
    got, ref = got.detach().to(F64), ref.detach().to(F64)
    err = (got - ref).abs()
    err = torch.where(torch.isfinite(got), err, torch.full_like(err, float('inf')))
    r = err / budget.to(F64).expand_as(err).clamp_min(1e-300)
    r = torch.where(err == 0, torch.zeros_like(r), r)
    if exempt is not None:
        r = torch.where(exempt.expand_as(r), torch.zeros_like(r), r)
    worst = float(r.max())
    print(f'ratio({name}) = {worst:.3g}   [max err {float(err.max()):.3g}, max |ref| {float(ref.abs().max()):.3g}]')
    return worst


def pixel_major(t):
    """same values, stored [B,H,W,C] (what the trainer's activations are)"""
    return t.contiguous(memory_format=torch.channels_last)


def header_define(name):
    text = open(os.path.join(ROOT, 'include', 'sininn.h')).read()
    return int(re.search(r'#define\s+' + name + r'\s+(\d+)', text).group(1))


# =================================================================================================================================
# A. MMD chain
# =================================================================================================================================
MMD_KC, MMD_MAXBLOCKS, MMD_THREADS = 128, 1024, 256
MMD_KERNELS = {False: ((0.2, 2.0), (1.5, 2.0), (3.0, 2.0)), True: ((0.2, 0.1), (0.2, 0.5), (0.2, 2.0))}   # loss.py:11-14: (C, a)


def mmd_plan(B, K):
    chunks = -(-K // MMD_KC)
    blocks = min(chunks, MMD_MAXBLOCKS)
    return dict(chunks=chunks, blocks=blocks, trips=-(-chunks // blocks), slots=min(blocks, 16),
                pair_trips=-(-(B * B) // MMD_THREADS), pad=chunks * MMD_KC - K,
                lds=2 * B * (MMD_KC + 1) * 4)


def run_gram(x, y):
    """the Gram entry exactly as functional._MMD.forward calls it: g = (1 + SININN_MMD_SLOTS) * 3 B^2 zeroed floats.  The buffer
    is followed by a NaN guard: a kernel whose slot layout is larger than that allocation would write into it."""
    from sin_inn_amd import ops
    b = x.shape[0]
    slots = header_define('SININN_MMD_SLOTS')
    assert 1 + slots == 17, 'functional.py allocates 17 * 3 * b * b floats'
    n = 17 * 3 * b * b
    buf = torch.full((n + 4096,), float('nan'), device=x.device)
    g = buf[:n]
    g.zero_()
    ops.mmd_gram(x, y, g)
    torch.cuda.synchronize()
    assert bool(torch.isnan(buf[n:]).all()), 'mmd_gram wrote past (1 + SININN_MMD_SLOTS) * 3 * B * B floats'
    return g


def gram_ref(x, y):
    """float64 Grams [3,B,B] and the sums of |terms| of each entry"""
    b = x.shape[0]
    xf, yf = x.to(F64).reshape(b, -1), y.to(F64).reshape(b, -1)     # reshape of a permuted view: logical (c,h,w) order, any layout
    G = torch.stack((xf @ xf.t(), yf @ yf.t(), xf @ yf.t()))
    xa, ya = xf.abs(), yf.abs()
    S = torch.stack((xa @ xa.t(), ya @ ya.t(), xa @ ya.t()))
    return G, S


def gram_depth(plan):
    """roundings on the longest path of one Gram entry: the product (not fused: 1) and 128 sequential adds inside a chunk, the
    atomics that land in one slot (chunks of the blocks with blockIdx % 16 == slot, every trip of them), the 16-slot sum"""
    per_slot = -(-plan['blocks'] // 16) * plan['trips']
    return 1 + MMD_KC + per_slot + 16


def mmd_terms(r, dlt, rev, B):
    """float64 kernel sums of one distance matrix r (before the clamp), with its fp32 rounding bound dlt:
    k = sum_q C^a ((C + d)/a)^-a, p = dk/dd, and absolute error bounds of the fp32 evaluation of k and p.
    Element-wise roundings counted in U: C^a by powf 4 (2 ulp), the base (C + d)/a 2, amplified by the exponent (<= 3) 6, powf 4,
    the product 1, the 3-term sum 3 -> 18; EL = 24 leaves the table-lookup powf of the device library one more ulp."""
    EL = 24
    d = r.clamp_min(0)
    k = torch.zeros_like(d); p = torch.zeros_like(d); dp = torch.zeros_like(d)
    for c, a in MMD_KERNELS[rev]:
        c, a = float(np.float32(c)), float(np.float32(a))
        base = (c + d) / a
        k += c ** a * base ** (-a)
        p -= c ** a * base ** (-a - 1)
        dp += c ** a * (a + 1) / a * base ** (-a - 2)          # |dp/dd|
    Ek = p.abs() * dlt + EL * U * k
    Ep = dp * dlt + EL * U * p.abs()
    return k, p, Ek, Ep


def finish_ref(G, rev, extra=None):
    """float64 loss.py:20-36 on Grams G [3,B,B] + the four coefficient matrices of mmd_finish_kernel (AX, BX, AY, BY with
    gx = AX x + BX y, gy = AY x + BY y), and absolute budgets for the kernel's fp32 evaluation FROM THE SAME Grams.
    extra [3,B,B]: an additional error bound of the Gram entries themselves (end-to-end budget)."""
    B = G.shape[1]
    xx, yy, xy = G
    dx, dy = xx.diag(), yy.diag()
    rs, dl = [], []
    ex = extra if extra is not None else torch.zeros_like(G)
    for (a, b, c, ea, eb, ec) in ((dx[:, None], dx[None, :], xx, ex[0].diag()[:, None], ex[0].diag()[None, :], ex[0]),
                                  (dy[:, None], dy[None, :], yy, ex[1].diag()[:, None], ex[1].diag()[None, :], ex[1]),
                                  (dx[:, None], dy[None, :], xy, ex[0].diag()[:, None], ex[1].diag()[None, :], ex[2])):
        r = a + b - 2 * c
        # fp32: (a + b) rounds once, (.. - 2 c) once, each by at most U * (|a| + |b| + 2 |c|); a + a - 2 a is exactly 0 whatever
        # the Gram entry a is
        delta = 2 * U * (a.abs() + b.abs() + 2 * c.abs()) + ea + eb + 2 * ec
        delta = torch.where((a == b) & (b == c), torch.zeros_like(delta), delta)      # the diagonal of dxx, dyy: exactly 0
        # the kernel masks the coefficient with r >= 0: the reference's mask is the kernel's unless |r| is within delta of 0
        assert bool(((r.abs() > delta) | (r == 0)).all()), 'a distance within rounding of the clamp: the case is ill-posed'
        rs.append(r); dl.append(delta)
    inv = 1.0 / (B * B)
    kxx, pxx, Ekxx, Epxx = mmd_terms(rs[0], dl[0], rev, B)
    kyy, pyy, Ekyy, Epyy = mmd_terms(rs[1], dl[1], rev, B)
    kxy, pxy, Ekxy, Epxy = mmd_terms(rs[2], dl[2], rev, B)
    loss = (kxx + kyy - 2 * kxy).sum() * inv
    # the reduction: ceil(B^2/256) sequential steps of 3 adds per thread, 6 wave-shuffle adds, 3 adds of the wave sums, * inv
    depth = 3 * -(-(B * B) // MMD_THREADS) + 6 + 3 + 2
    Eloss = ((Ekxx + Ekyy + 2 * Ekxy).sum() + depth * U * (kxx + kyy + 2 * kxy).sum()) * inv
    m = lambda r: (r >= 0).to(F64)
    gxx, gyy, gxy = m(rs[0]) * pxx * inv, m(rs[1]) * pyy * inv, m(rs[2]) * -2 * pxy * inv
    Egxx, Egyy = (Epxx + 2 * U * pxx.abs()) * inv, (Epyy + 2 * U * pyy.abs()) * inv      # * inv: 1 / B^2 and the product round
    Egxy = 2 * (Epxy + 2 * U * pxy.abs()) * inv
    eye = torch.eye(B, device=G.device, dtype=F64)

    def diag_block(g, Eg, cross, Ecross):
        """AX (cross = gxy summed over its row) or BY (cross = gxy summed over its column)"""
        off = -2 * (g + g.t())
        Eoff = 2 * (Eg + Eg.t()) + U * 2 * (g.abs() + g.t().abs())
        row = (g + g.t() + cross).sum(1)
        rowabs = (g.abs() + g.t().abs() + cross.abs()).sum(1)
        Erow = (Eg + Eg.t() + Ecross).sum(1) + 3 * B * U * rowabs                          # 3 B sequential adds
        val = off + eye * 2 * row[:, None]
        Eval = Eoff + eye * (2 * Erow[:, None] + U * (off.abs() + 2 * rowabs[:, None]))
        return val, Eval
    AX, EAX = diag_block(gxx, Egxx, gxy, Egxy)
    BY, EBY = diag_block(gyy, Egyy, gxy.t(), Egxy.t())
    BX, EBX = -2 * gxy, 2 * Egxy
    AY, EAY = -2 * gxy.t(), 2 * Egxy.t()
    return loss, Eloss, torch.stack((AX, BX, AY, BY)), torch.stack((EAX, EBX, EAY, EBY))


def mmd_data(kind, shape, seed, dev):
    g = gen(seed)
    if kind == 'image':                      # HR side: image-like, y a noisy copy of x
        x = torch.rand(shape, device=dev, generator=g)
        y = x + 0.05 * torch.randn(shape, device=dev, generator=g)
    else:                                    # latent side
        x = 0.3 * torch.randn(shape, device=dev, generator=g)
        y = 0.3 * torch.randn(shape, device=dev, generator=g)
    return x, y


def lds_limit():
    """the per-block LDS limit the runtime enforces for a dynamic-LDS launch"""
    p = torch.cuda.get_device_properties(0)
    return int(getattr(p, 'shared_memory_per_block_optin', 0) or p.shared_memory_per_block)


# name: (kind, shape, pixel-major, rev, property the case exists for)
MMD_CASES = {
    'hr_configs1': ('image', (16, 3, 256, 256), False, True, lambda p: p['trips'] >= 2 and p['slots'] == 16),
    'latent_configs1': ('latent', (16, 192, 32, 32), True, False, lambda p: p['trips'] >= 2 and p['slots'] == 16),
    'ragged_k': ('image', (4, 3, 211, 209), False, False, lambda p: p['pad'] > 0 and p['chunks'] > 1024 and p['trips'] >= 2),
    'ragged_k_pm': ('latent', (3, 5, 37, 75), True, True, lambda p: p['pad'] > 0 and p['chunks'] > 16),
    'b24': ('latent', (24, 5, 24, 40), True, False, lambda p: p['pair_trips'] >= 2 and p['chunks'] > 16),
    'b32': ('image', (32, 3, 40, 56), False, True, lambda p: p['pair_trips'] >= 4),
    'b1': ('image', (1, 3, 64, 64), False, False, lambda p: p['pair_trips'] == 1 and p['chunks'] > 16),
}


@pytest.mark.parametrize('case', sorted(MMD_CASES))
def test_mmd_stages_against_float64(dev, case):
    """Grams, finish (loss + AX, BX, AY, BY) and backward, each against float64 of the kernel's own staged input."""
    from sin_inn_amd import ops
    kind, shape, pm, rev, prop = MMD_CASES[case]
    B, K = shape[0], shape[1] * shape[2] * shape[3]
    plan = mmd_plan(B, K)
    print(case, plan)
    assert prop(plan), plan
    x, y = mmd_data(kind, shape, 11, dev)
    if pm:
        x, y = pixel_major(x), pixel_major(y)
        assert x.stride(1) == 1
    # stage 1
    g = run_gram(x, y)
    Gk = g[:3 * B * B].reshape(3, B, B)
    G, S = gram_ref(x, y)
    assert ratio(f'{case} gram', Gk, G, gram_depth(plan) * U * S) <= 1
    # stage 2: float64 of the formula on the KERNEL's Grams
    out = torch.full((1,), float('nan'), device=dev)
    coef = torch.full((4 * B * B,), float('nan'), device=dev)
    ops.mmd_finish(g, B, rev, out, coef)
    loss, Eloss, CF, ECF = finish_ref(Gk.to(F64), rev)
    assert ratio(f'{case} finish loss', out[0], loss, Eloss) <= 1
    ck = coef.reshape(4, B, B)
    assert ratio(f'{case} finish coef', ck, CF, ECF) <= 1
    # stage 3: float64 of AX x + BX y / AY x + BY y on the KERNEL's coefficients; both output layouts; gx or gy null
    c64 = ck.to(F64)
    xf, yf = x.to(F64).reshape(B, -1), y.to(F64).reshape(B, -1)
    sc = torch.tensor([0.75], device=dev)
    want_x = (0.75 * (c64[0] @ xf + c64[1] @ yf)).reshape(shape)
    want_y = (0.75 * (c64[2] @ xf + c64[3] @ yf)).reshape(shape)
    # 2 B sequential terms, each a rounded product, then * scale
    bud_x = ((2 * B + 2) * U * 0.75 * (c64[0].abs() @ xf.abs() + c64[1].abs() @ yf.abs())).reshape(shape)
    bud_y = ((2 * B + 2) * U * 0.75 * (c64[2].abs() @ xf.abs() + c64[3].abs() @ yf.abs())).reshape(shape)
    total = B * K
    blocks = min(-(-total // 256), 8192)
    if case.endswith('configs1'):
        assert total > blocks * 256, 'mmd_bwd must take its grid-stride loop'
    for lay_pm in (False, True):
        for want_gx, want_gy in ((True, True), (True, False), (False, True)):
            mk = (lambda: pixel_major(torch.full(shape, float('nan'), device=dev))) if lay_pm else \
                (lambda: torch.full(shape, float('nan'), device=dev))
            gx = mk() if want_gx else None
            gy = mk() if want_gy else None
            ops.mmd_bwd(x, y, coef, sc, gx, gy)
            tag = f'{case} bwd {"pm" if lay_pm else "nchw"}'
            if want_gx:
                assert ratio(tag + ' gx', gx, want_x, bud_x) <= 1
            if want_gy:
                assert ratio(tag + ' gy', gy, want_y, bud_y) <= 1


@pytest.mark.parametrize('case', ['hr_configs1', 'latent_configs1', 'ragged_k', 'b24'])
def test_mmd_loss_value_end_to_end(dev, case):
    """loss.mmd (the autograd front end) against float64 loss.py:9-36, held to the SUM of the stage budgets: the Gram budget
    pushed through |dk/dd|, plus the finish budget.

    The end-to-end GRADIENT is not compared with float64 here: the reference's own fp32 evaluation is 2e-2 .. 4e-1 (max-norm)
    from its float64 evaluation at batch 16, 3x256x256 / 48x64x64 / 3x512x512, because r_i + r_j - 2 g_ij cancels at
    |x|^2 ~ 6e4 and d/dd (C + d)^-a amplifies what is left.  That is the formula's arithmetic in fp32, not the kernels'
    (DESIGN 4); the gradient is covered by stages 2 and 3 of test_mmd_stages_against_float64, which start from the kernel's Grams."""
    import loss as L
    kind, shape, pm, rev, _ = MMD_CASES[case]
    B, K = shape[0], shape[1] * shape[2] * shape[3]
    x, y = mmd_data(kind, shape, 12, dev)
    if pm:
        x, y = pixel_major(x), pixel_major(y)
    got = L.mmd(x, y, rev=rev)
    G, S = gram_ref(x, y)
    want, Eloss, _, _ = finish_ref(G, rev, extra=gram_depth(mmd_plan(B, K)) * U * S)
    assert ratio(f'{case} loss.mmd value', got, want, Eloss) <= 1
    print(f'  relative: {abs(float(got) - float(want)) / abs(float(want)):.3g}')


def test_mmd_largest_batch_is_launched_or_refused(dev):
    """B = 64 needs 2 * 64 * 129 * 4 = 66 048 bytes of dynamic LDS, more than 64 KiB.  Whether that launch is legal is a property
    of the device (its per-block LDS limit): where it is, the result is held to the same budgets; where it is not, the entry
    refuses the batch with its ordinary error return.  B = 65 is refused everywhere."""
    from sin_inn_amd import ops
    shape = (64, 3, 32, 32)
    plan = mmd_plan(64, 3 * 32 * 32)
    assert plan['lds'] == 66048 and plan['pair_trips'] == 16
    x, y = mmd_data('image', shape, 13, dev)
    legal = plan['lds'] <= lds_limit()
    print(f'B 64: {plan["lds"]} bytes of LDS, device limit {lds_limit()}: launch is {"legal" if legal else "refused"}')
    if legal:
        g = run_gram(x, y)
        G, S = gram_ref(x, y)
        assert ratio('b64 gram', g[:3 * 64 * 64].reshape(3, 64, 64), G, gram_depth(plan) * U * S) <= 1
        out = torch.full((1,), float('nan'), device=dev)
        coef = torch.full((4 * 64 * 64,), float('nan'), device=dev)
        ops.mmd_finish(g, 64, True, out, coef)
        loss, Eloss, CF, ECF = finish_ref(g[:3 * 64 * 64].reshape(3, 64, 64).to(F64), True)
        assert ratio('b64 finish loss', out[0], loss, Eloss) <= 1
        assert ratio('b64 finish coef', coef.reshape(4, 64, 64), CF, ECF) <= 1
    else:
        with pytest.raises(RuntimeError, match='bytes of LDS'):
            ops.mmd_gram(x, y, torch.zeros(17 * 3 * 64 * 64, device=dev))
        torch.cuda.synchronize()
    x65 = torch.zeros(65, 1, 4, 4, device=dev)
    with pytest.raises(RuntimeError, match='batch must be in 1..64'):
        ops.mmd_gram(x65, x65, torch.zeros(17 * 3 * 65 * 65, device=dev))


# =================================================================================================================================
# bilinear sampling in float64 (both warps)
# =================================================================================================================================
class Bilinear:
    """float64 4-tap gather at pixel coordinates (ix, iy) [B,H,W] of img [B,C,H,W], zeros outside; keeps taps, weights and flat
    indices so the gradients and their budgets are a few lines each"""

    def __init__(self, img, ix, iy):
        B, C, H, W = img.shape
        self.shape = (B, C, H, W)
        x0, y0 = ix.floor(), iy.floor()
        self.wx1, self.wy1 = ix - x0, iy - y0
        self.wx0, self.wy0 = 1 - self.wx1, 1 - self.wy1
        self.x0, self.y0 = x0.long(), y0.long()
        flat = img.reshape(B, C, H * W)
        self.taps, self.ok, self.idx = [], [], []
        for dy, dx in ((0, 0), (0, 1), (1, 0), (1, 1)):
            yy, xx = self.y0 + dy, self.x0 + dx
            ok = (yy >= 0) & (yy < H) & (xx >= 0) & (xx < W)
            idx = (yy.clamp(0, H - 1) * W + xx.clamp(0, W - 1)).reshape(B, 1, H * W)
            self.taps.append(flat.gather(2, idx.expand(B, C, H * W)).reshape(B, C, H, W) * ok[:, None])
            self.ok.append(ok); self.idx.append(idx)
        self.w = [self.wy0 * self.wx0, self.wy0 * self.wx1, self.wy1 * self.wx0, self.wy1 * self.wx1]

    def value(self):
        """interpolated value and sum |tap * weight|"""
        v = sum(t * w[:, None] for t, w in zip(self.taps, self.w))
        a = sum(t.abs() * w[:, None] for t, w in zip(self.taps, self.w))
        return v, a

    def slopes(self, g=None):
        """d value / d ix, d value / d iy per channel (times g)"""
        t00, t01, t10, t11 = self.taps
        sx = (t01 - t00) * self.wy0[:, None] + (t11 - t10) * self.wy1[:, None]
        sy = (t10 - t00) * self.wx0[:, None] + (t11 - t01) * self.wx1[:, None]
        return sx, sy

    def scatter(self, vals, weighted=True):
        """adjoint of the gather: vals [B,C,H,W] (or [B,1,H,W]) spread onto the 4 taps"""
        B, C, H, W = self.shape
        c = vals.shape[1]
        out = torch.zeros(B, c, H * W, device=vals.device, dtype=F64)
        for ok, idx, w in zip(self.ok, self.idx, self.w):
            v = vals * ok[:, None] * (w[:, None] if weighted else 1.0)
            out.scatter_add_(2, idx.expand(B, c, H * W), v.reshape(B, c, H * W))
        return out.reshape(B, c, H, W)


def lipschitz(img):
    """largest horizontal / vertical difference of neighbouring pixels of the zero-padded image: a bound of |d value / d ix|,
    |d value / d iy| of the bilinear interpolant in every cell, the cells that straddle the border included"""
    p = F.pad(img.to(F64), (1, 1, 1, 1))
    return float((p[..., :, 1:] - p[..., :, :-1]).abs().max()), float((p[..., 1:, :] - p[..., :-1, :]).abs().max())


def gimg_budget(bl, gabs, dxy, rounding_extra):
    """budget of an image gradient accumulated with atomics.  gabs [B,C,H,W] = |g| of every output pixel, dxy [B,H,W] =
    delta_x + delta_y, the rounding bound of its fp32 coordinates.
      * coordinates: the four weights of a pixel are continuous in (ix, iy) and move by at most 2 (delta_x + delta_y) in total
        (also across a cell boundary, where a weight passes through 0 and the next tap takes over); the bound |g| (dx + dy) is put
        on all four taps and spread over their 3x3 neighbourhood, which covers the taps of the adjacent cell;
      * summation: a destination pixel receives n contributions (counted with a scatter of ones); its value passes through at
        most n + rounding_extra roundings: 3 for g * wy * wx, the lane merges, LDS atomics and global atomics together are n adds
        in some order (rounding_extra counts the products and the merge / flush steps)"""
    coord = bl.scatter(gabs * dxy[:, None], weighted=False)
    coord = F.avg_pool2d(coord, 3, 1, 1, divisor_override=1)
    n = bl.scatter(torch.ones_like(gabs[:, :1]), weighted=False)
    mag = bl.scatter(gabs, weighted=True)
    return coord + (n + rounding_extra) * U * mag, n


# =================================================================================================================================
# B. flow warp + photometric L1
# =================================================================================================================================
FB_TX, FB_TY, FB_R = 32, 8, 8


def flow_field(B, H, W, dev, seed):
    """one flow field built from six horizontal bands, one per code path:
      0 constant sub-pixel flow (every lane merges with its neighbours), 1 smooth random flow, 2 exact-integer flow,
      3 |flow_x| in 9..40 towards the image centre (taps outside the 8-pixel LDS window, inside the image),
      4 flow pointing outside the image (all taps dropped; the first columns straddle the left border instead),
      5 a checkerboard that breaks the neighbour relation at every lane.
    (With the kept quirk C-18 the sampling position of an integer flow is (x + f) W/(W-1) - 1/2, not an integer: weights that are
    exactly zero come from the zeros in the upstream gradients, see flow_grads.)"""
    g = gen(seed)
    f = torch.zeros(B, 2, H, W, device=dev)
    edges = [round(i * H / 6) for i in range(7)]
    band = lambda i: slice(edges[i], edges[i + 1])
    xs = torch.arange(W, device=dev).float()[None, None, :]
    ys = torch.arange(H, device=dev).float()[None, :, None]
    f[:, 0, band(0)], f[:, 1, band(0)] = 0.3, -0.6
    hb = edges[2] - edges[1]
    low = torch.randn(B, 2, max(hb // 8, 2), max(W // 8, 2), device=dev, generator=g) * 2.0
    f[:, :, band(1)] = F.interpolate(low, size=(hb, W), mode='bilinear', align_corners=False)
    f[:, 0, band(2)], f[:, 1, band(2)] = 3.0, -2.0
    mag = 9.0 + 31.0 * torch.rand(B, edges[4] - edges[3], W, device=dev, generator=g)
    f[:, 0, band(3)] = torch.where(xs < W / 2, mag, -mag)
    f[:, 1, band(3)] = torch.randn(B, edges[4] - edges[3], W, device=dev, generator=g) * 0.5
    f[:, 0, band(4)] = torch.where(xs < 6, -xs - 0.7, torch.full_like(xs, W + 50.0)).expand(B, edges[5] - edges[4], W)
    f[:, 1, band(4)] = 0.25
    cb = ((xs + ys) % 2 == 0).expand(B, H, W)[:, band(5)]
    f[:, 0, band(5)] = torch.where(cb, 0.4, -1.7)
    f[:, 1, band(5)] = torch.where(cb, -1.3, 0.6)
    assert bool(torch.isfinite(f).all())
    return f, edges


def flow_coords(flow, H, W):
    """float64 sampling positions of the kernel's formula (grid = (coords + flow)/(W-1, H-1)*2-1, align_corners=False) and the
    rounding bound of their fp32 evaluation: x + f, / (W-1), - 1, + 1, * W (- 1 fused or not), each at most U times a normalised
    magnitude <= |g| + 1, scaled by W/2 into pixels -> 6 U (|ix| + W + 1)"""
    B = flow.shape[0]
    dev = flow.device
    xs = torch.arange(W, device=dev, dtype=F64)[None, None, :]
    ys = torch.arange(H, device=dev, dtype=F64)[None, :, None]
    f = flow.to(F64)
    ix = (xs + f[:, 0]) * W / (W - 1) - 0.5
    iy = (ys + f[:, 1]) * H / (H - 1) - 0.5
    return ix, iy, 6 * U * (ix.abs() + W + 1), 6 * U * (iy.abs() + H + 1)


def flow_plan(bl, H, W):
    """tiles of flow_warp_l1_bwd_tiled_kernel and the in-image taps that fall outside a tile's LDS window"""
    B = bl.shape[0]
    dev = bl.x0.device
    xs = torch.arange(W, device=dev)[None, None, :]
    ys = torch.arange(H, device=dev)[None, :, None]
    bx0, by0 = xs // FB_TX * FB_TX, ys // FB_TY * FB_TY
    far = 0
    for (dy, dx), ok in zip(((0, 0), (0, 1), (1, 0), (1, 1)), bl.ok):
        qx, qy = bl.x0 + dx - (bx0 - FB_R), bl.y0 + dy - (by0 - FB_R)
        inside = (qx >= 0) & (qx < FB_TX + 2 * FB_R) & (qy >= 0) & (qy < FB_TY + 2 * FB_R)
        far += int((ok & ~inside).sum())
    tiles = B * -(-H // FB_TY) * -(-W // FB_TX)
    dropped = int(sum((~ok).sum() for ok in bl.ok))
    return dict(tiles=tiles, far_taps=far, dropped_taps=dropped, ragged_row=W % FB_TX, ragged_col=H % FB_TY)


def bf16_ulp(v):
    """one bf16 ulp at |v| (8 significand bits)"""
    _, e = torch.frexp(v.abs().clamp_min(2.0 ** -126))
    return torch.ldexp(torch.ones_like(v), e - 8)


FLOW_CASES = {'configs3': (16, 3, 512, 512), 'ragged': (2, 5, 37, 75), 'maxc': (1, 8, 40, 96)}


@pytest.mark.parametrize('dtype', [torch.float32, BF], ids=['fp32', 'bf16'])
@pytest.mark.parametrize('case', sorted(FLOW_CASES))
def test_flow_warp_l1_against_float64(dev, case, dtype):
    from sin_inn_amd import ops
    B, C, H, W = FLOW_CASES[case]
    g = gen(21)
    img = torch.rand(B, C, H, W, device=dev, generator=g).to(dtype)
    tgt = torch.rand(B, C, H, W, device=dev, generator=g).to(dtype)
    flow, edges = flow_field(B, H, W, dev, 22)
    ix, iy, dx, dy = flow_coords(flow, H, W)
    bl = Bilinear(img.to(F64), ix, iy)
    plan = flow_plan(bl, H, W)
    print(case, plan)
    # ---- the properties the cases exist for
    assert plan['dropped_taps'] >= 100 and plan['far_taps'] >= 100
    if case == 'configs3':
        assert plan['tiles'] == 16 * 64 * 16 and plan['far_taps'] >= 1000
    if case == 'ragged':
        assert 4 < C <= 8 and plan['ragged_row'] != 0 and plan['ragged_col'] != 0     # second channel pass; a row ends mid-wave
    if case == 'maxc':
        assert C == 8
    # ---- forward
    warped = torch.full((B, C, H, W), float('nan'), device=dev).to(dtype)
    metric = torch.full((B, 1, H, W), float('nan'), device=dev)
    ops.flow_warp_l1(img, flow, tgt, warped, metric)
    val, aval = bl.value()
    Lx, Ly = lipschitz(img)
    # 4 products of 3 factors and 3 adds: 8 roundings on sum |tap * weight|; the weights 1 - w: 1 more
    bud = Lx * dx[:, None] + Ly * dy[:, None] + 9 * U * aval
    if dtype == BF:
        bud = bud + bf16_ulp(val)
    tag = f'{case} {"bf16" if dtype == BF else "fp32"}'
    assert ratio(tag + ' warped', warped, val, bud) <= 1
    # metric: float64 of mean_c |target - warped| on the warped values the kernel STORED; C subtractions, C adds, one division
    w64, t64 = warped.to(F64), tgt.to(F64)
    m64 = (t64 - w64).abs().mean(1, keepdim=True)
    assert ratio(tag + ' metric', metric, m64, (2 * C + 1) * U * m64) <= 1
    # metric without `warped` (fp32: the same arithmetic; bf16 rounds the value it compares, so only fp32 is bit-identical)
    if dtype == torch.float32:
        m2 = torch.full_like(metric, float('nan'))
        ops.flow_warp_l1(img, flow, tgt, None, m2)
        assert torch.equal(m2, metric)
    # ---- backward.  Upstream gradients with exact zeros (a block of gwarped; gmetric on a stripe): g == 0 there, the tiled kernel
    # skips the tap (`val != 0`)
    gw = torch.randn(B, C, H, W, device=dev, generator=g)
    gw[:, :, :, W // 3: W // 2] = 0
    gw = gw.to(dtype)
    gm = torch.rand(B, 1, H, W, device=dev, generator=g)
    gm[:, :, :, W // 3: W // 3 + 5] = 0
    sx, sy = bl.slopes()
    t00, t01, t10, t11 = bl.taps
    near = ((bl.wx1 < 2 * dx) | (bl.wx0 < 2 * dx) | (bl.wy1 < 2 * dy) | (bl.wy0 < 2 * dy))[:, None]   # cell undecided in fp32
    print(f'  pixels whose cell fp32 cannot decide: {float(near.double().mean()):.3g} of all')
    assert float(near.double().mean()) < 0.02
    for use_gw, use_gm in ((True, False), (False, True), (True, True)):
        gg = torch.zeros(B, C, H, W, device=dev, dtype=F64)
        gabs = torch.zeros_like(gg)
        if use_gw:
            gg = gg + gw.to(F64)
            gabs = gabs + gw.to(F64).abs()
        if use_gm:
            # the sign comes from the staged target and warped the kernel reads: exact in fp32, nothing left to flip
            s = torch.sign(t64 - w64)
            gg = gg - s * gm.to(F64) / C
            gabs = gabs + s.abs() * gm.to(F64) / C
        want_gimg = bl.scatter(gg)
        bud_gimg, ncontrib = gimg_budget(bl, gabs, dx + dy, 8)
        # gflow = W/(W-1) sum_c g_c slope_c: the slope is bilinear in the weights -> |cross difference| * delta of the OTHER axis;
        # per channel ~8 roundings on sum |g| (|t| w), the C-term sum C more, g itself (gm / C, +) 3, the final scale 2
        cross = (t11 - t10 - t01 + t00).abs()
        sxa = (t01.abs() + t00.abs()) * bl.wy0[:, None] + (t11.abs() + t10.abs()) * bl.wy1[:, None]
        sya = (t10.abs() + t00.abs()) * bl.wx0[:, None] + (t11.abs() + t01.abs()) * bl.wx1[:, None]
        kx, ky = W / (W - 1), H / (H - 1)
        want_gf = torch.stack(((gg * sx).sum(1) * kx, (gg * sy).sum(1) * ky), 1)
        bud_gf = torch.stack((((gabs * cross).sum(1) * dy + (C + 13) * U * (gabs * sxa).sum(1)) * kx,
                              ((gabs * cross).sum(1) * dx + (C + 13) * U * (gabs * sya).sum(1)) * ky), 1)
        which = f'{tag} {"gw" if use_gw else ""}{"+" if use_gw and use_gm else ""}{"gm" if use_gm else ""}'
        gimg = torch.zeros(B, C, H, W, device=dev)
        gflow = torch.full((B, 2, H, W), float('nan'), device=dev)
        ops.flow_warp_l1_bwd(img, flow, tgt if use_gm else None, warped if use_gm else None, gw if use_gw else None,
                             gm if use_gm else None, gimg, gflow)
        assert int(ncontrib.max()) >= 8, 'some pixel must collect many atomics'
        assert ratio(which + ' gimg (tiled)', gimg, want_gimg, bud_gimg) <= 1
        # gflow is discontinuous where a coordinate sits on a cell boundary: there fp32 and float64 may take different cells
        assert ratio(which + ' gflow (tiled)', gflow, want_gf, bud_gf, exempt=near) <= 1
        gflow2 = torch.full((B, 2, H, W), float('nan'), device=dev)
        ops.flow_warp_l1_bwd(img, flow, tgt if use_gm else None, warped if use_gm else None, gw if use_gw else None,
                             gm if use_gm else None, None, gflow2)
        assert ratio(which + ' gflow (flow-only)', gflow2, want_gf, bud_gf, exempt=near) <= 1
        # the two kernels evaluate the same expression per pixel
        assert bool(torch.isfinite(gflow).all()) and bool(torch.isfinite(gflow2).all())
        assert ratio(which + ' gflow tiled vs flow-only', gflow, gflow2.to(F64), bud_gf) <= 1


# =================================================================================================================================
# C. affine warp
# =================================================================================================================================
def affine_coords(theta, H, W):
    """float64 source positions of affine_src() and the rounding bound of their fp32 evaluation.  xn = (2x+1)/W - 1 (2 roundings,
    |xn| <= 1), xs = t0 xn + t1 yn + t2 (3 roundings of at most |t0| + |t1| + |t2|, plus the 2 of xn and yn carried through
    t0, t1), ix = ((xs + 1) W - 1)/2 (3 roundings of |xs| + 1); all scaled by W/2 into pixels"""
    dev = theta.device
    th = theta.to(F64).reshape(-1, 6)
    xn = ((2 * torch.arange(W, device=dev, dtype=F64) + 1) / W - 1)[None, None, :]
    yn = ((2 * torch.arange(H, device=dev, dtype=F64) + 1) / H - 1)[None, :, None]
    t = [th[:, i, None, None] for i in range(6)]
    xs = t[0] * xn + t[1] * yn + t[2]
    ys = t[3] * xn + t[4] * yn + t[5]
    ix, iy = ((xs + 1) * W - 1) / 2, ((ys + 1) * H - 1) / 2
    dx = U * W / 2 * (5 * (t[0].abs() + t[1].abs() + t[2].abs()) + 3 * (xs.abs() + 1))
    dy = U * H / 2 * (5 * (t[3].abs() + t[4].abs() + t[5].abs()) + 3 * (ys.abs() + 1))
    return ix, iy, dx.expand_as(ix), dy.expand_as(iy)


def tcr_thetas(B, H, W, scale, dev, seed):
    """thetas as tcr.py draws them (rotation and translation 5, lit_wrapper's defaults); the last three samples get a rotation of
    35 degrees / a shift of a third of the image so that a visible share of the taps leaves the image"""
    from tcr import pixel_matrix, normalized_inverse
    rand = torch.rand(B, 3, generator=torch.Generator().manual_seed(seed))
    th = normalized_inverse(pixel_matrix(rand, H, W, 5.0, 5.0, scale), H, W)
    big = normalized_inverse(pixel_matrix(torch.tensor([[0.0, 1.0, 0.0], [1.0, 0.0, 1.0], [0.1, 0.9, 0.5]]), H, W, 35.0, W / 3.0, 1), H, W)
    th[-3:] = big
    return th.contiguous().to(dev)


# name: (shape, pixel-major, tcr scale)
AFFINE_CASES = {
    'hr_nchw': ((16, 3, 256, 256), False, 1),
    'hr_pm': ((16, 3, 256, 256), True, 1),
    'lr_window_pm': ((16, 84, 32, 32), True, 0.25),        # what tcr.py warps on the LR side at configs[1] (lr_window 10)
}
AFFINE_MAXBLOCKS = 8192


@pytest.mark.parametrize('case', sorted(AFFINE_CASES))
def test_affine_warp_against_float64(dev, case):
    from sin_inn_amd import ops
    shape, pm, scale = AFFINE_CASES[case]
    B, C, H, W = shape
    total = B * C * H * W
    blocks = min(-(-total // 256), AFFINE_MAXBLOCKS)
    trips = -(-total // (blocks * 256))
    print(case, dict(total=total, blocks=blocks, trips=trips))
    if case.startswith('hr'):
        assert blocks == AFFINE_MAXBLOCKS and trips >= 2, 'the grid-stride loop must run'
    else:
        assert blocks > 1000
    g = gen(31)
    lay = pixel_major if pm else (lambda t: t)
    img = lay(torch.rand(shape, device=dev, generator=g))
    ref = lay(torch.rand(shape, device=dev, generator=g))
    assert (img.stride(1) == 1) == pm
    theta = tcr_thetas(B, H, W, scale, dev, 32)
    ix, iy, dx, dy = affine_coords(theta, H, W)
    bl = Bilinear(img.to(F64), ix, iy)
    dropped = sum(int((~ok).sum()) for ok in bl.ok) / (4.0 * B * H * W)
    print(f'  taps outside the image: {dropped:.3g} of all')
    assert dropped > 0.02
    val, aval = bl.value()
    # the reference IS affine_grid + grid_sample in float64: the gather above restates it (difference at float64 rounding level)
    gs = F.grid_sample(img.to(F64), F.affine_grid(theta.to(F64), list(shape), align_corners=False), mode='bilinear',
                       padding_mode='zeros', align_corners=False)
    assert float((gs - val).abs().max()) < 1e-9
    Lx, Ly = lipschitz(img)
    bud = Lx * dx[:, None] + Ly * dy[:, None] + 9 * U * aval
    out = lay(torch.full(shape, float('nan'), device=dev))
    ops.affine_warp(img, theta, out)
    assert ratio(f'{case} warped', out, val, bud) <= 1
    # fused SSE: sum (val - ref)^2.  A value error e moves a term by 2 |d| e + e^2; the sum passes through the thread's trips,
    # 6 shuffle adds, 3 adds of the wave sums and one atomic per block, plus 2 roundings of d and d*d
    out2 = lay(torch.full(shape, float('nan'), device=dev))
    sse = torch.zeros(1, device=dev)
    ops.affine_warp(img, theta, out2, ref, sse)
    assert torch.equal(out2, out)
    d = val - ref.to(F64)
    sse_bud = (2 * d.abs() * bud + bud * bud).sum() + (trips + 6 + 3 + blocks + 2) * U * (d * d).sum()
    assert ratio(f'{case} sse', sse[0], (d * d).sum(), sse_bud) <= 1
    # backward
    gout = lay(torch.randn(shape, device=dev, generator=g))
    want = bl.scatter(gout.to(F64))
    gbud, n = gimg_budget(bl, gout.to(F64).abs(), dx + dy, 4)
    gimg = lay(torch.zeros(shape, device=dev))
    ops.affine_warp_bwd(gout, theta, gimg)
    assert ratio(f'{case} gimg', gimg, want, gbud) <= 1


@pytest.mark.parametrize('pm', [False, True], ids=['nchw', 'pm'])
def test_affine_warp_sse_counts_every_block_exactly(dev, pm):
    """The derived budget of the SSE above is ~8200 U of the sum: one block's share (1/8192) hides inside it.  So the SSE is also run
    on inputs where fp32 is exact: identity theta at a power-of-two size (xn, ix are dyadic: val == img bit for bit) and
    differences in {0, 1, 2, 3}, whose squares sum to an integer below 2^24 in any order.  The kernel's sum must then EQUAL the
    float64 sum; a block, a trip or a wave dropped changes it."""
    from sin_inn_amd import ops
    shape = (16, 3, 256, 256)
    total = 16 * 3 * 256 * 256
    blocks = min(-(-total // 256), AFFINE_MAXBLOCKS)
    assert blocks == AFFINE_MAXBLOCKS and total > blocks * 256
    g = gen(33)
    lay = pixel_major if pm else (lambda t: t)
    img = lay(torch.randint(0, 256, shape, device=dev, generator=g).float() / 256)
    # P(d) = .55, .3, .1, .05: every block of 256 consecutive work items sees a non-zero difference
    r = torch.rand(shape, device=dev, generator=g)
    d = (r > .55).float() + (r > .85).float() + (r > .95).float()
    ref = lay(img - d)
    assert torch.equal(img - ref, d)
    want = float((d.double() ** 2).sum())
    assert want < 2 ** 24
    flat = d.permute(0, 2, 3, 1).reshape(-1) if pm else d.reshape(-1)          # the kernel's work-item order
    per_block = torch.zeros(blocks, device=dev, dtype=F64)
    per_block.index_add_(0, (torch.arange(total, device=dev) // 256) % blocks, flat.double() ** 2)
    assert float(per_block.min()) > 0, 'every block must hold a part of the sum'
    theta = torch.tensor([[1.0, 0, 0], [0, 1.0, 0]], device=dev).repeat(16, 1, 1).contiguous()
    out = lay(torch.full(shape, float('nan'), device=dev))
    sse = torch.zeros(1, device=dev)
    ops.affine_warp(img, theta, out, ref, sse)
    assert torch.equal(out, img)
    print(f'exact SSE: kernel {float(sse[0])}, float64 {want}')
    assert float(sse[0]) == want


# =================================================================================================================================
# D. squared-difference losses
# =================================================================================================================================
def sqdiff_cases(dev):
    g = gen(41)
    hr_x = torch.rand(16, 3, 256, 256, device=dev, generator=g)
    hr_y = torch.rand(16, 3, 256, 256, device=dev, generator=g)
    a = pixel_major(torch.randn(16, 192, 48, 48, device=dev, generator=g))          # lr | z of a 384x384 clip, pixel-major
    lr = pixel_major(torch.rand(16, 84, 48, 48, device=dev, generator=g))
    return {'hr_nchw': (hr_x, hr_y), 'lr_slice_pm': (a[:, :84], lr), 'z_slice_pm_no_y': (a[:, 84:], None)}


@pytest.mark.parametrize('case', ['hr_nchw', 'lr_slice_pm', 'z_slice_pm_no_y'])
def test_sqdiff_against_float64(dev, case):
    from sin_inn_amd import ops
    x, y = sqdiff_cases(dev)[case]
    total = x.numel()
    blocks_sum = min(-(-total // 1024), 512)
    blocks_bwd = min(-(-total // 256), 8192)
    trips_sum = -(-total // (blocks_sum * 256))
    print(case, dict(total=total, blocks_sum=blocks_sum, trips_sum=trips_sum, blocks_bwd=blocks_bwd))
    assert total > 512 * 1024 and blocks_sum == 512 and trips_sum >= 2, 'sqdiff_sum must run at its block cap'
    assert total > 8192 * 256 and blocks_bwd == 8192, 'sqdiff_bwd must take its grid-stride loop'
    if 'slice' in case:
        assert x.stride(1) == 1 and not x.is_contiguous(memory_format=torch.channels_last)
    d = x.to(F64) - (y.to(F64) if y is not None else 0)
    out = torch.zeros(1, device=dev)
    ops.sqdiff_sum(x, y, out)
    # d and d*d round once each; then the thread's trips, 6 shuffle adds, 3 adds of the wave sums, one atomic per block
    depth = 2 + trips_sum + 6 + 3 + blocks_sum
    assert ratio(f'{case} sum', out[0], (d * d).sum(), depth * U * (d * d).sum()) <= 1
    # backward: gx = scale * gscale * d, gy = -gx: the factor, d and the product round once each
    scale = torch.tensor([0.7], device=dev)
    gscale = 2.0 / total
    k = float(np.float32(0.7)) * float(np.float32(gscale))
    want = k * d
    for want_gx, want_gy in ((True, True), (True, False), (False, True)):
        if y is None and want_gy:
            continue
        # gradients go to a channel slice of a larger pixel-major tensor (NCHW case: a dense tensor); the rest must stay untouched
        def mk():
            if 'slice' in case:
                full = pixel_major(torch.full((x.shape[0], x.shape[1] + 7, x.shape[2], x.shape[3]), -7.0, device=dev))
                return full, full[:, 3:3 + x.shape[1]]
            full = torch.full(x.shape, float('nan'), device=dev)
            return full, full
        fx, gx = mk() if want_gx else (None, None)
        fy, gy = mk() if want_gy else (None, None)
        ops.sqdiff_bwd(x, y, scale, gscale, gx, gy)
        if want_gx:
            assert ratio(f'{case} gx', gx, want, 4 * U * want.abs()) <= 1
        if want_gy:
            assert ratio(f'{case} gy', gy, -want, 4 * U * want.abs()) <= 1
        for full in (fx, fy):
            if full is not None and 'slice' in case:
                assert bool((full[:, :3] == -7).all()) and bool((full[:, 3 + x.shape[1]:] == -7).all())


def test_sqdiff_sum_counts_every_block_exactly(dev):
    """as for the affine SSE: integer differences whose squares sum below 2^24 make the fp32 sum exact in any order, so the 512
    same-address atomics and every grid-stride trip must be present for the result to EQUAL the float64 sum"""
    from sin_inn_amd import ops
    shape = (16, 3, 256, 256)
    total = 16 * 3 * 256 * 256
    g = gen(42)
    y = torch.randint(0, 64, shape, device=dev, generator=g).float()
    r = torch.rand(shape, device=dev, generator=g)
    d = (r > .55).float() + (r > .85).float() + (r > .95).float()
    x = y + d
    want = float((d.double() ** 2).sum())
    assert want < 2 ** 24 and min(-(-total // 1024), 512) == 512
    out = torch.zeros(1, device=dev)
    ops.sqdiff_sum(x, y, out)
    assert float(out[0]) == want
    out.zero_()
    ops.sqdiff_sum(pixel_major(d), None, out)
    assert float(out[0]) == want


# =================================================================================================================================
# E. Adam
# =================================================================================================================================
class Adam64:
    """float64 Adam (torch.optim.Adam semantics, L2 weight decay) fed the same fp32 gradients, with a running bound of the fp32
    kernel's distance from it.  The scalars are the fp32 values the kernel receives.  Per step and element, in U:
      gg = g * gscale + wd * p         2 roundings of |g gscale| + |wd p|, plus wd * (bound of p)
      m  = b1 m + (1 - b1) gg          3 roundings of |b1 m| + |(1 - b1) gg|, plus the carried bounds   (1 - b1 is exact in fp32)
      v  = b2 v + (1 - b2) gg^2        4 roundings of v (all terms positive), plus the carried bounds
      den = sqrt(v) / sqrt(bc2) + eps  3 roundings; a bound e of v moves sqrt(v) by at most sqrt(v) - sqrt(v - e)
      p -= (lr / bc1) * (m / den)      the quotient and product 2, the host-side scalars lr / bc1, sqrt(bc2) 4, the subtraction 1
    The bounds are carried from step to step, so the budget grows (about linearly) with the step."""

    def __init__(self, p, lr, b1, b2, eps, wd, gscale):
        f = lambda v: float(np.float32(v))
        self.lr, self.b1, self.b2, self.eps, self.wd, self.gs = f(lr), f(b1), f(b2), f(eps), f(wd), f(gscale)
        self.p = p.to(F64).clone()
        self.m, self.v = torch.zeros_like(self.p), torch.zeros_like(self.p)
        self.Ep, self.Em, self.Ev = torch.zeros_like(self.p), torch.zeros_like(self.p), torch.zeros_like(self.p)
        self.t = 0

    def step(self, g):
        self.t += 1
        g = g.to(F64)
        omb1, omb2 = float(np.float32(1) - np.float32(self.b1)), float(np.float32(1) - np.float32(self.b2))
        bc1 = float(np.float32(1.0 - self.b1 ** self.t))
        sbc2 = float(np.sqrt(np.float32(1.0 - self.b2 ** self.t)))
        ss = float(np.float32(self.lr) / np.float32(bc1))
        gg = g * self.gs + self.wd * self.p
        Egg = self.wd * self.Ep + 2 * U * ((g * self.gs).abs() + (self.wd * self.p).abs())
        m = self.b1 * self.m + omb1 * gg
        Em = self.b1 * self.Em + omb1 * Egg + 3 * U * ((self.b1 * self.m).abs() + (omb1 * gg).abs())
        v = self.b2 * self.v + omb2 * gg * gg
        Ev = self.b2 * self.Ev + omb2 * (2 * gg.abs() * Egg + Egg * Egg) + 4 * U * v
        sq = v.sqrt()
        Esq = sq - (v - Ev).clamp_min(0).sqrt()
        den = sq / sbc2 + self.eps
        Eden = Esq / sbc2 + 3 * U * den
        denlo = (den - Eden).clamp_min(self.eps / 2)
        upd = ss * (m / den)
        Eupd = ss * (Em / denlo + m.abs() * Eden / (den * denlo)) + 6 * U * upd.abs()
        self.p = self.p - upd
        self.Ep = self.Ep + Eupd + U * self.p.abs()
        self.m, self.v, self.Em, self.Ev = m, v, Em, Ev


def adam_classes(n, dev, seed):
    """a fixed class per element: 0 = the gradient is always exactly zero (m and v stay exactly 0), 1 = ordinary gradients (1e-3),
    2 = gradients near Adam's eps = 1e-8, where the `+ eps` of the denominator decides the step"""
    r = torch.rand(n, device=dev, generator=gen(seed))
    return (r > 0.05).long() + (r > 0.5).long()


def adam_grads(cls, step):
    """fresh gradients of every step; a tenth of the live elements gets an exact zero in any one step"""
    n, dev = cls.numel(), cls.device
    g = gen(500 + step)
    r = torch.randn(n, device=dev, generator=g)
    mag = torch.where(cls == 1, torch.full_like(r, 1e-3), 1e-8 * (0.1 + 9.9 * torch.rand(n, device=dev, generator=g)))
    out = r * mag
    out[torch.rand(n, device=dev, generator=g) > 0.9] = 0
    out[cls == 0] = 0
    return out


@pytest.mark.parametrize('wd,gscale', [(0.0, 1.0), (1e-5, 0.125)])
def test_adam_step_long_buffer_with_scalar_tail(dev, wd, gscale):
    from sin_inn_amd import ops
    n = 4 * (4096 * 256 + 5000) + 3
    n4 = n >> 2
    blocks = min(-(-n4 // 256), 4096)
    print(dict(n=n, n4=n4, blocks=blocks, tail=n - 4 * n4))
    assert n % 4 == 3 and n4 > 4096 * 256 and blocks == 4096, 'float4 body beyond the block cap, then a 3-element scalar tail'
    g0 = gen(51)
    p = torch.randn(n, device=dev, generator=g0) * 0.05
    m, v = torch.zeros(n, device=dev), torch.zeros(n, device=dev)
    ref = Adam64(p, 1e-4, 0.9, 0.99, 1e-8, wd, gscale)
    cls = adam_classes(n, dev, 53)
    cls[-3], cls[-2], cls[-1] = 1, 0, 2        # the tail: an ordinary element, one with zero gradients, one near eps
    zero_mask = cls == 0
    worst, where = 0.0, None
    for step in range(1, 21):
        g = adam_grads(cls, step)
        g[-3], g[-1] = 1e-3, -3e-8
        if gscale != 1.0:
            g = g / gscale                     # an accumulated gradient that the step scales back
        ops.adam_step(p, g, m, v, 1e-4, 0.9, 0.99, 1e-8, wd, step, gscale)
        ref.step(g)
        for name, got, want, bud in (('p', p, ref.p, ref.Ep), ('m', m, ref.m, ref.Em), ('v', v, ref.v, ref.Ev)):
            err = (got.to(F64) - want).abs()
            assert bool(torch.isfinite(got).all())
            r = float(torch.where(err == 0, torch.zeros_like(err), err / bud.clamp_min(1e-300)).max())
            if r > worst:
                worst, where = r, (name, step)
            assert r <= 1, (step, name, r)
            rt = float((err[-3:] / bud[-3:].clamp_min(1e-300)).nan_to_num(0).max())      # the scalar tail on its own
            assert rt <= 1, (step, name, 'tail', rt)
        if step == 1:
            # the tail was stepped: the two live elements always, the zero-gradient one only through the weight decay
            assert int((m[-3:] != 0).sum()) == (2 if wd == 0 else 3), 'the scalar tail must have been stepped'
    # (a ratio close to 1 is expected: the bound of ONE rounding, U |p|, is attained by some of 4e6 elements just above a power of 2)
    print(f'ratio(adam long buffer wd {wd} gscale {gscale}) = {worst:.3g} at {where}')
    # eps is a visible part of the denominator (>= 1 %, against a budget of ~1e-6) for a large share of the elements
    share = float(((ref.v.sqrt() < 1e-6) & (ref.v > 0)).double().mean())
    print(f'  elements with 0 < sqrt(v) < 100 eps after 20 steps: {share:.3g}')
    assert share > 0.2
    assert wd > 0 or bool((p[zero_mask] == ref.p[zero_mask].float()).all()), 'zero gradients, no decay: p must not move'


def test_fused_adam_at_configs1_parameter_count(dev):
    """FusedAdam over the real SRF model of BASELINE configs[1] (256x256, -c 4, lr_window 10): one flat buffer of its parameter
    count, 20 steps with weight decay and a gradient scale, p / m / v after every step"""
    import archs
    import sin_inn_amd as S
    from test_gpu_model import make_opt
    torch.manual_seed(5)
    net = archs.UncondSRFlow(3, 256, 256, make_opt(num_coupling=4, lr_window=10)).cuda()
    params = [p for p in net.parameters() if p.requires_grad]
    n = sum(p.numel() for p in params)
    opt = S.FusedAdam(params, lr=1e-4, betas=(0.9, 0.99), weight_decay=1e-5)
    fl = opt._flat[0]
    npad = fl['p'].numel()
    blocks = min(-(-(npad >> 2) // 256), 4096)
    print(dict(parameters=n, flat=npad, blocks=blocks, trips=-(-(npad >> 2) // (blocks * 256))))
    assert fl['n'] == n and n > 1_000_000 and blocks > 1000
    ref = Adam64(fl['p'], 1e-4, 0.9, 0.99, 1e-8, 1e-5, 0.5)
    cls = adam_classes(npad, dev, 52)
    worst = 0.0
    for step in range(1, 21):
        opt.zero_grad()
        g = adam_grads(cls, step) * 2.0
        fl['g'].copy_(g)
        opt.step(grad_scale=0.5)
        ref.step(g)
        for name, got, want, bud in (('p', fl['p'], ref.p, ref.Ep), ('m', fl['m'], ref.m, ref.Em), ('v', fl['v'], ref.v, ref.Ev)):
            err = (got.to(F64) - want).abs()
            r = float(torch.where(err == 0, torch.zeros_like(err), err / bud.clamp_min(1e-300)).max())
            worst = max(worst, r)
            assert r <= 1 and bool(torch.isfinite(got).all()), (step, name, r)
    print(f'ratio(FusedAdam configs[1], {n} parameters) = {worst:.3g}')
    # the parameters are views of the flat buffer: the module sees the stepped values
    off = 0
    for p in params:
        assert p.data_ptr() == fl['p'].data_ptr() + 4 * off
        off += p.numel()


# =================================================================================================================================
# LeakyReLU backward on a channel slot
# =================================================================================================================================
def test_lrelu_bwd_strided_slot(dev):
    """sininn_lrelu_bwd: g[m][j] *= (f[m][j] > 0 ? 1 : slope), in place on n columns of wider rows.  One fp32 product per element:
    the result is the float64 product rounded once, compared bit for bit; columns outside the slot stay untouched."""
    from sin_inn_amd import _lib, ops
    M, n, gs, fs, slope = 16 * 64 * 64, 40, 56, 48, 0.2
    total = M * n
    blocks = min(-(-total // 256), 8192)
    assert blocks == 8192 and total > blocks * 256, 'more than one block, and the grid-stride loop'
    g0 = gen(61)
    gbuf = torch.randn(M, gs, device=dev, generator=g0)
    fbuf = torch.randn(M, fs, device=dev, generator=g0)
    fbuf[::7, 3] = 0.0
    fbuf[::11, 5] = -0.0
    fbuf[::13, 8] = float('nan')               # !(f > 0): the slope applies, as for the forward's max(x, slope x) at NaN
    g_off, f_off = 8, 4
    before = gbuf.clone()
    _lib.check(_lib.lib().sininn_lrelu_bwd(ops.ptr(gbuf, g_off), gs, ops.ptr(fbuf, f_off), fs, M, n, slope, ops._stream()))
    f = fbuf[:, f_off:f_off + n]
    gin = before[:, g_off:g_off + n].to(F64)
    want = torch.where(f > 0, gin, gin * float(np.float32(slope))).float()
    assert torch.equal(gbuf[:, g_off:g_off + n], want)
    assert torch.equal(gbuf[:, :g_off], before[:, :g_off]) and torch.equal(gbuf[:, g_off + n:], before[:, g_off + n:])
    assert float((f > 0).float().mean()) > 0.3 and float((~(f > 0)).float().mean()) > 0.3
