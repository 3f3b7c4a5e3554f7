"""GPU: the fp32 conv engine at production tile counts, kernel by kernel and variant by variant, against float64.

The kernel-level tests of tests/test_gpu_kernels.py run every variant (test hooks) at shapes where a weight-gradient split holds ONE
pixel tile and a persistent block walks one tile; the default dispatch at size is held to 1e-4 of the tensor maximum against fp32
torch, which cannot see an error confined to a border tile, a padded column or the last channel quad.  Here the same entry points
(ops.conv, sininn_wgrad, sininn_wgrad_group through the C ABI) run at the level shapes of BASELINE configs[1] (batch 16: 64x64 and
32x32), configs[4] (180x320 / 90x160, batch 1), configs[3] level 0 at batch 2 (128x128) and ragged shapes, under every hook.  Every
test rebuilds the launch plan from the formulas of the kernel source (make_plan / plan_group of csrc/wgrad_mfma.hip, conv_prepare /
wino_dispatch of csrc/conv_mfma.hip / wino_impl.h), checks it against the library where the ABI reports it (workspace bytes) and
asserts that a split really walks several tiles.

Two data regimes for every linear case.

1. EXACT INTEGERS.  Inputs and output gradients in {-2..2}, weights, biases and addends small integers.  Every matrix of Winograd
   F(2x2, 3x3) has entries in {0, +-1, +-1/2}:
       A^T = [1 1 1 0; 0 1 -1 -1]    B^T = [1 0 -1 0; 0 1 1 0; 0 -1 1 0; 0 1 0 -1]    G = [1 0 0; .5 .5 .5; .5 -.5 .5; 0 0 1]
   so every transformed value, product and partial sum is a multiple of 1/4, and while its magnitude stays below 2^22 it is an
   exact fp32 number whatever the order of summation: the direct kernels, both Winograd kernels, the Winograd weight gradient
   (dU = sum over tiles of (B^T d B) . (A dY A^T), then G^T dU G) and the ordered slab reduces must EQUAL float64, every element.
   Each test asserts the precondition itself: the sum of |terms| of every output, taken with |A|, |B|, |G| in the transformed
   domain for the Winograd kernels, is below 2^22.  ReLU and MASK gates are exact too.  One dropped tile, slot, tap, channel quad or
   slab out of thousands changes an integer and fails; no derived budget at depth 65 536 can see that.

2. RANDOM NORMALS, per-element budget.  bf16 holds small integers exactly, so regime 1 cannot see a reduced-precision operand path.
   On randn data every element is held to
       budget = (chain + partials + c) 2^-24 sum |terms|
   where sum |terms| is evaluated in float64 for THAT element (including the bias, the addend and the starting value of a +=
   gradient).  An fp32 sum of n exact-product terms in ANY order is within (n - 1) u sum |terms| of the exact one with u = 2^-24
   (each of the n - 1 additions rounds a partial sum that is at most sum |terms|), each product adds u of its own term, so
   `chain + partials` additions are covered by (chain + partials) u and c covers the roundings that are not part of the chain:
     * direct kernels: c = 2 (the product, and the final add of bias / addend / starting value).
         forward / data gradient: chain = K = taps x Cin per pixel, one partial sum (the accumulator register).
         weight gradient: chain = pixels per split = tiles_per_split x tile rows x 16, partials = S slabs (the ordered reduce).
     * Winograd kernels: sum |terms| in the transformed domain, |A|^T [(|G| |g| |G|^T) . (|B|^T |d| |B|)] |A| summed over channels
       (weight gradient: |G|^T [sum over tiles (|B|^T |d| |B|) . (|A| |dY| |A|^T)] |G|), which bounds every intermediate of any
       factorisation of the transforms.  chain = Cin (weight gradient: 2x2 tiles per split); partials = 2 for the 32x32x2 kernel's
       two partial tiles (S slabs, x 2 with the in-block k split, for the weight gradient); c = 14: the transforms are two-stage sums
       of at most 2 (B), 3 (A) and 3 (G) terms = 2 + 4 + 4 roundings, plus the product, the weight transform's own final
       rounding in the pack, the bias and the final add.
   A bf16-rounded operand is an error of order 2^-9 per term.  Every random case prints error / budget (run with -s); the worst per
   part goes into DESIGN 4.  A ratio above 1 is a finding to explain, not a constant to raise.

The float64 references are per-image, per-tap matmuls (tests/float64_refs.py) evaluated on the GPU in float64, as are the
transformed-domain sums."""
import ctypes as C
import os
import sys

import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, 'tests'))
from float64_refs import ref_conv, ref_dgrad, ref_wgrad  # noqa: E402

U = 2.0 ** -24
EXACT_LIMIT = 2.0 ** 22
SENTINEL = 12345.0                     # channels of a wider output tensor that the kernel must leave alone


# ---- Winograd F(2x2, 3x3) in float64 ------------------------------------------------------------------------------------------------
def _mats(dev):
    at = torch.tensor([[1, 1, 1, 0], [0, 1, -1, -1]], dtype=torch.float64, device=dev)
    bt = torch.tensor([[1, 0, -1, 0], [0, 1, 1, 0], [0, -1, 1, 0], [0, 1, 0, -1]], dtype=torch.float64, device=dev)
    g = torch.tensor([[1, 0, 0], [.5, .5, .5], [.5, -.5, .5], [0, 0, 1]], dtype=torch.float64, device=dev)
    return at.abs(), bt.abs(), g.abs()


def _abs_patches(xi, ty, tx):
    """|x| of one image [H,W,C] -> |B|^T |d| |B| of every 4x4 input patch: [16, ty * tx, C]"""
    H, W, Cn = xi.shape
    _, bt, _ = _mats(xi.device)
    xp = F.pad(xi.abs().double(), (0, 0, 1, 2 * tx + 1 - W, 1, 2 * ty + 1 - H))
    P = xp.unfold(0, 4, 2).unfold(1, 4, 2)                                    # [ty, tx, C, 4, 4]
    return torch.einsum('ik,yxckl,jl->ijyxc', bt, P, bt).reshape(16, ty * tx, Cn)


def wino_abs_conv(x, w):
    """sum |terms| of the Winograd forward conv in the transformed domain: x [B,H,W,C], w [N,C,3,3] -> float64 [B,H,W,N]"""
    B, H, W, Cn = x.shape
    n = w.shape[0]
    at, _, gm = _mats(x.device)
    ty, tx = -(-H // 2), -(-W // 2)
    ua = torch.einsum('ik,nckl,jl->ijcn', gm, w.abs().double(), gm).reshape(16, Cn, n)
    out = torch.zeros(B, 2 * ty, 2 * tx, n, dtype=torch.float64, device=x.device)
    for i in range(B):
        m = torch.bmm(_abs_patches(x[i], ty, tx), ua).reshape(4, 4, ty, tx, n)
        out[i] = torch.einsum('ai,ijyxn,bj->yaxbn', at, m, at).reshape(2 * ty, 2 * tx, n)
    return out[:, :H, :W]


def flip_weight(w):
    """the data gradient of a conv is the conv with w'[c, n, ky, kx] = w[n, c, k-1-ky, k-1-kx]"""
    return w.flip(2, 3).transpose(0, 1).contiguous()


def wino_abs_wgrad(x, g):
    """sum |terms| of the Winograd weight gradient: (|G|^T [sum_tiles (|B|^T|d||B|) . (|A||dY||A|^T)] |G| as [N,C,3,3], max of the
    inner 4x4 sums)"""
    B, H, W, Cn = x.shape
    n = g.shape[3]
    at, _, gm = _mats(x.device)
    ty, tx = -(-H // 2), -(-W // 2)
    du = torch.zeros(16, n, Cn, dtype=torch.float64, device=x.device)
    for i in range(B):
        v = _abs_patches(x[i], ty, tx)                                                          # [16, T, C]
        gp = F.pad(g[i].abs().double(), (0, 0, 0, 2 * tx - W, 0, 2 * ty - H)).reshape(ty, 2, tx, 2, n)
        m = torch.einsum('ai,yaxbn,bj->ijyxn', at, gp, at).reshape(16, ty * tx, n)
        du += torch.bmm(m.transpose(1, 2), v)
    gw = torch.einsum('ik,ijnc,jl->nckl', gm, du.reshape(4, 4, n, Cn), gm)
    return gw, float(du.max())


# ---- comparisons ------------------------------------------------------------------------------------------------------------------------
WORST = {}                             # part -> worst error / budget seen in this process (printed by every random case)


def check_exact(name, got, ref64, ctx):
    g = got.double()
    if torch.equal(g, ref64):
        return
    bad = ~(g == ref64)
    idx = bad.nonzero()[0].tolist()
    pytest.fail(f'{name}: {int(bad.sum())} of {bad.numel()} elements differ from the exact float64 result; first at index {idx}: '
                f'got {float(g[tuple(idx)])}, want {float(ref64[tuple(idx)])}; {ctx}')


def check_budget(part, name, got, ref64, budget, ctx):
    g = got.double()
    assert bool(torch.isfinite(g).all()), f'{name}: {int((~torch.isfinite(g)).sum())} elements not written / not finite; {ctx}'
    err = (g - ref64).abs()
    ratio = torch.where(budget > 0, err / budget.clamp_min(1e-300), torch.where(err > 0, torch.full_like(err, float('inf')), err))
    worst = float(ratio.max())
    WORST[part] = max(WORST.get(part, 0.0), worst)
    print(f'[conv-fp32-sizes] part {part} {name}: error / budget = {worst:.4f} (worst so far in part {part}: {WORST[part]:.4f}); {ctx}')
    if worst > 1.0:
        idx = (ratio == ratio.max()).nonzero()[0].tolist()
        pytest.fail(f'{name}: error / budget = {worst:.3f} at index {idx} (error {float(err[tuple(idx)]):.3e}, budget '
                    f'{float(budget[tuple(idx)]):.3e}), {int((ratio > 1).sum())} elements over; {ctx}')


def make(regime, gen, shape, lo=-2, hi=2, scale=1.0):
    """operand values of a regime: integers in [lo, hi] or scale * randn"""
    dev = torch.device('cuda')
    if regime == 'int':
        return torch.randint(lo, hi + 1, shape, device=dev, generator=gen).float()
    return torch.randn(shape, device=dev, generator=gen) * scale


def view_nhwc(t, b, h, w, c0, c):
    return t[:, c0:c0 + c].reshape(b, h, w, c)


# =====================================================================================================================================
# A. fp32 weight gradients (csrc/wgrad_mfma.hip) through sininn_wgrad / sininn_wgrad_group
# =====================================================================================================================================
def wgrad_plan(n, cin, ksize, b, h, w, hook=0):
    """make_plan (csrc/wgrad_mfma.hip).  hook bits: 0 16-wide MFMA tiles, 1 direct 3x3 instead of Winograd, 2 8-row tiles in the
    Winograd kernel, 3 8-wave blocks with the in-block k split."""
    wino = ksize == 3 and not hook & 2
    use32 = n % 32 == 0 and not hook & 1 and not wino
    if n % 64 != 0 and n % 48 == 0:
        rt, ct = 3, 4
    else:
        rt, ct = 4, (4 if (cin >= 64 and ksize == 1) else 2)
    if use32:
        rt, ct = 2, 2
    if wino:
        rt, ct = 4, 2
    bnw, bcw = rt * 16, ct * 16
    nblk, cblk = -(-n // bnw), -(-cin // bcw)
    nr, cc = nblk * bnw, cblk * bcw
    kh = 2 if (wino and hook & 8) else 1
    th = 4 if (wino and not hook & 4 and kh == 1) else 8
    ntiles = b * -(-w // 16) * -(-h // th)
    s = (256 if ((rt == 3 and not wino) or kh == 2) else 512) // (nblk * cblk)
    s = min(max(s, 1), ntiles)
    tps = -(-ntiles // s)
    s = -(-ntiles // tps)
    taps = ksize * ksize
    return dict(wino=wino, use32=use32, th=th, kh=kh, ntiles=ntiles, S=s, tiles_per_split=tps, last=ntiles - (s - 1) * tps,
                nblk=nblk, cblk=cblk, bytes=(s * taps * nr * cc + s * nr) * 4)


def group_plan(items, b, h, w, ksize, hook=0):
    """plan_group (csrc/wgrad_mfma.hip) for fp32 operands.  items: (Cin, N) with Cin counting a channel gap.  hook bit 7 clears wide_c
    (32 n x 64 c blocks for N <= 32 in the Winograd kernel)."""
    wino = ksize == 3
    th = 4 if wino else 8
    bnw, bcw = (64 if wino else 32), 32
    taps = ksize * ksize
    ntiles = b * -(-w // 16) * -(-h // th)
    shapes = []
    for cin, n in items:
        wide_c = wino and n <= 32 and not hook & 128
        bn, bc = (32, 64) if wide_c else (bnw, bcw)
        shapes.append((-(-n // bn), -(-cin // bc), bn, bc, wide_c))
    out_tiles = sum(nb * cb for nb, cb, *_ in shapes)
    s = min(max(512 // out_tiles, 1), ntiles)
    tps = -(-ntiles // s)
    s = -(-ntiles // tps)
    floats = sum(s * taps * nb * bn * cb * bc + (s * nb * bn + 3) // 4 * 4 for nb, cb, bn, bc, _ in shapes)
    return dict(wino=wino, th=th, ntiles=ntiles, S=s, tiles_per_split=tps, last=ntiles - (s - 1) * tps, out_tiles=out_tiles,
                wide_c=[sh[4] for sh in shapes], bytes=floats * 4)


def wgrad_budget(pl, x, g, ksize, gw0, gb0):
    """(budget gw, budget gb, max sum |terms|) of a weight-gradient plan for operands x [B,H,W,C], g [B,H,W,N]"""
    if pl['wino']:
        terms, inner = wino_abs_wgrad(x, g)
        chain = pl['tiles_per_split'] * (pl['th'] // 2) * 8                       # 2x2 output tiles of the split's pixel tiles
        coeff = chain + pl['S'] * pl.get('kh', 1) + 14
    else:
        terms = ref_wgrad(x.abs(), g.abs(), ksize)
        inner = float(terms.max())
        chain = pl['tiles_per_split'] * pl['th'] * 16
        coeff = chain + pl['S'] + 2
    gsum = g.abs().double().sum((0, 1, 2))
    cb = pl['tiles_per_split'] * pl['th'] * 16 + pl['S'] + 2                      # the bias gradient is a plain sum over pixels
    return (coeff * U * (terms + gw0.abs().double()), cb * U * (gsum + gb0.abs().double()),
            max(inner, float(terms.max()), float(gsum.max())))


# level shapes: (b, h, w, level); level 0 convs 24 -> 256 -> 48, level 1 convs 96 -> 256 -> 192
LEVEL_CONVS = {0: [(24, 256), (256, 48)], 1: [(96, 256), (256, 192)]}
RAGGED_WG = (2, 75, 118)                # ragged in x and y; see test_ragged_shape_ends_in_a_single_tile_split
WGRAD_SHAPES = [(16, 64, 64, 0), (16, 32, 32, 1),                  # configs[1] at batch 16
                (1, 180, 320, 0), (1, 90, 160, 1),                 # configs[4]: 180 rows are not a multiple of 8
                (2, 128, 128, 0),                                  # configs[3] level 0 at a batch the reference can afford
                RAGGED_WG + (0,)]
WGRAD_HOOKS = [0, 1, 2, 3, 4, 8, 12]


def _wgrad_operands(regime, gen, b, h, w, cin, n, ksize):
    """operands inside wider tensors at channel offset 8 (8 spare channels after), gradients starting non-zero"""
    m = b * h * w
    s = 1.0
    xf = make(regime, gen, (m, cin + 16), scale=s)
    gf = make(regime, gen, (m, n + 16), scale=s)
    gw0 = make(regime, gen, (n, cin, ksize, ksize), -3, 3)
    gb0 = make(regime, gen, (n,), -3, 3)
    return xf, gf, gw0, gb0


def _run_wgrad(lib, ops, xf, gf, cin, n, b, h, w, ksize, gw0, gb0, nbytes):
    gw, gb = gw0.clone(), gb0.clone()
    ws = torch.full(((nbytes + 3) // 4,), float('nan'), device=xf.device)      # a slab the kernel does not write poisons the reduce
    from sin_inn_amd import _lib
    _lib.check(lib.sininn_wgrad(ops.ptr(xf, 8), cin + 16, cin, ops.ptr(gf, 8), n + 16, n, b, h, w, ksize, ops.ptr(gw), ops.ptr(gb),
                                ops.ptr(ws), nbytes, ops._stream()))
    torch.cuda.synchronize()
    return gw, gb


@pytest.mark.parametrize('ksize', [3, 1])
@pytest.mark.parametrize('shape', WGRAD_SHAPES, ids=lambda s: 'x'.join(map(str, s[:3])))
def test_wgrad_variants_many_tiles_per_split(shape, ksize):
    """sininn_wgrad, both convs of the level, under every hook of test_wgrad (tests/test_gpu_kernels.py): the plan is rebuilt,
    checked against the library's workspace size under the same hook, and must give >= 2 tiles per split; integers exactly, randn
    at the budget of the plan; += onto non-zero gradients, NaN workspace, second run bitwise identical."""
    import sin_inn_amd  # noqa: F401
    from sin_inn_amd import _lib, ops
    lib = _lib.lib()
    b, h, w, level = shape
    for cin, n in LEVEL_CONVS[level]:
        for regime in ('int', 'randn'):
            gen = torch.Generator(device='cuda').manual_seed(1000 * cin + 10 * ksize + b + h)
            xf, gf, gw0, gb0 = _wgrad_operands(regime, gen, b, h, w, cin, n, ksize)
            x, g = view_nhwc(xf, b, h, w, 8, cin), view_nhwc(gf, b, h, w, 8, n)
            gw_ref = ref_wgrad(x, g, ksize) + gw0.double()
            gb_ref = g.double().sum((0, 1, 2)) + gb0.double()
            cache = {}
            for hook in WGRAD_HOOKS:
                pl = wgrad_plan(n, cin, ksize, b, h, w, hook)
                ctx = f'{cin}->{n} k{ksize} {b}x{h}x{w} hook {hook} {regime} plan {pl}'
                assert pl['tiles_per_split'] >= 2, ctx                  # cross-tile accumulation and next-tile staging run
                lib.sininn_wgrad_test_hooks(hook)
                try:
                    nbytes = lib.sininn_wgrad_workspace_bytes(n, cin, ksize, b, h, w)
                    assert nbytes == pl['bytes'], ('the plan of this file is not the plan of the library', nbytes, ctx)
                    gw, gb = _run_wgrad(lib, ops, xf, gf, cin, n, b, h, w, ksize, gw0, gb0, nbytes)
                    gw2, gb2 = _run_wgrad(lib, ops, xf, gf, cin, n, b, h, w, ksize, gw0, gb0, nbytes)
                finally:
                    lib.sininn_wgrad_test_hooks(0)
                assert torch.equal(gw, gw2) and torch.equal(gb, gb2), f'second run differs; {ctx}'
                key = (pl['wino'], pl['th'], pl['kh'], pl['S'], pl['tiles_per_split'])
                if key not in cache:
                    cache[key] = wgrad_budget(pl, x, g, ksize, gw0, gb0)
                bw, bb, top = cache[key]
                if regime == 'int':
                    assert top + 4 < EXACT_LIMIT, (top, ctx)            # + |starting value|
                    check_exact('gw', gw, gw_ref, ctx)
                    check_exact('gb', gb, gb_ref, ctx)
                else:
                    check_budget('A', 'gw', gw, gw_ref, bw, ctx)
                    check_budget('A', 'gb', gb, gb_ref, bb, ctx)


def test_ragged_shape_ends_in_a_single_tile_split():
    """the ragged shape of part A gives a last split of ONE tile for the default Winograd and direct plans of the level-0 convs"""
    b, h, w = RAGGED_WG
    singles = [(cin, n, k) for cin, n in LEVEL_CONVS[0] for k in (3, 1) if wgrad_plan(n, cin, k, b, h, w)['last'] == 1]
    assert singles, [wgrad_plan(n, cin, k, b, h, w) for cin, n in LEVEL_CONVS[0] for k in (3, 1)]
    for cin, n, k in singles:
        assert wgrad_plan(n, cin, k, b, h, w)['tiles_per_split'] >= 2
    b, h, w = RAGGED_GROUP
    plans = [group_plan([(c, n) for c, n, _, _ in spec], b, h, w, k, hook) for k in (3, 1) for _, spec, hook in _groups(0)]
    assert sum(p['last'] == 1 and p['tiles_per_split'] >= 2 for p in plans) >= 2, plans


def _run_group(lib, ops, probs, b, h, w, ksize, expect_bytes, ctx):
    """probs: (xf, cin_op, gf, n, gw, gb, gap_begin, gap_len), operands at channel offset 8 of tensors 16 channels wider"""
    from sin_inn_amd import _lib
    arr = (_lib.WgradItem * len(probs))()
    for it, (xf, cin_op, gf, n, gw, gb, gap_begin, gap_len) in zip(arr, probs):
        it.struct_bytes = C.sizeof(_lib.WgradItem)
        it.inp, it.in_stride, it.Cin = ops.ptr(xf, 8), cin_op + 16, cin_op
        it.dout, it.dout_stride, it.N = ops.ptr(gf, 8), n + 16, n
        it.gw, it.gb = ops.ptr(gw), ops.ptr(gb)
        it.gap_begin, it.gap_len = gap_begin, gap_len
    nbytes = lib.sininn_wgrad_group_workspace_bytes(arr, len(probs), b, h, w, ksize)
    assert nbytes == expect_bytes, ('the plan of this file is not the plan of the library', nbytes, ctx)
    ws = torch.full((nbytes // 4,), float('nan'), device=probs[0][0].device)
    _lib.check(lib.sininn_wgrad_group(arr, len(probs), b, h, w, ksize, ops.ptr(ws), nbytes, ops._stream()))
    torch.cuda.synchronize()


# (name, [(Cin of the operand, N, gap_begin, gap_len)], hook)
def _groups(level):
    c1, c2 = LEVEL_CONVS[level]
    whole = [c2 + (0, 0), c1 + (0, 0)] * 2
    return [('block', whole, 0), ('half', whole[:2], 32)]


RAGGED_GROUP = (3, 68, 45)              # a last split of ONE tile in three of the four group plans
GROUP_SHAPES = WGRAD_SHAPES[:5] + [RAGGED_GROUP + (0,), (3, 75, 150, 0)]
NARROW = [(56, 32, 0, 0), (88, 32, 0, 0), (256, 24, 0, 0), (40, 32, 24, 8)]      # N <= 32: wide_c blocks; the last with a channel gap


def _group_case(lib, ops, name, spec, hook, b, h, w, ksize, want_wide=None, short=None):
    items = [(cin, n) for cin, n, _, _ in spec]
    pl = group_plan(items, b, h, w, ksize, hook)
    assert pl['tiles_per_split'] >= 2, (name, pl)
    if want_wide is not None:
        assert pl['wide_c'] == want_wide, (name, pl)
    if short is not None:
        assert (pl['last'] < pl['tiles_per_split']) == short, (name, pl)
    for regime in ('int', 'randn'):
        ctx = f'group {name} {spec} k{ksize} {b}x{h}x{w} hook {hook} {regime} plan {pl}'
        gen = torch.Generator(device='cuda').manual_seed(77 * len(spec) + 10 * ksize + b + h + hook)
        data = []
        for cin_op, n, gap_begin, gap_len in spec:
            xf, gf, gw0, gb0 = _wgrad_operands(regime, gen, b, h, w, cin_op, n, ksize)
            keep = [c for c in range(cin_op) if not gap_begin <= c < gap_begin + gap_len]
            gw0 = gw0[:, :len(keep)].contiguous()                       # the weight has no counterpart of the gap channels
            data.append((xf, gf, gw0, gb0, keep))
        outs = []
        for _ in range(2):
            probs, run = [], []
            for (cin_op, n, gap_begin, gap_len), (xf, gf, gw0, gb0, keep) in zip(spec, data):
                gw, gb = gw0.clone(), gb0.clone()
                probs.append((xf, cin_op, gf, n, gw, gb, gap_begin, gap_len))
                run.append((gw, gb))
            lib.sininn_wgrad_test_hooks(hook)
            try:
                _run_group(lib, ops, probs, b, h, w, ksize, pl['bytes'], ctx)
            finally:
                lib.sininn_wgrad_test_hooks(0)
            outs.append(run)
        for i, ((cin_op, n, _, _), (xf, gf, gw0, gb0, keep)) in enumerate(zip(spec, data)):
            gw, gb = outs[0][i]
            assert torch.equal(gw, outs[1][i][0]) and torch.equal(gb, outs[1][i][1]), f'second run differs, problem {i}; {ctx}'
            x = view_nhwc(xf, b, h, w, 8, cin_op)[..., keep]
            g = view_nhwc(gf, b, h, w, 8, n)
            gw_ref = ref_wgrad(x, g, ksize) + gw0.double()
            gb_ref = g.double().sum((0, 1, 2)) + gb0.double()
            bw, bb, top = wgrad_budget(pl, x, g, ksize, gw0, gb0)
            if regime == 'int':
                assert top + 4 < EXACT_LIMIT, (top, ctx)
                check_exact(f'gw[{i}]', gw, gw_ref, ctx)
                check_exact(f'gb[{i}]', gb, gb_ref, ctx)
            else:
                check_budget('A', f'group gw[{i}]', gw, gw_ref, bw, ctx)
                check_budget('A', f'group gb[{i}]', gb, gb_ref, bb, ctx)


@pytest.mark.parametrize('ksize', [3, 1])
@pytest.mark.parametrize('shape', GROUP_SHAPES, ids=lambda s: 'x'.join(map(str, s[:3])))
def test_wgrad_group_many_tiles_per_split(shape, ksize):
    """sininn_wgrad_group on fp32 operands: the four convs of a block as one group, and the two convs of a half-coupling under hook
    bit 5 (the executor's per-half grouping)."""
    import sin_inn_amd  # noqa: F401
    from sin_inn_amd import _lib, ops
    lib = _lib.lib()
    b, h, w, level = shape
    for name, spec, hook in _groups(level):
        _group_case(lib, ops, name, spec, hook, b, h, w, ksize)


@pytest.mark.parametrize('ksize', [3, 1])
@pytest.mark.parametrize('hook', [0, 128])
@pytest.mark.parametrize('shape', [(16, 32, 32), (3, 75, 150)], ids=lambda s: 'x'.join(map(str, s)))
def test_wgrad_group_narrow_outputs_and_channel_gap(shape, hook, ksize):
    """N <= 32 problems with wide_c (32 n x 64 c blocks of the Winograd kernel) on and off (hook bit 7), one of them reading an
    operand with a channel gap (gap_begin / gap_len: padding channels that have no counterpart in the weight)."""
    import sin_inn_amd  # noqa: F401
    from sin_inn_amd import _lib, ops
    b, h, w = shape
    want = [ksize == 3 and hook == 0] * len(NARROW)
    _group_case(_lib.lib(), ops, 'narrow', NARROW, hook, b, h, w, ksize, want_wide=want)


# =====================================================================================================================================
# B. forward and data-gradient convs through ops.conv (fp32 packs)
# =====================================================================================================================================
def conv_plan(cin, npk, ksize, cfg, force_ck):
    """conv_prepare / conv_launch (csrc/conv_mfma.hip): channel chunk = the largest of 32 / 24 / 16 / 8 dividing Cin unless force_ck
    overrides it; 32-wide MFMA column tiles when Np % 32 == 0 and cfg < 10"""
    ck = next(c for c in (32, 24, 16, 8) if cin % c == 0)
    if force_ck and cin % force_ck == 0 and force_ck % 8 == 0 and force_ck <= 32:
        ck = force_ck
    return dict(CK=ck, chunks=cin // ck, tile=32 if (npk % 32 == 0 and cfg < 10) else 16, K=ksize * ksize * cin)


def wino_plan(cin, npk, b, h, w, cg, col_tile=16):
    """wino_dispatch (csrc/wino_impl.h): 64-column blocks when the 32-column groups pair up and Cin >= 64; else the 32x32x2 kernel
    (two partial output tiles) when the column interleave is 16 (every non-coupling conv; a coupling conv packed with col_tile 16),
    Cin >= 128 and at most 256 blocks"""
    never32, always32, cg2 = bool(cg & 4), bool(cg & 8), cg & 3
    even = (-(-npk // 32)) % 2 == 0
    wide = even and cin >= 64
    if cg2 == 1:
        wide = False
    if cg2 == 2:
        wide = even
    blocks = b * -(-h // 16) * -(-w // 16) * -(-npk // 32)
    if wide:
        return dict(kernel='wino64', blocks=blocks // 2)
    use32 = col_tile == 16 and not never32 and (always32 or (cin >= 128 and blocks <= 256))
    return dict(kernel='wino32' if use32 else 'wino', blocks=blocks)


DIRECT_HOOKS = [(0, 0), (1, 0), (2, 0), (10, 0), (12, 0), (0, 8)]
WINO_HOOKS = [0, 1, 2, 5, 9]
CONV_SHAPES = WGRAD_SHAPES[:5] + [(3, 75, 150, 0)]
# where wino_dispatch takes the 32x32x2 kernel by itself: the data gradient of conv1 (Cin = 256, one / three 32-column groups)
WINO32_BY_ITSELF = {(16, 64, 64, 24), (2, 128, 128, 24), (1, 180, 320, 24), (1, 90, 160, 96)}


def _conv_family(family, shape, cin, n):
    """Every linear epilogue of one conv (cin -> n) and its data gradient (n -> cin) under every hook of the family."""
    import sin_inn_amd  # noqa: F401
    from sin_inn_amd import _lib, ops
    lib = _lib.lib()
    dev = torch.device('cuda')
    b, h, w, _ = shape
    m = b * h * w
    wino = family == 'wino'
    ksize = 1 if family == 'direct1' else 3
    hooks = [(cg, 0) for cg in WINO_HOOKS] if wino else DIRECT_HOOKS
    np_f, np_d = ops.pad16(n), (ops.pad32(cin) if wino else ops.pad16(cin))
    assert b * -(-h // 16) * -(-w // 16) >= 24                       # many pixel tiles: borders, interiors and ragged edges
    for regime in ('int', 'randn'):
        gen = torch.Generator(device='cuda').manual_seed(31 * cin + n + 7 * ksize + b + h)
        fan = (ksize * ksize * cin) ** -0.5
        weight = make(regime, gen, (n, cin, ksize, ksize), -1, 1, fan)
        bias = make(regime, gen, (n,), -1, 1, 0.1)
        wf, bfwd, wd = ops.pack_conv(weight, bias, None, True, wino_fwd=wino, wino_dgrad=wino)
        xf = make(regime, gen, (m, cin + 16))                        # operands at channel offset 8 of wider tensors
        gf = make(regime, gen, (m, n + 16))
        hf = torch.relu(make(regime, gen, (m, cin + 16)))            # the strided hidden tensor MASK reads its gates from
        add = make(regime, gen, (m, 2 * cin + 16))
        amap = torch.randperm(2 * cin, device=dev, generator=gen)[:cin].to(torch.int32)
        x, g = view_nhwc(xf, b, h, w, 8, cin), view_nhwc(gf, b, h, w, 8, n)
        wflip = flip_weight(weight)
        # float64 references and sum |terms|, once per regime
        pre = ref_conv(x, weight, bias)
        dg = ref_dgrad(g, weight)
        gate = view_nhwc(hf, b, h, w, 8, cin) > 0
        add_plain = view_nhwc(add, b, h, w, 8, cin).double()
        add_map = add[:, amap.long()].reshape(b, h, w, cin).double()
        if wino:
            t_f = wino_abs_conv(x, weight) + bias.abs().double()
            t_d = wino_abs_conv(g, wflip)
        else:
            t_f = ref_conv(x.abs(), weight.abs(), bias.abs())
            t_d = ref_dgrad(g.abs(), weight.abs())
        cases = [  # name, mode, forward?, reference, sum |terms|
            ('linear', _lib.CONV_LINEAR, True, pre, t_f), ('relu', _lib.CONV_RELU, True, torch.relu(pre), t_f),
            ('mask', _lib.CONV_MASK, False, dg * gate, t_d * gate), ('add', _lib.CONV_ADD, False, dg + add_plain, t_d + add_plain.abs()),
            ('add_map', _lib.CONV_ADD, False, dg + add_map, t_d + add_map.abs()),
            ('add_inplace', _lib.CONV_ADD, False, dg + add_plain, t_d + add_plain.abs())]
        if regime == 'int':
            assert max(float(t_f.max()), float(t_d.max())) + 4 < EXACT_LIMIT, (float(t_f.max()), float(t_d.max()))
        for cfg, ck in hooks:
            for name, mode, fwd, ref, terms in cases:
                k_in, n_out, npk = (cin, n, np_f) if fwd else (n, cin, np_d)
                if wino:
                    pl = wino_plan(k_in, npk, b, h, w, cfg)
                    if cfg == 0 and not fwd and (b, h, w, cin) in WINO32_BY_ITSELF:
                        assert pl['kernel'] == 'wino32' and k_in >= 128 and pl['blocks'] <= 256, pl
                    if cfg == 9:
                        assert pl['kernel'] == 'wino32', pl
                    if cfg == 5:
                        assert pl['kernel'] == 'wino', pl
                    if cfg == 2 and (-(-npk // 32)) % 2 == 0:
                        assert pl['kernel'] == 'wino64', pl
                    coeff = k_in + (2 if pl['kernel'] == 'wino32' else 1) + 14
                else:
                    pl = conv_plan(k_in, npk, ksize, cfg, ck)
                    if ck:
                        assert pl['CK'] == ck and pl['chunks'] >= 2, pl      # the forced chunk really splits the channels
                    if cfg >= 10:
                        assert pl['tile'] == 16, pl
                    coeff = pl['K'] + 1 + 2
                ctx = f'{family} {name} {cin}->{n} {b}x{h}x{w} hooks ({cfg}, {ck}) {regime} plan {pl}'
                wide = n_out + 16
                if name == 'add_inplace':
                    out = add[:, :wide].clone().contiguous()           # the addend IS the output's channel sub-range [8, 8 + N)
                    before = out.clone()
                else:
                    out = torch.full((m, wide), SENTINEL, device=dev)
                    out[:, 8:8 + n_out] = float('nan')                 # every element must be written
                kw = dict(in_=ops.ptr(xf if fwd else gf, 8), in_stride=k_in + 16, Cin=k_in, w=ops.ptr(wf if fwd else wd), Np=npk,
                          winograd=int(wino), B=b, H=h, W=w, ksize=ksize, mode=mode, out=ops.ptr(out, 8), out_stride=wide, N=n_out)
                if fwd:
                    kw['bias'] = ops.ptr(bfwd)
                if name == 'mask':
                    kw.update(mask=ops.ptr(hf, 8), mask_stride=cin + 16)
                elif name == 'add':
                    kw.update(addend=ops.ptr(add, 8), addend_stride=2 * cin + 16)
                elif name == 'add_map':
                    kw.update(addend=ops.ptr(add), addend_stride=2 * cin + 16, addend_map=ops.ptr(amap, dtype=torch.int32))
                elif name == 'add_inplace':
                    kw.update(addend=ops.ptr(out, 8), addend_stride=wide)
                lib.sininn_conv_test_hooks(cfg, ck)
                try:
                    ops.conv(**kw)
                    torch.cuda.synchronize()
                finally:
                    lib.sininn_conv_test_hooks(0, 0)
                got = view_nhwc(out, b, h, w, 8, n_out)
                if name == 'add_inplace':
                    assert torch.equal(out[:, :8], before[:, :8]) and torch.equal(out[:, 8 + n_out:], before[:, 8 + n_out:]), ctx
                else:
                    assert bool((out[:, :8] == SENTINEL).all()) and bool((out[:, 8 + n_out:] == SENTINEL).all()), \
                        f'channels outside [8, 8 + N) were written; {ctx}'
                if regime == 'int':
                    check_exact(name, got, ref, ctx)
                else:
                    check_budget('B', f'{family} {name}', got, ref, coeff * U * terms, ctx)


@pytest.mark.parametrize('family', ['direct3', 'direct1', 'wino'])
@pytest.mark.parametrize('conv', [0, 1], ids=['conv1', 'conv2'])
@pytest.mark.parametrize('shape', CONV_SHAPES, ids=lambda s: 'x'.join(map(str, s[:3])))
def test_conv_linear_epilogues_at_size(shape, conv, family):
    """ops.conv on fp32 packs: LINEAR and RELU of the conv, MASK (gates from a strided hidden tensor) and ADD (plain, through an
    addend_map, in place into a channel sub-range) of its data gradient; direct 3x3 / 1x1 under sininn_conv_test_hooks cfg 0, 1, 2,
    10, 12 and a forced channel chunk of 8, Winograd under cg 0, 1, 2, 5, 9.  Outputs start as NaN inside a wider tensor whose
    other channels must stay untouched."""
    cin, n = LEVEL_CONVS[shape[3]][conv]
    _conv_family(family, shape, cin, n)


# =====================================================================================================================================
# C. the fused fp32 1x1 forward kernels (csrc/conv_pair_k1.hip, csrc/conv_sub1.hip) against an independent reference
# =====================================================================================================================================
# Non-linear tail (also the COUPLE epilogue of part B's kernels): with integer operands the s, t the epilogue receives are exact, so
# what is measured is the epilogue's own fp32 arithmetic, L = clamp 0.636 atan(s / clamp), e = exp(L), y = v e + t or (v - t) / e.
# Element budget = 4 x the deviation of the same formula evaluated in fp32 torch from float64, measured here on the same s, t, v as a
# RELATIVE unit of the element's own scale |v| e + |t| (resp. (|v| + |t|) / e): unit_y = max over the tensor of |y32 - y64| / scale, so
# an element where fp32 torch happens to round exactly still gets the budget of its neighbours.  Log-det per image: every tile adds
# one partial (64 pixels x co channels summed in registers and across waves) with an atomic, so
#   budget = (64 co + tiles per image) 2^-24 sum |L| + 4 unit_L sum |L|,     unit_L = max |L32 - L64| / |L|.
S1_MAX_BLOCKS = 256                    # conv_sub1_types.h: persistent blocks


def sub1_fwd_plan(b, h, w):
    """conv_sub1.hip: 16 x 4 pixel tiles, image-major tile index; min(ntiles, 256) persistent blocks, block g walks g, g + G, ..."""
    tx, ty = -(-w // 16), -(-h // 4)
    ntiles = b * tx * ty
    blocks = min(ntiles, S1_MAX_BLOCKS)
    crossing = any((g // (tx * ty)) != ((g + blocks) // (tx * ty)) for g in range(blocks) if g + blocks < ntiles)
    return dict(tiles_img=tx * ty, ntiles=ntiles, blocks=blocks, max_tiles_per_block=-(-ntiles // blocks), crosses_image=crossing)


def glow_tail(s, t, v, clamp, inverse, dtype):
    s, t, v = s.to(dtype), t.to(dtype), v.to(dtype)
    L = clamp * 0.636 * torch.atan(s / clamp)
    e = torch.exp(L)
    return ((v - t) / e if inverse else v * e + t), L, e


# 1 024 and 900 tiles on 256 blocks (900 is not a multiple of 256: the last round is partial); 120 ragged tiles and 50 tiles, one per
# block, as controls
SUB1_SHAPES = [((16, 64, 64), True), ((1, 180, 320), True), ((3, 37, 50), False), ((2, 20, 70), False)]


@pytest.mark.parametrize('co', [8, 16, 24])
@pytest.mark.parametrize('shape,many', SUB1_SHAPES, ids=lambda v: 'x'.join(map(str, v)) if isinstance(v, tuple) else str(v))
def test_fused_1x1_forward_against_float64(shape, many, co):
    """sininn_conv_pair_k1 (with and without the stored hidden tensor) and its persistent twin sininn_conv_sub1_fwd (which never stores
    it), both coupling directions, from real nn.Conv2d weights packed with ops.pack_conv / ops.coupling_colmap.  Integer regime: the hidden tensor and s
    must equal float64 exactly, y and the log-det sit at the epilogue budgets; randn regime: h and s at the direct-kernel budgets
    (K = co, K = 256).  The pair kernel without the stored h is bitwise the launch with it; the persistent kernel's s is bitwise the pair's
    where both are exact."""
    import sin_inn_amd  # noqa: F401
    from sin_inn_amd import _lib, ops
    lib = _lib.lib()
    dev = torch.device('cuda')
    b, h, w = shape
    m, c, clamp = b * h * w, 2 * co, 1.2
    pl = sub1_fwd_plan(b, h, w)
    assert pl['blocks'] == min(pl['ntiles'], 256)
    if many:
        assert pl['ntiles'] > 256 and pl['max_tiles_per_block'] >= 2, pl          # a block walks a second tile: the double buffer runs
    else:
        assert pl['max_tiles_per_block'] == 1, pl
    if shape == (1, 180, 320):
        assert pl['ntiles'] % 256 != 0, pl                   # the only case whose last round of blocks is partial
    if shape == (16, 64, 64):
        assert pl['max_tiles_per_block'] == 4 and pl['crosses_image'], pl       # consecutive tiles of a block lie in different images
    for regime in ('int', 'randn'):
        gen = torch.Generator(device='cuda').manual_seed(100 * co + b + h)
        conv1 = torch.nn.Conv2d(co, 256, 1).to(dev)
        conv2 = torch.nn.Conv2d(256, c, 1).to(dev)
        with torch.no_grad():
            if regime == 'int':           # s stays small enough for atan / exp to be well inside their ranges: sparse conv2 weights
                conv1.weight.copy_(make('int', gen, (256, co, 1, 1), -1, 1))
                conv1.bias.copy_(make('int', gen, (256,), -1, 1))
                w2 = make('int', gen, (c, 256, 1, 1), -1, 1) * (torch.rand((c, 256, 1, 1), device=dev, generator=gen) < 0.02)
                conv2.weight.copy_(w2 * 0.25)
                conv2.bias.copy_(make('int', gen, (c,), -1, 1) * 0.25)
            else:
                conv2.weight.mul_(0.3)
        pk1 = ops.pack_conv(conv1.weight.detach().contiguous(), conv1.bias.detach().contiguous(), None, False)
        pk2 = ops.pack_conv(conv2.weight.detach().contiguous(), conv2.bias.detach().contiguous(), ops.coupling_colmap(co, dev), False)
        x = make(regime, gen, (m, c))
        ld0 = make(regime, gen, (b,), -3, 3)
        # ---- float64 reference ------------------------------------------------------------------------------------------------------------
        w1, b1 = conv1.weight.detach().reshape(256, co).double(), conv1.bias.detach().double()
        w2, b2 = conv2.weight.detach().reshape(c, 256).double(), conv2.bias.detach().double()
        x2, v = x[:, co:].double(), x[:, :co].double()
        h_pre = x2 @ w1.t() + b1
        h_ref = torch.relu(h_pre)
        h_terms = x2.abs() @ w1.abs().t() + b1.abs()
        common = dict(B=b, H=h, W=w, ksize=1)

        def args(**kw):
            a = _lib.ConvArgs()
            for k, val in kw.items():
                setattr(a, 'inp' if k == 'in_' else k, val)
            return a

        def run(persistent, mode, store_hidden):
            hid = torch.full((m, 256), float('nan'), device=dev)
            out = torch.full((m, c), SENTINEL, device=dev)
            out[:, :co] = float('nan')
            y2 = torch.full((m, co), float('nan'), device=dev)
            sb = torch.full((m, co), float('nan'), device=dev)
            ld = ld0.clone()
            f = args(in_=ops.ptr(x, co), in_stride=c, Cin=co, w=ops.ptr(pk1[0]), bias=ops.ptr(pk1[1]), Np=256, mode=_lib.CONV_RELU,
                     out=ops.ptr(hid) if store_hidden else None, out_stride=256, N=256, **common)
            s = args(in_=ops.ptr(hid), in_stride=256, Cin=256, w=ops.ptr(pk2[0]), bias=ops.ptr(pk2[1]), Np=c, mode=mode, out=ops.ptr(out),
                     out_stride=c, v=ops.ptr(x), v_stride=c, sbuf=ops.ptr(sb), logdet=ops.ptr(ld), Co=co, clamp=clamp, out2=ops.ptr(y2),
                     out2_stride=co, col_tile=ops.coupling_tile(co), **common)
            if persistent:
                assert lib.sininn_conv_sub1_fwd_supported(C.byref(f), C.byref(s)) == 1
                _lib.check(lib.sininn_conv_sub1_fwd(C.byref(f), C.byref(s), ops._stream()))
            else:
                assert lib.sininn_conv_pair_k1_supported(C.byref(f), C.byref(s)) == 1
                _lib.check(lib.sininn_conv_pair_k1(C.byref(f), C.byref(s), ops._stream()))
            torch.cuda.synchronize()
            return hid, out, y2, sb, ld

        for mode, inverse in ((_lib.CONV_COUPLE_FWD, False), (_lib.CONV_COUPLE_INV, True)):
            pair = None
            for persistent in (False, True):
                for store_hidden in ((False,) if persistent else (True, False)):    # sininn_conv_sub1_fwd never stores h
                    ctx = f'co {co} {b}x{h}x{w} {"sub1_fwd" if persistent else "pair_k1"} inverse {inverse} hidden {store_hidden} {regime} {pl}'
                    hid, out, y2, sb, ld = run(persistent, mode, store_hidden)
                    assert bool((out[:, co:] == SENTINEL).all()), f'channels outside the coupled half were written; {ctx}'
                    assert torch.equal(out[:, :co], y2), ctx
                    # the reference downstream of h uses the kernel's OWN stored h when there is one (a gate on the other side of 0
                    # within the budget of h is not an error of conv2)
                    if store_hidden:
                        if regime == 'int':
                            assert float(h_terms.max()) < EXACT_LIMIT
                            check_exact('h', hid, h_ref, ctx)
                        else:
                            check_budget('C', 'h', hid, h_ref, (co + 1 + 2) * U * h_terms, ctx)
                        h_used = hid.double()
                    else:
                        assert bool(torch.isnan(hid).all()), ctx
                        h_used = h_ref                  # the exact hidden tensor; its fp32 error is carried into the budget of s
                    r = h_used @ w2.t() + b2
                    r_terms = h_used.abs() @ w2.abs().t() + b2.abs()
                    s_ref, t_ref = r[:, :co], r[:, co:]
                    y_ref, L_ref, e_ref = glow_tail(s_ref, t_ref, v, clamp, inverse, torch.float64)
                    ld_ref = ld0.double() + (-1 if inverse else 1) * L_ref.reshape(b, -1).sum(1)
                    if regime == 'int':
                        assert float(r_terms.max()) * 4 < EXACT_LIMIT          # multiples of 1/4
                        check_exact('s', sb, s_ref, ctx)
                        y32, L32, _ = glow_tail(s_ref, t_ref, v, clamp, inverse, torch.float32)
                        scale = (v.abs() + t_ref.abs()) / e_ref if inverse else v.abs() * e_ref + t_ref.abs()
                        unit_y = float(((y32.double() - y_ref).abs() / scale.clamp_min(1e-30)).max())
                        unit_l = float(((L32.double() - L_ref).abs() / L_ref.abs().clamp_min(1e-30)).max())
                        print(f'[conv-fp32-sizes] part C units: y {unit_y:.3e} ({unit_y / U:.2f} u), L {unit_l:.3e} ({unit_l / U:.2f} u); {ctx}')
                        check_budget('C', 'y', out[:, :co], y_ref, 4 * unit_y * scale, ctx)
                        labs = L_ref.abs().reshape(b, -1).sum(1)
                        ld_budget = ((64 * co + pl['tiles_img'] + 1) * U + 4 * unit_l) * labs + U * ld_ref.abs()
                        check_budget('C', 'logdet', ld, ld_ref, ld_budget, ctx)
                    else:
                        carried = 0 if store_hidden else (co + 1 + 2) * U * (h_terms @ w2.abs().t())[:, :co]
                        check_budget('C', 's', sb, s_ref, (256 + 1 + 2) * U * r_terms[:, :co] + carried, ctx)
                    if not persistent and store_hidden:
                        pair = (out, sb)
                    elif not persistent or regime == 'int':
                        # the pair kernel without the stored h: bitwise the same launch; the persistent kernel sums in another
                        # order (1e-5 of the pair path in tests/test_gpu_kernels.py), so it is bitwise only where both are exact
                        assert torch.equal(sb, pair[1]), f's not bitwise the pair path; {ctx}'
                        if not persistent:
                            assert torch.equal(out, pair[0]), f'y not bitwise the pair path; {ctx}'


# =====================================================================================================================================
# B (non-linear tails). COUPLE_FWD / COUPLE_INV and ADD_CBWD_FWD / ADD_CBWD_INV through ops.conv, integer regime
# =====================================================================================================================================
CONV_ADD_CBWD_FWD, CONV_ADD_CBWD_INV = 9, 10          # SININN_CONV_ADD_CBWD_FWD / _INV (include/sininn.h)


def rel_unit(f32, f64, scale):
    """max over the tensor of |fp32 torch - float64| / scale: the relative unit of the formula's own fp32 evaluation"""
    return float(((f32.double() - f64).abs() / scale.clamp_min(1e-300)).max())


def _sparse_weight(gen, shape, density, dev):
    return make('int', gen, shape, -1, 1) * (torch.rand(shape, device=dev, generator=gen) < density) * 0.25


@pytest.mark.parametrize('family', ['direct3', 'direct1', 'wino'])
@pytest.mark.parametrize('shape', CONV_SHAPES, ids=lambda s: 'x'.join(map(str, s[:3])))
def test_conv_coupling_epilogues_at_size(shape, family):
    """The coupling epilogues of the direct and Winograd kernels at size, on integer operands (multiples of 1/4), so the s, t (and the
    data gradient g) the epilogue receives are exact and what is measured is its own fp32 arithmetic.
      COUPLE_FWD / COUPLE_INV on conv2 (256 -> 2 co, packed through ops.coupling_colmap): sbuf == s exactly; y (out and out2) at
        4 x the relative unit of the same formula in fp32 torch; log-det (+= onto non-zero values) at
        (256 co + partials per image) 2^-24 sum |L| + 4 unit_L sum |L|: a block sums at most 256 pixels x co channels and adds one atomic.
      ADD_CBWD_FWD / ADD_CBWD_INV on the data gradient of conv1 (256 -> co): g = dgrad + addend is exact; ds, dt, dv at 4 x their units.
    h, v, the outputs and the addend sit at channel offset 8 of wider tensors; outputs start as NaN; other channels stay untouched."""
    import sin_inn_amd  # noqa: F401
    from sin_inn_amd import _lib, ops
    lib = _lib.lib()
    dev = torch.device('cuda')
    b, h, w, level = shape
    m, clamp = b * h * w, 1.2
    co = LEVEL_CONVS[level][0][0]
    wino = family == 'wino'
    ksize = 1 if family == 'direct1' else 3
    taps = ksize * ksize
    hooks = [(cg, 0) for cg in WINO_HOOKS] if wino else [(0, 0), (1, 0), (2, 0), (0, 8)]
    gen = torch.Generator(device='cuda').manual_seed(17 * co + ksize + b + h)
    # ---- COUPLE: conv2 -------------------------------------------------------------------------------------------------------------------
    w2 = _sparse_weight(gen, (2 * co, 256, ksize, ksize), 0.02 / taps, dev)
    b2 = make('int', gen, (2 * co,), -1, 1) * 0.25
    pk2 = ops.pack_conv(w2.contiguous(), b2, ops.coupling_colmap(co, dev), False, wino_fwd=wino)
    hf = make('int', gen, (m, 256 + 16), 0, 2)
    vf = make('int', gen, (m, co + 16)) * 0.5
    ld0 = make('int', gen, (b,), -3, 3)
    hh, v = view_nhwc(hf, b, h, w, 8, 256), vf[:, 8:8 + co].double()
    r = ref_conv(hh, w2, b2).reshape(m, 2 * co)
    r_terms = (wino_abs_conv(hh, w2) if wino else ref_conv(hh.abs(), w2.abs())).reshape(m, 2 * co) + b2.abs().double()
    assert float(r_terms.max()) * 4 < EXACT_LIMIT
    s_ref, t_ref = r[:, :co], r[:, co:]
    # every block adds ONE atomic per image; the smallest pixel tile of any kernel here is 4 x 16 and the narrowest column block 32 packed
    # columns, so this bounds the partial sums per image of whichever kernel the plan below names
    partials = -(-h // 4) * -(-w // 16) * -(-2 * co // 32)
    tile = ops.coupling_tile(co)
    for cfg, ck in hooks:
        for mode, inverse in ((_lib.CONV_COUPLE_FWD, False), (_lib.CONV_COUPLE_INV, True)):
            pl = wino_plan(256, 2 * co, b, h, w, cfg, tile) if wino else conv_plan(256, 2 * co, ksize, cfg, ck)
            if wino:                                       # 2 co = 48 / 192 packed columns: an even number of 32-column groups
                want = {0: 'wino64', 2: 'wino64', 5: 'wino', 9: 'wino32' if tile == 16 else 'wino'}       # cg 1: 32-column blocks, either
                assert pl['kernel'] == want.get(cfg, pl['kernel']) and pl['kernel'] != ('wino64' if cfg == 1 else '') and pl['blocks'] >= 24, (pl, cfg)
            else:
                assert pl['K'] == 256 * taps and pl['chunks'] == 256 // pl['CK'], pl
            if ck:
                assert pl['CK'] == ck and pl['chunks'] >= 2, pl
            ctx = f'{family} couple inverse {inverse} 256->{2 * co} {b}x{h}x{w} hooks ({cfg}, {ck}) plan {pl}'
            out = torch.full((m, co + 16), SENTINEL, device=dev)
            out[:, 8:8 + co] = float('nan')
            y2 = torch.full((m, co + 16), SENTINEL, device=dev)
            y2[:, 8:8 + co] = float('nan')
            sb = torch.full((m, co), float('nan'), device=dev)
            ld = ld0.clone()
            lib.sininn_conv_test_hooks(cfg, ck)
            try:
                ops.conv(in_=ops.ptr(hf, 8), in_stride=256 + 16, Cin=256, w=ops.ptr(pk2[0]), bias=ops.ptr(pk2[1]), Np=2 * co,
                         winograd=int(wino), B=b, H=h, W=w, ksize=ksize, mode=mode, out=ops.ptr(out, 8), out_stride=co + 16,
                         v=ops.ptr(vf, 8), v_stride=co + 16, sbuf=ops.ptr(sb), logdet=ops.ptr(ld), Co=co, clamp=clamp,
                         out2=ops.ptr(y2, 8), out2_stride=co + 16, col_tile=ops.coupling_tile(co))
                torch.cuda.synchronize()
            finally:
                lib.sininn_conv_test_hooks(0, 0)
            for t in (out, y2):
                assert bool((t[:, :8] == SENTINEL).all()) and bool((t[:, 8 + co:] == SENTINEL).all()), f'channels outside written; {ctx}'
            assert torch.equal(out[:, 8:8 + co], y2[:, 8:8 + co]), ctx
            check_exact('s', sb, s_ref, ctx)
            y_ref, L_ref, e_ref = glow_tail(s_ref, t_ref, v, clamp, inverse, torch.float64)
            y32, L32, _ = glow_tail(s_ref, t_ref, v, clamp, inverse, torch.float32)
            scale = (v.abs() + t_ref.abs()) / e_ref if inverse else v.abs() * e_ref + t_ref.abs()
            unit_y, unit_l = rel_unit(y32, y_ref, scale), rel_unit(L32, L_ref, L_ref.abs())
            print(f'[conv-fp32-sizes] part B units: y {unit_y / U:.2f} u, L {unit_l / U:.2f} u; {ctx}')
            check_budget('B', f'{family} couple y', out[:, 8:8 + co], y_ref, 4 * unit_y * scale, ctx)
            ld_ref = ld0.double() + (-1 if inverse else 1) * L_ref.reshape(b, -1).sum(1)
            labs = L_ref.abs().reshape(b, -1).sum(1)
            check_budget('B', f'{family} couple logdet', ld, ld_ref, ((256 * co + partials + 1) * U + 4 * unit_l) * labs + U * ld_ref.abs(), ctx)
    # ---- ADD_CBWD: the data gradient of conv1 (co -> 256) with the fused coupling backward -------------------------------------------------
    w1 = _sparse_weight(gen, (256, co, ksize, ksize), 0.05 / taps, dev) * 4          # integers
    pk1 = ops.pack_conv(w1.contiguous(), torch.zeros(256, device=dev), None, True, wino_fwd=wino, wino_dgrad=wino)
    npk = ops.pad32(co) if wino else ops.pad16(co)
    dhf = make('int', gen, (m, 256 + 16))
    addf = make('int', gen, (m, co + 16))
    uf = torch.randn((m, co + 16), device=dev, generator=gen)
    sbuf = torch.randn((m, co), device=dev, generator=gen)
    gld = torch.randn((b,), device=dev, generator=gen)
    dh = view_nhwc(dhf, b, h, w, 8, 256)
    g = ref_dgrad(dh, w1).reshape(m, co) + addf[:, 8:8 + co].double()
    g_terms = (wino_abs_conv(dh, flip_weight(w1)) if wino else ref_dgrad(dh.abs(), w1.abs())).reshape(m, co) + addf[:, 8:8 + co].abs().double()
    assert float(g_terms.max()) * 4 < EXACT_LIMIT

    def cbwd(dtype, inverse):
        gg, s, u = g.to(dtype), sbuf.to(dtype), uf[:, 8:8 + co].to(dtype)
        gl = gld.to(dtype).repeat_interleave(h * w)[:, None]
        L = clamp * 0.636 * torch.atan(s / clamp)
        dL = 0.636 / (1 + (s / clamp) ** 2)
        e = torch.exp(L)
        if inverse:
            dv = gg / e
            return -(gg * u + gl) * dL, -dv, dv, ((gg * u).abs() + gl.abs()) * dL, dv.abs(), dv.abs()
        return (gg * u * e + gl) * dL, gg, gg * e, ((gg * u * e).abs() + gl.abs()) * dL, gg.abs(), (gg * e).abs()

    for cfg, ck in hooks:
        for mode, inverse in ((CONV_ADD_CBWD_FWD, False), (CONV_ADD_CBWD_INV, True)):
            pl = wino_plan(256, npk, b, h, w, cfg) if wino else conv_plan(256, npk, ksize, cfg, ck)
            if wino and cfg in (5, 9):
                assert pl['kernel'] == ('wino32' if cfg == 9 else 'wino'), pl
            if ck:
                assert pl['CK'] == ck and pl['chunks'] >= 2, pl
            ctx = f'{family} add_cbwd inverse {inverse} 256->{co} {b}x{h}x{w} hooks ({cfg}, {ck}) plan {pl}'
            out = torch.full((m, 2 * co + 16), SENTINEL, device=dev)
            out[:, 8:8 + 2 * co] = float('nan')
            dv = torch.full((m, co + 16), SENTINEL, device=dev)
            dv[:, 8:8 + co] = float('nan')
            lib.sininn_conv_test_hooks(cfg, ck)
            try:
                ops.conv(in_=ops.ptr(dhf, 8), in_stride=256 + 16, Cin=256, w=ops.ptr(pk1[2]), Np=npk, winograd=int(wino), B=b, H=h, W=w,
                         ksize=ksize, mode=mode, out=ops.ptr(out, 8), out_stride=2 * co + 16, N=co, addend=ops.ptr(addf, 8),
                         addend_stride=co + 16, v=ops.ptr(uf, 8), v_stride=co + 16, sbuf=ops.ptr(sbuf), out2=ops.ptr(dv, 8),
                         out2_stride=co + 16, logdet=ops.ptr(gld), Co=co, clamp=clamp)
                torch.cuda.synchronize()
            finally:
                lib.sininn_conv_test_hooks(0, 0)
            assert bool((out[:, :8] == SENTINEL).all()) and bool((out[:, 8 + 2 * co:] == SENTINEL).all()), f'channels outside written; {ctx}'
            assert bool((dv[:, :8] == SENTINEL).all()) and bool((dv[:, 8 + co:] == SENTINEL).all()), f'channels outside written; {ctx}'
            ref = cbwd(torch.float64, inverse)
            f32 = cbwd(torch.float32, inverse)
            for i, (name, got) in enumerate((('ds', out[:, 8:8 + co]), ('dt', out[:, 8 + co:8 + 2 * co]), ('dv', dv[:, 8:8 + co]))):
                unit = rel_unit(f32[i], ref[i], ref[3 + i])
                print(f'[conv-fp32-sizes] part B units: {name} {unit / U:.2f} u; {ctx}')
                if unit == 0:
                    check_exact(name, got, ref[i], ctx)
                else:
                    check_budget('B', f'{family} cbwd {name}', got, ref[i], 4 * unit * ref[3 + i], ctx)


# =====================================================================================================================================
# C (backward). the data-gradient pair of sininn_conv_pair_k1 and the persistent sininn_conv_sub1_bwd, integer regime
# =====================================================================================================================================
@pytest.mark.parametrize('no_dx', [False, True])
@pytest.mark.parametrize('co', [8, 16, 24])
@pytest.mark.parametrize('shape,many', SUB1_SHAPES, ids=lambda v: 'x'.join(map(str, v)) if isinstance(v, tuple) else str(v))
def test_fused_1x1_backward_exact_on_integers(shape, many, co, no_dx):
    """From real nn.Conv2d weights (set to small integers) packed with ops.pack_conv / ops.coupling_colmap: h of the forward pair, dh and dx
    of the data-gradient pair (MASK by the stored h, then ADD), and dx, gw2, gb2, gw1, gb1 of sininn_conv_sub1_bwd (h recomputed, dh on
    chip, gradients += onto non-zero integers, NaN workspace) all EQUAL float64; dx of the persistent kernel stays bitwise the pair's."""
    import sin_inn_amd  # noqa: F401
    from sin_inn_amd import _lib, ops
    lib = _lib.lib()
    dev = torch.device('cuda')
    b, h, w = shape
    k1, k2, m = co, 2 * co, b * h * w
    pl = sub1_fwd_plan(b, h, w)                          # conv_sub1.hip: the backward kernel walks the same 16 x 4 tiles on min(ntiles, 256) blocks
    assert pl['blocks'] == min(pl['ntiles'], S1_MAX_BLOCKS)
    assert (pl['max_tiles_per_block'] >= 2) == many, pl
    ctx = f'co {co} {b}x{h}x{w} no_dx {no_dx} {pl}'
    gen = torch.Generator(device='cuda').manual_seed(9 * co + b + h)
    cx = 2 * co + 16                                     # x: channels [8, 8 + co) of a wider tensor
    xfull = make('int', gen, (m, cx))
    conv1 = torch.nn.Conv2d(k1, 256, 1).to(dev)
    conv2 = torch.nn.Conv2d(256, k2, 1).to(dev)
    with torch.no_grad():
        conv1.weight.copy_(make('int', gen, (256, k1, 1, 1), -1, 1))
        conv1.bias.copy_(make('int', gen, (256,), -1, 1))
        conv2.weight.copy_(make('int', gen, (k2, 256, 1, 1), -1, 1) * (torch.rand((k2, 256, 1, 1), device=dev, generator=gen) < 0.1))
        conv2.bias.zero_()
    pk1 = ops.pack_conv(conv1.weight.detach().contiguous(), conv1.bias.detach().contiguous(), None, True)
    pk2 = ops.pack_conv(conv2.weight.detach().contiguous(), conv2.bias.detach().contiguous(), ops.coupling_colmap(co, dev), True)
    dr = make('int', gen, (m, k2))
    addend = make('int', gen, (m, k1))

    def args(**kw):
        a = _lib.ConvArgs()
        for k, val in kw.items():
            setattr(a, 'inp' if k == 'in_' else k, val)
        return a
    common = dict(B=b, H=h, W=w, ksize=1)
    # ---- float64 ---------------------------------------------------------------------------------------------------------------------------
    x = xfull[:, 8:8 + k1].double()
    w1, b1 = conv1.weight.detach().reshape(256, k1).double(), conv1.bias.detach().double()
    w2 = conv2.weight.detach().reshape(k2, 256).double()
    h_ref = torch.relu(x @ w1.t() + b1)
    drd = dr.double()
    dh_ref = (drd @ w2) * (h_ref > 0)
    dx_ref = dh_ref @ w1 + addend.double()
    g0 = [make('int', gen, (k2, 256, 1, 1), -3, 3), make('int', gen, (k2,), -3, 3), make('int', gen, (256, k1, 1, 1), -3, 3),
          make('int', gen, (256,), -3, 3)]
    want = [g0[0].double() + (drd.t() @ h_ref).reshape(k2, 256, 1, 1), g0[1].double() + drd.sum(0),
            g0[2].double() + (dh_ref.t() @ x).reshape(256, k1, 1, 1), g0[3].double() + dh_ref.sum(0)]
    tops = [float((drd.abs().t() @ h_ref).max()), float(drd.abs().sum(0).max()), float((dh_ref.abs().t() @ x.abs()).max()),
            float(dh_ref.abs().sum(0).max()), float((dh_ref.abs() @ w1.abs()).max())]
    assert max(tops) + 4 < EXACT_LIMIT, (tops, ctx)
    # ---- the h of the forward pair, then the data-gradient pair ----------------------------------------------------------------------------
    hid = torch.full((m, 256), float('nan'), device=dev)
    dump = torch.full((m, k2), float('nan'), device=dev)
    f = args(in_=ops.ptr(xfull, 8), in_stride=cx, Cin=k1, w=ops.ptr(pk1[0]), bias=ops.ptr(pk1[1]), Np=256, mode=_lib.CONV_RELU,
             out=ops.ptr(hid), out_stride=256, N=256, **common)
    s2 = args(in_=ops.ptr(hid), in_stride=256, Cin=256, w=ops.ptr(pk2[0]), bias=ops.ptr(pk2[1]), Np=k2, mode=_lib.CONV_LINEAR,
              out=ops.ptr(dump), out_stride=k2, N=k2, **common)
    _lib.check(lib.sininn_conv_pair_k1(C.byref(f), C.byref(s2), ops._stream()))
    torch.cuda.synchronize()
    check_exact('h', hid, h_ref, ctx)

    def dgrad_descs(dx, dh):
        d2 = args(in_=ops.ptr(dr), in_stride=k2, Cin=k2, w=ops.ptr(pk2[2]), Np=256, mode=_lib.CONV_MASK, out=ops.ptr(dh), out_stride=256,
                  N=256, mask=ops.ptr(hid), mask_stride=256, **common)
        d1 = args(in_=ops.ptr(dh), in_stride=256, Cin=256, w=ops.ptr(pk1[2]), Np=ops.pad16(k1), mode=_lib.CONV_ADD, out=ops.ptr(dx),
                  out_stride=k1, N=k1, addend=ops.ptr(addend), addend_stride=k1, **common)
        return d2, d1
    dx_pair = torch.full((m, k1), float('nan'), device=dev)
    dh_pair = torch.full((m, 256), float('nan'), device=dev)
    d2, d1 = dgrad_descs(dx_pair, dh_pair)
    assert lib.sininn_conv_pair_k1_supported(C.byref(d2), C.byref(d1)) == 1
    _lib.check(lib.sininn_conv_pair_k1(C.byref(d2), C.byref(d1), ops._stream()))
    torch.cuda.synchronize()
    check_exact('dh (pair)', dh_pair, dh_ref, ctx)
    check_exact('dx (pair)', dx_pair, dx_ref, ctx)
    # ---- the persistent backward ---------------------------------------------------------------------------------------------------------------
    gw2, gb2, gw1, gb1 = (t.clone().contiguous() for t in g0)
    dx = torch.full((m, k1), float('nan'), device=dev)
    rc = args(in_=ops.ptr(xfull, 8), in_stride=cx, Cin=k1, w=ops.ptr(pk1[0]), bias=ops.ptr(pk1[1]), Np=256, **common)
    d2f, d1f = dgrad_descs(dx, dh_pair)
    d2f.mask, d2f.out, d1f.inp = None, None, None      # ignored by the fused kernel: h is recomputed, dh stays on chip
    nbytes = lib.sininn_conv_sub1_bwd_workspace_bytes(k1, co)
    assert nbytes > 0
    ws = torch.full((nbytes // 4,), float('nan'), device=dev)
    _lib.check(lib.sininn_conv_sub1_bwd(C.byref(rc), C.byref(d2f), C.byref(d1f), int(no_dx), ops.ptr(gw2), ops.ptr(gb2), ops.ptr(gw1),
                                        ops.ptr(gb1), ops.ptr(ws), nbytes, ops._stream()))
    torch.cuda.synchronize()
    if no_dx:
        assert bool(torch.isnan(dx).all()), ctx
    else:
        assert torch.equal(dx, dx_pair), f'dx not bitwise the pair path; {ctx}'
        check_exact('dx', dx, dx_ref, ctx)
    for name, got, ref_ in zip(('gw2', 'gb2', 'gw1', 'gb1'), (gw2, gb2, gw1, gb1), want):
        check_exact(name, got, ref_, ctx)
