"""GPU: the mixed-precision (bf16) backward kernels at production tile counts, against float64.

The tight tests of tests/test_gpu_bf16.py and tests/test_gpu_irn_bf16.py run at shapes where every persistent block and every
split-K split handles ONE pixel tile.  Here the same kernels run at the sizes of BASELINE configs[3] (512x512, batch 16) and
configs[4] (1280x720), where a block or split walks many tiles: the next-tile prefetch, the double-buffered staging, the
accumulation across tiles and a short last split all run.  Every test computes the launch plan from the formulas of the kernel
source and asserts that its shape really gives more than one tile per block / split, so a planner change cannot quietly turn it
back into a one-tile test.

Every check compares with float64 arithmetic on the SAME bf16-rounded operands (round to nearest even, as bf() does), rounded
again exactly where the kernel stores or stages a bf16 value.  What remains is fp32 accumulation order.  Budgets (those the
small-shape tests state):
  * fp32 results, weight and bias gradients: 1e-4 of the max-norm;
  * fp32 tensors computed from a bf16 value the kernel rounded itself (dh -> dx): 2e-3 of the max-norm and 2e-5 in L2 -- a sum
    on a bf16 rounding boundary lands one ulp away from the reference's rounding;
  * bf16 outputs: at most one bf16 ulp from the reference's rounding, in fewer than 1e-3 of the elements (ReLU gates: see part C).
A truncating fp32 -> bf16 conversion, or one dropped tile per split / slab, is a biased error of ~2^-9 of the result and fails
these budgets; the network-level budgets (1e-2 .. 5e-2 L2) would not see it.

The references are per-image, per-tap float64 matmuls on the CPU (no unfold over the batch: GBs at these sizes)."""
import ctypes as C
import os
import sys

import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, 'tests'))

BF = torch.bfloat16


@pytest.fixture(autouse=True)
def _threads():
    old = torch.get_num_threads()
    torch.set_num_threads(16)
    yield
    torch.set_num_threads(old)


def relerr(a, b):
    a, b = a.detach().double().cpu(), b.detach().double().cpu()
    return float((a - b).abs().max() / b.abs().max().clamp_min(1e-30))


def rel_l2(a, b):
    a, b = a.detach().double().cpu(), b.detach().double().cpu()
    return float((a - b).norm() / b.norm().clamp_min(1e-30))


def bf(t):
    """round to bf16 (nearest even) and back to t's dtype"""
    return t.to(BF).to(t.dtype)


def bf_of(t64):
    """the bf16 value a kernel stores for a float64 reference value: the fp32 sum, rounded once"""
    return t64.float().to(BF)


def close(got, ref):
    return relerr(got, ref) < 2e-3 and rel_l2(got, ref) < 2e-5


def acc_bound(k, abs_sum):
    """worst-case difference of an fp32 sum of k products from the exact one: (k + 1) 2^-24 sum |terms| (the products of bf16
    values are exact in fp32)"""
    return (k + 1) * 2.0 ** -24 * abs_sum


def ulp_violations(got, ref64, slack, exempt=None):
    """(elements further than one bf16 ulp + `slack` from the reference's rounding, fraction of elements that differ at all).
    slack = acc_bound of the rounded sum: where the exact sum cancels to far below its terms, the fp32 accumulation error alone
    can exceed one ulp of the result.  `exempt` masks elements excluded from both counts."""
    rb = bf_of(ref64).double()
    d = (got.detach().cpu().double() - rb).abs()
    _, e = torch.frexp(rb)
    ulp = torch.where(rb != 0, torch.ldexp(torch.ones_like(rb), e - 8), torch.zeros_like(rb))
    bad, off = d > ulp + slack, d > 0
    if exempt is not None:
        bad, off = bad & ~exempt, off & ~exempt
    return int(bad.sum()), float(off.double().mean())


def nhwc_cpu(t, b, h, w, c0=0, c=None):
    """[B*H*W][stride] device tensor (optionally a channel range) -> [B,H,W,c] CPU"""
    c = t.shape[1] - c0 if c is None else c
    return t[:, c0:c0 + c].cpu().reshape(b, h, w, c)


# ---- float64 references, one image and one tap at a time: tests/float64_refs.py --------------------------------------------------
from float64_refs import ref_conv, ref_dgrad, ref_wgrad  # noqa: E402


def args(**kw):
    from sin_inn_amd import _lib
    a = _lib.ConvArgs()
    for k, v in kw.items():
        setattr(a, 'inp' if k == 'in_' else k, v)
    return a


# =====================================================================================================================================
# A. bf16 grouped weight gradient (wgrad_bf16_group_kernel, csrc/wgrad_mfma.hip) through ops.wgrad_group
# =====================================================================================================================================
def wgrad_group_plan(items, B, H, W, target_blocks=512):
    """plan_group (csrc/wgrad_mfma.hip) for a group on the bf16 matrix pipe: 8 x 16 pixel tiles (pl.th = 8); a problem's blocks are
    128 n x 32 c when Cin <= 32 and N >= 128 (narrow_c), else 64 x 64; S = 512 / out_tiles splits, clipped to [1, ntiles];
    tiles_per_split = ceil(ntiles / S), then S = ceil(ntiles / tiles_per_split).  items: (Cin, N)."""
    ntiles = B * -(-W // 16) * -(-H // 8)
    out_tiles = 0
    for cin, n in items:
        bn, bc = (128, 32) if (cin <= 32 and n >= 128) else (64, 64)
        out_tiles += -(-n // bn) * -(-cin // bc)
    S = min(max(target_blocks // out_tiles, 1), ntiles)
    tps = -(-ntiles // S)
    S = -(-ntiles // tps)
    return dict(ntiles=ntiles, S=S, tiles_per_split=tps, last=ntiles - (S - 1) * tps)


# the two subnets of a GLOW block: conv2's gradient reads h (bf16) and dr (fp32, rounded while staged), conv1's reads the block's
# fp32 input and dh (bf16).  Level 0 (SRF, configs[3] / [4]): 24 -> 256 -> 48; level 1: 96 -> 256 -> 192.
LEVEL_PROBLEMS = {0: [(256, 48, True, False), (24, 256, False, True)] * 2,
                  1: [(256, 192, True, False), (96, 256, False, True)] * 2}
WGRAD_SHAPES = [                # short: ntiles % tiles_per_split != 0, the last split's t_end is clipped
    (0, 3, (16, 128, 128), True),      # configs[3] level 0: 42 splits of 49 tiles, the last holds 39
    (0, 1, (16, 128, 128), True),
    (0, 3, (1, 180, 320), True),       # configs[4] level 0: 180 rows are not a multiple of 8 (a half-empty tile row); 42 x 11, last 9
    (0, 1, (1, 180, 320), True),
    (1, 3, (16, 64, 64), True),        # configs[3] level 1: 12 splits of 43 tiles, the last holds 39
    (1, 1, (16, 64, 64), True),
    (1, 3, (1, 90, 160), False),       # configs[4] level 1: 12 splits of 10 tiles
    (1, 1, (1, 90, 160), False),
    (0, 3, (1, 75, 150), True),        # ragged in x and y: 34 splits of 3 tiles, the last holds ONE
]


@pytest.mark.parametrize('level,ksize,shape,short', WGRAD_SHAPES)
def test_wgrad_group_bf16_many_tiles_per_split(level, ksize, shape, short):
    """The four weight gradients of a GLOW block as ONE mixed group (both block shapes of the bf16 kernel: 64 n x 64 c and, for
    conv1 with Cin <= 32, 128 n x 32 c), operands strided inside wider tensors at a channel offset, gradients starting from non-zero
    values (+=), a second run bitwise identical.  Reference: float64 on the bf16-rounded operands (gw from bf16 x bf16 products, gb
    from the bf16-rounded output gradient the kernel sums)."""
    import sin_inn_amd  # noqa: F401
    from sin_inn_amd import ops
    b, h, w = shape
    m = b * h * w
    dev = torch.device('cuda')
    probs = LEVEL_PROBLEMS[level]
    plan = wgrad_group_plan([(cin, n) for cin, n, _, _ in probs], b, h, w)
    assert plan['tiles_per_split'] >= 2, plan                       # the next-tile prefetch and cross-tile accumulation run
    assert (plan['last'] < plan['tiles_per_split']) == short, plan
    g = torch.Generator(device=dev).manual_seed(100 * level + 10 * ksize + b)
    items, refs = [], []
    for cin, n, in_b, dout_b in probs:
        # operands live inside wider tensors: channel offset 8 (16-byte aligned for bf16 and fp32), 8 spare channels after
        in_full = torch.randn(m, cin + 16, device=dev, generator=g)
        dout_full = torch.randn(m, n + 16, device=dev, generator=g)
        in_t = in_full.to(BF) if in_b else in_full
        dout_t = dout_full.to(BF) if dout_b else dout_full
        gw0 = torch.randn(n, cin, ksize, ksize, device=dev, generator=g)
        gb0 = torch.randn(n, device=dev, generator=g)
        gw, gb = gw0.clone(), gb0.clone()
        items.append((in_t, 8, cin + 16, cin, dout_t, 8, n + 16, n, gw, gb, in_b, dout_b))
        refs.append((in_t, dout_t, cin, n, gw0, gb0, gw, gb))
    ops.wgrad_group(items, b, h, w, ksize)
    torch.cuda.synchronize()
    first = [(gw.clone(), gb.clone()) for *_, gw, gb in refs]
    for (in_t, dout_t, cin, n, gw0, gb0, gw, gb) in refs:
        xin = bf(nhwc_cpu(in_t, b, h, w, 8, cin).float())
        dout = bf(nhwc_cpu(dout_t, b, h, w, 8, n).float())
        gw_ref = ref_wgrad(xin, dout, ksize)
        gb_ref = dout.double().sum((0, 1, 2))
        dgw = gw.cpu().double() - gw0.cpu().double()
        dgb = gb.cpu().double() - gb0.cpu().double()
        assert relerr(dgw, gw_ref) < 1e-4, ('gw', cin, n, relerr(dgw, gw_ref), plan)
        assert relerr(dgb, gb_ref) < 1e-4, ('gb', cin, n, relerr(dgb, gb_ref), plan)
    # same inputs, same starting values: bitwise the same result (every slab summed in split order)
    for (*_, gw0, gb0, gw, gb) in refs:
        gw.copy_(gw0)
        gb.copy_(gb0)
    ops.wgrad_group(items, b, h, w, ksize)
    torch.cuda.synchronize()
    for (gw_a, gb_a), (*_, gw, gb) in zip(first, refs):
        assert torch.equal(gw_a, gw) and torch.equal(gb_a, gb)


# =====================================================================================================================================
# B. level-1 fused bf16 backward with its weight-gradient riders (conv_sub1_bf16.hip: conv_sub1b_wide_bwd_kernel<.., true> +
#    wide_reduce_kernel; conv_sub1b_wide_wg2_kernel + wide_reduce2_kernel) through sininn_conv_sub1_wide_bwd / _wg2
# =====================================================================================================================================
S1_MAX_BLOCKS = 256                    # conv_sub1_types.h: persistent blocks (= slabs)


def wide_plan(b, h, w):
    """conv_sub1_bf16.hip: 16 x 2 pixel tiles, tiles_x = ceil(W / 16), tiles_y = ceil(H / 2); min(ntiles, 256) persistent blocks,
    block g takes tiles g, g + G, ..."""
    ntiles = b * -(-w // 16) * -(-h // 2)
    blocks = min(ntiles, S1_MAX_BLOCKS)
    return dict(ntiles=ntiles, blocks=blocks, max_tiles_per_block=-(-ntiles // blocks))


@pytest.mark.parametrize('epilogue', ['add', 'cbwd_fwd', 'cbwd_inv'])
@pytest.mark.parametrize('shape', [(16, 64, 64), (1, 90, 160), (2, 19, 40)])    # 2 048 and 450 tiles; 60 tiles (one per block) as control
def test_wide_1x1_backward_with_riders(shape, epilogue):
    """The executor's level-1 1x1 backward on the mixed-precision path: dh = (dr W2) . [h > 0] (bf16), dx = dh W1 through the ADD or the
    fused coupling-backward epilogue, gw1 / gb1 += from the rider's slabs, and gw2 / gb2 += from the conv2 rider.  Reference math as
    test_fused_1x1_subnet_bf16_c_abi (tests/test_gpu_bf16.py); dr / x / weights rounded to bf16, h bf16 as stored, db2 summed from
    the fp32 dr.  Run once with dh stored (checked with the ulp rule) and once without (the executor's call): bitwise the same
    dx and gradients."""
    import sin_inn_amd  # noqa: F401
    from sin_inn_amd import _lib, ops
    lib = _lib.lib()
    dev = torch.device('cuda')
    b, h, w = shape
    m = b * h * w
    plan = wide_plan(b, h, w)
    if shape != (2, 19, 40):
        assert plan['ntiles'] > plan['blocks'] and plan['max_tiles_per_block'] >= 2, plan
    else:
        assert plan['max_tiles_per_block'] == 1, plan
    co, k1, k2, hid_c = 96, 96, 192, 256
    g = torch.Generator(device=dev).manual_seed(7 * b + h)
    conv1_w = torch.randn(hid_c, k1, 1, 1, device=dev, generator=g) * k1 ** -0.5
    conv1_b = torch.randn(hid_c, device=dev, generator=g) * 0.1
    conv2_w = torch.randn(k2, hid_c, 1, 1, device=dev, generator=g) * 0.3 * hid_c ** -0.5
    conv2_b = torch.randn(k2, device=dev, generator=g) * 0.1
    pk1 = ops.pack_conv_bf16(conv1_w, conv1_b, None, True)
    pk2 = ops.pack_conv_bf16(conv2_w, conv2_b, ops.coupling_colmap(co, dev), True)
    pb = lambda t: ops.ptr(t, dtype=BF)
    cx = k1 + 2 * co                                              # x: channels [8, 8 + 96) of a wider tensor (cond_stride)
    xfull = torch.randn(m, cx, device=dev, generator=g)
    hmask = torch.relu(torch.randn(m, hid_c, device=dev, generator=g)).to(BF)     # the stored h: ~half the gates closed
    dr = torch.randn(m, k2, device=dev, generator=g)
    addend = torch.randn(m, k1, device=dev, generator=g)
    vy = torch.randn(m, co, device=dev, generator=g)
    sb = torch.randn(m, co, device=dev, generator=g)
    gld = torch.randn(b, device=dev, generator=g)
    clamp = 1.2
    common = dict(B=b, H=h, W=w, ksize=1, w_bf16=1)
    g0 = [torch.randn(k2, hid_c, 1, 1, device=dev, generator=g), torch.randn(k2, device=dev, generator=g),
          torch.randn(hid_c, k1, 1, 1, device=dev, generator=g), torch.randn(hid_c, device=dev, generator=g)]

    def run(store_dh):
        dh = torch.full((m, hid_c), float('nan'), device=dev, dtype=BF)
        out = torch.full((m, 2 * k1 if epilogue != 'add' else k1), float('nan'), device=dev)
        out2 = torch.full((m, co), float('nan'), device=dev)
        gw2, gb2, gw1, gb1 = (t.clone() for t in g0)
        d2 = args(in_=ops.ptr(dr), in_stride=k2, Cin=k2, w=pb(pk2[2]), Np=hid_c, mode=_lib.CONV_MASK, out=pb(dh) if store_dh else None,
                  out_stride=hid_c, N=hid_c, mask=pb(hmask), mask_stride=hid_c, out_bf16=1, mask_bf16=1, **common)
        d1 = args(in_stride=hid_c, Cin=hid_c, w=pb(pk1[2]), Np=ops.pad16(k1), mode=_lib.CONV_ADD, out=ops.ptr(out), out_stride=k1, N=k1,
                  addend=ops.ptr(addend), addend_stride=k1, in_bf16=1, **common)
        if epilogue != 'add':
            d1.mode = 9 if epilogue == 'cbwd_fwd' else 10                 # SININN_CONV_ADD_CBWD_FWD / _INV
            d1.out_stride = 2 * k1
            d1.v, d1.v_stride, d1.sbuf = ops.ptr(vy), co, ops.ptr(sb)
            d1.out2, d1.out2_stride, d1.logdet, d1.Co, d1.clamp = ops.ptr(out2), co, ops.ptr(gld), co, clamp
        nb1 = lib.sininn_conv_sub1_wide_bwd_workspace_bytes(k1, co)
        nb2 = lib.sininn_conv_sub1_wide_wg2_workspace_bytes(k1, co)
        assert nb1 > 0 and nb2 > 0
        ws1 = torch.empty(nb1 // 4, device=dev)
        ws2 = torch.empty(nb2 // 4, device=dev)
        _lib.check(lib.sininn_conv_sub1_wide_bwd(C.byref(d2), C.byref(d1), ops.ptr(xfull, 8), cx, ops.ptr(gw1), ops.ptr(gb1),
                                                 ops.ptr(ws1), nb1, ops._stream()))
        _lib.check(lib.sininn_conv_sub1_wide_wg2(ops.ptr(dr), k2, pb(hmask), hid_c, b, h, w, ops.ptr(gw2), ops.ptr(gb2), ops.ptr(ws2), nb2,
                                                 ops._stream()))
        torch.cuda.synchronize()
        return dh, out, out2, gw2, gb2, gw1, gb1

    dh, out, out2, gw2, gb2, gw1, gb1 = run(True)
    # ---- reference (float64 on the bf16-rounded operands) --------------------------------------------------------------------------
    w1 = bf(conv1_w.reshape(hid_c, k1)).cpu().double()
    w2 = bf(conv2_w.reshape(k2, hid_c)).cpu().double()
    drc = dr.cpu()
    drb = bf(drc).double()
    hc = hmask.cpu().double()
    dh_pre = (drb @ w2) * (hc > 0)
    dh_ref = bf_of(dh_pre).double()                                # the bf16 dh the kernel keeps on chip
    xb = bf(xfull[:, 8:8 + k1].cpu()).double()
    g_ref = dh_ref @ w1 + addend.cpu().double()
    bad, frac = ulp_violations(dh, dh_pre, acc_bound(k2, (drb.abs() @ w2.abs()) * (hc > 0)))
    assert bad == 0 and frac < 1e-3, ('dh', bad, frac)
    if epilogue == 'add':
        assert close(out, g_ref), ('dx', relerr(out, g_ref), rel_l2(out, g_ref))
    else:
        s = sb.cpu().double()
        u = vy.cpu().double()
        gl = gld.cpu().double().repeat_interleave(h * w)[:, None]
        L = clamp * 0.636 * torch.atan(s / clamp)
        dL = 0.636 / (1 + (s / clamp) ** 2)
        e = torch.exp(L)
        if epilogue == 'cbwd_fwd':
            dv, dt, ds = g_ref * e, g_ref, (g_ref * u * e + gl) * dL
        else:
            dv = g_ref / e
            dt, ds = -dv, -(g_ref * u + gl) * dL
        for name, got, ref_ in (('ds', out[:, :k1], ds), ('dt', out[:, k1:], dt), ('dv', out2, dv)):
            assert close(got, ref_), (name, relerr(got, ref_), rel_l2(got, ref_))
    want = [(drb.t() @ hc).reshape(k2, hid_c, 1, 1), drc.double().sum(0), (dh_ref.t() @ xb).reshape(hid_c, k1, 1, 1), dh_ref.sum(0)]
    for name, got, g_start, ref_ in zip(('gw2', 'gb2', 'gw1', 'gb1'), (gw2, gb2, gw1, gb1), g0, want):
        d = got.cpu().double() - g_start.cpu().double()
        assert relerr(d, ref_) < 1e-4, (name, relerr(d, ref_), plan)
    # ---- the executor's call: dh not stored -- the same values, bitwise ----------------------------------------------------------------
    dh2, *rest = run(False)
    assert bool(torch.isnan(dh2.float()).all())
    for a_, b_ in zip((out, out2, gw2, gb2, gw1, gb1), rest):
        assert torch.equal(torch.nan_to_num(a_, 12345.0), torch.nan_to_num(b_, 12345.0))


def test_wide_1x1_backward_refuses_unsupported_pairs():
    """the new entry points return an error (not a silent no-op) for a descriptor pair the wide kernel does not serve"""
    import sin_inn_amd  # noqa: F401
    from sin_inn_amd import _lib, ops
    lib = _lib.lib()
    dev = torch.device('cuda')
    t = torch.zeros(64, 256, device=dev)
    d2 = args(in_=ops.ptr(t), in_stride=192, Cin=48, w=ops.ptr(t), Np=256, mode=_lib.CONV_MASK, out_stride=256, N=256, mask=ops.ptr(t),
              mask_stride=256, out_bf16=1, mask_bf16=1, B=1, H=8, W=8, ksize=1, w_bf16=1)
    d1 = args(in_stride=256, Cin=256, w=ops.ptr(t), Np=96, mode=_lib.CONV_ADD, out=ops.ptr(t), out_stride=96, N=96, addend=ops.ptr(t),
              addend_stride=96, in_bf16=1, B=1, H=8, W=8, ksize=1, w_bf16=1)
    nb = lib.sininn_conv_sub1_wide_bwd_workspace_bytes(96, 96)
    ws = torch.empty(nb // 4, device=dev)
    with pytest.raises(RuntimeError, match='unsupported'):
        _lib.check(lib.sininn_conv_sub1_wide_bwd(C.byref(d2), C.byref(d1), ops.ptr(t), 96, ops.ptr(t), None, ops.ptr(ws), nb, ops._stream()))
    assert lib.sininn_conv_sub1_wide_bwd_workspace_bytes(24, 24) == 0 and lib.sininn_conv_sub1_wide_wg2_workspace_bytes(24, 24) == 0
    assert lib.sininn_conv3_smallk_bits_supported(C.byref(d2)) == 0
    with pytest.raises(RuntimeError):
        _lib.check(lib.sininn_conv3_smallk_bits(C.byref(d2), ops.ptr(t, dtype=torch.float32), ops._stream()))


# =====================================================================================================================================
# C. small-K 3x3 kernel with ReLU gate bits (conv3_smallk_bf16.hip) through sininn_conv3_smallk_bits
# =====================================================================================================================================
C3K_MAX_BLOCKS = 256


def smallk_plan(b, h, w):
    """conv3_smallk_bf16.hip: 16 x 16 pixel tiles, min(ntiles, 256) persistent blocks, block g takes tiles g, g + G, ..."""
    tx, ty = -(-w // 16), -(-h // 16)
    ntiles = b * tx * ty
    blocks = min(ntiles, C3K_MAX_BLOCKS)
    return dict(tiles_x=tx, tiles_y=ty, ntiles=ntiles, blocks=blocks, max_tiles_per_block=-(-ntiles // blocks))


def decode_bits(bits, b, h, w):
    """gate words [tile][8 steps][256 columns] -> bool [B,H,W,256] (bit p of step m: tile row 2 m + p // 16, column p % 16)"""
    tx, ty = -(-w // 16), -(-h // 16)
    words = bits.view(b, ty, tx, 8, 256)
    shifts = torch.arange(32, device=bits.device, dtype=torch.int32)
    g = ((words.unsqueeze(-1) >> shifts) & 1).to(torch.bool)                        # [b,ty,tx,8,256,32]
    g = g.permute(0, 1, 2, 3, 5, 4).reshape(b, ty, tx, 16, 16, 256)                  # (m, p) -> (2 m + p // 16, p % 16)
    return g.permute(0, 1, 3, 2, 4, 5).reshape(b, ty * 16, tx * 16, 256)[:, :h, :w]


SMALLK_CASES = [(24, 48, (16, 128, 128)),                   # configs[3] level 0: 1 024 tiles, 4 per block
                (8, 16, (2, 180, 320)), (16, 32, (2, 180, 320)), (24, 48, (2, 180, 320)), (32, 16, (2, 180, 320))]   # 240 tiles / image


@pytest.mark.parametrize('cin,n2,shape', SMALLK_CASES)
def test_smallk_3x3_gate_bits_against_float64(cin, n2, shape):
    """conv1 (Cin -> 256, bias, ReLU, bf16 h) writing the gate bits, then the masked data gradient of conv2 (dr: n2 channels -> 256, bf16
    dh) reading them, as a training pass runs them.  Bits == (h > 0) of the same launch exactly; they agree with the sign of the
    float64 pre-activation except where |pre| is within the worst-case fp32 accumulation bound (K + 1) 2^-24 (sum |x w| + |b|),
    K = 9 Cin, and only there may h differ from the reference by more than one ulp (a gate on the other side).  dh against
    float64 on the same gates (the ones the bits hold)."""
    import sin_inn_amd  # noqa: F401
    from sin_inn_amd import _lib, ops
    lib = _lib.lib()
    dev = torch.device('cuda')
    b, h, w = shape
    m = b * h * w
    plan = smallk_plan(b, h, w)
    assert plan['ntiles'] > plan['blocks'] and plan['max_tiles_per_block'] >= 2, plan    # the double-buffered next-tile halo runs
    hid = 256
    g = torch.Generator(device=dev).manual_seed(cin * 1000 + n2 + b)
    w1 = torch.randn(hid, cin, 3, 3, device=dev, generator=g) * (9 * cin) ** -0.5
    b1 = torch.randn(hid, device=dev, generator=g) * 0.1
    w2 = torch.randn(n2, hid, 3, 3, device=dev, generator=g) * (9 * hid) ** -0.5
    pk1 = ops.pack_conv_bf16(w1, b1, None, True)
    pk2 = ops.pack_conv_bf16(w2, torch.zeros(n2, device=dev), None, True)
    pb = lambda t: ops.ptr(t, dtype=BF)
    xfull = torch.randn(m, cin + 8, device=dev, generator=g)           # x: channels [4, 4 + cin) of a wider tensor
    hs = torch.full((m, hid), float('nan'), device=dev, dtype=BF)
    bits = torch.zeros(plan['ntiles'] * 8 * hid, device=dev, dtype=torch.int32)
    common = dict(B=b, H=h, W=w, ksize=3, w_bf16=1)
    f1 = args(in_=ops.ptr(xfull, 4), in_stride=cin + 8, Cin=cin, w=pb(pk1[0]), bias=ops.ptr(pk1[1]), Np=hid, mode=_lib.CONV_RELU,
              out=pb(hs), out_stride=hid, N=hid, out_bf16=1, **common)
    assert lib.sininn_conv3_smallk_bits_supported(C.byref(f1)) == 1
    _lib.check(lib.sininn_conv3_smallk_bits(C.byref(f1), ops.ptr(bits, dtype=torch.int32), ops._stream()))
    torch.cuda.synchronize()
    gates = decode_bits(bits, b, h, w)
    hv = hs.view(b, h, w, hid)
    assert torch.equal(gates, hv > 0)                                  # the bits are the gates of the same launch, exactly
    # ---- conv1 against float64 ---------------------------------------------------------------------------------------------------------
    xb = bf(nhwc_cpu(xfull, b, h, w, 4, cin))
    w1b = bf(w1).cpu()
    pre = ref_conv(xb, w1b, b1.cpu())
    bound = acc_bound(9 * cin, ref_conv(xb.abs(), w1b.abs()) + b1.cpu().double().abs())
    near = pre.abs() <= bound
    gates_c = gates.cpu()
    assert bool(((gates_c == (pre > 0)) | near).all()), int(((gates_c != (pre > 0)) & ~near).sum())
    bad, frac = ulp_violations(hv, torch.relu(pre), bound, exempt=near)
    assert bad == 0 and frac < 1e-3, ('h', bad, frac, int(near.sum()))
    # ---- masked data gradient reading the bits ---------------------------------------------------------------------------------------------
    dr = torch.randn(m, n2, device=dev, generator=g)
    dh = torch.full((m, hid), float('nan'), device=dev, dtype=BF)
    d2 = args(in_=ops.ptr(dr), in_stride=n2, Cin=n2, w=pb(pk2[2]), Np=hid, mode=_lib.CONV_MASK, out=pb(dh), out_stride=hid, N=hid,
              mask=pb(hs), mask_stride=hid, out_bf16=1, mask_bf16=1, **common)
    assert lib.sininn_conv3_smallk_bits_supported(C.byref(d2)) == 1
    _lib.check(lib.sininn_conv3_smallk_bits(C.byref(d2), ops.ptr(bits, dtype=torch.int32), ops._stream()))
    torch.cuda.synchronize()
    drb = bf(dr.cpu()).reshape(b, h, w, n2)
    dh_pre = ref_dgrad(drb, bf(w2).cpu()) * gates_c
    slack = acc_bound(9 * n2, ref_dgrad(drb.abs(), bf(w2).cpu().abs()) * gates_c)
    bad, frac = ulp_violations(dh.view(b, h, w, hid), dh_pre, slack)
    assert bad == 0 and frac < 1e-3, ('dh', bad, frac)


# =====================================================================================================================================
# D. IRN bf16 DenseBlock backward (sininn_dense_backward_bf16, csrc/dense_exec.cpp) through irn.DenseBlock
# =====================================================================================================================================
def dense_wgrad_plan(cin, cout, b, h, w):
    """the DenseBlock's five weight gradients as one mixed group (dense_items_bf16: conv i reads pad8(cin) + 32 i channels of the
    feature buffer, conv1-4 have N = 32, conv5 N = cout) -- wgrad_group_plan's formulas"""
    cinp = -(-cin // 8) * 8
    return wgrad_group_plan([(cinp + 32 * i, 32) for i in range(4)] + [(cinp + 128, cout)], b, h, w)


# (channel_in, channel_out) of the IRN DenseBlocks whose conv5 has N = 84, 108, 12, 180: InvBlockExp(192, 84) / (192, 12) at the
# coarsest level of `-a IRN` (lr_window 10 / 1); batch 16 at 32 x 32 = the 256 x 256 frames of tools/bench_irn.py after three Haar levels
DENSE_CASES = [(108, 84), (84, 108), (180, 12), (12, 180)]


def _seeded_block(cin, cout, seed):
    import archs
    blk = archs.DenseBlock(cin, cout)
    gen = torch.Generator().manual_seed(seed)
    with torch.no_grad():
        for cv in blk.convs():
            fan = cv.weight[0].numel()
            cv.weight.copy_(torch.randn(cv.weight.shape, generator=gen) * (1.5 / fan) ** 0.5)
            cv.bias.copy_(torch.randn(cv.bias.shape, generator=gen) * 0.05)
    return blk


@pytest.mark.parametrize('cin,cout', DENSE_CASES)
def test_dense_block_bf16_backward_against_float64(cin, cout):
    """Backward of a bf16 DenseBlock from its saved feature buffer against float64, stage by stage, at the contract's rounding points
    (module docstring of tests/test_gpu_irn_bf16.py): dD = bf16(dout); conv5's data gradient fills dF; slot k, once finished (after
    the data gradient of conv k + 1), is multiplied by the LeakyReLU gate read from the STORED feature (> 0: 1, else 0.2), and its
    bf16 rounding feeds conv k's data and weight gradients; dF accumulates in fp32.  The finished slots stay in dF (a conv's data
    gradient writes only the channels before its own slot), so every stage is checked from the kernel's OWN fp32 inputs, rounded
    to bf16 here: each slot, dx and the ten parameter gradients at 1e-4 of the max-norm.  (A float64 chain rounded at its own
    values is not a usable reference: a value within fp32 noise of a bf16 rounding boundary lands on the other side, the
    difference feeds the next rounding, and over four slots the two chains drift to 2e-5 .. 2e-4 in L2 -- measured.)  The weight
    gradients of the five convs run as one mixed group whose splits hold several tiles (the f32_quads plan for N % 8 != 0)."""
    import sin_inn_amd as S
    b, h, w = 16, 32, 32
    m = b * h * w
    plan = dense_wgrad_plan(cin, cout, b, h, w)
    assert plan['tiles_per_split'] >= 2, plan
    blk = _seeded_block(cin, cout, cin * 1000 + cout).cuda()
    blk.precision = 'bf16'
    cinp = -(-cin // 8) * 8
    g = torch.Generator().manual_seed(cin + cout)
    x = torch.randn(b, h, w, cin, generator=g).cuda().requires_grad_(True)
    dout = torch.randn(b, h, w, cout, generator=g)
    grads = []

    def keep_dF(gx):                                    # dx is a view of the executor's dF [M][pad8(cin) + 128]
        base = gx._base
        assert base is not None and base.numel() == m * (cinp + 128) and base.dtype == torch.float32
        grads.append(base.detach().reshape(b, h, w, cinp + 128).clone())
    x.register_hook(keep_dF)
    out = blk.run(x)
    buf = out.grad_fn.saved_tensors[0]
    assert buf.dtype == BF
    out.backward(dout.cuda())
    S.modules.join_side_streams()
    torch.cuda.synchronize()
    dF = grads[0].cpu()
    # ---- float64 references from the saved buffer and the kernel's own finished slots --------------------------------------------------
    fb = buf.cpu().reshape(b, h, w, cinp + 128)
    assert bool((fb[..., cin:cinp] == 0).all())

    def feats(i):                                       # conv i's input in the UNPADDED channel order of the torch weight
        return torch.cat([fb[..., :cin]] + [fb[..., cinp + 32 * j:cinp + 32 * (j + 1)] for j in range(i)], -1)

    def slot(t, i):
        return t[..., cinp + 32 * i:cinp + 32 * (i + 1)]

    ws = [bf(cv.weight.detach().cpu()) for cv in blk.convs()]
    douts = [bf(slot(dF, i)) for i in range(4)] + [bf(dout)]            # what conv i's data and weight gradients stage
    acc = torch.zeros(b, h, w, cin + 128, dtype=torch.float64)
    for i in range(4, -1, -1):
        acc[..., :cin + 32 * i] += ref_dgrad(douts[i], ws[i])
        if i > 0:                                       # slot i - 1 is finished now: the gate from the stored feature
            sl = slice(cin + 32 * (i - 1), cin + 32 * i)
            ref_ = acc[..., sl] * torch.where(slot(fb, i - 1).double() > 0, 1.0, 0.2)
            assert relerr(slot(dF, i - 1), ref_) < 1e-4, ('slot', i - 1, relerr(slot(dF, i - 1), ref_))
    dx_ref = acc[..., :cin]
    assert torch.equal(x.grad.cpu(), dF[..., :cin])
    assert relerr(x.grad, dx_ref) < 1e-4, ('dx', relerr(x.grad, dx_ref), rel_l2(x.grad, dx_ref))
    for i, cv in enumerate(blk.convs()):
        gw_ref = ref_wgrad(feats(i), douts[i], 3)
        gb_ref = douts[i].double().sum((0, 1, 2))
        assert relerr(cv.weight.grad, gw_ref) < 1e-4, ('gw', i, relerr(cv.weight.grad, gw_ref), plan)
        assert relerr(cv.bias.grad, gb_ref) < 1e-4, ('gb', i, relerr(cv.bias.grad, gb_ref), plan)
