"""GPU: the bf16 conv engine (conv_bf16_kernel, csrc/conv_bf16.hip) at production tile counts, epilogue by epilogue, against float64.

The bf16 twin of tests/test_gpu_conv_fp32_sizes.py.  tests/test_gpu_bf16.py runs the general bf16 conv at one or two tiles per
direction and holds the whole tensor to one max-norm bound; the coupling, ADD_CBWD, LRELU and IRN epilogues, addend_map, the
in-place ADD and channel sub-ranges are reached only through block tests with budgets of 8e-3 .. 5e-2.  Here ops.conv runs on
bf16 packs (ops.pack_conv_bf16) at the level shapes of BASELINE configs[3] (batch 2 at level 0, batch 16 at level 1), configs[4]
(180 x 320 / 90 x 160) and a shape ragged in x and y.  Every test recomputes the tile grid (16 x 16 pixels for 3x3, 8 x 16 for
1x1) and the launch plan (launch_ks / launch_ht: channel chunk CK, 32- or 64-column blocks, coupling half-width; the persistent
conv3_smallk kernel) from the formulas of the kernel source, asserts >= 24 pixel tiles and that the ragged shapes cut a tile.  Of
that plan only the conv3_smallk choice is checked against the library (sininn_conv3_smallk_bits_supported).  The ABI does not report
CK, the column block or whether the forced 16-channel chunk took effect, and a correct kernel gives the same exact sums at every
chunk size: the plan asserts below state which kernel each case is MEANT to reach by the source's formulas, and a dispatch that
went elsewhere (a hook that is not wired, say) is not seen by them.  Operands sit at channel offset 8 of wider tensors; outputs
start as NaN inside a wider tensor whose other channels, and one image row of pixels past the last image, must come back untouched.

All references are float64 on the GPU (tests/float64_refs.py), computed from the bf16-ROUNDED operands the kernel consumes (bf():
round to nearest even; weights always, an fp32 input because it is rounded while it is staged).  None calls the kernel under test.

Two regimes for every linear case (part A), as in the fp32 file:
1. EXACT INTEGERS.  Inputs / gradients in {-2..2}, weights, biases, addends small integers: exact in bf16, every product and
   partial sum an exact fp32 integer while sum |terms| < 2^24 (asserted from the float64 sum |terms|).  fp32 outputs EQUAL
   float64; bf16 outputs equal bf_of(ref) (the LRELU slope is 1/4 here, a power of two, so the product is exact).  A dropped
   tap or chunk and a wrong image fail here.  A truncating store does NOT: a value of fewer than nine significant bits is
   exact in bf16, and |pre| >= 256 is rare at these depths (K <= 2304, inputs in {-2..2}); regime 2 is what sees it.
2. RANDOM NORMALS.  fp32 outputs per element within (K + 1 + 2) 2^-24 sum |terms|, K = taps x Cin (the direct-kernel coefficient of
   the fp32 file: K - 1 additions and the bias add <= K + 1, 2 for the product and the final addend).  bf16 outputs: no
   element further than one bf16 ulp + acc_bound(K, sum |terms|) from the reference's rounding, and fewer than 1e-3 of the
   elements differ at all (the cap of tests/test_gpu_bf16_tiles.py: a truncating fp32 -> bf16 store moves about half of the
   elements off the reference's rounding and fails it); nothing is exempt -- ReLU, LeakyReLU are 1-Lipschitz and a
   MASK gate is read from the given hidden tensor.  LRELU is held to the same acc_bound(K, .): the one extra rounding of its slope
   product is 2^-24 of the value, far inside the bf16 ulp the rule grants.
   That fp32 torch on the same rounded operands stays inside both caps against float64 was checked on the CPU at 3 x 75 x 150
   before relying on them (3x3 and 1x1, 24 -> 256 -> 48, conv and data gradient, linear / ReLU / LeakyReLU: fp32 error / budget
   <= 0.11, no ulp violation, at most 2.7e-4 of the bf16 roundings differ).
Part B: the non-linear tails on integer operands (s, t, g exact): y, ds, dt, dv at 4 x the relative unit of the same formula in
fp32 torch, the log-det at (pixels per tile x co + tiles per image) 2^-24 sum |L| + 4 unit_L sum |L|.  Part C: the same tails on
randn data with sparse weights; the accumulation budget of part A is carried through the tail (see _carry_couple).  Part D: the
forward of the bf16 IRN DenseBlock, stage by stage from the kernel's own stored feature buffer.

Every random case prints ratio(...) = error / budget (run with -s).  Worst per part on an MI355X:
  A  fp32 outputs: LINEAR 0.11 (bf16 and fp32 input alike), ADD 0.042, through an addend_map 0.039, in place 0.042.
     bf16 outputs: RELU 0.9997, LRELU 0.9997, MASK 0.9991 -- an element ONE bf16 ulp from the reference's rounding has the ratio
     ulp / (ulp + slack), just below 1 by construction; what is measured is how many there are: at most 2.0e-4 of the elements
     (LRELU; RELU 1.0e-4, MASK 1.1e-4) under the cap of 1e-3.  Integers: every element equal.
  B  y 0.25, log-det 0.0007 (second run within 0.0006 of the first), ds 0.26, dt 0.25, dv 0.25, IRN tails 0.25; sbuf == s.
  C  s 0.005, y 0.13, log-det 0.0003, ds 0.15, dt 0.012, dv 0.014.
  D  slots 0.96 (at most 1.9e-4 of a slot's elements differ), conv5 0.0025; pad channels zero, x stored as bf16(x).
  48 tests, 4.3 s.  (The LRELU and slot ratios were read with a slack of acc_bound(K + 1, .); the tests pass with the acc_bound(K, .)
  they now use, and since the slack is below 4 % of the ulp and changes by 1 / (K + 2) of itself, the figures hold as quoted.)
A ratio above 1 is a finding to explain in the kernel, not a constant to raise."""
import ctypes as C
import os
import sys

import pytest
import torch

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, 'tests'))
from float64_refs import ref_conv, ref_dgrad  # noqa: E402
from test_gpu_bf16_tiles import DENSE_CASES, _seeded_block, acc_bound, bf, bf_of  # noqa: E402
from test_gpu_conv_fp32_sizes import LEVEL_CONVS, _sparse_weight, check_exact, glow_tail, make, rel_unit, view_nhwc  # noqa: E402

BF = torch.bfloat16
U = 2.0 ** -24
EXACT_LIMIT = 2.0 ** 24                # integers: exact fp32 sums in any order below this
FRACTION_CAP = 1e-3                    # bf16 outputs that differ from the reference's rounding at all
SENTINEL = 12352.0                     # exact in bf16 and fp32: channels / rows the kernel must leave alone
CONV_LRELU, CONV_IRN_FWD, CONV_IRN_INV, CONV_ADD_CBWD_FWD, CONV_ADD_CBWD_INV = 6, 7, 8, 9, 10      # include/sininn.h
WORST = {}                             # part -> worst ratio(...) of this process

# (B, H, W, level): configs[3] level 0 at batch 2; configs[4] level 0 (180 rows cut the last tile row); level 1 of both; ragged
SHAPES = [(2, 128, 128, 0), (1, 180, 320, 0), (16, 64, 64, 1), (1, 90, 160, 1), (3, 75, 150, 0)]
CUTS = {(1, 180, 320): (False, True), (1, 90, 160): (False, True), (3, 75, 150): (True, True)}       # (in x, in y), 3x3 and 1x1 alike
_ids = lambda s: 'x'.join(map(str, s[:3]))  # noqa: E731


def pad16(n):
    return -(-n // 16) * 16


def tile_grid(ksize, b, h, w):
    """conv_bf16_prepare: tiles_x = ceil(W / 16), tiles_y = ceil(H / TH), TH = 16 (3x3) / 8 (1x1); blockIdx.x = tiles_x tiles_y B.
    Asserts what every test here relies on: many tiles, and the ragged shapes cut one."""
    th = 16 if ksize == 3 else 8
    tx, ty = -(-w // 16), -(-h // th)
    g = dict(TH=th, tiles_x=tx, tiles_y=ty, tiles_img=tx * ty, tiles=tx * ty * b, cut_x=w % 16 != 0, cut_y=h % th != 0)
    assert g['tiles'] >= 24, g
    assert (g['cut_x'], g['cut_y']) == CUTS.get((b, h, w), (False, False)), g
    if b > 1:
        assert g['tiles'] > g['tiles_img']          # the image index is part of blockIdx.x
    return g


def bf16_plan(ksize, cin, npk, in_bf16, col_tile=16, force16=False):
    """launch_ks / launch_ht (csrc/conv_bf16.hip).  Kp = Cin rounded up to 16; 1x1 with Kp % 128 == 0 -> CK 128 (the forced
    16-channel chunk does not reach that branch); Kp % 32 == 0 and no force -> CK 32; else CK 16.  HT = 16 for col_tile 32.  3x3,
    CK 32, bf16 input, Np <= 32, HT 8 -> 32-column blocks."""
    kp = pad16(cin)
    if ksize == 1 and kp % 128 == 0:
        ck = 128
    elif kp % 32 == 0 and not force16:
        ck = 32
    else:
        ck = 16
    ht = 16 if col_tile == 32 else 8
    bn = 32 if (ksize == 3 and ck == 32 and in_bf16 and npk <= 32 and ht == 8) else 64
    return dict(Kp=kp, CK=ck, chunks=kp // ck, BN=bn, HT=ht, col_blocks=-(-npk // bn), K=ksize * ksize * cin)


def smallk_serves(ksize, mode, cin, n, npk, in_bf16, out_bf16):
    """conv3_smallk_bf16_supported: 3x3, fp32 in, bf16 out, 256 columns; RELU from 8 / 16 / 24 / 32 channels, MASK from 16 / 32 / 48"""
    from sin_inn_amd import _lib
    if ksize != 3 or in_bf16 or not out_bf16 or npk != 256 or n != 256:
        return False
    return cin in (8, 16, 24, 32) if mode == _lib.CONV_RELU else (mode == _lib.CONV_MASK and cin in (16, 32, 48))


def conv_args(**kw):
    from sin_inn_amd import _lib
    a = _lib.ConvArgs()
    for k, v in kw.items():
        setattr(a, 'inp' if k == 'in_' else k, v)
    return a


def run_conv(a, smallk=1, force16=False):
    """sininn_conv under the two hooks: sininn_sub1_bwd_test_hook(0) takes the persistent conv3_smallk kernel out of the dispatch,
    sininn_conv_test_hooks(0, 16) forces 16-channel chunks where Kp % 32 == 0"""
    from sin_inn_amd import _lib, ops
    lib = _lib.lib()
    try:
        lib.sininn_sub1_bwd_test_hook(smallk)
        lib.sininn_conv_test_hooks(0, 16 if force16 else 0)
        _lib.check(lib.sininn_conv(C.byref(a), ops._stream()))
        torch.cuda.synchronize()
    finally:
        lib.sininn_conv_test_hooks(0, 0)
        lib.sininn_sub1_bwd_test_hook(1)


def pt(t, off=0):
    from sin_inn_amd import ops
    return ops.ptr(t, off, dtype=t.dtype)


def fresh_out(m, w, c, dtype=torch.float32):
    """[m + w][c + 16]: NaN in the channels [8, 8 + c) of the m pixels the kernel owns, SENTINEL in the other channels and in one
    image row of pixels past the last image (a store guard relaxed by one row lands there)"""
    out = torch.full((m + w, c + 16), SENTINEL, device='cuda', dtype=dtype)
    out[:m, 8:8 + c] = float('nan')
    return out


def untouched(out, before, m, c, ctx):
    """everything outside [0, m) x [8, 8 + c) is bitwise what it was (before: a clone, or None for a fresh_out tensor)"""
    ref = before if before is not None else torch.full_like(out, SENTINEL)
    ok = torch.equal(out[:m, :8], ref[:m, :8]) and torch.equal(out[:m, 8 + c:], ref[:m, 8 + c:])
    assert ok, f'channels outside [8, 8 + N) were written; {ctx}'
    assert torch.equal(out[m:], ref[m:]), f'pixels past the last image were written; {ctx}'


def ratio(part, name, worst, ctx):
    WORST[part] = max(WORST.get(part, 0.0), worst)
    print(f'[conv-bf16-sizes] ratio({part} {name}) = {worst:.4f} (worst so far in part {part}: {WORST[part]:.4f}); {ctx}')


def held(part, name, got, ref64, budget, ctx):
    """fp32 output: every element within its budget (the rule of check_budget of the fp32 file, under this file's parts and tag)"""
    g = got.double()
    assert bool(torch.isfinite(g).all()), f'{name}: {int((~torch.isfinite(g)).sum())} elements not written / not finite; {ctx}'
    err = (g - ref64).abs()
    r = torch.where(budget > 0, err / budget.clamp_min(1e-300), torch.where(err > 0, torch.full_like(err, float('inf')), err))
    worst = float(r.max())
    ratio(part, name, worst, ctx)
    if worst > 1.0:
        idx = (r == r.max()).nonzero()[0].tolist()
        pytest.fail(f'{name}: error / budget = {worst:.3f} at index {idx} (error {float(err[tuple(idx)]):.3e}, budget '
                    f'{float(budget[tuple(idx)]):.3e}), {int((r > 1).sum())} elements over; {ctx}')


def held_bf16(part, name, got, ref64, slack, ctx):
    """bf16 output, the rule of ulp_violations (tests/test_gpu_bf16_tiles.py; copied because that one works on the CPU and these
    tensors hold up to 17 M elements) evaluated on the device: no element further than one
    bf16 ulp + slack from bf_of(ref), fewer than FRACTION_CAP of the elements different at all"""
    g = got.double()
    assert bool(torch.isfinite(g).all()), f'{name}: {int((~torch.isfinite(g)).sum())} elements not written / not finite; {ctx}'
    rb = bf_of(ref64).double()
    d = (g - rb).abs()
    _, e = torch.frexp(rb)
    ulp = torch.where(rb != 0, torch.ldexp(torch.ones_like(rb), e - 8), torch.zeros_like(rb))
    budget = ulp + slack
    r = torch.where(budget > 0, d / budget.clamp_min(1e-300), torch.where(d > 0, torch.full_like(d, float('inf')), d))
    worst, frac = float(r.max()), float((d > 0).double().mean())
    ratio(part, name, worst, f'{frac:.2e} of the elements differ; {ctx}')
    if worst > 1.0:
        idx = (r == r.max()).nonzero()[0].tolist()
        pytest.fail(f'{name}: error / (ulp + slack) = {worst:.3f} at index {idx} (got {float(g[tuple(idx)])}, reference rounds to '
                    f'{float(rb[tuple(idx)])}), {int((r > 1).sum())} elements over; {ctx}')
    assert frac < FRACTION_CAP, f'{name}: {frac:.3e} of the elements differ from the rounding of the reference; {ctx}'


# =====================================================================================================================================
# A. linear epilogues: LINEAR, RELU, LRELU, MASK, ADD (plain, addend_map, in place)
# =====================================================================================================================================
def _linear_family(ksize, shape, cin, n, force16=False):
    """Every linear epilogue of one conv (cin -> n) and of its data gradient (n -> cin) on bf16 packs"""
    import sin_inn_amd  # noqa: F401
    from sin_inn_amd import _lib, ops
    lib = _lib.lib()
    dev = torch.device('cuda')
    b, h, w, _ = shape
    m, taps = b * h * w, ksize * ksize
    grid = tile_grid(ksize, b, h, w)
    np_f, np_d = pad16(n), pad16(cin)
    ran = 0
    for regime in ('int', 'randn'):
        gen = torch.Generator(device='cuda').manual_seed(31 * cin + n + 7 * ksize + b + h)
        slope = 0.25 if regime == 'int' else 0.2               # a power of two keeps the LeakyReLU product exact
        weight = make(regime, gen, (n, cin, ksize, ksize), -1, 1, (taps * cin) ** -0.5)
        bias = make(regime, gen, (n,), -1, 1, 0.1)
        wf, bfw, wd = ops.pack_conv_bf16(weight.contiguous(), bias, None, True)
        xf = make(regime, gen, (m, cin + 16))                  # operands at channel offset 8 of wider tensors
        gf = make(regime, gen, (m, n + 16))
        hf = torch.relu(make(regime, gen, (m, cin + 16))).to(BF)         # the strided bf16 hidden tensor MASK reads its gates from
        add = make(regime, gen, (m, 2 * cin + 16))
        amap = torch.randperm(2 * cin, device=dev, generator=gen)[:cin].to(torch.int32)
        xb, gb = xf.to(BF), gf.to(BF)                          # the bf16 operands; an fp32 operand is rounded while it is staged
        # ---- float64 references on the rounded operands, once per regime -------------------------------------------------------------------
        wq = bf(weight)
        x, g = view_nhwc(xb, b, h, w, 8, cin), view_nhwc(gb, b, h, w, 8, n)
        pre = ref_conv(x, wq, bias)
        t_f = ref_conv(x.abs(), wq.abs(), bias.abs())
        dg = ref_dgrad(g, wq)
        t_d = ref_dgrad(g.abs(), wq.abs())
        gate = view_nhwc(hf, b, h, w, 8, cin) > 0
        add_plain = view_nhwc(add, b, h, w, 8, cin).double()
        add_map = add[:, amap.long()].reshape(b, h, w, cin).double()
        if regime == 'int':
            assert max(float(t_f.max()), float(t_d.max())) + 4 < EXACT_LIMIT, (float(t_f.max()), float(t_d.max()))
        sl = float(torch.tensor(slope, dtype=torch.float32))   # the fp32 slope the kernel multiplies by
        cases = [  # name, mode, forward?, bf16 in, bf16 out, reference, sum |terms|, roundings beyond the K-term sum
            ('linear_bf16in', _lib.CONV_LINEAR, True, 1, 0, pre, t_f),
            ('linear_f32in', _lib.CONV_LINEAR, True, 0, 0, pre, t_f),
            ('relu', _lib.CONV_RELU, True, 0, 1, torch.relu(pre), t_f),
            ('lrelu', CONV_LRELU, True, 1, 1, torch.where(pre > 0, pre, pre * sl), t_f),
            ('mask', _lib.CONV_MASK, False, 0, 1, dg * gate, t_d * gate),
            ('add', _lib.CONV_ADD, False, 1, 0, dg + add_plain, t_d + add_plain.abs()),
            ('add_map', _lib.CONV_ADD, False, 1, 0, dg + add_map, t_d + add_map.abs()),
            ('add_inplace', _lib.CONV_ADD, False, 1, 0, dg + add_plain, t_d + add_plain.abs())]
        for name, mode, fwd, in_b, out_b, ref, terms in cases:
            k_in, n_out, npk = (cin, n, np_f) if fwd else (n, cin, np_d)
            pl = bf16_plan(ksize, k_in, npk, in_b, 16, force16)
            base = bf16_plan(ksize, k_in, npk, in_b)
            # ---- the dispatch this case pins ----------------------------------------------------------------------------------------------
            if ksize == 1 and base['Kp'] % 128 == 0:
                assert base['CK'] == 128 and pl['CK'] == 128 and base['chunks'] == base['Kp'] // 128
            elif base['Kp'] % 32 == 0:
                assert base['CK'] == 32 and pl['CK'] == (16 if force16 else 32)
            else:
                assert base['Kp'] in (16, 48) and base['CK'] == 16, base         # 48: data gradient of conv2 at level 0
            if (cin, n) == (24, 256) and not fwd and ksize == 3 and in_b and not force16:
                assert pl['BN'] == 32 and npk == 32                               # data gradient of conv1, N = 24: 32-column blocks
            small = smallk_serves(ksize, mode, k_in, n_out, npk, in_b, out_b)
            if (k_in <= 32 and n_out == 256 and mode == _lib.CONV_RELU and ksize == 3):
                assert small                                                      # cin <= 32 -> 256 RELU: persistent kernel by default
            if force16:
                if pl['CK'] == base['CK']:
                    continue                                   # the force changes nothing here: already run by the default test
                assert pl['CK'] == 16 and pl['chunks'] >= 6    # Kp = 96 / 256 really in 16-channel chunks
            variants = [('smallk' if small else 'general', 1)] + ([('general', 0)] if small else [])
            for kernel, smallk_on in variants:
                ctx = f'k{ksize} {name} {cin}->{n} {b}x{h}x{w} {regime} {kernel} plan {pl} grid {grid}'
                odt = BF if out_b else torch.float32
                if name == 'add_inplace':
                    out = torch.cat([add[:, :n_out + 16], torch.full((w, n_out + 16), SENTINEL, device=dev)]).contiguous()
                    before = out.clone()                       # the addend IS the output's channel sub-range [8, 8 + N)
                else:
                    out, before = fresh_out(m, w, n_out, odt), None
                a = conv_args(in_=pt(xb if in_b else xf, 8) if fwd else pt(gb if in_b else gf, 8), in_stride=k_in + 16, Cin=k_in,
                              w=pt(wf if fwd else wd), Np=npk, B=b, H=h, W=w, ksize=ksize, mode=mode, out=pt(out, 8),
                              out_stride=n_out + 16, N=n_out, w_bf16=1, in_bf16=in_b, out_bf16=out_b)
                if fwd:
                    a.bias = pt(bfw)
                if mode == CONV_LRELU:
                    a.clamp = slope
                if name == 'mask':
                    a.mask, a.mask_stride, a.mask_bf16 = pt(hf, 8), cin + 16, 1
                elif name == 'add':
                    a.addend, a.addend_stride = pt(add, 8), 2 * cin + 16
                elif name == 'add_map':
                    a.addend, a.addend_stride, a.addend_map = pt(add), 2 * cin + 16, pt(amap)
                elif name == 'add_inplace':
                    a.addend, a.addend_stride = pt(out, 8), n_out + 16
                lib.sininn_sub1_bwd_test_hook(smallk_on)
                try:
                    assert lib.sininn_conv3_smallk_bits_supported(C.byref(a)) == int(small and smallk_on == 1), ctx
                finally:
                    lib.sininn_sub1_bwd_test_hook(1)
                run_conv(a, smallk_on, force16)
                ran += 1
                untouched(out, before, m, n_out, ctx)
                got = out[:m, 8:8 + n_out].reshape(b, h, w, n_out)
                if regime == 'int':
                    check_exact(name, got, bf_of(ref).double() if out_b else ref, ctx)
                elif out_b:
                    held_bf16('A', f'k{ksize} {name}', got, ref, acc_bound(pl['K'], terms), ctx)
                else:
                    held('A', f'k{ksize} {name}', got, ref, (pl['K'] + 1 + 2) * U * terms, ctx)
    return ran


@pytest.mark.parametrize('ksize', [3, 1])
@pytest.mark.parametrize('conv', [0, 1], ids=['conv1', 'conv2'])
@pytest.mark.parametrize('shape', SHAPES, ids=_ids)
def test_conv_bf16_linear_epilogues_at_size(shape, conv, ksize):
    """ops.conv(w_bf16 = 1): LINEAR (fp32 out, from bf16 and from fp32 input), RELU (bf16 out, fp32 input: through the persistent
    conv3_smallk kernel where it serves the conv, and through the general kernel with it switched off), LRELU (bf16 in and out,
    slope in clamp) of the conv; MASK (bf16 out, gates from a strided bf16 hidden tensor, fp32 input; both kernels likewise) and ADD
    (fp32 out, bf16 input: plain, through an addend_map, in place into a channel sub-range) of its data gradient.  No case is
    refused by conv_bf16_prepare, none is dropped."""
    cin, n = LEVEL_CONVS[shape[3]][conv]
    assert _linear_family(ksize, shape, cin, n) >= 16


@pytest.mark.parametrize('ksize', [3, 1])
def test_conv_bf16_kp16_takes_the_16_channel_chunk(ksize):
    """Kp = 16 (16 -> 256, and its data gradient 256 -> 16) at the ragged shape: the CK 16 kernels from a one-chunk K loop"""
    assert bf16_plan(ksize, 16, 256, 0)['CK'] == 16 and bf16_plan(ksize, 16, 256, 0)['chunks'] == 1
    assert _linear_family(ksize, (3, 75, 150, 0), 16, 256) >= 16


@pytest.mark.parametrize('ksize', [3, 1])
@pytest.mark.parametrize('conv', [0, 1], ids=['conv1', 'conv2'])
@pytest.mark.parametrize('shape', [s for s in SHAPES if s[3] == 1], ids=_ids)
def test_conv_bf16_forced_16_channel_chunks(shape, conv, ksize):
    """The level-1 shapes once more under sininn_conv_test_hooks(0, 16): Kp = 96 and Kp = 256 in 16-channel chunks (launch_ht<KS, 16>,
    three blocks per CU).  A 1x1 conv with Kp % 128 == 0 keeps CK 128 in launch_ks whatever the hook says; those cases are not run twice."""
    cin, n = LEVEL_CONVS[1][conv]
    ran = _linear_family(ksize, shape, cin, n, force16=True)
    assert ran >= (16 if ksize == 3 else 8), ran


# =====================================================================================================================================
# B. non-linear tails on integer operands; C. the same tails on randn data with sparse weights
# =====================================================================================================================================
def _carry_couple(v, t_ref, e_ref, bs, bt, inverse):
    """What an error |ds| <= bs, |dt| <= bt of the conv does to y.  L(s) = clamp 0.636 atan(s / clamp) has |L'| <= 0.636, so
    exp(L) moves by a factor within exp(+-0.636 bs):  forward  y = v e + t:  |dy| <= |v| e expm1(0.636 bs) + bt;
    inverse  y = (v - t) / e:  |dy| <= (|v - t| expm1(0.636 bs) + bt exp(0.636 bs)) / e.  (|dy / ds| = |v| e |L'|, |dy / dt| = 1
    resp. |v - t| |L'| / e, 1 / e to first order.)"""
    grow = torch.expm1(0.636 * bs)
    if inverse:
        return ((v - t_ref).abs() * grow + bt * (1 + grow)) / e_ref
    return v.abs() * e_ref * grow + bt


def logdet_budget(ppt, co, tiles_img, unit_l, labs, acc_s=None):
    """Budget of the log-det added per image by a coupling epilogue: a block sums the L of at most ppt pixels x co channels in fp32 and
    adds ONE atomic per image tile, each L is within 4 unit_l of float64 (unit_l: the relative unit of L's formula in fp32 torch);
    labs = sum |L| per image.  acc_s [pixels][co] (optional): what the conv's own error in s carries over, |L'| <= 0.636."""
    budget = ((ppt * co + tiles_img) * U + 4 * unit_l) * labs
    return budget if acc_s is None else budget + 0.636 * acc_s.reshape(labs.shape[0], -1).sum(1)


def _tails(ksize, shape, regime):
    import sin_inn_amd  # noqa: F401
    from sin_inn_amd import _lib, ops
    dev = torch.device('cuda')
    b, h, w, level = shape
    m, clamp, taps = b * h * w, 1.2, ksize * ksize
    co = LEVEL_CONVS[level][0][0]
    grid = tile_grid(ksize, b, h, w)
    part = 'B' if regime == 'int' else 'C'
    gen = torch.Generator(device='cuda').manual_seed(17 * co + ksize + b + h + (regime == 'randn'))

    def weights(shape_, density, scale):
        """sparse multiples of 1/4 (integer regime: exact in bf16 and in every sum); randn regime: times a random factor, so the
        rounding of the pack matters"""
        wt = _sparse_weight(gen, shape_, density, dev) * scale
        return wt if regime == 'int' else wt * (0.5 + torch.rand(shape_, device=dev, generator=gen))

    def exact(terms, unit=4):
        if regime == 'int':
            assert float(terms.max()) * unit < EXACT_LIMIT, float(terms.max())

    # ---- COUPLE_FWD / COUPLE_INV: conv2, 256 -> 2 co, bf16 input, pack through ops.coupling_colmap ----------------------------------------------
    tile = ops.coupling_tile(co)
    assert tile == {24: 16, 96: 32}[co]
    w2 = weights((2 * co, 256, ksize, ksize), 0.02 / taps, 1.0)
    b2 = make('int', gen, (2 * co,), -1, 1) * 0.25
    pk2 = ops.pack_conv_bf16(w2.contiguous(), b2, ops.coupling_colmap(co, dev), False)
    hb = (make('int', gen, (m, 256 + 16), 0, 2) if regime == 'int' else torch.relu(make('randn', gen, (m, 256 + 16)))).to(BF)
    vf = make('int', gen, (m, co + 16)) * 0.5 if regime == 'int' else make('randn', gen, (m, co + 16))
    hh, v = view_nhwc(hb, b, h, w, 8, 256), vf[:, 8:8 + co].double()
    w2q = bf(w2)
    r = ref_conv(hh, w2q, b2).reshape(m, 2 * co)
    r_terms = ref_conv(hh.abs(), w2q.abs(), b2.abs()).reshape(m, 2 * co)
    exact(r_terms)
    s_ref, t_ref = r[:, :co], r[:, co:]
    pl = bf16_plan(ksize, 256, 2 * co, 1, tile)
    assert pl['HT'] == tile // 2 and pl['BN'] == 64 and pl['CK'] == (128 if ksize == 1 else 32), pl
    acc = (pl['K'] + 1 + 2) * U * r_terms if regime == 'randn' else torch.zeros_like(r_terms)        # part A's budget of s, t
    ppt = grid['TH'] * 16                                  # pixels per tile: 256 (3x3) / 128 (1x1)
    for mode, inverse in ((_lib.CONV_COUPLE_FWD, False), (_lib.CONV_COUPLE_INV, True)):
        ctx = f'k{ksize} couple inverse {inverse} 256->{2 * co} col_tile {tile} {b}x{h}x{w} {regime} plan {pl} grid {grid}'
        y_ref, L_ref, e_ref = glow_tail(s_ref, t_ref, v, clamp, inverse, torch.float64)
        y32, L32, _ = glow_tail(s_ref, t_ref, v, clamp, inverse, torch.float32)
        scale = (v.abs() + t_ref.abs()) / e_ref if inverse else v.abs() * e_ref + t_ref.abs()
        unit_y, unit_l = rel_unit(y32, y_ref, scale), rel_unit(L32, L_ref, L_ref.abs())
        ld_ref = (-1 if inverse else 1) * L_ref.reshape(b, -1).sum(1)
        labs = L_ref.abs().reshape(b, -1).sum(1)
        ld_budget = logdet_budget(ppt, co, grid['tiles_img'], unit_l, labs, acc[:, :co])
        lds = []
        for _ in range(2):                                 # float atomics: two runs agree within the budget, not bitwise
            out, y2 = fresh_out(m, w, co), fresh_out(m, w, co)
            sb = torch.full((m, co), float('nan'), device=dev)
            ld = torch.zeros(b, device=dev)
            run_conv(conv_args(in_=pt(hb, 8), in_stride=256 + 16, Cin=256, w=pt(pk2[0]), bias=pt(pk2[1]), Np=2 * co, B=b, H=h, W=w,
                               ksize=ksize, mode=mode, out=pt(out, 8), out_stride=co + 16, v=pt(vf, 8), v_stride=co + 16, sbuf=pt(sb),
                               logdet=pt(ld), Co=co, clamp=clamp, out2=pt(y2, 8), out2_stride=co + 16, col_tile=tile, w_bf16=1,
                               in_bf16=1))
            untouched(out, None, m, co, ctx)
            untouched(y2, None, m, co, ctx)
            assert torch.equal(out[:m, 8:8 + co], y2[:m, 8:8 + co]), ctx
            if regime == 'int':
                check_exact('s', sb, s_ref, ctx)
            else:
                held(part, f'k{ksize} couple s', sb, s_ref, acc[:, :co], ctx)
            carried = _carry_couple(v, t_ref, e_ref, acc[:, :co], acc[:, co:], inverse)
            held(part, f'k{ksize} couple y', out[:m, 8:8 + co], y_ref, 4 * unit_y * scale + carried, ctx)
            held(part, f'k{ksize} couple logdet', ld, ld_ref, ld_budget, ctx)
            lds.append(ld)
        held(part, f'k{ksize} couple logdet, second run', lds[1], lds[0].double(), ld_budget, ctx)
    # ---- ADD_CBWD_FWD / _INV: the data gradient of conv1 (co -> 256), bf16 input, with the fused coupling backward --------------------------------
    w1 = weights((256, co, ksize, ksize), 0.05 / taps, 4.0)
    pk1 = ops.pack_conv_bf16(w1.contiguous(), torch.zeros(256, device=dev), None, True)
    npk = pad16(co)
    pl = bf16_plan(ksize, 256, npk, 1)
    assert pl['BN'] == (32 if (ksize == 3 and co == 24) else 64), pl                # level 0, 3x3: the 32-column blocks carry this tail
    dhb = make(regime, gen, (m, 256 + 16)).to(BF)
    addf = make(regime, gen, (m, co + 16))
    uf = torch.randn((m, co + 16), device=dev, generator=gen)
    sbuf = torch.randn((m, co), device=dev, generator=gen)
    gld = torch.randn((b,), device=dev, generator=gen)
    dh, w1q, ad = view_nhwc(dhb, b, h, w, 8, 256), bf(w1), addf[:, 8:8 + co].double()
    g = ref_dgrad(dh, w1q).reshape(m, co) + ad
    g_terms = ref_dgrad(dh.abs(), w1q.abs()).reshape(m, co) + ad.abs()
    exact(g_terms)
    gacc = (pl['K'] + 1 + 2) * U * g_terms if regime == 'randn' else torch.zeros_like(g_terms)

    def cbwd(dtype, inverse):
        """(ds, dt, dv, their scales, |d ./ dg|) of the fused coupling backward, as the epilogue of conv_mfma_impl.h states it"""
        gg, s, u = g.to(dtype), sbuf.to(dtype), uf[:, 8:8 + co].to(dtype)
        gl = gld.to(dtype).repeat_interleave(h * w)[:, None]
        L = clamp * 0.636 * torch.atan(s / clamp)
        dL = 0.636 / (1 + (s / clamp) ** 2)
        e = torch.exp(L)
        one = torch.ones_like(e)
        if inverse:
            dv = gg / e
            return (-(gg * u + gl) * dL, -dv, dv), (((gg * u).abs() + gl.abs()) * dL, dv.abs(), dv.abs()), (u.abs() * dL, 1 / e, 1 / e)
        return ((gg * u * e + gl) * dL, gg, gg * e), (((gg * u * e).abs() + gl.abs()) * dL, gg.abs(), (gg * e).abs()), (u.abs() * e * dL, one, e)

    for mode, inverse in ((CONV_ADD_CBWD_FWD, False), (CONV_ADD_CBWD_INV, True)):
        ctx = f'k{ksize} add_cbwd inverse {inverse} 256->{co} {b}x{h}x{w} {regime} plan {pl} grid {grid}'
        out, dv = fresh_out(m, w, 2 * co), fresh_out(m, w, co)
        run_conv(conv_args(in_=pt(dhb, 8), in_stride=256 + 16, Cin=256, w=pt(pk1[2]), Np=npk, B=b, H=h, W=w, ksize=ksize, mode=mode,
                           out=pt(out, 8), out_stride=2 * co + 16, N=co, addend=pt(addf, 8), addend_stride=co + 16, v=pt(uf, 8),
                           v_stride=co + 16, sbuf=pt(sbuf), out2=pt(dv, 8), out2_stride=co + 16, logdet=pt(gld), Co=co, clamp=clamp,
                           w_bf16=1, in_bf16=1))
        untouched(out, None, m, 2 * co, ctx)
        untouched(dv, None, m, co, ctx)
        ref, scales, slopes = cbwd(torch.float64, inverse)
        f32 = cbwd(torch.float32, inverse)[0]
        for i, (name, got) in enumerate((('ds', out[:m, 8:8 + co]), ('dt', out[:m, 8 + co:8 + 2 * co]), ('dv', dv[:m, 8:8 + co]))):
            unit = rel_unit(f32[i], ref[i], scales[i])
            if unit == 0 and regime == 'int':
                check_exact(name, got, ref[i], ctx)        # dt = g: nothing is rounded
            else:
                held(part, f'k{ksize} cbwd {name}', got, ref[i], 4 * unit * scales[i] + slopes[i] * gacc, ctx)
    if regime != 'int':
        return
    # ---- IRN_FWD / IRN_INV: 256 -> co with bias, v, clamp and an fp32 mask holding H's output (conv5 of G in an InvBlockExp) ----------------------
    w5 = weights((co, 256, ksize, ksize), 0.02 / taps, 1.0)
    b5 = make('int', gen, (co,), -1, 1) * 0.25
    pk5 = ops.pack_conv_bf16(w5.contiguous(), b5, None, False)
    hmask = torch.randn((m, co + 16), device=dev, generator=gen)
    gg = ref_conv(hh, bf(w5), b5).reshape(m, co)
    exact(ref_conv(hh.abs(), bf(w5).abs(), b5.abs()))
    pl = bf16_plan(ksize, 256, npk, 1)

    def irn(dtype, inverse):
        """irn_tail_kernel (csrc/elementwise.hip): s = clamp (2 sigmoid(h) - 1); out = v exp(s) + g or (v - g) / exp(s)"""
        s = clamp * (2 * torch.sigmoid(hmask[:, 8:8 + co].to(dtype)) - 1)
        e, vv, g_ = torch.exp(s), vf[:, 8:8 + co].to(dtype), gg.to(dtype)
        return ((vv - g_) / e, (vv.abs() + g_.abs()) / e) if inverse else (vv * e + g_, vv.abs() * e + g_.abs())

    for mode, inverse in ((CONV_IRN_FWD, False), (CONV_IRN_INV, True)):
        ctx = f'k{ksize} irn inverse {inverse} 256->{co} {b}x{h}x{w} plan {pl} grid {grid}'
        out = fresh_out(m, w, co)
        run_conv(conv_args(in_=pt(hb, 8), in_stride=256 + 16, Cin=256, w=pt(pk5[0]), bias=pt(pk5[1]), Np=npk, B=b, H=h, W=w, ksize=ksize,
                           mode=mode, out=pt(out, 8), out_stride=co + 16, N=co, v=pt(vf, 8), v_stride=co + 16, mask=pt(hmask, 8),
                           mask_stride=co + 16, clamp=clamp, w_bf16=1, in_bf16=1))
        untouched(out, None, m, co, ctx)
        (ref, scale), (f32, _) = irn(torch.float64, inverse), irn(torch.float32, inverse)
        held(part, f'k{ksize} irn', out[:m, 8:8 + co], ref, 4 * rel_unit(f32, ref, scale) * scale, ctx)


@pytest.mark.parametrize('ksize', [3, 1])
@pytest.mark.parametrize('shape', SHAPES, ids=_ids)
def test_conv_bf16_tails_on_integers(shape, ksize):
    """COUPLE_FWD / COUPLE_INV on conv2 (co = 24 with col_tile 16, co = 96 with col_tile 32): sbuf == s exactly, y (out and out2) at
    4 x its fp32-torch unit, the log-det of two runs into a zeroed buffer.  ADD_CBWD_FWD / _INV on the data gradient of conv1: ds,
    dt, dv at 4 x their units.  IRN_FWD / IRN_INV at 4 x the unit of the same formula in fp32 torch."""
    _tails(ksize, shape, 'int')


@pytest.mark.parametrize('ksize', [3, 1])
@pytest.mark.parametrize('shape', [SHAPES[4], SHAPES[3]], ids=_ids)
def test_conv_bf16_tails_on_randn_with_sparse_weights(shape, ksize):
    """Part C, one shape per level: COUPLE and ADD_CBWD on randn data, so a reduced-precision path INTO the tail is seen.  Budget = the
    tail budget of part B + the accumulation budget of part A carried through the tail (_carry_couple; ADD_CBWD is linear in g)."""
    _tails(ksize, shape, 'randn')


# =====================================================================================================================================
# D. forward of the bf16 IRN DenseBlock (sininn_dense_forward_bf16) through irn.DenseBlock.run
# =====================================================================================================================================
@pytest.mark.parametrize('cin,cout', DENSE_CASES)
def test_dense_block_bf16_forward_against_float64(cin, cout):
    """Stage by stage from the kernel's OWN stored feature buffer (the docstring of part D of tests/test_gpu_bf16_tiles.py says why a
    float64 chain rounded at its own values is no reference): slot i = bf16(lrelu_0.2(conv_i(feats(i)) + b_i)) within one bf16 ulp +
    acc_bound of the reference's rounding and < 1e-3 of its elements different; conv5's fp32 output on the stored features at the
    per-element budget of part A; x stored as bf16(x); the pad channels [cin, pad8(cin)) exact zeros."""
    import sin_inn_amd  # noqa: F401
    b, h, w = 16, 32, 32
    grid = tile_grid(3, b, h, w)
    blk = _seeded_block(cin, cout, cin * 1000 + cout).cuda()
    blk.precision = 'bf16'
    cinp = -(-cin // 8) * 8
    gen = torch.Generator().manual_seed(cin + cout)
    x = torch.randn(b, h, w, cin, generator=gen).cuda().requires_grad_(True)       # requires_grad: the feature buffer is saved
    out = blk.run(x)
    buf = out.grad_fn.saved_tensors[0]
    torch.cuda.synchronize()
    assert buf.dtype == BF and buf.numel() == b * h * w * (cinp + 128)
    fb = buf.reshape(b, h, w, cinp + 128)
    assert bool((fb[..., cin:cinp] == 0).all())
    assert torch.equal(fb[..., :cin], x.detach().to(BF))
    slope = float(torch.tensor(0.2, dtype=torch.float32))

    def feats(i):                                       # conv i's input in the UNPADDED channel order of the torch weight
        return torch.cat([fb[..., :cin]] + [fb[..., cinp + 32 * j:cinp + 32 * (j + 1)] for j in range(i)], -1)

    for i, cv in enumerate(blk.convs()):
        wq, bias = bf(cv.weight.detach()), cv.bias.detach()
        k_in = cinp + 32 * i                            # the Cin of the call: the pad channels are zeros in the buffer and the pack
        pl = bf16_plan(3, k_in, pad16(32 if i < 4 else cout), 1)
        ctx = f'dense {cin}->{cout} conv{i + 1} plan {pl} grid {grid}'
        pre = ref_conv(feats(i), wq, bias)
        terms = ref_conv(feats(i).abs(), wq.abs(), bias.abs())
        k = 9 * (cin + 32 * i)
        if i < 4:
            got = fb[..., cinp + 32 * i:cinp + 32 * (i + 1)]
            ref = torch.where(pre > 0, pre, pre * slope)
            held_bf16('D', f'slot {i}', got, ref, acc_bound(k, terms), ctx)
        else:
            held('D', 'conv5', out.detach(), pre, (k + 1 + 2) * U * terms, ctx)
