"""GPU: the mixed-precision (bf16) fused 1x1 FORWARD kernels past one tile per block, against float64.

csrc/conv_sub1_bf16.hip runs every 1x1 coupling subnet of the bf16 path through two persistent kernels: conv_sub1b_wide_fwd_kernel
<96, 192, 16> at level 1 (96 -> 256 -> 2 x 96, behind sininn_conv_pair_k1) and conv_sub1b_fwd_kernel<K1, 2 K1, HT> at level 0
(K1 = 8, 16, 24, behind sininn_conv_sub1_fwd).  A block walks tiles g, g + G, g + 2 G, ...: the x tile is requested three grid
strides ahead and staged into alternating LDS buffers, v two strides ahead, and the log-det partial of a tile is added one tile
later, when the block may already be in another image.  The tight tests of tests/test_gpu_bf16.py run these kernels where (almost)
every block has ONE tile; here they run at the level-1 / level-0 sizes of BASELINE configs[3] and [4] and at ragged shapes.  Every
test rebuilds the launch plan from the formulas of the kernel source and asserts what its shape is there for.

Asserted tile plans (wide kernel: 16 x 2 pixel tiles, min(ntiles, 256) blocks; level 0: 16 x 4 pixel tiles, the same cap):
  wide  (16, 64, 64)   2 048 tiles, 8 per block (>= 3: a buffer is reused, the three-ahead request is consumed)
  wide  (1, 90, 160)   450 tiles: 256 < ntiles < 512, blocks 0 .. 193 take the second `body`, the others skip it
  wide  (3, 45, 83)    6 x 23 x 3 = 414 tiles, H odd (a half-empty last tile row), W % 16 != 0; block g < 158 goes from image
                       g // 138 to image (g + 256) // 138, so the deferred log-det partial crosses an image
  wide  (2, 19, 40)    60 tiles, one per block (control)
  lvl 0 (4, 128, 128)  8 x 32 x 4 = 1 024 tiles, 4 per block (>= 3)
  lvl 0 (2, 45, 83)    6 x 12 x 2 = 144 tiles, one per block (control)

Regime A / C (random normals): float64 on the CPU from the SAME bf16-rounded operands.  The budgets are the project's standing ones:
  h            gates == sign of the float64 pre-activation except where |pre| <= acc_bound(96, sum |x w| + |b1|); elsewhere at most
               one bf16 ulp (+ that bound) from the reference's rounding, in fewer than 1e-3 of the elements
  s (own h)    per element: |s - s64| <= acc_bound(256, |h| |W2|^T + |b2|), s64 from the KERNEL's stored h -- no constant
  y (own h)    1e-4 of the max-norm; out2 == out bitwise; log-det added per image: 1e-4 of the max-norm
  whole subnet `close` (2e-3 of the max-norm and 2e-5 in L2) against the reference with its own rounding of h; log-det 1e-4
  bitwise      h stored / not stored, out2 + sbuf passed / not passed, a repeated call: the same out, out2, sbuf, h.  The log-det
               of two launches is held to 1e-4 instead (also between the h-stored and the h-not-stored run): its per-image
               atomics arrive in an order that is not fixed, so bits may differ between any two launches
  pair kernel  with sininn_sub1_bwd_test_hook(0) the same descriptors run conv_pair_bf16_kernel: its stored h is bitwise the wide
               kernel's (the claim of the source comment), its out agrees within `close`
Regime B (exact integers): x in {-2..2}, W1 sparse in {-1, 0, 1}, conv2's s rows and s biases zero, t rows in {-1, 0, 1}: s == 0, L == 0,
e^L == 1, and sbuf == 0, out == out2 == v +- t, h == the float64 h, the log-det keeps its bits -- torch.equal for EVERY element, which
sees one dropped, doubled or stale tile in 2 048 (regime A's max-norm sees it too, its L2 budget alone would not).

Measured on an MI355X (worst error / budget per quantity over all cases of a part; printed with -s):
  part A, wide kernel (8 cases)                       part C, level 0 (8 cases)
    h: fraction off the reference rounding  0.016 (1.6e-5; no element beyond one ulp, no gate beyond the bound)
    s from own h, per element               0.0094
    y from own h                            0.0012
    log-det from own h                      0.0095
    y whole subnet, max-norm / L2           0.084 / 0.176       0.027 / 0.048
    s whole subnet, max-norm / L2           0.272 / 0.676       0.190 / 0.497
    log-det whole subnet                    0.091               0.012
    log-det, two identical calls            0.0054              0.0039
    log-det, variants against training pass 0.0061              0.0062
    pair kernel: h                          0 of 16 777 216 elements differ (every shape, both directions)
    pair kernel: out, sbuf against wide     0 (bitwise the same in this run as well); log-det 0.0096
    pair kernel: whole subnet               as the wide kernel's; log-det 0.10
  part B (wide and level 0): 0 elements differ in out, out2, sbuf, h; the log-det kept its bits.
  The log-det of two launches was bitwise the same in 5 of 56 comparisons: the order of its atomics is indeed not fixed.

What the file found: nothing wrong in the kernels.  Every check passes with room, the source's claim about h holds bit for bit, and the
largest ratio (s of the whole subnet in L2, 0.68) is the rounding of h on a bf16 boundary that the budget was set for.  Tried once each
on a scratch build, never committed: not staging the second x buffer (store_tile(buf ^ 1) skipped for buffer 1), adding the log-det
partial to the current tile's image instead of ld_b[ld_pending], and dropping the last tile of every block with more than one.  The
first and the third fail every multi-tile case of parts A and B at "not written or not finite" (stale LDS / NaN left in out); the
second fails the log-det checks of part A at (16, 64, 64) and (3, 45, 83), the shapes whose blocks change image, and rightly not
at (1, 90, 160) (one image) or in part B (every partial is 0).  The one-tile control (2, 19, 40) passes under all three."""
import ctypes as C
import os
import sys

import pytest
import torch

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, 'tests'))

from float64_refs import ref_conv  # noqa: E402
from test_gpu_bf16_tiles import (BF, S1_MAX_BLOCKS, _threads, acc_bound, args, bf, bf_of, close, rel_l2, relerr, ulp_violations,  # noqa: E402,F401
                                 wide_plan)

TAG = '[bf16-pair-fwd-sizes]'
CLAMP = 1.2
HID = 256
WORST = {}
_CASES = {}


@pytest.fixture(scope='module', autouse=True)
def _release_references():
    """the float64 references are computed once per (kernel, shape, regime) and shared by the direction / variant parameters"""
    yield
    _CASES.clear()
    torch.cuda.synchronize()
    torch.cuda.empty_cache()                                       # the 65 536-pixel operands: hand the cached blocks back


def report(part, name, err, budget, ctx):
    """print error / budget of one quantity (and the worst so far of the part); the caller asserts on err and budget themselves"""
    ratio = err / budget
    key = (part, name)
    WORST[key] = max(WORST.get(key, 0.0), ratio)
    print(f'{TAG} part {part} {name}: {err:.3e} / {budget:.3e} = {ratio:.4f} (worst so far {WORST[key]:.4f}); {ctx}')
    return ratio


def mm(x, w, b, shape):
    """float64 x [M][C] @ w [N][C]^T + b as a 1x1 conv of tests/float64_refs.py, one image at a time"""
    bb, h, ww = shape
    return ref_conv(x.reshape(bb, h, ww, -1), w.reshape(w.shape[0], w.shape[1], 1, 1), b).reshape(bb * h * ww, -1)


def couple(st, v, co, inverse, b):
    """(y, log-det added per image) of the affine coupling from (s | t), float64"""
    s, t = st[:, :co], st[:, co:]
    L = CLAMP * 0.636 * torch.atan(s / CLAMP)
    if inverse:
        return (v - t) / torch.exp(L), -L.reshape(b, -1).sum(1)
    return torch.exp(L) * v + t, L.reshape(b, -1).sum(1)


def all_nan(t):
    return bool(torch.isnan(t.float()).all())


def bits_equal(a, b):
    """bitwise equality of two tensors of one dtype (NaN == NaN of the same bits, -0 != 0)"""
    it = {2: torch.int16, 4: torch.int32}[a.element_size()]
    return a.dtype == b.dtype and a.shape == b.shape and torch.equal(a.contiguous().view(it), b.contiguous().view(it))


def int_sparse(gen, shape, density, dev):
    """entries in {-1, 0, 1}, a fraction `density` of them non-zero candidates"""
    return (torch.randint(-1, 2, shape, device=dev, generator=gen).float()
            * (torch.rand(shape, device=dev, generator=gen) < density))


def small_ints(gen, shape, dev, lo=-2, hi=2):
    return torch.randint(lo, hi + 1, shape, device=dev, generator=gen).float()


class Subnet:
    """Weights, packs, operands and float64 references of one (kernel, shape, regime): built once, never changed.
    wide: x sits at channel offset 8 of a [pixels][k1 + 16] tensor, v and out at channel offset 8 of [pixels][co + 16] tensors.
    level 0 (the layout of test_fused_1x1_subnet_bf16_c_abi): x at channel offset 8 of [pixels][2 co + 8], v and out the first co
    channels of such tensors.  Every tensor carries one extra image row of pixels (W of them) past the last image."""

    def __init__(self, wide, co, shape, regime):
        import sin_inn_amd  # noqa: F401
        from sin_inn_amd import ops
        dev = torch.device('cuda')
        self.wide, self.co, self.shape, self.regime = wide, co, shape, regime
        b, h, w = shape
        self.m, self.mp = b * h * w, b * h * w + w
        k1, k2 = co, 2 * co
        g = torch.Generator(device=dev).manual_seed(1000 * co + 7 * b + h + (500 if regime == 'int' else 0))
        if wide:
            self.cx, self.x_off, self.cv, self.v_off = k1 + 16, 8, co + 16, 8
        else:
            self.cx, self.x_off, self.cv, self.v_off = 2 * co + 8, 8, 2 * co + 8, 0
        if regime == 'int':
            conv1_w = int_sparse(g, (HID, k1, 1, 1), 0.15 if wide else 0.5, dev)
            conv1_b = small_ints(g, (HID,), dev)
            conv2_w = int_sparse(g, (k2, HID, 1, 1), 0.1, dev)
            conv2_b = small_ints(g, (k2,), dev)
            conv2_w[:co] = 0                                       # the s rows (OIHW order: s | t) and their biases: s == 0 exactly
            conv2_b[:co] = 0
            self.xfull = small_ints(g, (self.mp, self.cx), dev)
            self.vfull = small_ints(g, (self.mp, self.cv), dev, -4, 4)
        else:
            if wide:                                               # part B of tests/test_gpu_bf16_tiles.py
                conv1_w = torch.randn(HID, k1, 1, 1, device=dev, generator=g) * k1 ** -0.5
                conv1_b = torch.randn(HID, device=dev, generator=g) * 0.1
                conv2_w = torch.randn(k2, HID, 1, 1, device=dev, generator=g) * 0.3 * HID ** -0.5
                conv2_b = torch.randn(k2, device=dev, generator=g) * 0.1
            else:                                                  # test_fused_1x1_subnet_bf16_c_abi: Conv2d's default init, conv2 x 0.3
                u = lambda shp, fan: (torch.rand(shp, device=dev, generator=g) * 2 - 1) * fan ** -0.5
                conv1_w, conv1_b = u((HID, k1, 1, 1), k1), u((HID,), k1)
                conv2_w, conv2_b = u((k2, HID, 1, 1), HID) * 0.3, u((k2,), HID)
            self.xfull = torch.randn(self.mp, self.cx, device=dev, generator=g)
            self.vfull = torch.randn(self.mp, self.cv, device=dev, generator=g)
        self.ld0 = torch.randn(b + 1, device=dev, generator=g)    # one spare entry past the last image
        self.pk1 = ops.pack_conv_bf16(conv1_w.contiguous(), conv1_b.contiguous(), None, True)
        self.pk2 = ops.pack_conv_bf16(conv2_w.contiguous(), conv2_b.contiguous(), ops.coupling_colmap(co, dev), True)
        self.x_keep, self.v_keep = self.xfull.clone(), self.vfull.clone()
        torch.cuda.synchronize()
        # ---- float64 on the bf16-rounded operands ----------------------------------------------------------------------------------
        m = self.m
        self.xb = bf(self.xfull[:m, self.x_off:self.x_off + k1].cpu()).double()
        self.v = self.vfull[:m, self.v_off:self.v_off + co].cpu().double()
        self.w1 = bf(conv1_w.reshape(HID, k1)).cpu().double()
        self.w2 = bf(conv2_w.reshape(k2, HID)).cpu().double()
        self.b1, self.b2 = conv1_b.cpu().double(), conv2_b.cpu().double()
        self.pre = mm(self.xb, self.w1, self.b1, shape)
        self.terms1 = mm(self.xb.abs(), self.w1.abs(), self.b1.abs(), shape)
        self.hid = bf_of(torch.relu(self.pre)).double()            # one rounding of the fp32 sum
        self.st = mm(self.hid, self.w2, self.b2, shape)
        if not wide and regime != 'int':                           # level 0 never stores h: only the wide and the exact checks read these
            self.pre = self.terms1 = None
        self._hk = self._st_k = self._terms_k = None
        self._h_checked = None

    def ctx(self, inverse, **kw):
        extra = ''.join(f' {k}={v}' for k, v in kw.items())
        return f'{"wide" if self.wide else "level0"} co={self.co} {self.shape} {self.regime} {"INV" if inverse else "FWD"}{extra}'

    # ---- one launch -----------------------------------------------------------------------------------------------------------------
    def run(self, inverse, store_h=True, train=True):
        """One call of sininn_conv_pair_k1 (wide) / sininn_conv_sub1_fwd (level 0: h is never stored) on fresh NaN-filled outputs.
        Asserts that everything outside the result came back as it was, returns the results' valid regions."""
        from sin_inn_amd import _lib, ops
        lib = _lib.lib()
        dev = self.xfull.device
        b, h, w = self.shape
        m, mp, co, k1, k2 = self.m, self.mp, self.co, self.co, 2 * self.co
        nan = float('nan')
        outfull = torch.full((mp, self.cv), nan, device=dev)
        out2 = torch.full((mp, co), nan, device=dev)
        sbuf = torch.full((mp, co), nan, device=dev)
        hs = torch.full((mp, HID), nan, device=dev, dtype=BF)
        ld = self.ld0.clone()
        pb = lambda t: ops.ptr(t, dtype=BF)
        common = dict(B=b, H=h, W=w, ksize=1, w_bf16=1)
        f1 = args(in_=ops.ptr(self.xfull, self.x_off), in_stride=self.cx, Cin=k1, w=pb(self.pk1[0]), bias=ops.ptr(self.pk1[1]), Np=HID,
                  mode=_lib.CONV_RELU, out=pb(hs) if (store_h and self.wide) else None, out_stride=HID, N=HID, out_bf16=1, **common)
        f2 = args(in_=pb(hs), in_stride=HID, Cin=HID, w=pb(self.pk2[0]), bias=ops.ptr(self.pk2[1]), Np=k2,
                  mode=_lib.CONV_COUPLE_INV if inverse else _lib.CONV_COUPLE_FWD, out=ops.ptr(outfull, self.v_off), out_stride=self.cv,
                  v=ops.ptr(self.vfull, self.v_off), v_stride=self.cv, sbuf=ops.ptr(sbuf) if train else None, logdet=ops.ptr(ld), Co=co,
                  clamp=CLAMP, out2=ops.ptr(out2) if train else None, out2_stride=co, col_tile=ops.coupling_tile(co), in_bf16=1, **common)
        if self.wide:
            assert lib.sininn_conv_pair_k1_supported(C.byref(f1), C.byref(f2)) == 1
            _lib.check(lib.sininn_conv_pair_k1(C.byref(f1), C.byref(f2), ops._stream()))
        else:
            assert lib.sininn_conv_sub1_fwd_supported(C.byref(f1), C.byref(f2)) == 1
            _lib.check(lib.sininn_conv_sub1_fwd(C.byref(f1), C.byref(f2), ops._stream()))
        torch.cuda.synchronize()
        c = self.ctx(inverse, store_h=store_h, train=train)
        lo, hi = self.v_off, self.v_off + co
        # the extra image row, the other channels of the wider tensors, the operands, the spare log-det entry: as they were
        assert all_nan(outfull[m:]) and all_nan(outfull[:m, :lo]) and all_nan(outfull[:m, hi:]), f'out written outside its region; {c}'
        assert all_nan(out2[m:] if train else out2) and all_nan(sbuf[m:] if train else sbuf), f'out2 / sbuf written outside; {c}'
        assert all_nan(hs[m:] if (store_h and self.wide) else hs), f'h written outside; {c}'
        assert bits_equal(ld[b:], self.ld0[b:]) and bits_equal(self.xfull, self.x_keep) and bits_equal(self.vfull, self.v_keep), c
        res = dict(out=outfull[:m, lo:hi].contiguous(), ld=ld[:b].clone(), ld_add=(ld[:b].double() - self.ld0[:b].double()).cpu())
        assert bool(torch.isfinite(res['out']).all()), f'{int((~torch.isfinite(res["out"])).sum())} elements of out not written or not finite; {c}'
        if train:
            res['out2'], res['sbuf'] = out2[:m], sbuf[:m]
            assert bool(torch.isfinite(out2[:m]).all()) and bool(torch.isfinite(sbuf[:m]).all()), f'out2 / sbuf not written; {c}'
        if store_h and self.wide:
            res['h'] = hs[:m]
            assert bool(torch.isfinite(hs[:m].float()).all()), f'h not written; {c}'
        return res

    # ---- checks ---------------------------------------------------------------------------------------------------------------------
    def check_h(self, part, hk, c):
        """check 1: the stored h against relu(bf(x) bf(W1)^T + b1), the gate rule of part C of tests/test_gpu_bf16_tiles.py"""
        hk = hk.cpu()
        if self._h_checked is not None and bits_equal(self._h_checked, hk):
            return                                                  # the same bits passed already
        bound = acc_bound(self.co, self.terms1)
        near = self.pre.abs() <= bound
        gates = hk > 0
        wrong = (gates != (self.pre > 0)) & ~near
        assert not bool(wrong.any()), f'{int(wrong.sum())} gates disagree with a pre-activation beyond the accumulation bound; {c}'
        bad, frac = ulp_violations(hk, torch.relu(self.pre), bound, exempt=near)
        report(part, 'h fraction off the reference rounding', frac, 1e-3, f'{c} near-zero gates={int(near.sum())} bad={bad}')
        assert bad == 0 and frac < 1e-3, ('h', bad, frac, c)
        self._h_checked = hk

    def stage2(self, hk):
        """(s | t) and sum |terms| of conv2 in float64 from the kernel's own stored h"""
        hk = hk.cpu()
        if self._hk is None or not bits_equal(self._hk, hk):
            hd = hk.double()
            self._st_k = mm(hd, self.w2, self.b2, self.shape)
            self._terms_k = mm(hd.abs(), self.w2.abs(), self.b2.abs(), self.shape)
            self._hk = hk
        return self._st_k, self._terms_k

    def check_from_own_h(self, part, res, inverse, c):
        """check 2: stage 2 from the kernel's own h"""
        b, co = self.shape[0], self.co
        st_k, terms_k = self.stage2(res['h'])
        err = (res['sbuf'].cpu().double() - st_k[:, :co]).abs()
        budget = acc_bound(HID, terms_k[:, :co])
        ratio = float((err / budget.clamp_min(1e-300)).max())
        report(part, 's from own h (per element)', ratio, 1.0, c)
        assert bool((err <= budget).all()), ('s', ratio, int((err > budget).sum()), c)
        y_k, ld_k = couple(st_k, self.v, co, inverse, b)
        e = relerr(res['out'], y_k)
        report(part, 'y from own h', e, 1e-4, c)
        assert e < 1e-4, ('y', e, c)
        assert bits_equal(res['out2'], res['out']), f'out2 != out; {c}'
        e = relerr(res['ld_add'], ld_k)
        report(part, 'log-det from own h', e, 1e-4, c)
        assert e < 1e-4, ('logdet', e, res['ld_add'].tolist(), ld_k.tolist(), c)

    def check_whole(self, part, res, inverse, c):
        """check 3: the whole subnet against the reference with its own rounding of h"""
        b, co = self.shape[0], self.co
        y_ref, ld_ref = couple(self.st, self.v, co, inverse, b)
        for name, got, ref_ in (('y', res['out'], y_ref), ('s', res['sbuf'], self.st[:, :co])):
            e, l2 = relerr(got, ref_), rel_l2(got, ref_)
            report(part, f'{name} whole subnet (max-norm)', e, 2e-3, c)
            report(part, f'{name} whole subnet (L2)', l2, 2e-5, c)
            assert close(got, ref_), (name, e, l2, c)
        assert bits_equal(res['out2'], res['out']), f'out2 != out; {c}'
        e = relerr(res['ld_add'], ld_ref)
        report(part, 'log-det whole subnet', e, 1e-4, c)
        assert e < 1e-4, ('logdet', e, res['ld_add'].tolist(), ld_ref.tolist(), c)


def case(wide, co, shape, regime):
    key = (wide, co, shape, regime)
    if key not in _CASES:
        _CASES[key] = Subnet(wide, co, shape, regime)
    return _CASES[key]


def checked_wide_plan(shape):
    """wide_plan of the shape, with what the shape is there for asserted"""
    b, h, w = shape
    plan = wide_plan(b, h, w)
    tiles_img = -(-w // 16) * -(-h // 2)
    nt, G = plan['ntiles'], plan['blocks']
    assert nt == b * tiles_img and G == min(nt, S1_MAX_BLOCKS), plan
    if shape == (16, 64, 64):
        assert nt == 2048 and nt // G >= 3, plan                   # a buffer is reused, the three-ahead request is consumed
    elif shape == (1, 90, 160):
        assert 256 < nt < 512 and G == 256, plan                  # some blocks take the second body, the others skip it
    elif shape == (3, 45, 83):
        assert h % 2 == 1 and w % 16 != 0 and nt == 414, plan
        assert any(g // tiles_img != (g + G) // tiles_img for g in range(G) if g + G < nt), plan   # ld_pending crosses an image
    else:
        assert plan['max_tiles_per_block'] == 1, plan
    return plan


def level0_plan(shape):
    """conv_sub1_bf16.hip, fill_common: 16 x 4 pixel tiles, min(ntiles, 256) persistent blocks"""
    b, h, w = shape
    ntiles = b * -(-w // 16) * -(-h // 4)
    blocks = min(ntiles, S1_MAX_BLOCKS)
    plan = dict(ntiles=ntiles, blocks=blocks, max_tiles_per_block=-(-ntiles // blocks))
    if shape == (4, 128, 128):
        assert ntiles == 1024 and ntiles // blocks >= 3, plan
    else:
        assert ntiles == 144 and plan['max_tiles_per_block'] == 1, plan
    return plan


def same_logdet(part, name, a, b_, c):
    """two launches' log-det: the same partials, added by atomics in an order that is not fixed"""
    e = relerr(a['ld_add'], b_['ld_add'])
    report(part, name, e, 1e-4, f'{c} bitwise={bits_equal(a["ld"], b_["ld"])}')
    assert e < 1e-4, (name, e, c)


WIDE_SHAPES = [(16, 64, 64), (1, 90, 160), (3, 45, 83), (2, 19, 40)]
ids = lambda s: 'x'.join(map(str, s)) if isinstance(s, tuple) else None


# =====================================================================================================================================
# A. wide forward, random normals
# =====================================================================================================================================
@pytest.mark.parametrize('inverse', [False, True], ids=['fwd', 'inv'])
@pytest.mark.parametrize('shape', WIDE_SHAPES, ids=ids)
def test_wide_forward_against_float64(shape, inverse):
    """checks 1 - 3 of the module docstring on a training pass (h stored, out2 + sbuf passed)"""
    plan = checked_wide_plan(shape)
    cs = case(True, 96, shape, 'normal')
    c = cs.ctx(inverse, tiles=plan['ntiles'])
    res = cs.run(inverse)
    cs.check_h('A', res['h'], c)
    cs.check_from_own_h('A', res, inverse, c)
    cs.check_whole('A', res, inverse, c)


@pytest.mark.parametrize('inverse', [False, True], ids=['fwd', 'inv'])
@pytest.mark.parametrize('shape', WIDE_SHAPES, ids=ids)
def test_wide_forward_variants_are_bitwise_the_same(shape, inverse):
    """check 4: h stored or not, out2 + sbuf passed or not (inference), and a repeated call give the same bits; the inference run
    (no stored h to start from) is checked against float64 as a whole subnet on its own"""
    checked_wide_plan(shape)
    cs = case(True, 96, shape, 'normal')
    c = cs.ctx(inverse)
    base = cs.run(inverse, store_h=True, train=True)
    again = cs.run(inverse, store_h=True, train=True)
    for k in ('out', 'out2', 'sbuf', 'h'):
        assert bits_equal(base[k], again[k]), f'{k} differs between two identical calls; {c}'
    same_logdet('A', 'log-det, two identical calls', again, base, c)
    for store_h, train in ((False, True), (True, False), (False, False)):
        res = cs.run(inverse, store_h=store_h, train=train)
        for k in ('out', 'out2', 'sbuf', 'h'):
            if k in res:
                assert bits_equal(base[k], res[k]), f'{k} differs with store_h={store_h} train={train}; {c}'
        same_logdet('A', f'log-det, store_h={store_h} train={train} against the training pass', res, base, c)
    y_ref, ld_ref = couple(cs.st, cs.v, 96, inverse, shape[0])
    assert close(res['out'], y_ref) and relerr(res['ld_add'], ld_ref) < 1e-4, (relerr(res['out'], y_ref), rel_l2(res['out'], y_ref), c)


@pytest.mark.parametrize('inverse', [False, True], ids=['fwd', 'inv'])
@pytest.mark.parametrize('shape', WIDE_SHAPES, ids=ids)
def test_wide_forward_stores_the_pair_kernels_h(shape, inverse):
    """check 5: with the persistent kernels switched off the same descriptors run conv_pair_bf16_kernel (64-pixel blocks, one per
    tile); its stored h is bitwise the wide kernel's -- "bitwise the pair kernel's h" in conv_sub1_bf16.hip -- and its out agrees
    within `close`; the pair kernel's own results against float64 at the whole-subnet budgets"""
    from sin_inn_amd import _lib
    checked_wide_plan(shape)
    cs = case(True, 96, shape, 'normal')
    c = cs.ctx(inverse)
    wide = cs.run(inverse)
    try:
        _lib.lib().sininn_sub1_bwd_test_hook(0)
        pair = cs.run(inverse)
    finally:
        _lib.lib().sininn_sub1_bwd_test_hook(1)
    ndiff = int((wide['h'].view(torch.int16) != pair['h'].view(torch.int16)).sum())
    print(f'{TAG} part A h, wide kernel against pair kernel: {ndiff} of {wide["h"].numel()} elements differ; {c}')
    assert ndiff == 0, (ndiff, c)
    for name in ('out', 'sbuf'):
        e, l2 = relerr(pair[name], wide[name]), rel_l2(pair[name], wide[name])
        report('A', f'{name}, pair kernel against wide kernel (max-norm)', e, 2e-3, c)
        report('A', f'{name}, pair kernel against wide kernel (L2)', l2, 2e-5, c)
        assert close(pair[name], wide[name]), (name, e, l2, c)
    same_logdet('A', 'log-det, pair kernel against wide kernel', pair, wide, c)
    cs.check_whole('A-pair', pair, inverse, c)


# =====================================================================================================================================
# B. wide forward, exact integers
# =====================================================================================================================================
def check_exact_integers(cs, inverse, plan):
    """every element of every result of the integer regime, training pass and inference pass"""
    b, co = cs.shape[0], cs.co
    c = cs.ctx(inverse, tiles=plan['ntiles'])
    # the test's own preconditions: every sum is an integer that fp32 holds, h is exact in bf16
    assert float(cs.terms1.max()) < 2 ** 24 and float(cs.hid.max()) <= 256 and torch.equal(cs.hid, torch.relu(cs.pre)), c
    terms_t = mm(cs.hid, cs.w2.abs(), cs.b2.abs(), cs.shape)[:, co:]
    assert float(terms_t.max()) < 2 ** 22, c
    assert bool((cs.st[:, :co] == 0).all()) and float(cs.hid.max()) >= 8 and float(cs.st[:, co:].abs().max()) >= 8, c
    t = cs.st[:, co:]
    y_ref = (cs.v - t) if inverse else (cs.v + t)
    for store_h, train in ((True, True), (False, False)):
        res = cs.run(inverse, store_h=store_h, train=train)
        what = f'{c} store_h={store_h} train={train}'
        nbad = int((res['out'].cpu().double() != y_ref).sum())
        print(f'{TAG} part B out: {nbad} of {y_ref.numel()} elements differ from v +- t; {what}')
        assert torch.equal(res['out'].cpu(), y_ref.float()), f'out: {nbad} elements differ from the exact result; {what}'
        assert bits_equal(res['ld'], cs.ld0[:b]), f'the log-det changed: {res["ld_add"].tolist()}; {what}'
        if train:
            assert torch.equal(res['out2'], res['out']), f'out2 != out; {what}'
            assert torch.equal(res['sbuf'], torch.zeros_like(res['sbuf'])), f'sbuf != 0 in {int((res["sbuf"] != 0).sum())} elements; {what}'
        if 'h' in res:
            nbad = int((res['h'].cpu().double() != cs.hid).sum())
            assert torch.equal(res['h'].cpu(), cs.hid.to(BF)), f'h: {nbad} elements differ from the float64 h; {what}'


@pytest.mark.parametrize('inverse', [False, True], ids=['fwd', 'inv'])
@pytest.mark.parametrize('shape', [(16, 64, 64), (3, 45, 83)], ids=ids)
def test_wide_forward_exact_integers(shape, inverse):
    """regime B of the module docstring: torch.equal against float64 cast down, for every element"""
    plan = checked_wide_plan(shape)
    check_exact_integers(case(True, 96, shape, 'int'), inverse, plan)


# =====================================================================================================================================
# C. level-0 forward (conv_sub1b_fwd_kernel<8, 16>, <16, 32>, <24, 48>) where it has not been
# =====================================================================================================================================
LEVEL0_CASES = [(8, (4, 128, 128), False), (16, (4, 128, 128), False),
                (8, (2, 45, 83), True), (16, (2, 45, 83), True), (24, (2, 45, 83), True),
                (8, (4, 128, 128), True), (16, (4, 128, 128), True), (24, (4, 128, 128), True)]


@pytest.mark.parametrize('co,shape,inverse', LEVEL0_CASES, ids=[f'co{co}-{ids(s)}-{"inv" if i else "fwd"}' for co, s, i in LEVEL0_CASES])
def test_level0_forward_against_float64(co, shape, inverse):
    """sininn_conv_sub1_fwd with the method of test_fused_1x1_subnet_bf16_c_abi (tests/test_gpu_bf16.py): the whole subnet against
    float64 on the bf16-rounded operands with `close`, 1e-4 for the log-det; out2 == out; a second call and the inference call
    (no out2 / sbuf) give the same bits"""
    plan = level0_plan(shape)
    cs = case(False, co, shape, 'normal')
    c = cs.ctx(inverse, tiles=plan['ntiles'])
    res = cs.run(inverse)
    cs.check_whole('C', res, inverse, c)
    again = cs.run(inverse)
    for k in ('out', 'out2', 'sbuf'):
        assert bits_equal(res[k], again[k]), f'{k} differs between two identical calls; {c}'
    same_logdet('C', 'log-det, two identical calls', again, res, c)
    infer = cs.run(inverse, train=False)
    assert bits_equal(res['out'], infer['out']), f'out differs without out2 / sbuf; {c}'
    same_logdet('C', 'log-det, inference against the training pass', infer, res, c)


@pytest.mark.parametrize('inverse', [False, True], ids=['fwd', 'inv'])
def test_level0_forward_exact_integers(inverse):
    """regime B for co = 24 at (4, 128, 128)"""
    shape = (4, 128, 128)
    plan = level0_plan(shape)
    check_exact_integers(case(False, 24, shape, 'int'), inverse, plan)
