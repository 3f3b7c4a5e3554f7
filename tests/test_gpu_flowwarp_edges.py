"""GPU: the Resample2d warp and the affine warp at coordinates no int holds (csrc/elementwise.hip), against float64.

The rule (tests/flowwarp_edge_refs.py states it and builds the inputs): a pixel whose fp32 sampling coordinate is not finite, or is
1e9 or more in size, has no footprint -- warped value 0, metric mean_c |target|, gflow 0, nothing added to gimg -- and no neighbour of
it changes by a bit.  NaN, +-inf, 3e9, -2e9, 1e30, -3.4e38, 5e8 and 1e6 are planted at pixel 0, at the last pixel (the forward's dead
lanes clone it), across a wave and a block boundary, at two tile corners of the tiled backward, three in a row, in one component only,
and beside a clean pixel whose east taps are the taps a lane without a footprint walks (the share hazard).

Method, budgets and helpers are those of tests/test_gpu_elementwise_sizes.py (`Bilinear`, `lipschitz`, `gimg_budget`, `ratio`): no
new constant.  The float64 reference samples every planted pixel at a coordinate whose four taps are outside the frame, which is the
rule (tests/test_flowwarp_edges_host.py holds that against the rule written out); the coordinate rounding bound of a planted pixel is
0, so every budget is 0 there and the kernel must give the exact value.  Every clean pixel sits 0.2 or more inside its cell, so no
pixel is exempt from any comparison.  `flowsynth.composed` against `flowsynth.synthesize` uses tests/test_gpu_flowsynth.py's budget.

Worst error / budget ratios as printed on an MI355X (run with -s), over both shapes; every exact check (0 at the planted pixels,
bitwise neighbours, finite outputs) held:
                                     fp32      bf16
  warped                             0.107     0.496   (bf16: half an ulp of the stored value)
  metric                             0.303     0.0952
  metric at planted pixels           0.188     0.0898
  gflow, tiled and flow-only         0.164     0.164   (the two kernels print the same ratio in every combination)
  gimg, tiled                        0.0144    0.0141
  affine warped / sse / gimg         0.0699 / 0.00447 (pm; nchw 0.0012: the atomics' order) / 0.00833
  synthesize against float64 0.25, against composed 0.0949 of max(4 * unit, 4 * 2^-24), unit 4.71e-07
"""
import functools
import os
import sys

import pytest
import torch

pytestmark = pytest.mark.gpu
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import flowwarp_edge_refs as R  # noqa: E402
from test_gpu_elementwise_sizes import (BF, F64, U, Bilinear, affine_coords, bf16_ulp, dev, flow_coords, gen, gimg_budget,  # noqa: E402,F401
                                        lipschitz, pixel_major, ratio)

DTYPES = {'fp32': torch.float32, 'bf16': BF}


@functools.lru_cache(maxsize=None)
def prepared(dev, name, dname):
    """inputs, the float64 footprints and the two forward runs (planted flows; the same with the planted flows set to 0) of one case,
    computed once and left unchanged"""
    from sin_inn_amd import ops
    dtype = DTYPES[dname]
    c = R.flow_case(name)
    B, C, H, W = c['shape']
    g = gen(41)
    img = torch.rand(B, C, H, W, device=dev, generator=g).to(dtype)
    tgt = torch.rand(B, C, H, W, device=dev, generator=g).to(dtype)
    flow, zeroed, planted = c['flow'].to(dev), c['zeroed'].to(dev), c['planted'].to(dev)
    # float64 footprints: the clean pixels by the kernel's formula, the planted ones with four taps outside; a planted pixel has no
    # coordinate whose rounding could matter, so its bound is 0
    _, _, dx, dy = flow_coords(zeroed, H, W)
    ix, iy = (t.to(dev) for t in R.sanitised(c['flow'], c['planted'], H, W))
    dx, dy = dx.masked_fill(planted, 0.0), dy.masked_fill(planted, 0.0)
    bl = Bilinear(img.to(F64), ix, iy)
    near = ((bl.wx1 < 2 * dx) | (bl.wx0 < 2 * dx) | (bl.wy1 < 2 * dy) | (bl.wy0 < 2 * dy)) & ~planted
    assert not bool(near.any()), 'no clean pixel is close enough to a cell boundary for fp32 to take the other cell'
    nofoot = R.no_footprint(*R.coords32(c['flow'], H, W)).to(dev)
    assert bool((nofoot & ~planted).sum() == 0) and int(nofoot.sum()) >= 7
    runs = []
    for f in (flow, zeroed):
        warped = torch.full((B, C, H, W), float('nan'), device=dev).to(dtype)
        metric = torch.full((B, 1, H, W), float('nan'), device=dev)
        ops.flow_warp_l1(img, f, tgt, warped, metric)
        runs.append((warped, metric))
    gw = torch.randn(B, C, H, W, device=dev, generator=g)
    gw[:, :, :, W // 3: W // 2] = 0                               # exact zeros upstream, as in test_flow_warp_l1_against_float64
    gm = torch.rand(B, 1, H, W, device=dev, generator=g)
    gm[:, :, :, W // 3: W // 3 + 5] = 0
    return dict(shape=c['shape'], dtype=dtype, img=img, tgt=tgt, flow=flow, zeroed=zeroed, planted=planted, nofoot=nofoot, bl=bl, dx=dx,
                dy=dy, warped=runs[0][0], metric=runs[0][1], warped0=runs[1][0], metric0=runs[1][1], gw=gw.to(dtype), gm=gm)


def px(mask, t):
    """the pixels of `mask` [B,H,W] in every channel of t [B,c,H,W]"""
    return t[mask[:, None].expand_as(t)]


@pytest.mark.parametrize('dname', list(DTYPES))
@pytest.mark.parametrize('name', list(R.SHAPES))
def test_forward_planted_pixels_are_zero_and_neighbours_untouched(dev, name, dname):
    from sin_inn_amd import ops
    p = prepared(dev, name, dname)
    B, C, H, W = p['shape']
    bl, planted, clean = p['bl'], p['planted'], ~p['planted']
    warped, metric = p['warped'], p['metric']
    tag = f'{name} {dname}'
    val, aval = bl.value()
    Lx, Ly = lipschitz(p['img'])
    bud = Lx * p['dx'][:, None] + Ly * p['dy'][:, None] + 9 * U * aval            # test_flow_warp_l1_against_float64's budget
    if p['dtype'] == BF:
        bud = bud + bf16_ulp(val)
    bud = bud.masked_fill(planted[:, None], 0.0)
    assert float(px(planted, val).abs().max()) == 0
    assert ratio(tag + ' warped', warped, val, bud) <= 1
    assert bool((px(planted, warped) == 0).all()), 'a pixel without a footprint (or with four outside taps) is exactly 0'
    w64, t64 = warped.to(F64), p['tgt'].to(F64)
    m64 = (t64 - w64).abs().mean(1, keepdim=True)
    assert ratio(tag + ' metric', metric, m64, (2 * C + 1) * U * m64) <= 1
    assert ratio(tag + ' metric at planted pixels', px(planted, metric), px(planted, t64.abs().mean(1, keepdim=True)),
                 (2 * C + 1) * U * px(planted, m64)) <= 1
    assert bool(torch.isfinite(warped).all()) and bool(torch.isfinite(metric).all())
    # no neighbour changes by a bit: no atomics here, and `share` only replaces a load by an equal value
    assert torch.equal(px(clean, warped), px(clean, p['warped0']))
    assert torch.equal(px(clean, metric), px(clean, p['metric0']))
    if p['dtype'] == torch.float32:
        m2 = torch.full_like(metric, float('nan'))
        ops.flow_warp_l1(p['img'], p['flow'], p['tgt'], None, m2)
        assert torch.equal(m2, metric)


@pytest.mark.parametrize('dname', list(DTYPES))
@pytest.mark.parametrize('name', list(R.SHAPES))
def test_backward_planted_pixels_give_no_gradient(dev, name, dname):
    from sin_inn_amd import ops
    p = prepared(dev, name, dname)
    B, C, H, W = p['shape']
    bl, planted, clean, nofoot = p['bl'], p['planted'], ~p['planted'], p['nofoot']
    img, tgt, gw, gm, dx, dy = p['img'], p['tgt'], p['gw'], p['gm'], p['dx'], p['dy']
    w64, t64 = p['warped'].to(F64), tgt.to(F64)
    sx, sy = bl.slopes()
    t00, t01, t10, t11 = bl.taps
    for use_gw, use_gm in ((True, False), (False, True), (True, True)):
        gg = torch.zeros(B, C, H, W, device=dev, dtype=F64)
        gabs = torch.zeros_like(gg)
        if use_gw:
            gg = gg + gw.to(F64)
            gabs = gabs + gw.to(F64).abs()
        if use_gm:
            s = torch.sign(t64 - w64)                             # from the staged target and warped the kernel reads
            gg = gg - s * gm.to(F64) / C
            gabs = gabs + s.abs() * gm.to(F64) / C
        # the float64 scatter: a planted pixel's taps are all outside, so it contributes nothing
        want_gimg = bl.scatter(gg)
        bud_gimg, _ = gimg_budget(bl, gabs, dx + dy, 8)
        cross = (t11 - t10 - t01 + t00).abs()
        sxa = (t01.abs() + t00.abs()) * bl.wy0[:, None] + (t11.abs() + t10.abs()) * bl.wy1[:, None]
        sya = (t10.abs() + t00.abs()) * bl.wx0[:, None] + (t11.abs() + t01.abs()) * bl.wx1[:, None]
        kx, ky = W / (W - 1), H / (H - 1)
        want_gf = torch.stack(((gg * sx).sum(1) * kx, (gg * sy).sum(1) * ky), 1)
        bud_gf = torch.stack((((gabs * cross).sum(1) * dy + (C + 13) * U * (gabs * sxa).sum(1)) * kx,
                              ((gabs * cross).sum(1) * dx + (C + 13) * U * (gabs * sya).sum(1)) * ky), 1)
        assert float(px(planted, want_gf).abs().max()) == 0 and float(px(planted, bud_gf).abs().max()) == 0
        which = f'{name} {dname} {"gw" if use_gw else ""}{"+" if use_gw and use_gm else ""}{"gm" if use_gm else ""}'

        def run(flow, warped, with_gimg):
            gimg = torch.zeros(B, C, H, W, device=dev) if with_gimg else None
            gflow = torch.full((B, 2, H, W), float('nan'), device=dev)
            ops.flow_warp_l1_bwd(img, flow, tgt if use_gm else None, warped if use_gm else None, gw if use_gw else None,
                                 gm if use_gm else None, gimg, gflow)
            return gimg, gflow

        for kernel, with_gimg in (('tiled', True), ('flow-only', False)):
            gimg, gflow = run(p['flow'], p['warped'], with_gimg)
            assert bool(torch.isfinite(gflow).all())
            assert bool((px(nofoot, gflow) == 0).all()) and bool((px(planted, gflow) == 0).all())
            assert ratio(f'{which} gflow ({kernel})', gflow, want_gf, bud_gf) <= 1
            _, gflow0 = run(p['zeroed'], p['warped0'], with_gimg)
            assert torch.equal(px(clean, gflow), px(clean, gflow0))
            if with_gimg:
                assert ratio(f'{which} gimg (tiled)', gimg, want_gimg, bud_gimg) <= 1


@pytest.mark.parametrize('dname', list(DTYPES))
def test_autograd_returns_the_same_zeros_with_and_without_an_image_gradient(dev, dname):
    """which backward kernel `functional.flow_warp_l1` runs depends only on whether the image requires a gradient"""
    from sin_inn_amd import functional
    p = prepared(dev, 'ragged', dname)
    got = []
    for img_grad in (True, False):
        img = p['img'].clone().requires_grad_(img_grad)
        flow = p['flow'].clone().requires_grad_(True)
        warped, metric = functional.flow_warp_l1(img, flow, p['tgt'])
        ((warped.float() * p['gw'].float()).sum() + (metric * p['gm']).sum()).backward()
        assert bool(torch.isfinite(flow.grad).all())
        assert (img.grad is not None) == img_grad and (not img_grad or bool(torch.isfinite(img.grad).all()))
        got.append(flow.grad)
    assert bool((px(p['planted'], got[0]) == 0).all()) and bool((px(p['planted'], got[1]) == 0).all())
    assert torch.equal(got[0] == 0, got[1] == 0)


@pytest.mark.parametrize('pm', [False, True], ids=['nchw', 'pm'])
def test_affine_warp_bad_thetas(dev, pm):
    from sin_inn_amd import ops
    shape = R.AFFINE_SHAPE
    B, C, H, W = shape
    total = B * C * H * W
    blocks, trips = -(-total // 256), 1                            # one trip of affine_warp_launch's grid
    assert blocks < 8192
    g = gen(43)
    lay = pixel_major if pm else (lambda t: t)
    img = lay(torch.rand(shape, device=dev, generator=g))
    ref = lay(torch.rand(shape, device=dev, generator=g))
    assert (img.stride(1) == 1) == pm
    theta = R.affine_thetas(H, W).to(dev)
    bad = R.no_footprint(*R.affine_coords32(theta.cpu(), H, W)).to(dev)
    assert not bool(bad[0].any()) and bool(bad[1:].all())
    # float64: sample 0 by affine_src's formula, samples 1 and 2 with four taps outside
    good = torch.where(torch.isfinite(theta) & (theta.abs() < 1e9), theta, torch.zeros_like(theta))
    ix, iy, dx, dy = affine_coords(good, H, W)
    out_of_frame = torch.full_like(ix, R.OUTSIDE)
    ix, iy = torch.where(bad, out_of_frame, ix), torch.where(bad, out_of_frame, iy)
    dx, dy = dx.masked_fill(bad, 0.0), dy.masked_fill(bad, 0.0)
    bl = Bilinear(img.to(F64), ix, iy)
    dropped = sum(int((~ok[0]).sum()) for ok in bl.ok) / (4.0 * H * W)
    assert dropped > 0.02, 'a visible share of sample 0 leaves the frame'
    val, aval = bl.value()
    Lx, Ly = lipschitz(img)
    bud = Lx * dx[:, None] + Ly * dy[:, None] + 9 * U * aval
    tag = f'affine {"pm" if pm else "nchw"}'
    out = lay(torch.full(shape, float('nan'), device=dev))
    ops.affine_warp(img, theta, out)
    assert ratio(tag + ' warped', out, val, bud) <= 1
    assert bool((out[1:] == 0).all())
    alone = lay(torch.full((1, C, H, W), float('nan'), device=dev))
    ops.affine_warp(img[:1], theta[:1].contiguous(), alone)
    assert torch.equal(out[:1], alone)
    # fused SSE (test_affine_warp_against_float64's budget): the bad samples contribute sum ref^2
    out2 = lay(torch.full(shape, float('nan'), device=dev))
    sse = torch.zeros(1, device=dev)
    ops.affine_warp(img, theta, out2, ref, sse)
    assert torch.equal(out2, out)
    d = val - ref.to(F64)
    assert torch.equal(d[1:], -ref.to(F64)[1:])
    sse_bud = (2 * d.abs() * bud + bud * bud).sum() + (trips + 6 + 3 + blocks + 2) * U * (d * d).sum()
    assert ratio(tag + ' sse', sse[0], (d * d).sum(), sse_bud) <= 1
    # backward, into a zeroed buffer
    gout = lay(torch.randn(shape, device=dev, generator=g))
    want = bl.scatter(gout.to(F64))
    gbud, _ = gimg_budget(bl, gout.to(F64).abs(), dx + dy, 4)
    gimg = lay(torch.zeros(shape, device=dev))
    ops.affine_warp_bwd(gout, theta, gimg)
    assert bool((gimg[1:] == 0).all())
    assert float(want[1:].abs().max()) == 0
    assert ratio(tag + ' gimg', gimg, want, gbud) <= 1


def test_composed_and_synthesize_agree_at_non_finite_flows(dev):
    """`composed` runs flow_warp_l1, `synthesize` the fused `warp_taps`: with one rule they agree at a NaN and an inf flow.  The float64
    form cannot take a NaN, so it gets a flow of 1e6 at those pixels, which is the rule for 0 < tau < 1: the warp samples outside the
    frame (metric mean |target|) and tau * 1e6 lands outside it (nothing is splatted)."""
    import flowsynth_refs as SR
    from test_gpu_flowsynth import FLOOR, MULT
    from sin_inn_amd import flowsynth
    taus = (0.3, 0.7)
    i0, i1, f01, f10 = SR.random_inputs(0, 1, 3, 13, 37)
    sites = ((0, slice(None), 4, 9, float('nan')), (1, slice(None), 7, 20, float('inf')), (0, 0, 9, 30, float('-inf')))
    sub01, sub10 = f01.clone(), f10.clone()
    for which, comp, y, x, v in sites:
        (f01, f10)[which][0, comp, y, x] = v
        (sub01, sub10)[which][0, :, y, x] = 1e6
    x64 = SR.composed64(i0, i1, sub01, sub10, taus)
    keep = ~SR.excluded(sub01, sub10, taus)
    assert float((~keep).float().mean()) <= SR.MAX_EXCLUDED
    keep = keep[:, :, None].expand_as(x64)
    a = [t.to(dev) for t in (i0, i1, f01, f10)]
    x32 = flowsynth.composed(*a, taus)
    got = flowsynth.synthesize(*a, taus)
    assert bool(torch.isfinite(x32).all()) and bool(torch.isfinite(got).all())
    unit = float(((x32.to(F64).cpu() - x64).abs() * keep).max())
    budget = max(MULT * unit, FLOOR)
    err = float(((got.to(F64).cpu() - x64).abs() * keep).max())
    each = float(((got.to(F64) - x32.to(F64)).cpu().abs() * keep).max())
    print(f'ratio(synthesize vs float64) = {err / budget:.3g}   ratio(synthesize vs composed) = {each / budget:.3g}   '
          f'[fp32-composed unit {unit:.3g}, budget {budget:.3g}]')
    assert err <= budget and each <= budget
