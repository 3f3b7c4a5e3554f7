"""CPU: the conditions the inputs of tests/test_gpu_flowwarp_edges.py exist for, checked on the reference alone
(tests/flowwarp_edge_refs.py).  No kernel runs here."""
import math
import os
import sys

import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import flowwarp_edge_refs as R  # noqa: E402

F64 = torch.float64


@pytest.fixture(scope='module')
def cases():
    return {name: R.flow_case(name) for name in R.SHAPES}


def _same_class(a, b):
    return (math.isnan(a) and math.isnan(b)) or a == b


@pytest.mark.parametrize('name', list(R.SHAPES))
def test_every_value_class_is_planted_where_it_belongs(cases, name):
    c = cases[name]
    B, C, H, W = c['shape']
    bad = R.no_footprint(*R.coords32(c['flow'], H, W))
    assert bool((bad & ~c['planted']).sum() == 0), 'only planted pixels lose their footprint'
    seen = {v: 0 for v in R.VALUES if not math.isnan(v)}
    seen_nan = 0
    for b, y, x, vx, vy in c['sites']:
        v = vx if vx is not None else vy
        if math.isnan(v):
            seen_nan += 1
        else:
            seen[v] += 1
        assert bool(bad[b, y, x]) == (not any(_same_class(v, h) for h in R.HUGE_VALUES)), (b, y, x, v)
    assert seen_nan >= 1 and all(n >= 1 for n in seen.values()), seen
    # one pixel with only fx bad, one with only fy bad: the other component is a clean flow
    only = [s for s in c['sites'] if (s[3] is None) != (s[4] is None)]
    assert sorted((s[3] is None, s[4] is None) for s in only) == [(False, True), (True, False)]
    for b, y, x, vx, vy in only:
        other = c['flow'][b, 1 if vy is None else 0, y, x]
        assert bool(torch.isfinite(other)) and abs(float(other)) < 100 and bool(bad[b, y, x])
    # the sites the kernels' launch shapes make special
    where = {s[:3] for s in c['sites']}
    flat = lambda i: (0, i // W, i % W)
    assert {flat(0), (B - 1, H - 1, W - 1), flat(63), flat(64), flat(255), flat(256), (0, 7, 31), (0, 8, 32)} <= where
    if name == 'ragged':
        assert B * H * W == 1710 and (B * H * W) % 64 != 0, 'the last wave has dead lanes'
    row = sorted(x for b, y, x in where if (b, y) == (0, 12))
    assert row == [row[0], row[0] + 1, row[0] + 2]


@pytest.mark.parametrize('name', list(R.SHAPES))
def test_huge_flows_below_the_guard_keep_a_footprint_of_four_outside_taps(cases, name):
    c = cases[name]
    B, C, H, W = c['shape']
    ix32, iy32 = R.coords32(c['flow'], H, W)
    found = set()
    for b, y, x, vx, vy in c['sites']:
        if vx in R.HUGE_VALUES:
            found.add(vx)
            cx, cy = float(ix32[b, y, x]), float(iy32[b, y, x])
            assert abs(cx) < R.GUARD and abs(cy) < R.GUARD and abs(cx) < 2 ** 31 - 2
            x0, y0 = math.floor(cx), math.floor(cy)
            assert all(not (0 <= yy < H and 0 <= xx < W) for yy in (y0, y0 + 1) for xx in (x0, x0 + 1))
    assert found == set(R.HUGE_VALUES)


@pytest.mark.parametrize('name', list(R.SHAPES))
def test_clean_pixels_sit_inside_their_cells_and_reach_every_path(cases, name):
    c = cases[name]
    B, C, H, W = c['shape']
    clean = ~c['planted']
    ix, iy = R.sanitised(c['flow'], c['planted'], H, W)
    # the exempt set of test_flow_warp_l1_against_float64 (a fraction within 2 delta of a cell boundary) is empty: every fraction is 0.2
    # or more from a boundary, in float64 and in the fp32 formula, and both take the same cell
    ix32, iy32 = R.coords32(c['zeroed'], H, W)
    for c64, c32 in ((ix, ix32), (iy, iy32)):
        for coord in (c64, c32.to(F64)):
            fr = (coord - coord.floor())[clean]
            assert float(fr.min()) >= 0.2 and float(fr.max()) <= 0.8
        assert torch.equal(c64.floor()[clean], c32.to(F64).floor()[clean])
    dropped, far = R.window_census(ix, iy, clean)
    print(name, dict(dropped=dropped, far=far))
    assert dropped >= 100 and far >= 100
    # the three kinds
    zx, zy = R.coords64(torch.zeros_like(c['flow']), H, W)
    move = torch.maximum((ix - zx).abs(), (iy - zy).abs())[clean]
    assert int((move < 1).sum()) >= 100 and int(((move >= 8) & (move <= 42)).sum()) >= 100
    if name == 'ragged':
        assert W % R.FB_TX != 0 and H % R.FB_TY != 0, 'tiles ragged on both axes'
    if name == 'pass2':
        assert C > 4, 'the second channel pass of the tiled window'


@pytest.mark.parametrize('name', list(R.SHAPES))
def test_share_pair_has_the_intended_footprints_in_fp32(cases, name):
    c = cases[name]
    B, C, H, W = c['shape']
    ix32, iy32 = R.coords32(c['flow'], H, W)
    (y, x), (by, bx) = R.SHARE_CLEAN, R.SHARE_BAD
    assert (by, bx) == (y, x + 1) and x + 1 < W, 'the next lane of the same row'
    assert not bool(c['planted'][0, y, x]) and bool(R.no_footprint(ix32, iy32)[0, by, bx])
    x0, y0 = math.floor(float(ix32[0, y, x])), math.floor(float(iy32[0, y, x]))
    # the sentinel of a lane without a footprint is the north-west tap of coordinate (0, 0): (0, 0) == (y0, x0 + 1)
    assert (y0, x0) == (0, -1)
    assert (0 * H * W + y * W + x) % 64 != 63, 'both pixels in one wave'


@pytest.mark.parametrize('name', list(R.SHAPES))
def test_reference_of_clean_pixels_ignores_the_planted_flows(cases, name):
    c = cases[name]
    B, C, H, W = c['shape']
    g = torch.Generator().manual_seed(1)
    img, tgt = torch.rand(B, C, H, W, generator=g), torch.rand(B, C, H, W, generator=g)
    w_planted, w_zeroed = R.warp64(img, c['flow']), R.warp64(img, c['zeroed'])
    keep = (~c['planted'])[:, None].expand_as(w_planted)
    assert torch.equal(w_planted[keep], w_zeroed[keep])
    m_planted, m_zeroed = R.metric64(tgt, w_planted), R.metric64(tgt, w_zeroed)
    assert torch.equal(m_planted[~c['planted'][:, None]], m_zeroed[~c['planted'][:, None]])
    # the rule at the planted pixels: 0, and mean |target|; the sanitised coordinates state the same reference
    assert float(w_planted[c['planted'][:, None].expand_as(w_planted)].abs().max()) == 0
    assert torch.equal(m_planted[c['planted'][:, None]], tgt.to(F64).abs().mean(1, keepdim=True)[c['planted'][:, None]])
    ix, iy = R.sanitised(c['flow'], c['planted'], H, W)
    again = sum(t * w[:, None] for t, w, _, _, _ in R.taps64(img, ix, iy))
    assert torch.equal(again, w_planted)


def test_affine_thetas():
    B, C, H, W = R.AFFINE_SHAPE
    th = R.affine_thetas(H, W)
    assert th.shape == (B, 2, 3) and th.dtype == torch.float32
    assert math.isnan(float(th.reshape(B, 6)[1, 2])) and float(th.reshape(B, 6)[2, 5]) == 1e10
    assert bool(torch.isfinite(th[0]).all()) and int(torch.isfinite(th).sum()) == 6 * B - 1
    bad = R.no_footprint(*R.affine_coords32(th, H, W))
    assert not bool(bad[0].any()) and bool(bad[1].all()) and bool(bad[2].all())
    # sample 0 drops a visible share of its taps
    ix, iy = R.affine_coords32(th[:1], H, W)
    dropped = sum(int((~inside).sum()) for _, _, inside, _, _ in R.taps64(torch.zeros(1, 1, H, W), ix.to(F64), iy.to(F64)))
    assert dropped / (4.0 * H * W) > 0.02
