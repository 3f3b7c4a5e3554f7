"""CPU: the occlusion-aware gather rule (sin_inn_amd.flowsynth.gather_composed(.., visible=)) from its definition, and
`flowdata.LayeredClip`, the clip with real occlusion that shows what the rule is for.

The float64 restatement and the cases are those of tests/flowgather_visible_refs.py.  What runs the new code and fails without it:
every test here but the parser's -- the keyword, the clip and the option do not exist before.
"""
import importlib.util
import os
import sys

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import flowgather_visible_refs as V  # noqa: E402
from sin_inn_amd import flowdata, flowsynth  # noqa: E402

F64 = torch.float64


def _composed(dtype, i0, i1, fl, slots, taus, m0, m1):
    return flowsynth.gather_composed(i0.to(dtype), i1.to(dtype), fl.to(dtype), slots, taus, visible=(m0, m1))


# ---- 1(a), 1(c): against the float64 restatement, at the smallest shapes where taps, masks and edges interact ----

@pytest.mark.parametrize('name', V.HOST_CASES)
def test_composed_float64_agrees_with_the_restatement(name):
    i0, i1, fl, slots, taus, m0, m1 = V.case(name)
    x64, budget = V.gather_visible64(i0, i1, fl, slots, taus, m0, m1)
    got = _composed(F64, i0, i1, fl, slots, taus, m0, m1)
    assert got.dtype == F64 and got.shape == x64.shape == (i0.shape[0], len(taus)) + tuple(i0.shape[1:])
    assert bool(torch.isfinite(got).all())
    err = float((got - x64).abs().max())
    print(f'gather_composed(visible=) fp64 {name}: largest difference {err:.3g}')
    assert err <= 1e-12
    # and in fp32 it stays inside the budget of its roundings
    got32 = _composed(torch.float32, i0, i1, fl, slots, taus, m0, m1)
    ratio = float(((got32.to(F64) - x64).abs() / budget).max())
    print(f'gather_composed(visible=) fp32 {name}: worst err / budget {ratio:.3f}')
    assert got32.dtype == torch.float32 and ratio <= 1.0


def test_the_cases_hold_what_they_claim():
    """landing points outside the frame on every side, exactly on integer pixels, non-finite; masks 0, 1, between and outside [0, 1]"""
    i0, i1, fl, slots, taus, m0, m1 = V.case('9x33')
    b, c, h, w = i0.shape
    coef = flowsynth.slot_coefficients(slots)
    ys, xs = torch.meshgrid(torch.arange(h, dtype=torch.float32), torch.arange(w, dtype=torch.float32), indexing='ij')
    sides = {'left': False, 'right': False, 'above': False, 'below': False, 'integer': False, 'non-finite': False}
    for bb in range(b):
        for kk in range(len(taus)):
            for which in (0, 1):
                g = fl[slots[bb, kk, which], slots[bb, kk, 2 + which]:slots[bb, kk, 2 + which] + 2]
                qx, qy = xs + coef[bb, kk, which] * g[0], ys + coef[bb, kk, which] * g[1]
                fin = torch.isfinite(qx) & torch.isfinite(qy)
                sides['left'] |= bool((qx[fin] < -1).any())
                sides['right'] |= bool((qx[fin] > w).any())
                sides['above'] |= bool((qy[fin] < -1).any())
                sides['below'] |= bool((qy[fin] > h).any())
                moved = fin & ((g[0] != 0) | (g[1] != 0)) & (coef[bb, kk, which] != 0)
                sides['integer'] |= bool(((qx == qx.floor()) & (qy == qy.floor()) & moved).any())
                sides['non-finite'] |= bool((~fin).any())
    assert all(sides.values()), sides
    for m in (m0, m1):
        assert bool((m == 0).any()) and bool((m == 1).any()) and bool(((m > 0) & (m < 1)).any())
        assert bool((m > 1).any()) and bool((m < 0).any())
    assert bool(((m0 == 0) & (m1 == 0)).any())
    assert V.CASES['1x1'][5] == (0.5,) and len(V.CASES['2x3'][5]) == 3 and V.CASES['2x3'][2] == 1 and V.CASES['9x33'][2] == 3


# ---- 1(b): all-ones masks are the plain rule, to the bit ----

@pytest.mark.parametrize('name', V.HOST_CASES)
def test_all_ones_masks_give_the_plain_rule_bits(name):
    i0, i1, fl, slots, taus, m0, _ = V.case(name)
    ones = torch.ones_like(m0)
    plain = flowsynth.gather_composed(i0, i1, fl, slots, taus)
    got = flowsynth.gather_composed(i0, i1, fl, slots, taus, visible=(ones, ones))
    assert got.dtype == torch.float32 and torch.equal(got, plain)
    assert torch.equal(flowsynth.gather_composed(i0, i1, fl, slots, taus, visible=(ones.bool(), ones.bool())), plain)
    assert not torch.equal(flowsynth.gather_composed(i0, i1, fl, slots, taus, visible=(m0, ones)), plain) or name == '1x1'


# ---- 1(c): both masks zero falls back to L ----

@pytest.mark.parametrize('dtype', [torch.float32, F64])
def test_both_masks_zero_is_the_linear_blend(dtype):
    """flows 0, so q = p and every sample has its one tap inside: o0 = o1 = 1, v = 0, b = 0 and out = e L / e"""
    i0, i1, _, _, _, _, _ = V.case('9x33')
    b, c, h, w = i0.shape
    taus = (0.0, 0.3, 1.0)
    _, slots = flowsynth.gather_slots([0.0] * b, taus, 1.0, 'reverse')
    fl = torch.zeros(b * len(taus), 4, h, w)
    zero = torch.zeros(b, 1, h, w)
    got = _composed(dtype, i0, i1, fl, slots, taus, zero, zero)
    tau = torch.tensor(taus, dtype=torch.float32).to(dtype).view(1, -1, 1, 1, 1)
    lin = (1 - tau) * i0.to(dtype)[:, None] + tau * i1.to(dtype)[:, None]
    assert torch.equal(got, lin) if dtype == torch.float32 else float((got - lin).abs().max()) <= 1e-12
    # one mask zero: the other frame's sample alone (plus the e L term)
    one = torch.ones(b, 1, h, w)
    only0 = _composed(F64, i0, i1, fl, slots, taus, one, zero)         # m1 = 0: what frame 1 shows is hidden in frame 0 -> v0 = 0
    t = float(np.float32(0.3))                                         # the time as the rule sees it
    if dtype == F64:
        assert float((only0[:, 1] - (t * i1.to(F64) + V.EPS * lin[:, 1]) / (t + V.EPS)).abs().max()) <= 1e-12


# ---- 1(d): LayeredClip ----

@pytest.fixture(scope='module')
def clip():
    return flowdata.LayeredClip(5, 24, 40)


def test_layered_clip_interface(clip):
    assert clip.video.shape == (5, 3, 24, 40) and clip.video.dtype == torch.float32
    assert clip.flow.shape == (4, 2, 24, 40) and clip.flow.dtype == torch.float32
    assert clip.gt_available is True and clip.flow_scale == 40 / 5 and torch.equal(clip.T, torch.linspace(-1, 1, 5))
    assert len(clip) == 4 and len(clip[1]) == 5 and torch.equal(clip[1][0], clip.video[1]) and torch.equal(clip[1][4], clip.flow[1])
    assert (clip.rh, clip.rw) == (8, 13)
    for i in range(5):
        front = clip.covered(float(i), clip.xx, clip.yy)
        assert int(front.sum()) == 8 * 13                                  # inside the frame for the whole clip, pixel-exact
        assert torch.equal(clip.frame_at(i).to(torch.float32), clip.video[i])
    held = flowdata.Holdout(clip, 2)
    assert held.video.shape[0] == 3 and torch.equal(held.video[1], clip.video[2]) and torch.equal(held.held(0)[0][0], clip.video[1])
    with pytest.raises(ValueError, match='leaves a frame'):
        flowdata.LayeredClip(40, 24, 40)


def test_layered_clip_flow_warps_visible_pixels_exactly(clip):
    for i in range(4):
        fl = clip.flow_between(i, i + 1)
        assert torch.equal(fl.to(torch.float32), clip.flow[i])
        there = clip.sample_at(float(i + 1), clip.xx + fl[0], clip.yy + fl[1])            # frame i + 1 where the flow lands, float64
        here = clip.frame_at(i)
        vis = clip.visible(i, i + 1)
        err = (there - here).abs().amax(0)
        assert float(err[vis].max()) <= 1e-9
        hidden = ~vis
        assert int(hidden.sum()) > 0 and float(err[hidden].min()) > 1e-6                  # another surface is found there
        # the band the rectangle's motion predicts: background pixels of frame i that the rectangle, moving by fg - bg relative to
        # the background, sweeps over by i + 1
        x0, y0 = clip.x0 + i * clip.fg[0], clip.y0 + i * clip.fg[1]
        x1, y1 = x0 + clip.fg[0] - clip.bg[0], y0 + clip.fg[1] - clip.bg[1]                # the rectangle at i + 1, carried back
        inside = lambda x, y: (clip.xx >= x) & (clip.xx < x + clip.rw) & (clip.yy >= y) & (clip.yy < y + clip.rh)  # noqa: E731
        assert torch.equal(hidden, inside(x1, y1) & ~inside(x0, y0))
        print(f'LayeredClip pair {i}: {int(hidden.sum())} of {hidden.numel()} pixels of frame {i} are hidden in frame {i + 1}, '
              f'{int((~clip.visible(i + 1, i)).sum())} the other way')
        assert int((~clip.visible(i + 1, i)).sum()) > 0


# ---- 1(e): the point of the feature ----

def test_masked_rule_beats_the_plain_rule_where_one_frame_shows_the_surface():
    """Analytic flows and masks at s = i + 1/2, velocities of whole pixels per half frame: every landing point is an integer pixel, so
    a sample is one tap and a mask value is read unmixed.  The 8 x 13 rectangle moves by (-2, 1) per half frame relative to the
    background, so it uncovers 2 * 8 + 1 * 13 - 2 * 1 = 27 background pixels behind it and covers as many ahead: a one-frame band of 54
    pixels per pair (required below: a condition on the clip, not a measurement)."""
    clip = flowdata.LayeredClip(5, 24, 40, bg=(2.0, 0.0), fg=(-2.0, 2.0))
    one = int(np.float32(1.0).view(np.int32))
    slots = torch.tensor([[[0, 0, 2, 0, one, one]]], dtype=torch.int32)
    for i in range(4):
        s = i + 0.5
        flows = torch.cat([clip.flow_between(s, i + 1), clip.flow_between(s, i)])[None]        # channels 0-1: G1, 2-3: G0
        i0, i1 = clip.frame_at(i)[None], clip.frame_at(i + 1)[None]
        m0, m1 = clip.visible(i, i + 1)[None, None].to(F64), clip.visible(i + 1, i)[None, None].to(F64)
        truth = clip.frame_at(s)
        plain = flowsynth.gather_composed(i0, i1, flows, slots, [0.5])[0, 0]
        masked = flowsynth.gather_composed(i0, i1, flows, slots, [0.5], visible=(m0, m1))[0, 0]
        assert masked.dtype == F64
        back = ~clip.covered(s, clip.xx, clip.yy)
        shown0 = ~(back & clip.covered(float(i), clip.xx - 0.5 * clip.bg[0], clip.yy - 0.5 * clip.bg[1]))
        shown1 = ~(back & clip.covered(float(i + 1), clip.xx + 0.5 * clip.bg[0], clip.yy + 0.5 * clip.bg[1]))
        band, both = shown0 ^ shown1, shown0 & shown1
        assert int(band.sum()) == 54 and int(both.sum()) > 0 and not bool((~shown0 & ~shown1).any())
        assert int((band & shown0).sum()) == 27 and int((band & shown1).sum()) == 27             # both worked cases of DESIGN 26.2 occur
        err_plain = float((plain - truth).abs()[:, band].mean())
        err_masked = float((masked - truth).abs()[:, band].mean())
        print(f'pair {i}: one-frame band {int(band.sum())} pixels, mean |error| plain {err_plain:.4f}, masked {err_masked:.4f}; '
              f'both-frames pixels {int(both.sum())}, largest difference {float((plain - masked).abs()[:, both].max()):.3g}')
        assert err_masked < err_plain
        assert float((plain - masked).abs()[:, both].max()) <= 1e-12


# ---- 1(f): refusals ----

def test_refusals():
    i0, i1, fl, slots, taus, m0, m1 = V.case('9x33')
    for fn in (flowsynth.gather, flowsynth.gather_composed):
        with pytest.raises(ValueError, match='no gradient yet'):
            fn(i0, i1, fl.clone().requires_grad_(True), slots, taus, visible=(m0, m1), flow_grad=True)
        with pytest.raises(ValueError, match=r'\(2, 1, 9, 33\)'):
            fn(i0, i1, fl, slots, taus, visible=(m0[:, :, :-1], m1))
        with pytest.raises(ValueError, match=r'\(2, 1, 9, 33\)'):
            fn(i0, i1, fl, slots, taus, visible=(m0, m1.expand(2, 3, 9, 33)))
        with pytest.raises(ValueError, match='pair of masks'):
            fn(i0, i1, fl, slots, taus, visible=m0)
        with pytest.raises(RuntimeError, match='no gradient'):
            fn(i0, i1, fl, slots, taus, visible=(m0.clone().requires_grad_(True), m1))
    with pytest.raises(NotImplementedError):
        flowsynth.gather(i0, i1, fl, slots, taus, visible=(m0, m1))           # the fused operator runs on the GPU only
    with pytest.raises(TypeError):
        flowsynth.gather_at(i0, i1, fl, None, None, None, visible=(m0, m1))


def _interpolate_cli():
    spec = importlib.util.spec_from_file_location('interpolate_cli', os.path.join(ROOT, 'video-interpolation', 'interpolate.py'))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def test_occlusion_option_needs_the_gather_synthesis(capsys):
    cli = _interpolate_cli()
    base = ['--layered', '5', '24', '40', '--name', 'x', '--net', 'RBF']
    a = cli.get_args(base + ['--synthesis', 'gather', '--occlusion', 'wang'])
    assert a.occlusion == 'wang' and a.layered == [5, 24, 40] and a.synthetic is None
    assert cli.get_args(base + ['--synthesis', 'gather']).occlusion is None
    for argv in (base + ['--occlusion', 'wang'], base + ['--synthesis', 'splat', '--occlusion', 'brox']):
        with pytest.raises(SystemExit) as e:
            cli.get_args(argv)
        assert e.value.code == 2
        assert 'only with --synthesis gather' in capsys.readouterr().err
    with pytest.raises(SystemExit):
        cli.get_args(base + ['--synthetic', '5', '24', '40'])                  # one clip


def test_layered_option_reaches_the_data_module():
    cli = _interpolate_cli()
    m = cli.flow_main()
    args = m.get_args(['train', '--layered', '5', '24', '40', '--holdout', '2'])
    assert args.layered == [5, 24, 40] and not hasattr(m.get_args(['train']), 'layered')
    video, scene = flowdata.get_video(None, args)
    assert scene == 'layered' and isinstance(video.trainset, flowdata.Holdout) and isinstance(video.trainset.base, flowdata.LayeredClip)
    assert video.trainset.video.shape == (3, 3, 24, 40)
    with pytest.raises(SystemExit):
        m.get_args(['train', '--layered', '5', '24', '40', '--synthetic', '5', '24', '40'])
