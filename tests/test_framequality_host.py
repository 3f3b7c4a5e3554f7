"""CPU: the frame-quality operator (sin_inn_amd.flowsynth.quality) without a device -- the composed form against the direct
numpy restatement, the error budget proved on fp32 against float64 and against seeded defects, the binding's symbols, sizes and
refusals, the held-out data set, and the command lines' new flag."""
import ctypes as C
import importlib.util
import os
import sys

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import framequality_refs as R  # noqa: E402
from sin_inn_amd import _lib, flowdata, flowsynth  # noqa: E402

SHAPES = R.shapes()
RAGGED = SHAPES[-1]


def test_window_is_the_standard_one():
    g = np.array(flowsynth.gaussian_window())
    assert g.shape == (11,) and abs(g.sum() - 1) < 1e-15 and np.array_equal(g, g[::-1])
    assert np.abs(g - R.window()).max() < 1e-16
    assert abs(g[5] / g[4] - np.exp(1 / 4.5)) < 1e-14


@pytest.mark.parametrize('shape', SHAPES, ids=str)
def test_composed_fp64_equals_the_direct_restatement(shape):
    """two separable conv2d against one direct 2-D sum per window, both in float64: apart by float64 rounding, which is the fp32 budget
    scaled by 2^-53 / 2^-24 (the derivation does not depend on the format)"""
    for kind in R.KINDS:
        pred, target, ref, budget = R.case(kind, shape)
        got = flowsynth.quality_composed(pred.double(), target.double(), ssim_map=True)
        assert got.map.dtype == torch.float64 and got.map.shape == ref['map'].shape
        ratio = float((np.abs(got.map.numpy() - ref['map']) / (budget * 2.0 ** -29)).max())
        assert ratio <= 1, (kind, ratio)
        assert np.abs(got.ssim.numpy() - ref['ssim']).max() <= (budget.reshape(shape[0], -1).mean(1) * 2.0 ** -29).max() + 2.0 ** -52
        assert np.allclose(got.mse.numpy(), ref['mse'], rtol=1e-14, atol=0)
        assert np.array_equal(np.isinf(got.psnr.numpy()), ref['mse'] == 0)
        fin = ref['mse'] > 0
        assert np.allclose(got.psnr.numpy()[fin], ref['psnr'][fin], rtol=1e-13, atol=0)


@pytest.mark.parametrize('shape', SHAPES, ids=str)
@pytest.mark.parametrize('quantize', [False, True])
def test_composed_fp32_stays_within_the_budget(shape, quantize):
    worst = 0.0
    for kind in R.KINDS:
        pred, target, ref, budget = R.case(kind, shape, quantize)
        got = flowsynth.quality_composed(pred, target, quantize=quantize, ssim_map=True)
        ratio = float((np.abs(got.map.numpy().astype(np.float64) - ref['map']) / budget).max())
        worst = max(worst, ratio)
        assert ratio <= 1, (kind, ratio)
        assert np.abs(got.ssim.numpy().astype(np.float64) - ref['ssim']).max() <= budget.reshape(shape[0], -1).mean(1).max() + 2.0 ** -23
        if quantize:
            assert np.array_equal(got.mse.numpy(), (ref['sqerr'] / (65025.0 * pred[0].numel())).astype(np.float32))
        else:
            assert np.all(np.abs(got.mse.numpy().astype(np.float64) - ref['mse']) <= 4 * R.U * ref['mse'])
        if kind == 'self':
            assert np.all(got.map.numpy() == 1.0) and np.all(got.ssim.numpy() == 1.0) and np.all(got.mse.numpy() == 0)
            assert np.all(np.isposinf(got.psnr.numpy()))
    print(f'{shape} quantize={quantize}: worst |fp32 - float64| / budget = {worst:.4f}')


def test_quantised_composed_in_fp64_uses_the_same_bytes_where_no_tie_is_near():
    pred, target = R.inputs('noise', 1, 3, 20, 23)
    a = flowsynth.quality_composed(pred, target, quantize=True)
    b = flowsynth.quality_composed(pred.double(), target.double(), quantize=True)
    assert abs(float(a.mse) - float(b.mse)) <= 1e-3 * float(b.mse)


@pytest.mark.parametrize('name', R.DEFECTS)
def test_seeded_defects_fall_outside_the_budget(name):
    """each mistake, made in float64 on the ragged 2 x 2-tile shape with noise inputs, is told from the definition by the checks the
    GPU test applies: the per-window budget, the scalar's budget, the 4 u relative bound of mse, or the map's shape"""
    pred, target, ref, budget = R.case('noise', RAGGED)
    bad = R.defect(name, pred, target)
    caught = []
    if bad['map'].shape != ref['map'].shape:
        caught.append('shape')
    elif float((np.abs(bad['map'] - ref['map']) / budget).max()) > 1:
        caught.append('map')
    if np.any(np.abs(bad['ssim'] - ref['ssim']) > budget.reshape(RAGGED[0], -1).mean(1) + 2.0 ** -23):
        caught.append('ssim')
    if np.any(np.abs(bad['sqerr'] - ref['sqerr']) > 4 * R.U * ref['sqerr']):
        caught.append('sqerr')
    print(name, '->', caught)
    assert caught, name
    expected = {'halo counted twice': 'sqerr', 'dropped last row': 'shape'}.get(name, 'map')
    assert expected in caught


def test_budget_accounts_for_the_cancellation():
    """where the variance is small against C2 the budget is set by the absolute error of E[pp] - mu^2 over C2, far above the few u of
    a well-conditioned window"""
    flat = np.full((1, 1, 11, 11), 0.75)
    rough = np.random.default_rng(0).random((1, 1, 11, 11))
    b_flat, b_rough = float(R.budget(flat, flat * 0.5).max()), float(R.budget(rough, rough[..., ::-1].copy()).max())
    assert b_flat > 2 * R.gamma(25) * 0.75 ** 2 / R.C2 > 50 * R.U      # the absolute error of E[pp] alone, over C2
    assert b_rough < b_flat


# ---- the binding ----

def test_c_symbols_and_signature():
    lib = _lib.lib()
    assert 'sininn_frame_quality' in _lib.EXPORTED and 'sininn_frame_quality_workspace_floats' in _lib.EXPORTED
    fn = lib.sininn_frame_quality
    assert fn.restype is C.c_int and len(fn.argtypes) == 14
    header = open(os.path.join(ROOT, 'include', 'sininn.h')).read()
    assert ('int sininn_frame_quality(const float* pred, const float* target, int B, int C, int H, int W, int quantize, '
            'const float* window,') in header
    assert 'int64_t sininn_frame_quality_workspace_floats(int B, int C, int H, int W);' in header


def test_workspace_query():
    lib = _lib.lib()
    ty, tx = R.tile()
    for b, c, h, w in SHAPES + [(21, 3, 436, 1024)]:
        blocks = b * c * -(-(h - 10) // ty) * -(-(w - 10) // tx)
        assert lib.sininn_frame_quality_workspace_floats(b, c, h, w) == 4 * blocks == flowsynth.quality_workspace_floats(b, c, h, w)
    for b, c, h, w in ((0, 3, 20, 20), (1, 2, 20, 20), (1, 4, 20, 20), (1, 3, 10, 20), (1, 3, 20, 10), (3, 3, 20000, 20000)):
        assert lib.sininn_frame_quality_workspace_floats(b, c, h, w) == 0


def test_c_refusals_need_no_device():
    lib = _lib.lib()
    p = C.c_void_p(256)                                                # never dereferenced: every call below is refused first
    win = (C.c_float * 11)(*flowsynth.gaussian_window())

    def refused(*a):
        assert lib.sininn_frame_quality(*a) != 0
        return lib.sininn_last_error().decode()

    big = 1 << 40
    assert refused(None, p, 1, 3, 20, 20, 0, win, p, big, p, p, None, None) == 'frame_quality: null pointer'
    assert refused(p, None, 1, 3, 20, 20, 0, win, p, big, p, p, None, None) == 'frame_quality: null pointer'
    assert refused(p, p, 1, 3, 20, 20, 0, None, p, big, p, p, None, None) == 'frame_quality: null pointer'
    assert refused(p, p, 1, 3, 20, 20, 0, win, None, big, p, p, None, None) == 'frame_quality: null pointer'
    assert refused(p, p, 1, 3, 20, 20, 0, win, p, big, None, p, None, None) == 'frame_quality: null pointer'
    assert refused(p, p, 1, 3, 20, 20, 0, win, p, big, p, None, None, None) == 'frame_quality: null pointer'
    assert refused(p, p, 1, 2, 20, 20, 0, win, p, big, p, p, None, None) == 'frame_quality: frames have 1 or 3 channels (got 2)'
    assert 'smaller than the 11 x 11 window' in refused(p, p, 1, 3, 10, 20, 0, win, p, big, p, p, None, None)
    assert 'smaller than the 11 x 11 window' in refused(p, p, 1, 3, 20, 10, 1, win, p, big, p, p, None, None)
    assert refused(p, p, 1, 3, 20, 20, 0, win, p, 11, p, p, None, None) == 'frame_quality: workspace of 11 floats, need 12'
    assert 'past an int index' in refused(p, p, 3, 3, 20000, 20000, 0, win, p, big, p, p, None, None)
    assert 'positive' in refused(p, p, 0, 3, 20, 20, 0, win, p, big, p, p, None, None)


def test_python_refusals():
    pred, target = R.inputs('noise', 1, 3, 12, 13)
    with pytest.raises(NotImplementedError, match='GPU only'):
        flowsynth.quality(pred, target)
    with pytest.raises(RuntimeError, match='flowsynth.quality is an inference operator'):
        flowsynth.quality(pred.clone().requires_grad_(True), target)
    with pytest.raises(RuntimeError, match='flowsynth.quality_composed'):
        flowsynth.quality_composed(pred, target.clone().requires_grad_(True))
    with pytest.raises(ValueError, match='1 or 3 channels'):
        flowsynth.quality_composed(pred[:, :2], target[:, :2])
    with pytest.raises(ValueError, match='smaller than the 11 x 11 window'):
        flowsynth.quality_composed(pred[..., :10], target[..., :10])


def test_composed_flattens_leading_dimensions():
    pred, target = R.inputs('noise', 6, 3, 12, 13)
    flat = flowsynth.quality_composed(pred, target, ssim_map=True)
    five = flowsynth.quality_composed(pred.view(2, 3, 3, 12, 13), target.view(2, 3, 3, 12, 13), ssim_map=True)
    assert five.psnr.shape == (2, 3) and five.map.shape == (2, 3, 3, 2, 3)
    assert torch.equal(five.ssim.reshape(-1), flat.ssim) and torch.equal(five.map.reshape(flat.map.shape), flat.map)


# ---- Holdout ----

@pytest.mark.parametrize('frames, step, kept, dropped', [(9, 2, [0, 2, 4, 6, 8], 0), (10, 2, [0, 2, 4, 6, 8], 1), (9, 3, [0, 3, 6], 2),
                                                         (10, 3, [0, 3, 6, 9], 0)])
def test_holdout_indices_times_and_held_frames(frames, step, kept, dropped):
    base = flowdata.SyntheticClip(frames, 12, 16)
    ho = flowdata.Holdout(base, step)
    assert ho.kept_indices == kept and ho.dropped == dropped and len(ho) == len(kept) - 1
    assert torch.equal(ho.video, base.video[kept]) and torch.equal(ho.T, torch.linspace(-1, 1, len(kept)))
    assert ho.flow_scale == base.flow_scale and ho.gt_available is False
    for i in range(len(ho)):
        item = ho[i]
        assert len(item) == 4 and torch.equal(item[0], base.video[kept[i]]) and torch.equal(item[1], base.video[kept[i + 1]])
        assert float(item[2]) == float(ho.T[i]) and item[3] == base.flow_scale
        held, taus = ho.held(i)
        assert torch.equal(held, base.video[kept[i] + 1:kept[i + 1]]) and held.shape[0] == step - 1
        assert taus.tolist() == [np.float32(j / step) for j in range(1, step)]
        six = ho.with_held()[i]
        assert len(six) == 6 and torch.equal(six[4], held) and torch.equal(six[5], taus)
    with pytest.raises(IndexError):
        ho.held(len(ho))


def test_holdout_refusals():
    base = flowdata.SyntheticClip(3, 12, 16)
    with pytest.raises(ValueError, match='Holdout: step = 1'):
        flowdata.Holdout(base, 1)
    with pytest.raises(ValueError, match='Holdout: a clip of 3 frames is too short for step 3'):
        flowdata.Holdout(base, 3)
    assert len(flowdata.Holdout(base, 2)) == 1


def test_get_video_wraps_both_sets():
    import types
    args = types.SimpleNamespace(synthetic=(9, 12, 16), batch=1, test_batch=2, holdout=2)
    video, scene = flowdata.get_video(None, args)
    assert scene == 'synthetic' and isinstance(video.trainset, flowdata.Holdout) and isinstance(video.testset, flowdata.Holdout)
    assert len(next(iter(video.val_dataloader()))) == 6 and len(next(iter(video.test_dataloader()))) == 4
    args.holdout = None
    plain, _ = flowdata.get_video(None, args)
    assert type(plain) is flowdata.LightningLoader and isinstance(plain.trainset, flowdata.SyntheticClip)


def test_flowtrainer_has_holdout_quality():
    from sin_inn_amd.flowtrainer import FlowTrainer
    assert callable(FlowTrainer.holdout_quality)


# ---- the command lines ----

def _load(name):
    spec = importlib.util.spec_from_file_location(name.replace('.', '_') + '_cmd', os.path.join(ROOT, 'video-interpolation', name))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def test_main_parses_holdout(capsys):
    m = _load('main.py')
    assert not hasattr(m.get_args(['train']), 'holdout')               # absent unless given: every other run is what it was
    for op in ('train', 'test'):
        assert m.get_args([op, '--synthetic', '9', '24', '40', '--holdout', '2']).holdout == 2
    with pytest.raises(SystemExit) as e:
        m.get_args(['train', '--holdout', '1'])
    assert e.value.code == 2 and 'S >= 2' in capsys.readouterr().err


def test_interpolate_holdout_sets_the_factor_and_refuses_a_conflict(capsys):
    m = _load('interpolate.py')
    base = ['--synthetic', '9', '24', '40', '--name', 'smoke', '--net', 'RBF', '--fit-epochs', '2']
    a = m.get_args(base + ['--holdout', '2'])
    assert (a.holdout, a.factor) == (2, 2)
    a = m.get_args(base + ['--holdout', '3', '--factor', '3'])
    assert (a.holdout, a.factor) == (3, 3)
    assert m.get_args(base).holdout is None and m.get_args(base).factor == 2
    with pytest.raises(SystemExit) as e:
        m.get_args(base + ['--holdout', '2', '--factor', '3'])
    assert e.value.code == 2 and 'disagree' in capsys.readouterr().err
    with pytest.raises(SystemExit):
        m.get_args(base + ['--holdout', '1'])
    capsys.readouterr()


def test_quality_records_and_means():
    m = _load('interpolate.py')
    q = lambda v: flowsynth.Quality(torch.tensor([[v, v + 1]]), torch.tensor([[v / 10, v / 10]]), torch.tensor([[v / 100, v / 100]]), None)
    recs = m.quality_records({'net': q(3.0), 'blend': q(2.0), 'repeat': q(1.0)}, first=4)
    assert [(r['pair'], r['j'], r['tau']) for r in recs] == [(4, 1, 1 / 3), (4, 2, 2 / 3)]
    assert recs[1]['psnr_net'] == 4.0 and recs[0]['psnr_repeat'] == 1.0
    means = m.quality_means(recs)
    assert means['frames'] == 2 and means['psnr_net'] == 3.5 and abs(means['ssim_blend'] - 0.2) < 1e-7
    assert len(m.quality_table(means).splitlines()) == 4
