"""GPU: the fused frame-quality operator (csrc/framequality.hip, sin_inn_amd.flowsynth.quality) against float64.

The reference is tests/framequality_refs.reference, the definition summed directly in numpy float64 on the same fp32 inputs; the
tolerance of `ssim_map` is framequality_refs.budget, derived per window from the roundings of the operations (its module text) and
proved on the CPU in tests/test_framequality_host.py.  Nothing is excluded.

The scalars.  `ssim` is the double mean of the fp32 window values, rounded to fp32 once: within the mean of the window budgets plus
2^-23.  `mse` in float mode: the difference is rounded (u = 2^-24 relative), squaring doubles that (2 u), the square is rounded (3 u),
the sum and the division run in double, and the cast to fp32 rounds once more: 4 u relative.  In quantised mode `sqerr` is an integer
sum and is compared exactly, `mse` is that integer divided once.  `psnr` has no tolerance of its own: it is 10 log10(1 / mse) of the
double mse, held to the rounding of its fp32 cast (and one unit for log10 itself).

No loop of the kernels is grid-strided (one block per tile; the finish kernel's loop strides over a frame's partials, which the
shapes above fill with at most 12 and `test_many_tiles` with 270, past the kernel's 256 threads).
"""
import json
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import framequality_refs as R  # noqa: E402
import flowtrainer_refs as TR  # noqa: E402
from sin_inn_amd import flowdata, flowsynth, flowtrainer  # noqa: E402

U = R.U
SHAPES = R.shapes()


@pytest.fixture(scope='module')
def dev():
    assert torch.cuda.is_available(), 'GPU tests need a GPU'
    return torch.device('cuda', 0)


def _check(what, got, sqerr, ref, budget, quantize, pixels):
    """every check of one call against its float64 reference; returns the worst |ssim_map - float64| / budget"""
    b = ref['mse'].shape[0]
    smap = got.map.cpu().numpy().astype(np.float64).reshape(ref['map'].shape)
    ratio = float((np.abs(smap - ref['map']) / budget).max())
    ssim, mse, psnr = (t.cpu().numpy().astype(np.float64).reshape(b) for t in (got.ssim, got.mse, got.psnr))
    ssim_err = np.abs(ssim - ref['ssim'])
    ssim_budget = budget.reshape(b, -1).mean(1) + 2.0 ** -23
    print(f'framequality {what}: ssim_map worst |err| / budget {ratio:.4f} (budget up to {budget.max():.3g}); '
          f'ssim err {ssim_err.max():.3g} of {ssim_budget.min():.3g}; mse rel err '
          f'{float((np.abs(mse - ref["mse"]) / np.where(ref["mse"] == 0, 1, ref["mse"])).max()):.3g}')
    assert np.all(np.isfinite(smap)) and ratio <= 1, (what, ratio)
    assert np.all(ssim_err <= ssim_budget), (what, ssim_err, ssim_budget)
    if quantize:
        assert np.array_equal(sqerr, ref['sqerr']), (what, sqerr, ref['sqerr'])
        assert np.array_equal(got.mse.cpu().numpy().reshape(b), (ref['sqerr'] / (65025.0 * pixels)).astype(np.float32)), what
    else:
        assert np.all(np.abs(sqerr - ref['sqerr']) <= (3 * U + 1e-13) * ref['sqerr']), what
        assert np.all(np.abs(mse - ref['mse']) <= 4 * U * ref['mse']), (what, mse, ref['mse'])
    mse64 = sqerr / ((65025.0 if quantize else 1.0) * pixels)
    zero = mse64 == 0
    assert np.all(np.isposinf(psnr[zero]))
    want = 10 * np.log10(1 / mse64[~zero])
    assert np.all(np.abs(psnr[~zero] - want) <= 2.0 ** -23 * np.abs(want) + 1e-12), (what, psnr, want)
    return ratio


def _sqerr(pred, target, dev, quantize):
    """the operator's double sqerr output, through the C call"""
    import ctypes as C
    from sin_inn_amd import _lib
    from sin_inn_amd.ops import _stream, ptr
    p, t = pred.to(dev).contiguous(), target.to(dev).contiguous()
    b, c, h, w = p.shape
    ws = torch.empty(flowsynth.quality_workspace_floats(b, c, h, w), device=dev)
    sq = torch.empty(b, device=dev, dtype=torch.float64)
    out = torch.empty(3, b, device=dev)
    _lib.check(_lib.lib().sininn_frame_quality(ptr(p), ptr(t), b, c, h, w, int(quantize), flowsynth._WINDOW32, ptr(ws), ws.numel(),
                                               C.c_void_p(sq.data_ptr()), ptr(out), None, _stream()))
    return sq.cpu().numpy(), out.cpu()


@pytest.mark.parametrize('shape', SHAPES, ids=str)
@pytest.mark.parametrize('quantize', [False, True])
def test_quality_against_float64(dev, shape, quantize):
    worst = 0.0
    for kind in R.KINDS:
        pred, target, ref, budget = R.case(kind, shape, quantize)
        got = flowsynth.quality(pred.to(dev), target.to(dev), quantize=quantize, ssim_map=True)
        sqerr, out = _sqerr(pred, target, dev, quantize)
        assert torch.equal(out[0], got.mse.cpu()) and torch.equal(out[1], got.psnr.cpu()) and torch.equal(out[2], got.ssim.cpu())
        worst = max(worst, _check(f'{kind} {shape} quantize={quantize}', got, sqerr, ref, budget, quantize, pred[0].numel()))
        if kind == 'self':
            assert bool((got.mse == 0).all()) and bool(torch.isposinf(got.psnr).all())
            assert bool((got.map == 1.0).all()) and bool((got.ssim == 1.0).all())
    print(f'framequality {shape} quantize={quantize}: worst ratio over the input families {worst:.4f}')


def test_many_tiles(dev):
    """3 x 9 x 10 = 270 tiles per frame, more than the finish kernel has threads: some of them add two partials"""
    ty, tx = R.tile()
    shape = (1, 3, 9 * ty + 10 - 7, 10 * tx + 10 - 9)
    for quantize in (False, True):
        pred, target, ref, budget = R.case('texture', shape, quantize)
        got = flowsynth.quality(pred.to(dev), target.to(dev), quantize=quantize, ssim_map=True)
        sqerr, _ = _sqerr(pred, target, dev, quantize)
        _check(f'texture {shape} quantize={quantize}', got, sqerr, ref, budget, quantize, pred[0].numel())


def test_bitwise_repeatable_and_workspace_needs_no_initialisation(dev):
    shape = SHAPES[-1]
    pred, target = (t.to(dev) for t in R.inputs('noise', *shape))
    ws = torch.full((flowsynth.quality_workspace_floats(*shape),), float('nan'), device=dev)
    a = flowsynth.quality(pred, target, ssim_map=True, workspace=ws)
    ws.fill_(float('nan'))
    b = flowsynth.quality(pred, target, ssim_map=True, workspace=ws)
    c = flowsynth.quality(pred, target, ssim_map=True)
    for x, y in ((a, b), (a, c)):
        for f in ('psnr', 'ssim', 'mse', 'map'):
            assert torch.equal(getattr(x, f), getattr(y, f)), f
    assert bool(torch.isfinite(a.ssim).all())


def test_five_dimensional_call_equals_the_flattened_one(dev):
    pred, target = (t.to(dev) for t in R.inputs('texture', 6, 3, 27, 43))
    flat = flowsynth.quality(pred, target, ssim_map=True, quantize=True)
    five = flowsynth.quality(pred.view(2, 3, 3, 27, 43), target.view(2, 3, 3, 27, 43), ssim_map=True, quantize=True)
    assert five.psnr.shape == (2, 3) and five.ssim.shape == (2, 3) and five.mse.shape == (2, 3) and five.map.shape == (2, 3, 3, 17, 33)
    for f in ('psnr', 'ssim', 'mse', 'map'):
        assert torch.equal(getattr(five, f).reshape(getattr(flat, f).shape), getattr(flat, f)), f
    assert flowsynth.quality(pred, target).map is None


def test_a_frame_does_not_depend_on_its_batch(dev):
    pred, target = (t.to(dev) for t in R.inputs('noise', 3, 3, 39, 69))
    whole = flowsynth.quality(pred, target, ssim_map=True)
    for n in range(3):
        one = flowsynth.quality(pred[n:n + 1], target[n:n + 1], ssim_map=True)
        for f in ('psnr', 'ssim', 'mse', 'map'):
            assert torch.equal(getattr(one, f)[0], getattr(whole, f)[n]), (n, f)
    swapped = flowsynth.quality(pred.flip(0), target.flip(0))
    assert torch.equal(swapped.ssim.flip(0), whole.ssim) and torch.equal(swapped.mse.flip(0), whole.mse)


def test_composed_on_the_device_stays_within_the_budget(dev):
    shape = SHAPES[-1]
    for quantize in (False, True):
        pred, target, ref, budget = R.case('texture', shape, quantize)
        got = flowsynth.quality_composed(pred.to(dev), target.to(dev), quantize=quantize, ssim_map=True)
        ratio = float((np.abs(got.map.cpu().numpy().astype(np.float64) - ref['map']) / budget).max())
        print(f'framequality composed on the device, quantize={quantize}: worst ratio {ratio:.4f}')
        assert ratio <= 1


def test_refusals_on_the_device(dev):
    pred, target = (t.to(dev) for t in R.inputs('noise', 1, 3, 12, 13))
    with pytest.raises(RuntimeError, match='frame_quality: workspace of 2 floats, need 12'):
        flowsynth.quality(pred, target, workspace=torch.empty(2, device=dev))
    with pytest.raises(ValueError, match='1 or 3 channels'):
        flowsynth.quality(pred[:, :2], target[:, :2])
    with pytest.raises(RuntimeError, match='no gradient'):
        flowsynth.quality(pred.clone().requires_grad_(True), target)


# ---- the trainer ----

def _args(net):
    import argparse
    return argparse.Namespace(**{**TR.GRAD_ARGS, 'net': net})


def test_holdout_quality_is_interpolate_then_quality(dev):
    clip = flowdata.Holdout(flowdata.SyntheticClip(7, 24, 40), 3)
    model = flowtrainer.FlowTrainer(_args(TR.step_net('RBF').to(dev))).to(dev)
    items = [clip.with_held()[i] for i in range(len(clip))]
    batch = [torch.stack([it[k] for it in items]).to(dev) for k in (0, 1, 2)] + [torch.tensor([clip.flow_scale] * len(items))]
    held, taus = torch.stack([it[4] for it in items]).to(dev), items[0][5]
    seen, interpolate = [], model.interpolate
    model.interpolate = lambda *a, **kw: seen.append(interpolate(*a, **kw)) or seen[-1]      # the splat's atomics: keep ITS frames
    for quantize in (True, False):
        got = model.holdout_quality(batch, held, taus, quantize=quantize)
        assert set(got) == {'net', 'blend', 'repeat'} and got['net'].psnr.shape == (2, 2)
        frames = seen.pop()
        assert not seen and float((frames - interpolate(batch, taus)).abs().max()) < 1e-5
        want = flowsynth.quality(frames, held, quantize=quantize)
        given = model.holdout_quality(batch, held, taus, quantize=quantize, frames=frames)
        assert not seen and all(torch.equal(getattr(given['net'], f), getattr(want, f)) for f in ('psnr', 'ssim', 'mse'))
        tau = taus.to(dev).view(1, -1, 1, 1, 1)
        blend = flowsynth.quality((1 - tau) * batch[0][:, None] + tau * batch[1][:, None], held, quantize=quantize)
        repeat = flowsynth.quality(torch.stack([batch[0], batch[1]], 1), held, quantize=quantize)      # tau = 1/3 -> frame1, 2/3 -> frame2
        for name, ref in (('net', want), ('blend', blend), ('repeat', repeat)):
            for f in ('psnr', 'ssim', 'mse'):
                assert torch.equal(getattr(got[name], f), getattr(ref, f)), (name, f)
    assert bool(torch.isfinite(got['net'].ssim).all())


def test_interpolate_holdout_command(tmp_path):
    """the smoke command: nine frames, every 2nd kept -> four pairs with one held-out frame each; quality.jsonl has four lines and the
    means; the network's numbers are those of the written PNGs against the clip's own frames"""
    from PIL import Image
    out = tmp_path / 'frames'
    r = subprocess.run([sys.executable, os.path.join(ROOT, 'video-interpolation', 'interpolate.py'), '--synthetic', '9', '24', '40',
                        '--fit-epochs', '2', '--holdout', '2', '--name', 'smoke', '--net', 'RBF', '--out', str(out)],
                       cwd=tmp_path, capture_output=True, text=True, timeout=300)
    print(r.stdout[-2000:], r.stderr[-2000:])
    assert r.returncode == 0
    lines = [json.loads(x) for x in open(out / 'quality.jsonl')]
    assert len(lines) == 5 and lines[-1]['mean'] is True and lines[-1]['frames'] == 4
    assert [(x['pair'], x['j'], x['tau']) for x in lines[:-1]] == [(i, 1, 0.5) for i in range(4)]
    assert 'network' in r.stdout and 'linear blend' in r.stdout and 'nearer frame' in r.stdout
    clip = flowdata.SyntheticClip(9, 24, 40)
    written = []
    for i in range(4):
        with Image.open(out / f'frame_{i + 1:04d}_01.png') as im:
            written.append(torch.from_numpy(np.asarray(im).copy()).permute(2, 0, 1).float() / 255)
    dev = torch.device('cuda', 0)
    got = flowsynth.quality(torch.stack(written).to(dev), clip.video[1::2].to(dev), quantize=True)
    mse, psnr, ssim = (t.cpu().tolist() for t in (got.mse, got.psnr, got.ssim))
    for i, rec in enumerate(lines[:-1]):
        assert rec['mse_net'] == mse[i] and rec['psnr_net'] == psnr[i] and rec['ssim_net'] == ssim[i], (i, rec)
    assert lines[-1]['mse_net'] == sum(mse) / 4 and lines[-1]['psnr_net'] == sum(psnr) / 4 and lines[-1]['ssim_net'] == sum(ssim) / 4
    assert sorted(os.listdir(out)) == sorted([f'frame_{i:04d}_{j:02d}.png' for i in (1, 2, 3, 4) for j in (0, 1)]
                                             + ['frame_0005_00.png', 'quality.jsonl'])


def test_train_holdout_logs_psnr_and_ssim(tmp_path):
    r = subprocess.run([sys.executable, os.path.join(ROOT, 'video-interpolation', 'main.py'), 'train', '--synthetic', '9', '24', '40',
                        '--holdout', '2', '--epochs', '2', '--val-iter', '1', '--net', 'RBF', '--name', 'ho', '--wandb', 'log'],
                       cwd=tmp_path, capture_output=True, text=True, timeout=300)
    print(r.stdout[-2000:], r.stderr[-2000:])
    assert r.returncode == 0
    records = [json.loads(x) for x in open(tmp_path / 'log_synthetic_ho.jsonl')]
    val = [x for x in records if 'val/PSNR' in x]
    assert len(val) >= 2 and all('val/SSIM' in x and 'val/EPE' not in x for x in val)
    assert all(0 < x['val/PSNR'] < 100 and -1 <= x['val/SSIM'] <= 1 for x in val)
