"""GPU: the fused frame synthesis (csrc/flowsynth.hip, sin_inn_amd.flowsynth) per element against float64.

Method (that of tests/test_gpu_flownet_pair.py): the reference is the float64 evaluation of the definition on the same fp32 inputs
(tests/flowsynth_refs.composed64); the unit of error of a case is max |x32 - x64|, x32 = `flowsynth.composed` in fp32 on the same
device from the existing operators (the same atomics, the same exp); `synthesize` is allowed max(MULT * unit, MULT * 2^-24), MULT = 4:
one unit each for the summation order of the atomics, exp, the division and the blend.  Frames lie in [0, 1], so errors are absolute.
Output pixels whose hole decision may differ between the precisions (flowsynth_refs.excluded) are left out; their share is asserted to
stay below 0.5 % per case, and the constructed cases leave out none.
"""
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import flowsynth_refs as R  # noqa: E402
import flowtrainer_refs as TR  # noqa: E402
from sin_inn_amd import flowdata, flowsynth, flowtrainer  # noqa: E402

F64 = torch.float64
MULT = 4.0
FLOOR = MULT * 2.0 ** -24


@pytest.fixture(scope='module')
def dev():
    assert torch.cuda.is_available(), 'GPU tests need a GPU'
    return torch.device('cuda', 0)


def _budget_check(what, got, x32, x64, keep):
    """`keep`: (B, K, H, W) bool of the pixels compared; returns (err, budget)"""
    keep = keep[:, :, None].expand_as(x64)
    assert bool(torch.isfinite(got).all()), what
    unit = float(((x32.to(F64).cpu() - x64).abs() * keep).max())
    err = float(((got.to(F64).cpu() - x64).abs() * keep).max())
    budget = max(MULT * unit, FLOOR)
    print(f'flowsynth {what}: err {err:.3g}  fp32-composed unit {unit:.3g}  budget {budget:.3g}  err / budget {err / budget:.3f}')
    assert err <= budget, (what, err, unit, budget)
    return err, budget


@pytest.mark.parametrize('name', list(R.CASES) + list(R.CONSTRUCTED))
def test_synthesize_against_float64(dev, name):
    i0, i1, f01, f10, taus = R.case(name)
    x64 = R.composed64(i0, i1, f01, f10, taus)
    ex = R.excluded(f01, f10, taus)
    share = float(ex.float().mean())
    assert share <= R.MAX_EXCLUDED, (name, share)
    if name in R.CONSTRUCTED:
        assert not bool(ex.any())
    a = [t.to(dev) for t in (i0, i1, f01, f10)]
    b, c, h, w = i0.shape
    ws = torch.full((flowsynth.workspace_floats(b, len(taus), c, h, w),), float('nan'), device=dev)     # poisoned: the call zeroes it
    got, u8 = flowsynth.synthesize(*a, taus, u8=True, workspace=ws)
    x32 = flowsynth.composed(*a, taus)
    assert got.shape == x64.shape == x32.shape == (b, len(taus), c, h, w) and got.dtype == torch.float32
    _budget_check(f'{name} {tuple(i0.shape)} K={len(taus)} excluded {share:.3%}', got, x32, x64, ~ex)
    # hole decisions outside the excluded pixels: where both splats are empty in float64 the output is the fallback, rounded once per step
    h0, h1 = R.hole_maps(i0, i1, f01, f10, taus)
    if name in R.CONSTRUCTED:
        t = torch.tensor(R.taus32(taus), dtype=torch.float32, device=dev).reshape(1, -1, 1, 1, 1)
        fallback = (1 - t) * a[0][:, None] + t * a[1][:, None]
        both = (h0 & h1)[:, :, None].expand_as(got).to(dev)
        assert torch.equal(got[both], fallback[both])
    # the bytes of the same call
    assert u8.dtype == torch.uint8 and u8.shape == got.shape
    assert torch.equal(u8, (got * 255).round().clamp(0, 255).to(torch.uint8))


def test_workspace_and_out_are_reused(dev):
    """a second call into the same workspace and out, with other inputs, gives that call's result (the accumulator is zeroed again);
    NaN in the workspace before a call changes nothing; a first and a repeated call agree to the order of the atomics"""
    b, c, h, w, taus = 2, 3, 13, 37, (0.25, 0.5)
    first = [t.to(dev) for t in R.random_inputs(11, b, c, h, w)]
    second_cpu = R.random_inputs(12, b, c, h, w)
    second = [t.to(dev) for t in second_cpu]
    ws = torch.empty(flowsynth.workspace_floats(b, len(taus), c, h, w), device=dev)
    out = torch.empty(b, len(taus), c, h, w, device=dev)
    flowsynth.synthesize(*first, taus, out=out, workspace=ws)
    ret = flowsynth.synthesize(*second, taus, out=out, workspace=ws)
    assert ret.data_ptr() == out.data_ptr()
    reused = out.clone()
    ws.fill_(float('nan'))
    poisoned = flowsynth.synthesize(*second, taus, workspace=ws)
    fresh = flowsynth.synthesize(*second, taus)
    x64 = R.composed64(*second_cpu, taus)
    x32 = flowsynth.composed(*second, taus)
    keep = ~R.excluded(second_cpu[2], second_cpu[3], taus)
    for what, t in (('reused', reused), ('poisoned', poisoned), ('fresh', fresh)):
        _budget_check(f'workspace {what}', t, x32, x64, keep)


def test_strided_flows_and_device_taus(dev):
    """the flows as the two channel-slice views of one (B, 4, H, W) tensor (what flow_fields returns) and taus as a device tensor"""
    b, c, h, w = 2, 3, 13, 37
    cpu = R.random_inputs(13, b, c, h, w)
    i0, i1, f01, f10 = [t.to(dev) for t in cpu]
    both = torch.cat([f01, f10], 1)
    taus = [0.125, 0.75]
    got = flowsynth.synthesize(i0, i1, both[:, :2], both[:, 2:], torch.tensor(taus, device=dev))
    assert not both[:, 2:].is_contiguous()
    _budget_check('channel-slice flows, device taus', got, flowsynth.composed(i0, i1, f01, f10, taus), R.composed64(*cpu, taus),
                  ~R.excluded(cpu[2], cpu[3], taus))


def test_refusals_on_the_device(dev):
    i0, i1, f01, f10 = [t.to(dev) for t in R.random_inputs(1, 1, 3, 9, 14)]
    with pytest.raises(RuntimeError, match='workspace of 10 floats, need'):
        flowsynth.synthesize(i0, i1, f01, f10, [0.5], workspace=torch.empty(10, device=dev))
    with pytest.raises(RuntimeError, match='no gradient'):
        flowsynth.synthesize(i0, i1, f01.clone().requires_grad_(True), f10, [0.5])
    with torch.no_grad():
        assert not flowsynth.synthesize(i0, i1, f01.clone().requires_grad_(True), f10, [0.5]).requires_grad


# ---- FlowTrainer.interpolate ----

def _args(net):
    import argparse
    return argparse.Namespace(**{**TR.GRAD_ARGS, 'net': net})


@pytest.mark.parametrize('name', ['RBF', 'PRBF'])
@pytest.mark.parametrize('training', [True, False])
def test_flowtrainer_interpolate(dev, name, training):
    net = TR.step_net(name).to(dev)
    model = flowtrainer.FlowTrainer(_args(net)).to(dev)
    batch = [t.to(dev) for t in TR.step_batch()]
    taus = (0.0, 1 / 3, 0.5, 1.0)
    model.net.train(training)
    got = model.interpolate(batch, taus)
    assert model.net.training is training
    assert got.shape == (2, len(taus), 3, 24, 40) and got.dtype == torch.float32 and not got.requires_grad
    model.net.eval()
    with torch.no_grad():
        flow12, flow21 = model(batch[0], batch[2], batch[3])
        want = flowsynth.synthesize(batch[0], batch[1], flow12, flow21, taus)
        x32 = flowsynth.composed(batch[0], batch[1], flow12, flow21, taus)
    model.net.train(training)
    f01, f10 = flow12.contiguous().cpu(), flow21.contiguous().cpu()
    x64 = R.composed64(batch[0], batch[1], f01, f10, taus)
    keep = ~R.excluded(f01, f10, taus)
    assert float((~keep).float().mean()) <= R.MAX_EXCLUDED
    _budget_check(f'interpolate {name} training={training}', got, x32, x64, keep)
    _budget_check(f'synthesize on forward {name}', want, x32, x64, keep)


# ---- the command, in a child process ----

def test_interpolate_command_end_to_end(tmp_path):
    """--synthetic 4 24 40 --fit-epochs 2 --factor 3: the ten PNGs of the plan (three pairs x (source, two new frames), then the last
    source frame), each 24 x 40 RGB, the j = 0 files the clip's own frames"""
    from PIL import Image
    out = tmp_path / 'frames'
    r = subprocess.run([sys.executable, os.path.join(ROOT, 'video-interpolation', 'interpolate.py'), '--synthetic', '4', '24', '40',
                        '--name', 'e2e', '--net', 'RBF', '--fit-epochs', '2', '--factor', '3', '--out', str(out), '--gif'],
                       cwd=tmp_path, capture_output=True, text=True, timeout=300)
    print(r.stdout[-2000:], r.stderr[-2000:])
    assert r.returncode == 0
    names = [f'frame_{i:04d}_{j:02d}.png' for i in (1, 2, 3) for j in (0, 1, 2)] + ['frame_0004_00.png']
    assert sorted(os.listdir(out)) == sorted(names)
    clip = flowdata.SyntheticClip(4, 24, 40)
    source = (clip.video * 255).round().clamp(0, 255).to(torch.uint8).permute(0, 2, 3, 1).numpy()
    for n in names:
        with Image.open(out / n) as im:
            assert im.mode == 'RGB' and im.size == (40, 24), n
            a = np.asarray(im)
        if n.endswith('_00.png'):
            assert np.array_equal(a, source[int(n[6:10]) - 1]), n
    assert (tmp_path / 'results' / 'interp_synthetic_e2e_x3.gif').is_file()
