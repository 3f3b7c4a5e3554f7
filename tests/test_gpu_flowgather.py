"""GPU: the fused gather synthesis (csrc/flowgather.hip, sin_inn_amd.flowsynth.gather) per element against float64.

The reference and the budget are those of tests/flowgather_refs.py: the definition in float64 by index arithmetic, and a bound on the
fp32 evaluation derived from its roundings (stated there and in DESIGN 19.4), checked on every pixel -- none is left out.  The launch
has no block cap and no grid stride (one block per 256 pixels of a frame), so there is no past-the-cap case.
"""
import json
import os
import subprocess
import sys

import pytest
import torch

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import flowgather_refs as R  # noqa: E402
import flowtrainer_refs as TR  # noqa: E402
from sin_inn_amd import flowdata, flowsynth, flowtrainer  # noqa: E402

F64 = torch.float64


@pytest.fixture(scope='module')
def dev():
    assert torch.cuda.is_available(), 'GPU tests need a GPU'
    return torch.device('cuda', 0)


@pytest.fixture(scope='module')
def refs():
    out = {}
    for name in R.CASES:
        inputs = R.case(name)
        out[name] = (inputs, *R.gather64(*inputs))
    return out


def _within(what, got, x64, budget):
    assert bool(torch.isfinite(got).all()), what
    err = (got.to(F64).cpu() - x64).abs()
    ratio = float((err / budget).max())
    print(f'flowgather {what}: worst err {float(err.max()):.3g}, worst err / budget {ratio:.3f}')
    assert ratio <= 1.0, (what, ratio)


@pytest.mark.parametrize('k_loop', [False, True])
@pytest.mark.parametrize('name', list(R.CASES))
def test_gather_against_float64(dev, refs, name, k_loop):
    (i0, i1, fl, slots, taus), x64, budget = refs[name]
    b, c, h, w = i0.shape
    assert fl.shape[0] > b * len(taus)                                  # T' > B K
    assert bool((slots[..., 2] == 0).any()) == (name != '1x1') and bool((slots[..., 2] == 2).any())      # regular and reverse entries
    got, u8 = flowsynth.gather(i0.to(dev), i1.to(dev), fl.to(dev), slots, taus, u8=True, k_loop=k_loop)
    assert got.shape == x64.shape == (b, len(taus), c, h, w) and got.dtype == torch.float32
    _within(f'{name} {tuple(i0.shape)} K={len(taus)} k_loop={k_loop}', got, x64, budget)
    assert u8.dtype == torch.uint8 and u8.shape == got.shape
    assert torch.equal(u8, (got * 255).round().clamp(0, 255).to(torch.uint8))


def test_both_launch_shapes_and_repeated_calls_give_equal_bits(dev, refs):
    (i0, i1, fl, slots, taus), _, _ = refs['13x37']
    a = [t.to(dev) for t in (i0, i1, fl)]
    first = flowsynth.gather(*a, slots, taus, k_loop=False)
    again = flowsynth.gather(*a, slots, taus, k_loop=False)
    walked = flowsynth.gather(*a, slots, taus, k_loop=True)
    default = flowsynth.gather(*a, flowsynth.upload_slots(slots, dev), torch.tensor(taus, device=dev))
    assert torch.equal(first, again) and torch.equal(first, walked) and torch.equal(first, default)


def test_non_finite_flows(dev, refs):
    """a NaN and an inf flow value: the pixel is the linear blend to the budget, the other pixels keep their bits"""
    (i0, i1, fl, slots, taus), _, _ = refs['13x37']
    bad = fl.clone()
    bad[:, 0, 6, 20] = float('nan')
    bad[:, 2, 6, 20] = float('nan')
    bad[:, 1, 3, 9] = float('inf')
    bad[:, 3, 3, 9] = float('-inf')
    y64, budget = R.gather64(i0, i1, bad, slots, taus)
    clean = flowsynth.gather(i0.to(dev), i1.to(dev), fl.to(dev), slots, taus)
    got = flowsynth.gather(i0.to(dev), i1.to(dev), bad.to(dev), slots, taus)
    _within('NaN and inf flows', got, y64, budget)
    tau = torch.tensor(taus, dtype=torch.float32).to(F64).view(1, -1, 1)
    for y, x in ((6, 20), (3, 9)):
        lin = (1 - tau) * i0[:, None, :, y, x].to(F64) + tau * i1[:, None, :, y, x].to(F64)
        assert float(((got[..., y, x].cpu().to(F64) - lin).abs() / budget[..., y, x]).max()) <= 1.0
    keep = torch.ones_like(got, dtype=torch.bool)
    keep[..., 6, 20] = False
    keep[..., 3, 9] = False
    assert torch.equal(got[keep], clean[keep])


def test_strided_flows_are_read_in_place(dev, refs):
    """a sample stride larger than 4 H W: every second slice of a larger tensor, and a tensor with a gap after each slice"""
    (i0, i1, fl, slots, taus), x64, budget = refs['13x37']
    t, _, h, w = fl.shape
    want = flowsynth.gather(i0.to(dev), i1.to(dev), fl.to(dev), slots, taus)
    wide = torch.full((2 * t, 4, h, w), float('nan'), device=dev)
    wide[::2] = fl.to(dev)
    view = wide[::2]
    assert view.stride(0) == 8 * h * w and not view.is_contiguous()
    got = flowsynth.gather(i0.to(dev), i1.to(dev), view, slots, taus)
    assert torch.equal(got, want)
    _within('stride 8 H W', got, x64, budget)
    gap = torch.full((t, 4 * h * w + 5), float('nan'), device=dev)
    gap[:, :4 * h * w] = fl.to(dev).reshape(t, -1)
    odd = gap[:, :4 * h * w].view(t, 4, h, w)
    assert odd.stride(0) == 4 * h * w + 5
    assert torch.equal(flowsynth.gather(i0.to(dev), i1.to(dev), odd, slots, taus), want)
    with pytest.raises(ValueError, match='contiguous'):
        flowsynth.gather(i0.to(dev), i1.to(dev), fl.to(dev).permute(0, 1, 3, 2).contiguous().permute(0, 1, 3, 2), slots, taus)


def test_a_frame_does_not_depend_on_the_batch(dev, refs):
    (i0, i1, fl, slots, taus), _, _ = refs['13x37']
    a0, a1, f = i0.to(dev), i1.to(dev), fl.to(dev)
    both = flowsynth.gather(a0, a1, f, slots, taus)
    for b in range(i0.shape[0]):
        alone = flowsynth.gather(a0[b:b + 1], a1[b:b + 1], f, slots[b:b + 1].contiguous(), taus)
        assert torch.equal(alone[0], both[b])
    swapped = flowsynth.gather(a0.flip(0), a1.flip(0), f, slots.flip(0).contiguous(), taus)
    assert torch.equal(swapped.flip(0), both)


def test_refusals(dev, refs):
    (i0, i1, fl, slots, taus), _, _ = refs['13x37']
    a0, a1, f = i0.to(dev), i1.to(dev), fl.to(dev)
    with pytest.raises(RuntimeError, match='no gradient'):
        flowsynth.gather(a0, a1, f.clone().requires_grad_(True), slots, taus)
    with torch.no_grad():
        assert not flowsynth.gather(a0, a1, f.clone().requires_grad_(True), slots, taus).requires_grad
    with pytest.raises(ValueError, match='time slice'):
        flowsynth.gather(a0, a1, f[:2], slots, taus)
    bad = slots.clone()
    bad[0, 0, 2] = 1
    with pytest.raises(ValueError, match='channel'):
        flowsynth.gather(a0, a1, f, bad, taus)
    with pytest.raises(ValueError, match=r'range \[0, 1\]'):
        flowsynth.gather(a0, a1, f, slots, (0.0, 0.3, 1.5))
    with pytest.raises(NotImplementedError):
        flowsynth.gather(i0, i1, fl, slots, taus)


# ---- FlowTrainer.interpolate(synthesis='gather') ----

def _args(net):
    import argparse
    return argparse.Namespace(**{**TR.GRAD_ARGS, 'net': net})


@pytest.fixture(scope='module')
def clip_batch():
    """SyntheticClip 4 x 24 x 40, all three pairs (the first one included), as the loader collates them"""
    clip = flowdata.SyntheticClip(4, 24, 40, seed=0)
    return [clip.video[0:3], clip.video[1:4], clip.T[0:3], torch.tensor([clip.flow_scale] * 3, dtype=torch.float64)], 2 / 3


@pytest.mark.parametrize('back', ['network', 'reverse'])
@pytest.mark.parametrize('name', ['RBF', 'PRBF'])
def test_flowtrainer_interpolate_gather(dev, clip_batch, name, back):
    cpu_batch, dt = clip_batch
    net = TR.step_net(name).to(dev)
    model = flowtrainer.FlowTrainer(_args(net)).to(dev)
    batch = [t.to(dev) for t in cpu_batch]
    taus = (0.0, 1 / 3, 0.5, 1.0)
    model.net.train(True)
    got = model.interpolate(batch, taus, synthesis='gather', dt=dt, back=back)
    assert model.net.training is True
    assert got.shape == (3, len(taus), 3, 24, 40) and got.dtype == torch.float32 and not got.requires_grad
    stamps, slots = flowsynth.gather_slots(cpu_batch[2], taus, dt, back)
    assert len(stamps) == (12 if back == 'reverse' else 12 + 12 - 3)         # the first pair falls back at tau < 1
    model.net.eval()
    with torch.no_grad():
        fw, bw = model(batch[0], torch.tensor(stamps, dtype=torch.float32, device=dev), batch[3])
        flows = flowsynth.joined_flows(fw, bw)
        assert flows.data_ptr() == fw.data_ptr() and flows.shape == (len(stamps), 4, 24, 40)
        want = flowsynth.gather(batch[0], batch[1], flows, slots, taus)
    assert torch.equal(got, want)
    x64, budget = R.gather64(cpu_batch[0], cpu_batch[1], flows.cpu(), slots, taus)
    _within(f'interpolate gather {name} back={back}', got, x64, budget)
    # holdout_quality passes the rule through and keeps its keys and shapes
    held = torch.stack([cpu_batch[0], cpu_batch[1]], 1).to(dev)
    scores = model.holdout_quality(batch, held, (0.25, 0.75), synthesis='gather', dt=dt, back=back)
    assert sorted(scores) == ['blend', 'net', 'repeat'] and all(tuple(s.psnr.shape) == (3, 2) for s in scores.values())


def test_flowtrainer_interpolate_gather_past_the_grid_limit(dev, clip_batch, monkeypatch):
    """more stamps than one flow_fields call takes (t h w > GRID_POINTS): several calls, joined -- the same bits as one call"""
    cpu_batch, dt = clip_batch
    model = flowtrainer.FlowTrainer(_args(TR.step_net('RBF').to(dev))).to(dev)
    batch = [t.to(dev) for t in cpu_batch]
    taus = (0.25, 0.5, 1.0)
    whole = model.interpolate(batch, taus, synthesis='gather', dt=dt)
    monkeypatch.setattr(flowtrainer, 'GRID_POINTS', 4 * 24 * 40 + 7)          # four stamps a call: 16 stamps in four calls
    parts = model.interpolate(batch, taus, synthesis='gather', dt=dt)
    assert torch.equal(parts, whole)


def test_flowtrainer_interpolate_gather_refusals(dev, clip_batch):
    cpu_batch, dt = clip_batch
    model = flowtrainer.FlowTrainer(_args(TR.step_net('RBF').to(dev))).to(dev)
    batch = [t.to(dev) for t in cpu_batch]
    with pytest.raises(ValueError, match='needs dt'):
        model.interpolate(batch, (0.5,), synthesis='gather')
    with pytest.raises(ValueError, match='synthesis'):
        model.interpolate(batch, (0.5,), synthesis='scatter')
    from sin_inn_amd import flownet
    torch.manual_seed(0)
    pair_net = flownet.flow_model_dict['RBF'](flownet.ModelParams(domain_dim=2)).to(dev)
    pair_model = flowtrainer.FlowTrainer(_args(pair_net)).to(dev)
    with pytest.raises(ValueError, match='domain_dim 2'):
        pair_model.interpolate(batch, (0.5,), synthesis='gather', dt=dt)


# ---- the command, in a child process ----

def test_interpolate_command_gather(tmp_path):
    """--holdout 2 --synthesis gather writes the file set of the splat run (nine PNGs and quality.jsonl) and names the rule in the
    last line of quality.jsonl"""
    out = tmp_path / 'frames'
    r = subprocess.run([sys.executable, os.path.join(ROOT, 'video-interpolation', 'interpolate.py'), '--synthetic', '9', '24', '40',
                        '--fit-epochs', '2', '--holdout', '2', '--synthesis', 'gather', '--name', 'smoke', '--net', 'RBF',
                        '--out', str(out)], cwd=tmp_path, capture_output=True, text=True, timeout=300)
    print(r.stdout[-2000:], r.stderr[-2000:])
    assert r.returncode == 0
    assert sorted(os.listdir(out)) == sorted([f'frame_{i:04d}_{j:02d}.png' for i in (1, 2, 3, 4) for j in (0, 1)]
                                             + ['frame_0005_00.png', 'quality.jsonl'])
    lines = [json.loads(x) for x in open(out / 'quality.jsonl')]
    assert len(lines) == 5 and lines[-1]['mean'] is True and lines[-1]['frames'] == 4 and lines[-1]['synthesis'] == 'gather/network'
    assert [(x['pair'], x['j'], x['tau']) for x in lines[:-1]] == [(i, 1, 0.5) for i in range(4)]
    assert all(0 < x['psnr_net'] < 100 and -1 <= x['ssim_net'] <= 1 for x in lines[:-1])
