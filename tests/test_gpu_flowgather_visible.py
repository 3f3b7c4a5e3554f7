"""GPU: the occlusion-aware gather rule (csrc/flowgather.hip, flowgather_kernel<.., VIS = true>; sin_inn_amd.flowsynth.gather(..,
visible=)) per element against float64, against its composed form and against the plain rule.

The reference and the budget are those of tests/flowgather_visible_refs.py (the method of tests/flowgather_refs.py, with the terms of
the masks added), checked on every pixel.  The plain rule's GPU test (tests/test_gpu_flowgather.py) holds the fused operator to that
budget, not to the bits of `gather_composed`; so does this one: the composed form on the device and the fused operator each lie within
one budget of float64, hence within two of each other, and the number of elements whose bits differ is printed.
"""
import argparse
import os
import sys

import pytest
import torch

pytestmark = pytest.mark.gpu
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import flowgather_visible_refs as V  # noqa: E402
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
    for name in V.CASES:
        inputs = V.case(name)
        out[name] = (inputs, *V.gather_visible64(*inputs))
    return out


def _on(dev, inputs):
    i0, i1, fl, slots, taus, m0, m1 = inputs
    return (i0.to(dev), i1.to(dev), fl.to(dev), slots, taus), (m0.to(dev), m1.to(dev))


def _ratio(got, x64, budget):
    assert bool(torch.isfinite(got).all())
    return float(((got.to(F64).cpu() - x64).abs() / budget).max())


@pytest.mark.parametrize('k_loop', [False, True])
@pytest.mark.parametrize('name', list(V.CASES))
def test_fused_against_float64(dev, refs, name, k_loop):
    inputs, x64, budget = refs[name]
    args, vis = _on(dev, inputs)
    got = flowsynth.gather(*args, visible=vis, k_loop=k_loop)
    assert got.shape == x64.shape and got.dtype == torch.float32
    ratio = _ratio(got, x64, budget)
    print(f'flowgather visible {name} {tuple(inputs[0].shape)} K={len(inputs[4])} k_loop={k_loop}: worst err / budget {ratio:.3f}')
    assert ratio <= 1.0


@pytest.mark.parametrize('name', list(V.CASES))
def test_fused_against_composed_on_the_device(dev, refs, name):
    inputs, x64, budget = refs[name]
    args, vis = _on(dev, inputs)
    fused = flowsynth.gather(*args, visible=vis)
    composed = flowsynth.gather_composed(*args, visible=vis)
    assert composed.is_cuda and composed.dtype == torch.float32
    differ = int((fused != composed).sum())
    gap = float(((fused.to(F64) - composed.to(F64)).abs().cpu() / (2 * budget)).max())
    print(f'flowgather visible {name}: fused and composed differ in the bits of {differ} of {fused.numel()} elements, largest '
          f'difference {float((fused - composed).abs().max()):.3g}, |difference| / (2 budget) {gap:.3f}; composed err / budget '
          f'{_ratio(composed, x64, budget):.3f}')
    assert _ratio(composed, x64, budget) <= 1.0 and _ratio(fused, x64, budget) <= 1.0 and gap <= 1.0


@pytest.mark.parametrize('k_loop', [False, True])
@pytest.mark.parametrize('name', list(V.CASES))
def test_all_ones_masks_give_the_plain_gather_bits(dev, refs, name, k_loop):
    inputs, _, _ = refs[name]
    args, vis = _on(dev, inputs)
    ones = torch.ones_like(vis[0])
    plain, plain_u8 = flowsynth.gather(*args, u8=True, k_loop=k_loop)
    got, got_u8 = flowsynth.gather(*args, visible=(ones, ones), u8=True, k_loop=k_loop)
    assert torch.equal(got, plain) and torch.equal(got_u8, plain_u8)
    assert torch.equal(flowsynth.gather(*args, visible=(ones.bool(), ones.bool())), plain)
    if name != '1x1':
        assert not torch.equal(flowsynth.gather(*args, visible=vis), plain)             # the masks are read


def test_repeated_calls_launch_shapes_and_bytes(dev, refs):
    inputs, _, _ = refs['7x300']
    args, vis = _on(dev, inputs)
    first, u8 = flowsynth.gather(*args, visible=vis, u8=True, k_loop=False)
    again = flowsynth.gather(*args, visible=vis, k_loop=False)
    walked = flowsynth.gather(*args, visible=vis, k_loop=True)
    assert torch.equal(first, again) and torch.equal(first, walked)
    assert u8.dtype == torch.uint8 and torch.equal(u8, (first * 255).round().clamp(0, 255).to(torch.uint8))
    into = torch.empty_like(first)
    assert flowsynth.gather(*args, visible=vis, out=into) is into and torch.equal(into, first)


def test_both_masks_zero_is_the_linear_blend(dev, refs):
    (i0, i1, _, _, _, _, _), _, _ = refs['9x33']
    b, c, h, w = i0.shape
    taus = (0.0, 0.3, 1.0)
    _, slots = flowsynth.gather_slots([0.0] * b, taus, 1.0, 'reverse')
    zero = torch.zeros(b, 1, h, w, device=dev)
    got = flowsynth.gather(i0.to(dev), i1.to(dev), torch.zeros(b * len(taus), 4, h, w, device=dev), slots, taus, visible=(zero, zero))
    want = flowsynth.gather_composed(i0, i1, torch.zeros(b * len(taus), 4, h, w), slots, taus, visible=(zero.cpu(), zero.cpu()))
    assert torch.equal(got.cpu(), want)                                  # e L / e: exact in both


def test_c_entry_point_refusals(dev, refs):
    import ctypes as C
    from sin_inn_amd import _lib
    from sin_inn_amd.ops import ptr
    inputs, _, _ = refs['9x33']
    (i0, i1, fl, slots, taus), (m0, m1) = _on(dev, inputs)
    b, c, h, w = i0.shape
    k = len(taus)
    table, tau = slots.to(dev), torch.tensor(taus, device=dev)
    out = torch.empty(b, k, c, h, w, device=dev)
    lib = _lib.lib()

    def call(a0, a1, o=out):
        return lib.sininn_flow_gather_visible(ptr(i0), ptr(i1), ptr(fl), 4 * h * w, C.c_void_p(table.data_ptr()), ptr(tau), a0, a1, b, k,
                                              c, h, w, 0, ptr(o), None, None)

    assert call(ptr(m0), ptr(m1)) == 0
    for bad, text in (((None, ptr(m1)), 'null'), ((ptr(m0), C.c_void_p(m1.data_ptr() + 2)), 'aligned'),
                      ((ptr(m0), C.c_void_p(out.data_ptr() + 64)), 'overlaps')):
        assert call(*bad) != 0 and text in lib.sininn_last_error().decode()
    torch.cuda.synchronize()


# ---- FlowTrainer.interpolate(synthesis='gather', occlusion=) ----

@pytest.mark.parametrize('occlusion', ['wang', 'brox'])
def test_flowtrainer_interpolate_occlusion(dev, occlusion, tmp_path, monkeypatch):
    from sin_inn_amd.lightning import Trainer
    monkeypatch.chdir(tmp_path)
    clip = flowdata.LayeredClip(5, 24, 40)
    args = argparse.Namespace(**{**TR.GRAD_ARGS, 'net': TR.step_net('RBF')})
    model = flowtrainer.FlowTrainer(args)
    Trainer(gpus=[0], max_epochs=2, check_val_every_n_epoch=3).fit(model, flowdata.LightningLoader(clip, clip, 2, 2))
    model = model.to(dev)
    batch = [clip.video[0:4].to(dev), clip.video[1:5].to(dev), clip.T[0:4].to(dev), torch.tensor([clip.flow_scale] * 4, dtype=F64).to(dev)]
    taus, dt = (0.25, 0.5), 2 / 4
    got = model.interpolate(batch, taus, synthesis='gather', dt=dt, occlusion=occlusion)
    assert got.shape == (4, 2, 3, 24, 40) and got.dtype == torch.float32 and bool(torch.isfinite(got).all())
    stamps, slots = flowsynth.gather_slots(clip.T[0:4], taus, dt, 'network')
    model.net.eval()
    with torch.no_grad():
        flows = flowsynth.joined_flows(*model(batch[0], torch.tensor(stamps, dtype=torch.float32, device=dev), batch[3]))
        flow12, flow21 = model(batch[0], batch[2], batch[3])
        mask1, mask2 = model.visibility_masks(flow12, flow21, occlusion)
        want = flowsynth.gather(batch[0], batch[1], flows, slots, taus, visible=(mask1, mask2))
    assert mask1.shape == (4, 1, 24, 40) and torch.equal(got, want)
    held = torch.stack([clip.video[0:4], clip.video[1:5]], 1).to(dev)
    scores = model.holdout_quality(batch, held, taus, synthesis='gather', dt=dt, occlusion=occlusion)
    assert torch.equal(scores['net'].psnr, flowsynth.quality(want, held, quantize=True).psnr)
    with pytest.raises(ValueError, match="needs synthesis='gather'"):
        model.interpolate(batch, taus, occlusion=occlusion)
    with pytest.raises(ValueError, match='occlusion is'):
        model.interpolate(batch, taus, synthesis='gather', dt=dt, occlusion='unity')
