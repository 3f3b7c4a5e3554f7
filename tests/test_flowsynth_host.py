"""CPU: the frame synthesis (sin_inn_amd.flowsynth) without a device -- the float64 restatement against the step-by-step
composition of the oracle's operators, the identities of the definition, the binding's sizes and refusals, the seeds of the GPU
cases under the exclusion rule, and the command line's argument parsing and file plan."""
import ctypes as C
import importlib.util
import os
import sys

import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import flowsynth_refs as R  # noqa: E402
from sin_inn_amd import _lib, flowsynth  # noqa: E402

F64 = torch.float64


def _inputs(seed=0, b=1, c=3, h=9, w=14, amplitude=3.0):
    return [t.to(F64) for t in R.random_inputs(seed, b, c, h, w, amplitude)]


def test_restatement_equals_the_stepwise_composition():
    i0, i1, f01, f10 = _inputs(seed=5, b=2)
    taus = (0.0, 0.375, 1.0)
    got, want = R.composed64(i0, i1, f01, f10, taus), R.stepwise64(i0, i1, f01, f10, taus)
    assert got.shape == (2, 3, 3, 9, 14) and got.dtype == F64
    h0, h1 = R.hole_maps(i0, i1, f01, f10, taus)
    assert bool(h0.any() or h1.any()), 'the case has no hole: the masks are not exercised'
    assert float((got - want).abs().max()) <= 1e-12


def test_zero_flows_give_the_linear_blend():
    """Exact in real arithmetic.  In float64 the definition rounds I * exp(Z) and its quotient by exp(Z) (each 2^-53 relative), so a
    splat of a frame in [0, 1] that has not moved is the frame to 2^-52, and the blend of two such to 4 * 2^-53 with its own roundings."""
    i0, i1, f01, f10 = _inputs()
    for tau in (0.0, 0.25, 1.0):
        got = R.composed64(i0, i1, torch.zeros_like(f01), torch.zeros_like(f10), [tau])[:, 0]
        assert float((got - ((1 - tau) * i0 + tau * i1)).abs().max()) <= 4 * 2.0 ** -53, tau


def test_end_times_give_the_end_frames():
    """tau = 0 puts all weight on frame1, which has not moved (no hole); tau = 1 likewise on frame2; whatever the other splat does"""
    i0, i1, f01, f10 = _inputs(seed=2)
    got = R.composed64(i0, i1, f01, f10, [0.0, 1.0])
    assert float((got[:, 0] - i0).abs().max()) <= 1e-15 and float((got[:, 1] - i1).abs().max()) <= 1e-15


def test_flows_out_of_frame_give_the_fallback_everywhere():
    i0, i1, f01, f10 = _inputs()
    far = torch.full_like(f01, 1000.0)
    tau = 0.3
    got = R.composed64(i0, i1, far, -far, [tau])[:, 0]
    h0, h1 = R.hole_maps(i0, i1, far, -far, [tau])
    assert bool(h0.all() and h1.all())
    t = R.taus32([tau])[0]
    assert torch.equal(got, (1 - t) * i0 + t * i1)


def test_swapping_the_frames_mirrors_time():
    i0, i1, f01, f10 = _inputs(seed=3, b=2)
    taus = [0.0, 0.25, 0.5, 1.0]                                      # 1 - tau is exact for each
    a = R.composed64(i0, i1, f01, f10, taus)
    b = R.composed64(i1, i0, f10, f01, [1 - t for t in taus])
    assert float((a - b).abs().max()) <= 1e-14


@pytest.mark.parametrize('name', list(R.CASES) + list(R.CONSTRUCTED))
def test_committed_cases_respect_the_exclusion_cap(name):
    """the seeds of the GPU cases leave out at most MAX_EXCLUDED of their output pixels; the constructed cases leave out nothing and
    have the holes they are built for"""
    i0, i1, f01, f10, taus = R.case(name)
    ex = R.excluded(f01, f10, taus)
    share = float(ex.float().mean())
    print(f'{name}: {tuple(i0.shape)} x {len(taus)} times, excluded {int(ex.sum())} of {ex.numel()} = {share:.4%}')
    assert share <= R.MAX_EXCLUDED
    if name in R.CONSTRUCTED:
        assert not bool(ex.any())
        h0, h1 = R.hole_maps(i0, i1, f01, f10, taus)
        mid = list(taus).index(0.5)
        if name == 'diverge':
            assert bool(h0[:, mid].any()) and not bool(h1.any())
        if name == 'band':
            assert bool((h0 & h1)[:, mid, 4:8].all()) and not bool((h0 & h1)[:, mid, :4].any())
        if name == 'converge':
            n = R.FO.softsplat_sum(torch.ones(1, 1, *i0.shape[-2:], dtype=F64), 0.5 * f01.to(F64))
            assert float(n.max()) >= 3.0, 'several sources on one target'
    if name == 'past cap':
        cap, tx, ty = R.scatter_block_cap()
        h, w = i0.shape[-2:]
        assert 2 * -(-h // ty) * -(-w // tx) > cap and h % ty and w % tx


# ---- the binding ----

def test_workspace_size():
    lib = _lib.lib()
    for b, k, c, h, w in ((1, 1, 3, 1, 1), (2, 3, 1, 13, 37), (3, 7, 3, 436, 1024)):
        assert lib.sininn_flow_synth_workspace(b, k, c, h, w) == b * k * 2 * (c + 1) * h * w == flowsynth.workspace_floats(b, k, c, h, w)
    assert lib.sininn_flow_synth_workspace(3, 7, 3, 436, 1024) == 75005952
    assert lib.sininn_flow_synth_workspace(1, 0, 3, 4, 4) == 0


def test_c_refusals_need_no_device():
    lib = _lib.lib()
    p = C.c_void_p(256)                                                # never dereferenced: every call below is refused first

    def refused(*a):
        assert lib.sininn_flow_synth(*a) != 0
        return lib.sininn_last_error().decode()

    assert refused(None, p, p, p, p, 1, 1, 3, 4, 4, p, 128, p, None, None) == 'flow_synth: null pointer'
    assert refused(p, p, p, p, p, 1, 1, 3, 4, 4, p, 128, None, None, None) == 'flow_synth: null pointer'
    assert refused(p, p, p, p, p, 1, 65, 3, 4, 4, p, 1 << 40, p, None, None) == 'flow_synth: K = 65 times in one call, at most 64'
    assert refused(p, p, p, p, p, 1, 2, 3, 4, 4, p, 255, p, None, None) == 'flow_synth: workspace of 255 floats, need 256'
    assert 'positive' in refused(p, p, p, p, p, 1, 1, 3, 0, 4, p, 128, p, None, None)
    assert '1 or 3 channels' in refused(p, p, p, p, p, 1, 1, 2, 4, 4, p, 128, p, None, None)


def test_python_refusals():
    i0, i1, f01, f10 = (t.float() for t in _inputs())
    with pytest.raises(NotImplementedError, match='GPU only'):
        flowsynth.synthesize(i0, i1, f01, f10, [0.5])
    with pytest.raises(NotImplementedError, match='GPU only'):
        flowsynth.composed(i0, i1, f01, f10, [0.5])
    with pytest.raises(ValueError, match=r'range \[0, 1\]'):
        flowsynth.synthesize(i0, i1, f01, f10, [1.5])
    with pytest.raises(ValueError, match=r'range \[0, 1\]'):
        flowsynth.synthesize(i0, i1, f01, f10, torch.tensor([0.5, -0.1]))
    with pytest.raises(ValueError, match='at most 64'):
        flowsynth.synthesize(i0, i1, f01, f10, [0.5] * 65)
    with pytest.raises(RuntimeError, match='flowsynth.synthesize'):
        flowsynth.synthesize(i0, i1, f01.clone().requires_grad_(True), f10, [0.5])
    with pytest.raises(RuntimeError, match='flowsynth.composed'):
        flowsynth.composed(i0.clone().requires_grad_(True), i1, f01, f10, [0.5])


def test_flowtrainer_has_interpolate():
    from sin_inn_amd.flowtrainer import FlowTrainer
    assert callable(FlowTrainer.interpolate)


# ---- video-interpolation/interpolate.py ----

def _command():
    spec = importlib.util.spec_from_file_location('interpolate_cmd', os.path.join(ROOT, 'video-interpolation', 'interpolate.py'))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def test_command_defaults_and_exclusive_sources(capsys):
    m = _command()
    a = m.get_args(['--synthetic', '4', '24', '40', '--name', 'n', '--net', 'RBF'])
    assert (a.factor, a.size, a.out, a.gif, a.fit_epochs, a.synthetic, a.input_video) == (2, 436, None, False, 0, [4, 24, 40], None)
    a = m.get_args(['--input-video', 'scene', '--name', 'n', '--net', 'PRBF', '--factor', '8', '--size', '200', '--out', 'o', '--gif',
                    '--fit-epochs', '3'])
    assert (a.input_video, a.net, a.factor, a.size, a.out, a.gif, a.fit_epochs, a.synthetic) == ('scene', 'PRBF', 8, 200, 'o', True, 3, None)
    for argv in (['--name', 'n', '--net', 'RBF'],
                 ['--input-video', 'scene', '--synthetic', '4', '24', '40', '--name', 'n', '--net', 'RBF'],
                 ['--synthetic', '4', '24', '40', '--name', 'n', '--net', 'RBF', '--factor', '0']):
        with pytest.raises(SystemExit) as e:
            m.get_args(argv)
        assert e.value.code == 2
    capsys.readouterr()


def test_command_file_plan():
    """T = 4, factor = 3: per pair j = 0 (the source frame), 1, 2; then the last source frame -- six synthesized names and four
    source names, ten files in writing order"""
    m = _command()
    plan = m.frame_plan(4, 3)
    names = [p[0] for p in plan]
    assert names == ['frame_0001_00.png', 'frame_0001_01.png', 'frame_0001_02.png',
                     'frame_0002_00.png', 'frame_0002_01.png', 'frame_0002_02.png',
                     'frame_0003_00.png', 'frame_0003_01.png', 'frame_0003_02.png', 'frame_0004_00.png']
    assert [p[1:] for p in plan if p[2] == 0] == [(0, 0), (1, 0), (2, 0), (3, 0)]
    assert len([p for p in plan if p[2] != 0]) == 6
