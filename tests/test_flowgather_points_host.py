"""CPU: the gather rule at a list of points (sin_inn_amd.flowsynth.gather_at_composed, the trainer's point table, the command line and
the C entry points) against the float64 reference and its derived per-element budget (tests/flowgather_points_refs.py).  No
element is excluded: every case first checks that fp32 and float64 take the same cell at every point.

Every test here calls a name this feature adds (gather_at_composed, gather_at_from, FlowTrainer.between_points_table, --between-points,
sininn_flow_gather_at) and fails without it.  A seeded defect must miss the budget, that is, exceed it somewhere: worst error / budget
above 1; the ratios are printed."""
import ctypes as C
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import flowgather_grad_refs as G  # noqa: E402
import flowgather_points_refs as P  # noqa: E402
from sin_inn_amd import _lib, flowsynth  # noqa: E402

F64 = torch.float64


@pytest.fixture(scope='module')
def refs():
    """name -> (inputs, out64, budget, grad64, grad budget), computed once and left unchanged"""
    out = {}
    for name in P.CASES:
        inputs = P.case(name)
        i0, i1, fl, pix, pair, tau, rev, blend, g = inputs
        assert P.cells_agree(fl, pix, tau, rev), name
        out[name] = (inputs, *P.gather_at64(i0, i1, fl, pix, pair, tau, rev, blend, g))
    return out


def _ratio(got, x64, budget):
    """the worst |got - x64| / budget over every element (an element with budget 0 must be exact)"""
    err = (got.to(F64) - x64).abs()
    err = torch.where(torch.isfinite(err), err, torch.full_like(err, float('inf')))
    return float(torch.where(err == 0, torch.zeros_like(err), err / budget).max())


def composed(inputs, dtype=torch.float32, **kw):
    """(out, d flows) of gather_at_composed for the case's upstream gradient"""
    i0, i1, fl, pix, pair, tau, rev, blend, g = inputs
    flows = fl.to(dtype).clone().requires_grad_(True)
    out = flowsynth.gather_at_composed(i0.to(dtype), i1.to(dtype), flows, pix, pair, tau, rev, blend=blend, flow_grad=True, **kw)
    out.backward(g.to(dtype))
    return out.detach(), flows.grad


# ---- 1. the reference against float64 autograd, and the composed fp32 operator within the budget ----

@pytest.mark.parametrize('name', list(P.CASES))
def test_reference_matches_float64_autograd(refs, name):
    inputs, o64, _, d64, _ = refs[name]
    out, grad = composed(inputs, dtype=F64)
    assert float((out - o64).abs().max()) <= 1e-12 * max(float(o64.abs().max()), 1e-30)
    assert float((grad - d64).abs().max()) <= 1e-12 * max(float(d64.abs().max()), 1e-30)


@pytest.mark.parametrize('name', list(P.CASES))
def test_composed_fp32_within_budget_everywhere(refs, name):
    inputs, o64, ob, d64, db = refs[name]
    out, grad = composed(inputs)
    assert out.dtype == torch.float32 and out.shape == o64.shape and grad.shape == d64.shape
    fwd, bwd = _ratio(out, o64, ob), _ratio(grad, d64, db)
    print(f'gather_at_composed fp32 {name}: worst err / budget forward {fwd:.3f}, gradient {bwd:.3f}')
    assert fwd <= 1.0 and bwd <= 1.0
    fl, rev = inputs[2], inputs[6]
    assert float(grad[0, 2:].abs().max()) == 0.0                            # unused values of a column: exact zeros
    if fl.shape[0] == 2:
        assert float(grad[1, :2].abs().max()) == 0.0
        if rev is not None:
            assert bool(rev.any()) and not bool(rev.all())
            assert float(grad[1, 2:, rev].abs().max()) == 0.0 and float(grad[1, 2:, ~rev].abs().max()) > 0


def test_cases_cover_borders_and_integer_points(refs):
    (i0, i1, fl, pix, pair, tau, rev, blend, g), o64, _, d64, _ = refs['256']
    h, w = i0.shape[-2:]
    whole = (pix == pix.floor()).all(1)
    assert int(whole.sum()) >= 256 // 8 and bool(((pix[:, 0] == h - 1) & (pix[:, 1] == w - 1)).any())
    (q0x, q0y), (q1x, q1y) = P._coordinates(fl, pix, tau, rev, np.float64)
    outside = (q1x < -1) | (q1x > w) | (q1y < -1) | (q1y > h)
    partly = ((q1x > -1) & (q1x < 0)) | ((q1x > w - 1) & (q1x < w)) | ((q1y > -1) & (q1y < 0)) | ((q1y > h - 1) & (q1y < h))
    assert outside.any() and partly.any() and float(d64.abs().max()) > 0


# ---- 2. bad rows ----

def test_pair_out_of_range_and_non_finite_rows(refs):
    i0, i1, fl, pix, pair, tau, rev, blend, g = refs['256'][0]
    clean_out, clean_grad = composed((i0, i1, fl, pix, pair, tau, rev, blend, g))
    pair2, fl2, pix2 = pair.clone(), fl.clone(), pix.clone()
    pair2[3], pair2[4] = -1, i0.shape[0]
    keep = [k for k in range(40, 256) if not bool(rev[k])][:3]               # three network rows
    fl2[0, 0, keep[0]], fl2[1, 3, keep[1]], fl2[0, 1, keep[2]] = float('nan'), float('inf'), 4.0e9
    pix2[7, 1] = float('nan')
    inputs = (i0, i1, fl2, pix2, pair2, tau, rev, blend, g)
    for dtype in (torch.float32, F64):
        out, grad = composed(inputs, dtype=dtype)
        assert bool(torch.isfinite(out).all()) and bool(torch.isfinite(grad).all())
        assert float(out[:, [3, 4, 7]].abs().max()) == 0.0 and float(grad[:, :, [3, 4, 7]].abs().max()) == 0.0
        assert float(grad[0, :2, keep[0]].abs().max()) == 0.0 and float(grad[1, 2:, keep[1]].abs().max()) == 0.0
        assert float(grad[0, :2, keep[2]].abs().max()) == 0.0
        assert float(grad[1, 2:, keep[0]].abs().max()) > 0                   # the other sample keeps its gradient
    out, grad = composed(inputs)
    same = torch.ones(256, dtype=torch.bool)
    same[[3, 4, 7] + keep] = False
    assert torch.equal(out[:, same], clean_out[:, same]) and torch.equal(grad[:, :, same], clean_grad[:, :, same])
    o64, ob, d64, db = P.gather_at64(*inputs[:8], g)
    assert _ratio(out, o64, ob) <= 1.0 and _ratio(grad, d64, db) <= 1.0


# ---- 3. seeded defects of the composed gradient ----

def _defect(inputs, defect):
    """(out, d flows) of the composed fp32 operator with one defect seeded through the `sample` hook of gather_at_from; R = 1"""
    i0, i1, fl, pix, pair, tau, rev, blend, g = inputs
    flows = fl.clone().requires_grad_(True)
    with torch.no_grad():
        calls = []
        flowsynth.gather_at_from(i0, i1, fl, pix, pair, tau, rev, blend,
                                 sample=lambda *a: calls.append(flowsynth.bilinear_gather_at(*a)) or calls[-1])
        a1 = tau if blend is None else torch.full_like(tau, blend[0])
        den = ((1 - a1) * calls[0][1] + a1 * calls[1][1]) + flowsynth.GATHER_EPS
    back = torch.ones_like(tau, dtype=torch.bool) if fl.shape[0] == 1 else (rev if rev is not None else torch.zeros_like(tau, dtype=torch.bool))
    state = {'which': 0}

    def sample(img, at, qx, qy):
        which = state['which']
        state['which'] += 1
        scale = None
        if defect == 'no 1/D' and which < 2:
            scale = den
        if defect == 'c0 sign under rev' and which == 0:
            scale = torch.where(back, -torch.ones_like(tau), torch.ones_like(tau))
        if scale is not None:
            qx, qy = qx * 1, qy * 1
            qx.register_hook(lambda gr: gr * scale)
            qy.register_hook(lambda gr: gr * scale)
        if defect == 'left cell' and which < 2:
            qx, qy = qx - 2.0 ** -12, qy - 2.0 ** -12
        total, n = flowsynth.bilinear_gather_at(img, at, qx, qy)
        if defect == 'no e H' and which >= 2:
            total = torch.zeros_like(total)
        return total, n

    out = flowsynth.gather_at_from(i0, i1, flows, pix, pair, tau, rev, blend, sample=sample)
    out.backward(g)
    return out.detach(), flows.grad


@pytest.fixture(scope='module')
def single(refs):
    """case 256 with one blend, a1 = 0.3: (inputs, out64, budget, grad64, grad budget)"""
    i0, i1, fl, pix, pair, tau, rev, _, g = refs['256'][0]
    inputs = (i0, i1, fl, pix, pair, tau, rev, (0.3,), g[:1].contiguous())
    return (inputs, *P.gather_at64(*inputs))


@pytest.mark.parametrize('defect', ['no 1/D', 'c0 sign under rev', 'no e H'])
def test_seeded_defect_misses_the_budget(single, defect):
    inputs, o64, ob, d64, db = single
    sound_out, sound = composed(inputs)
    assert _ratio(sound_out, o64, ob) <= 1.0 and _ratio(sound, d64, db) <= 1.0
    none_out, none = _defect(inputs, 'none')
    assert torch.equal(none_out, sound_out) and torch.equal(none, sound)    # the hook itself changes nothing
    out, grad = _defect(inputs, defect)
    ratio = _ratio(grad, d64, db)
    print(f'seeded defect {defect!r}: gradient worst err / budget {ratio:.3g} (sound: {_ratio(sound, d64, db):.3f}); '
          f'forward {_ratio(out, o64, ob):.3g}')
    assert ratio > 1.0
    if defect == 'no e H':
        assert _ratio(out, o64, ob) > 1.0


def _integer_case():
    """integer pixels, tau = 1/2, even integer flows that keep q1 inside: every q on a cell border"""
    g = torch.Generator().manual_seed(11)
    h, w, n = 6, 9, 40
    i0, i1 = torch.rand(1, 3, h, w, generator=g), torch.rand(1, 3, h, w, generator=g)
    pix = torch.stack((torch.randint(1, h - 2, (n,), generator=g), torch.randint(1, w - 2, (n,), generator=g)), 1).float()
    fl = torch.zeros(2, 4, n)
    fl[0, 0], fl[1, 3] = 2.0, -2.0
    return i0, i1, fl, pix, torch.zeros(n, dtype=torch.int32), torch.full((n,), 0.5), None, (0.5,), torch.rand(1, n, 3, generator=g) + 0.5


def test_left_hand_cell_on_a_border_misses_the_budget():
    inputs = _integer_case()
    assert P.cells_agree(inputs[2], inputs[3], inputs[5], None)
    o64, ob, d64, db = P.gather_at64(*inputs)
    out, grad = composed(inputs)
    assert _ratio(out, o64, ob) <= 1.0 and _ratio(grad, d64, db) <= 1.0
    _, bad = _defect(inputs, 'left cell')
    ratio = _ratio(bad, d64, db)
    print(f"seeded defect 'left cell': worst err / budget {ratio:.3g}")
    assert ratio > 1.0


# ---- 4. the surface ----

def test_refusals_and_keywords(refs):
    i0, i1, fl, pix, pair, tau, rev, blend, g = refs['256'][0]
    flows = fl.clone().requires_grad_(True)
    for fn in (flowsynth.gather_at, flowsynth.gather_at_composed):
        with pytest.raises(RuntimeError, match='is an inference operator and has no gradient'):
            fn(i0, i1, flows, pix, pair, tau, rev, blend=blend)
        with pytest.raises(RuntimeError, match='flows only'):
            fn(i0.clone().requires_grad_(True), i1, flows, pix, pair, tau, rev, blend=blend, flow_grad=True)
        with pytest.raises(RuntimeError, match='pix'):
            fn(i0, i1, flows, pix.clone().requires_grad_(True), pair, tau, rev, blend=blend, flow_grad=True)
        with pytest.raises(ValueError, match='1 or 3 channels'):
            fn(i0[:, :2], i1[:, :2], fl, pix, pair, tau, rev, blend=blend)
        with pytest.raises(ValueError, match='S = 1 or 2'):
            fn(i0, i1, torch.cat([fl, fl[:1]]), pix, pair, tau, rev, blend=blend)
        with pytest.raises(ValueError, match='int32'):
            fn(i0, i1, fl, pix, pair.long(), tau, rev, blend=blend)
        with pytest.raises(ValueError, match='blend'):
            fn(i0, i1, fl, pix, pair, tau, rev, blend=(0.1,) * 5)
        with pytest.raises(ValueError, match='blend'):
            fn(i0, i1, fl, pix, pair, tau, rev, blend=())
        with pytest.raises(ValueError, match='pix is'):
            fn(i0, i1, fl, pix[:-1], pair, tau, rev, blend=blend)
    with pytest.raises(NotImplementedError, match='GPU only'):
        flowsynth.gather_at(i0, i1, fl, pix, pair, tau, rev, blend=blend)
    plain = flowsynth.gather_at_composed(i0, i1, fl, pix, pair, tau, rev, blend=blend, flow_grad=True)
    assert not plain.requires_grad and tuple(plain.shape) == (2, 256, 3)
    with torch.no_grad():
        assert not flowsynth.gather_at_composed(i0, i1, flows, pix, pair, tau, rev, blend=blend, flow_grad=True).requires_grad
    # blend=None is a1 = tau per point
    per_point = flowsynth.gather_at_composed(i0, i1, fl, pix, pair, tau, rev)
    for k in (5, 17):
        one = flowsynth.gather_at_composed(i0, i1, fl, pix, pair, tau, rev, blend=(float(tau[k]),))
        assert torch.equal(per_point[0, k], one[0, k])


def test_entry_point_refusals():
    lib = _lib.lib()
    fake = C.c_void_p(4096)
    blend = (C.c_float * 4)(0.0, 1.0, 0.5, 0.25)

    def call(bwd=False, **kw):
        a = dict(i0=fake, i1=fake, flows=fake, pix=fake, pair=fake, tau=fake, rev=None, blend=blend, go=fake, r=2, s=2, n=7, b=1, c=3,
                 h=2, w=3, out=fake)
        a.update(kw)
        head = (a['i0'], a['i1'], a['flows'], a['pix'], a['pair'], a['tau'], a['rev'], a['blend'])
        tail = (a['r'], a['s'], a['n'], a['b'], a['c'], a['h'], a['w'], a['out'], None)
        rc = lib.sininn_flow_gather_at_bwd(*head, a['go'], *tail) if bwd else lib.sininn_flow_gather_at(*head, *tail)
        assert rc != 0
        return lib.sininn_last_error().decode()

    for bwd, who in ((False, 'flow_gather_at'), (True, 'flow_gather_at_bwd')):
        for name in ('i0', 'i1', 'flows', 'pix', 'pair', 'tau'):
            assert call(bwd, **{name: None}) == f'{who}: null pointer'
        assert call(bwd, c=2) == f'{who}: frames have 1 or 3 channels (got 2)'
        assert call(bwd, s=0) == f'{who}: flows is (S, 4, N) with S = 1 or 2 (got 0)'
        assert call(bwd, s=3) == f'{who}: flows is (S, 4, N) with S = 1 or 2 (got 3)'
        assert call(bwd, r=0) == f'{who}: R = 0 blends in one call, 1 to 4 are supported'
        assert call(bwd, r=5) == f'{who}: R = 5 blends in one call, 1 to 4 are supported'
        assert 'blend == NULL' in call(bwd, blend=None, r=2)
        assert call(bwd, n=0) == f'{who}: N = 0 points, at least one is needed'
        assert call(bwd, n=2 ** 31) == f'{who}: N = 2147483648 is past an int index'
        assert call(bwd, h=65536, w=65536) == f'{who}: H * W = 4294967296 is past an int index'
        assert call(bwd, b=0) == f'{who}: bad shape (every size must be positive)'
        assert '8-byte aligned' in call(bwd, pix=C.c_void_p(4100))
    assert call(out=None) == 'flow_gather_at: null pointer'
    assert call(True, go=None) == 'flow_gather_at_bwd: the gradient of the output is null'
    assert call(True, out=None) == 'flow_gather_at_bwd: the gradient of the flows is null'


# ---- 5. the trainer and the command line ----

def _trainer(argv, **kw):
    from sin_inn_amd import flowtrainer
    return flowtrainer.FlowTrainer(G.trainer_args(argv=argv, between_dt=2 / 3, **kw))


def test_trainer_point_table():
    times = torch.tensor([-1.0, -1 / 3, 1 / 3], dtype=torch.float64)
    model = _trainer(['--loss-between', '1', '--between-points', '512'])
    assert model.between_points == 512 and model.between_back == 'network'
    pix, pair, tau, rev, poses = model.between_points_table(times, 3, 24, 40)
    assert pair.dtype == torch.int32 and rev.dtype == torch.bool and pix.dtype == tau.dtype == torch.float32
    assert tuple(pix.shape) == (512, 2) and len(poses) == 2 and all(tuple(p.shape) == (512, 3) for p in poses)
    assert int(pair.min()) == 0 and int(pair.max()) == 2 and float(tau.min()) >= 0 and float(tau.max()) < 1
    assert float(pix[:, 0].min()) >= 0 and float(pix[:, 0].max()) <= 23 and float(pix[:, 1].min()) >= 0 and float(pix[:, 1].max()) <= 39
    assert float(pix[:, 0].max()) > 20 and float(pix[:, 1].max()) > 35 and bool((pix != pix.floor()).any())
    # stamps: s = times[pair] + tau dt, then s - dt; rev exactly at the pairs of the clip's first frame
    dt = 2 / 3
    s = times.float()[pair.long()] + tau * dt
    assert torch.equal(poses[0][:, 0], s) and torch.equal(poses[1][:, 0], s - dt)
    assert torch.equal(rev, pair == 0) and bool(rev.any()) and not bool(rev.all())
    # the pixel-to-pose map is the grid's: linspace(-1, 1, h)[i] at pixel i
    for slab in poses:
        assert torch.equal(slab[:, 1], 2 * pix[:, 0] / 23 - 1) and torch.equal(slab[:, 2], 2 * pix[:, 1] / 39 - 1)
    model.between_points_table(times, 1, 1, 1)                              # an axis of length 1: no division by zero
    ends = torch.tensor([[0.0, 0.0], [23.0, 39.0]])
    assert torch.equal(2 * ends[:, 0] / 23 - 1, torch.tensor([-1.0, 1.0])) and torch.equal(2 * ends[:, 1] / 39 - 1, torch.tensor([-1.0, 1.0]))
    # one seed, one sequence: a second trainer repeats it, a second draw differs
    again = _trainer(['--loss-between', '1', '--between-points', '512'])
    first = again.between_points_table(times, 3, 24, 40)
    assert all(torch.equal(a, b) for a, b in zip((pix, pair, tau, rev), first[:4]))
    second = again.between_points_table(times, 3, 24, 40)
    assert not torch.equal(second[0], first[0])
    other = _trainer(['--loss-between', '1', '--between-points', '512'], between_seed=1)
    assert not torch.equal(other.between_points_table(times, 3, 24, 40)[0], pix)
    # reverse: one slab, no rev
    back = _trainer(['--loss-between', '1', '--between-points', '64', '--between-back', 'reverse'])
    _, _, _, rev1, poses1 = back.between_points_table(times, 3, 24, 40)
    assert rev1 is None and len(poses1) == 1


def test_command_line_and_trainer_refusals(capsys):
    m = G.flow_main()
    base = ['train', '--synthetic', '4', '24', '40']
    args = m.get_args(base + ['--loss-between', '1', '--between-points', '4096'])
    assert args.between_points == 4096 and not hasattr(args, 'between_taus')
    assert not hasattr(m.get_args(base), 'between_points')                  # present only when given
    for bad in (['--between-points', '8', '--between-taus', '2'], ['--between-points', '0']):
        with pytest.raises(SystemExit):
            m.get_args(base + ['--loss-between', '1'] + bad)
    assert 'give one of them' in capsys.readouterr().err
    from sin_inn_amd import flowtrainer
    with pytest.raises(ValueError, match='give one of them'):
        _trainer(['--loss-between', '1', '--between-points', '8'], between_taus=2)
    with pytest.raises(ValueError, match='between-points'):
        _trainer(['--loss-between', '1'], between_points=0)
    args = G.trainer_args(argv=['--loss-between', '1', '--between-points', '8'], between_dt=2 / 3)

    class Flat(torch.nn.Module):
        domain_dim = 2
    args.net = Flat()
    with pytest.raises(ValueError, match='domain_dim 2'):
        flowtrainer.FlowTrainer(args)
    off = _trainer(['--between-points', '8'])                               # no weight: the parent's trainer
    assert off.between_weight == 0 and off.between_points is None and off.between_rng is None


def test_interpolate_passes_the_switch_on(capsys):
    import importlib.util
    spec = importlib.util.spec_from_file_location('flow_interp_points', os.path.join(G.ROOT, 'video-interpolation', 'interpolate.py'))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    base = ['--synthetic', '4', '24', '40', '--name', 'x', '--net', 'RBF', '--fit-epochs', '1', '--loss-between', '1']
    _, args = mod.trainer_args(mod.get_args(base + ['--between-points', '128']))
    assert args.between_points == 128 and not hasattr(args, 'between_taus')
    _, args = mod.trainer_args(mod.get_args(base))
    assert args.between_taus == 1 and not hasattr(args, 'between_points')
    with pytest.raises(SystemExit):
        mod.get_args(base + ['--between-points', '128', '--between-taus', '2'])
    assert 'give one of them' in capsys.readouterr().err


def _stub_step(model, calls):
    """run training_step on the host with the network and the losses stubbed: what is left is the step's own control flow"""
    from sin_inn_amd import flownet
    zero = torch.zeros((), requires_grad=True)

    def forward(frame, times, scale):
        calls.append('flow_fields')
        flows = torch.zeros(times.numel(), 4, *frame.shape[-2:])
        return flows[:, :2], flows[:, 2:]

    def flow_at(net, poses, scale=1.0, **kw):
        calls.append('flow_at')
        assert kw == {'planar': True} and poses.dtype == torch.float32
        return (torch.zeros(4, poses.shape[0]) + 0.25).requires_grad_(True)

    model.forward = forward
    model.losses = lambda f1, f2, a, b: (zero, zero, zero, zero, (None, None, None, None))
    model.log = lambda *a, **kw: None
    model._scale = lambda scale, frame: 8.0
    real = flownet.flow_at
    flownet.flow_at = flow_at
    try:
        batch = G.trainer_batch()
        return model.training_step([batch[0], batch[1], batch[2], batch[3]], 0)
    finally:
        flownet.flow_at = real


def test_step_order_and_weight_zero_issues_no_extra_call(monkeypatch):
    def never(*a, **kw):
        raise AssertionError('a between call at weight 0')
    for argv in ([], ['--loss-between', '0', '--between-points', '64'], ['--between-points', '64']):
        model = _trainer(argv)
        model.between_points_loss = model.between_points_table = model.between_loss = never
        monkeypatch.setattr(flowsynth, 'gather_at', never)
        monkeypatch.setattr(flowsynth, 'gather_at_composed', never)
        calls = []
        _stub_step(model, calls)
        assert calls == ['flow_fields']                                     # the step's one network call, nothing else
    monkeypatch.undo()
    # with the loss: one flow_at per slab, ahead of the step's own flow_fields; fused = False goes through gather_at_composed
    for back, slabs in (('network', 2), ('reverse', 1)):
        model = _trainer(['--loss-between', '0.5', '--between-points', '64', '--between-back', back])
        model.fused = False
        seen = []
        real = flowsynth.gather_at_composed
        monkeypatch.setattr(flowsynth, 'gather_at_composed', lambda *a, **kw: seen.append(kw) or real(*a, **kw))
        monkeypatch.setattr(flowsynth, 'gather_at', lambda *a, **kw: (_ for _ in ()).throw(AssertionError('fused = False')))
        calls = []
        loss = _stub_step(model, calls)
        assert calls == ['flow_at'] * slabs + ['flow_fields']
        assert seen == [dict(blend=(0.0, 1.0), flow_grad=True)] and tuple(model.between_flows.shape) == (slabs, 4, 64)
        out = model.between_frames
        assert tuple(out.shape) == (2, 64, 3) and torch.equal(loss.detach(), 0.5 * (out[0] - out[1]).abs().mean().detach())
        loss.backward()
        monkeypatch.undo()


def test_spatial_controller_keeps_the_frame_grid_for_its_stash():
    """flow_at notes its pose list with the controller, the step's own flow_fields call after it notes the frame grid: the cells the
    error stash uses are the grid's"""
    from sin_inn_amd import flownet, progressive
    net = flownet.all_model_dict['PRBF'](flownet.ModelParams())
    ctrl = progressive.StashedSpatialController(net, 4, block_iterations=2, epsilon=1e-3)
    grid = (torch.tensor([-1.0, 0.0]), torch.linspace(-1, 1, 5), torch.linspace(-1, 1, 7))
    ctrl.note_poses(torch.zeros(9, 3))
    ctrl.note_grid(*grid)
    assert ctrl._last_list is None and all(a is b for a, b in zip(ctrl._last_grid, grid))
    ctrl.note_poses(torch.zeros(9, 3))                                      # the other order is the one stash_grid refuses
    with pytest.raises(RuntimeError, match='pose list'):
        ctrl.stash_grid(*(torch.zeros(2, 3, 5, 7),) * 6)
