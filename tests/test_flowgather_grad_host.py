"""CPU: the gradient of the gather synthesis with respect to its flows (sin_inn_amd.flowsynth.gather_composed(.., flow_grad=True),
gather_reduce_list, the trainer's between table) against the float64 reference and its derived per-element budget
(tests/flowgather_grad_refs.py), border and non-finite cases with exact coordinates, the accumulation order, seeded defects and the
surface.  No element is excluded: every case first checks that fp32 and float64 take the same cell everywhere.

What runs the new code and fails without it: every test that calls gather_composed(.., flow_grad=True), gather_reduce_list or the
trainer's between_* (groups 1 autograd, 2, 3, 4, 6, and the sound baseline of group 5).  The central-difference test checks the
reference alone, and the seeded defects themselves go through `gather_from`'s `sample` hook, which existed before: they measure how
tight the budget is, not the feature.

Seeded defects at 13x37, worst error / budget (each must miss by more than MISS = 100; the sound gradient: 0.088): out grad n dropped
1.5e+05, c0 dropped 1.9e+05, a0 dropped 9.6e+05, 1 / D dropped 6.3e+04, x and y swapped 2.7e+05, the reverse row's dG1 overwriting
dG0 7.4e+04; the left-hand cell on a border (integer targets, 6x9) 3.2e+06.  Composed fp32 against the budget: 1x1 0.002, 13x37 0.088,
5x1031 0.110; central differences of the forward reference (h = 2^-20): 6.8e-10 of max(1, |g|)."""
import argparse
import os
import sys

import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import flowgather_grad_refs as G  # noqa: E402
import flowgather_refs as R  # noqa: E402
from sin_inn_amd import flowsynth  # noqa: E402

F64 = torch.float64
MISS = 100.0


@pytest.fixture(scope='module')
def refs():
    """name -> (inputs, float64 gradient, budget), computed once and left unchanged"""
    out = {}
    for name in G.HOST_CASES:
        inputs = G.case(name)
        i0, i1, fl, slots, taus, g = inputs
        assert G.cells_agree(fl, slots, *i0.shape[-2:]), name
        out[name] = (inputs, *G.gather_grad64(*inputs))
    return out


def composed_grad(i0, i1, fl, slots, taus, g, dtype=torch.float32, **kw):
    flows = fl.to(dtype).clone().requires_grad_(True)
    out = flowsynth.gather_composed(i0.to(dtype), i1.to(dtype), flows, slots, taus, flow_grad=True, **kw)
    out.backward(g.to(dtype))
    return flows.grad


def _ratio(got, x64, budget):
    """the worst |got - x64| / budget over every element (0 / 0 counts as 0: an element with budget 0 must be exact)"""
    err = (got.to(F64) - x64).abs()
    err = torch.where(torch.isfinite(err), err, torch.full_like(err, float('inf')))
    ratio = torch.where(err == 0, torch.zeros_like(err), err / budget)
    return float(ratio.max())


# ---- 1. the reference against autograd in float64 and against central differences of the forward reference ----

@pytest.mark.parametrize('name', G.HOST_CASES)
def test_reference_matches_float64_autograd(refs, name):
    inputs, d64, _ = refs[name]
    got = composed_grad(*inputs, dtype=F64)
    scale = max(float(d64.abs().max()), 1e-30)
    assert float((got - d64).abs().max()) <= 1e-12 * scale


def test_reference_matches_central_differences(refs):
    """out at a pixel depends on the flows at that pixel only, so one perturbed channel plane gives every pixel's derivative at once"""
    (i0, i1, fl, slots, taus, g), d64, _ = refs['13x37']
    h = 2.0 ** -20
    fl64, g64 = fl.to(F64), g.to(F64)
    named = {(int(r[s]), int(r[2 + s]) + a) for r in slots.reshape(-1, 6).tolist() for s in range(2) for a in range(2)}
    worst = 0.0
    for t in range(fl.shape[0]):
        for ch in range(4):
            if (t, ch) not in named:
                assert float(d64[t, ch].abs().max()) == 0.0
                continue
            sides = []
            for sign in (1, -1):
                moved = fl64.clone()
                moved[t, ch] += sign * h
                out, _ = R.gather64(i0, i1, moved, slots, taus)
                sides.append((out * g64).sum(dim=(0, 1, 2)))
            fd = (sides[0] - sides[1]) / (2 * h)
            worst = max(worst, float(((fd - d64[t, ch]).abs() / d64[t, ch].abs().clamp(min=1.0)).max()))
    print(f'central differences, h = 2^-20: worst |fd - g| / max(1, |g|) = {worst:.3g}')
    assert worst <= 1e-8


# ---- 2. the composed fp32 gradient within the budget on every element ----

@pytest.mark.parametrize('name', G.HOST_CASES)
def test_composed_fp32_gradient_within_budget_everywhere(refs, name):
    inputs, d64, budget = refs[name]
    got = composed_grad(*inputs)
    assert got.dtype == torch.float32 and got.shape == d64.shape
    ratio = _ratio(got, d64, budget)
    print(f'gather_composed fp32 gradient {name}: worst err / budget {ratio:.3f}')
    assert ratio <= 1.0
    if name == '13x37':
        slots = inputs[3]
        assert bool((slots[0, :, 0] == slots[0, :, 1]).all()) and bool((slots[0, :, 2] == 0).all())      # pair 0: reverse rows


# ---- 3. borders and non-finite flows, with exactly representable coordinates ----

def _integer_case(h=6, w=9):
    """tau = 1/2, c = 1/2, one row, G0 = channels 2-3 of slice 1, G1 = channels 0-1 of slice 0; flows 2 (q - p) with q set per test"""
    g = torch.Generator().manual_seed(7)
    i0, i1 = torch.rand(1, 3, h, w, generator=g), torch.rand(1, 3, h, w, generator=g)
    half = G._bits(0.5)
    slots = torch.tensor([[[1, 0, 2, 0, half, half]]], dtype=torch.int32)
    go = torch.rand(1, 1, 3, h, w, generator=g) + 0.5
    return i0, i1, torch.zeros(2, 4, h, w), slots, (0.5,), go


def test_right_hand_derivative_on_a_cell_border():
    i0, i1, fl, slots, taus, go = _integer_case()
    fl[0, 0] = 2.0                         # q1 = p + (1, 0): an integer target, on the border of two cells
    d64, _ = G.gather_grad64(i0, i1, fl, slots, taus, go)
    for dtype in (torch.float32, F64):
        got = composed_grad(i0, i1, fl, slots, taus, go, dtype=dtype)
        assert float((got.to(F64) - d64).abs().max()) < (1e-5 if dtype == torch.float32 else 1e-12)
    # by hand at pixel (2, 3): q1 = (4, 2) exactly; the cell floor(q) has wx0 = 1, so d W / d qx = I1[2, 5] - I1[2, 4]
    y, x = 2, 3
    den = 0.5 + 0.5 + flowsynth.GATHER_EPS
    out = (0.5 * i0[0, :, y, x] + 0.5 * i1[0, :, y, x + 1] + flowsynth.GATHER_EPS * (0.5 * i0[0, :, y, x] + 0.5 * i1[0, :, y, x])) / den
    slope = (i1[0, :, y, x + 2] - i1[0, :, y, x + 1]).to(F64)
    want = 0.5 * 0.5 / den * float((go[0, 0, :, y, x].to(F64) * slope).sum())
    assert abs(float(d64[0, 0, y, x]) - want) < 1e-12 and out.shape == (3,)
    left = (i1[0, :, y, x + 1] - i1[0, :, y, x]).to(F64)
    assert abs(want - 0.5 * 0.5 / den * float((go[0, 0, :, y, x].to(F64) * left).sum())) > 1e-3     # the left-hand one differs


def test_one_column_inside_and_fully_outside():
    i0, i1, fl, slots, taus, go = _integer_case()
    h, w = i0.shape[-2:]
    fl[0, 0, :, 0] = -1.0                  # q1x = -1/2 at x = 0: in (-1, 0), the right column of taps inside
    fl[0, 0, :, w - 1] = 1.0               # q1x = W - 1/2 at x = W - 1: in (W - 1, W), the left column inside
    fl[0, 0, :, 4] = 2.0 * w               # fully outside
    d64, budget = G.gather_grad64(i0, i1, fl, slots, taus, go)
    got = composed_grad(i0, i1, fl, slots, taus, go)
    assert _ratio(got, d64, budget) <= 1.0
    assert float(d64[0, 0, :, 0].abs().min()) > 1e-3 and float(d64[0, 0, :, w - 1].abs().min()) > 1e-3      # d/dqx = +-(t - out) != 0
    assert float(d64[0, :2, :, 4].abs().max()) == 0.0 and float(got[0, :2, :, 4].abs().max()) == 0.0
    assert bool(torch.isfinite(got).all())


@pytest.mark.parametrize('bad', [float('nan'), float('inf'), float('-inf')])
def test_non_finite_flow_gives_zero_for_that_sample_only(bad):
    i0, i1, fl, slots, taus, go = _integer_case()
    fl[1, 2:] = 0.5                        # G0: a fractional sample, so its gradient is not zero
    clean, _ = G.gather_grad64(i0, i1, fl, slots, taus, go)
    fl2 = fl.clone()
    fl2[0, 0, 3, 5] = bad                  # G1's x component at one pixel
    far = fl.clone()
    far[0, 0, 3, 5] = 4.0e9                # the same sample refused for its size: the same D, the same out
    want, budget = G.gather_grad64(i0, i1, far, slots, taus, go)
    for dtype in (torch.float32, F64):
        got = composed_grad(i0, i1, fl2, slots, taus, go, dtype=dtype)
        assert bool(torch.isfinite(got).all())
        assert float(got[0, :2, 3, 5].abs().max()) == 0.0                                   # the non-finite sample: exactly 0
        assert _ratio(got, want, budget) <= 1.0                                             # the other sample: as if G1 were far away
    keep = torch.ones_like(clean, dtype=torch.bool)
    keep[:, :, 3, 5] = False
    assert torch.equal(want[keep], clean[keep])                                             # no other pixel moves
    assert float(want[1, 2:, 3, 5].abs().max()) > 0


# ---- 4. accumulation ----

def test_reverse_row_sums_both_samples_into_one_slice():
    i0, i1, fl, slots, taus, go = _integer_case()
    half = G._bits(0.5)
    rev = torch.tensor([[[0, 0, 0, 0, G._bits(-0.5), half]]], dtype=torch.int32)
    fl[0, 0], fl[0, 1] = 0.25, -0.75
    both, _ = G.gather_grad64(i0, i1, fl, rev, taus, go)
    # the same two samples through two slices that hold the same flows
    two = torch.tensor([[[1, 0, 0, 0, G._bits(-0.5), half]]], dtype=torch.int32)
    fl2 = torch.cat([fl[:1], fl[:1]])
    split, _ = G.gather_grad64(i0, i1, fl2, two, taus, go)
    assert float((both[0, :2] - (split[0, :2] + split[1, :2])).abs().max()) < 1e-15
    assert float(split[0, :2].abs().max()) > 0 and float(split[1, :2].abs().max()) > 0
    assert float(both[:, 2:].abs().max()) == 0.0 and float(both[1].abs().max()) == 0.0     # unnamed: exactly 0
    got = composed_grad(i0, i1, fl, rev, taus, go)
    assert float((got.to(F64) - both).abs().max()) < 1e-5 and float(got[1].abs().max()) == 0.0


def test_two_rows_name_one_slice(refs):
    (i0, i1, fl, slots, taus, g), d64, _ = refs['13x37']
    assert int(slots[1, 0, 1]) == int(slots[1, 2, 1])                       # rows 3 and 5 read the same G1
    ints, distinct = flowsynth.gather_reduce_list(slots, fl.shape[0])
    assert not distinct
    # without row 5 the shared slice holds row 3's part alone: the difference is row 5's
    alone = g.clone()
    alone[1, 2] = 0
    part, _ = G.gather_grad64(i0, i1, fl, slots, taus, alone)
    t = int(slots[1, 0, 1])
    assert float((d64[t, :2] - part[t, :2]).abs().max()) > 0
    assert float(d64[-1].abs().max()) == 0.0                                # the last slice is unnamed


def test_reduce_list_order():
    slots, slices = G.table(2, 3, reverse_first=True, shared=((3, 5),))
    ints, distinct = flowsynth.gather_reduce_list(slots, slices)
    begins, entries = ints[:2 * slices + 1], ints[2 * slices + 1:]
    assert begins[0] == 0 and begins[-1] == len(entries) == 2 * 6 and not distinct
    rows = slots.reshape(-1, 6).tolist()
    for target in range(2 * slices):
        mine = entries[begins[target]:begins[target + 1]]
        assert mine == sorted(mine)                                         # ascending 2 (b K + k) + which: G0 before G1 within a row
        want = [2 * r + s for r, row in enumerate(rows) for s in range(2) if 2 * row[s] + row[2 + s] // 2 == target]
        assert mine == want
    assert entries[begins[0]:begins[1]] == [0, 1]                           # row 0 is a reverse row: its dG0, then its dG1
    assert [e for e in entries[begins[2 * 3]:begins[2 * 3 + 1]]] == [2 * 3 + 1, 2 * 5 + 1]         # rows 3 and 5 share slice 3
    assert begins[2 * (slices - 1)] == begins[2 * slices] == len(entries)   # the unnamed slice has no entry
    plain, _ = G.table(2, 2)
    assert flowsynth.gather_reduce_list(plain, 9)[1] is True
    with pytest.raises(ValueError):
        flowsynth.gather_reduce_list(plain, 3)


# ---- 5. seeded defects of the composed gradient ----

class _Swap(torch.autograd.Function):
    @staticmethod
    def forward(ctx, qx, qy):
        return qx.clone(), qy.clone()

    @staticmethod
    def backward(ctx, gx, gy):
        return gy, gx


def _defect_grad(inputs, defect):
    """the composed fp32 gradient with one defect seeded through the `sample` hook of gather_from"""
    i0, i1, fl, slots, taus, g = inputs
    flows = fl.clone().requires_grad_(True)
    coef = flowsynth.slot_coefficients(slots)
    a1 = torch.tensor(taus, dtype=torch.float32).view(1, -1, 1, 1)
    a = (1 - a1, a1)
    with torch.no_grad():
        calls = []
        flowsynth.gather_from(i0, i1, fl, slots, list(taus), sample=lambda img, qx, qy: calls.append(flowsynth.bilinear_gather(img, qx, qy)) or calls[-1])
        den = (a[0] * calls[0][1] + a[1] * calls[1][1]) + flowsynth.GATHER_EPS
    state = {'which': 0}

    def sample(img, qx, qy):
        which = state['which']
        state['which'] += 1
        if defect == 'swap':
            qx, qy = _Swap.apply(qx, qy)
        scale = None
        if defect == 'no c0' and which == 0:
            scale = 1 / coef[:, :, 0, None, None]
        if defect == 'no a0' and which == 0:
            scale = 1 / a[0].expand_as(qx)
        if defect == 'no 1/D':
            scale = den
        if scale is not None:
            qx, qy = qx * 1, qy * 1
            qx.register_hook(lambda gr: gr * scale)
            qy.register_hook(lambda gr: gr * scale)
        if defect == 'left cell':
            qx, qy = qx - 2.0 ** -12, qy - 2.0 ** -12
        if defect == 'only' and which != state['keep']:
            qx, qy = qx.detach(), qy.detach()
        total, n = flowsynth.bilinear_gather(img, qx, qy)
        return total, (n.detach() if defect == 'no out grad n' else n)

    if defect == 'overwrite':
        parts = []
        for keep in (0, 1):
            parts.append(_defect_grad_only(inputs, keep))
        shared = (slots[..., 0] == slots[..., 1]) & (slots[..., 2] == slots[..., 3])
        out = parts[0] + parts[1]
        for t in slots[..., 1][shared].tolist():
            out[t, :2] = parts[1][t, :2]                                    # dG1 written over dG0
        return out
    out = flowsynth.gather_from(i0, i1, flows, slots, list(taus), sample=sample)
    out.backward(g)
    return flows.grad


def _defect_grad_only(inputs, keep):
    i0, i1, fl, slots, taus, g = inputs
    flows = fl.clone().requires_grad_(True)
    state = {'which': 0}

    def sample(img, qx, qy):
        which = state['which']
        state['which'] += 1
        if which != keep:
            qx, qy = qx.detach(), qy.detach()
        return flowsynth.bilinear_gather(img, qx, qy)

    flowsynth.gather_from(i0, i1, flows, slots, list(taus), sample=sample).backward(g)
    return flows.grad if flows.grad is not None else torch.zeros_like(fl)


@pytest.mark.parametrize('defect', ['no out grad n', 'no c0', 'no a0', 'no 1/D', 'swap', 'overwrite'])
def test_seeded_defect_misses_the_budget(refs, defect):
    inputs, d64, budget = refs['13x37']
    sound = _ratio(composed_grad(*inputs), d64, budget)
    assert sound <= 1.0                                                     # the gradient the feature returns
    assert torch.equal(_defect_grad(inputs, 'none'), composed_grad(*inputs))               # the hook itself changes nothing
    ratio = _ratio(_defect_grad(inputs, defect), d64, budget)
    print(f'seeded defect {defect!r}: worst err / budget {ratio:.3g} (sound: {sound:.3f})')
    assert ratio > MISS


def test_left_hand_cell_on_a_border_misses_the_budget():
    i0, i1, fl, slots, taus, go = _integer_case()
    fl[0, 0] = 2.0
    fl[1, 3] = -2.0
    inputs = (i0, i1, fl, slots, taus, go)
    d64, budget = G.gather_grad64(*inputs)
    assert _ratio(composed_grad(*inputs), d64, budget) <= 1.0
    assert torch.equal(_defect_grad(inputs, 'none'), composed_grad(*inputs))
    ratio = _ratio(_defect_grad(inputs, 'left cell'), d64, budget)
    print(f"seeded defect 'left cell': worst err / budget {ratio:.3g}")
    assert ratio > MISS


# ---- 6. the surface ----

def test_refusals_and_keywords(refs):
    i0, i1, fl, slots, taus, g = refs['13x37'][0]
    flows = fl.clone().requires_grad_(True)
    for fn in (flowsynth.gather, flowsynth.gather_composed):
        with pytest.raises(RuntimeError, match='is an inference operator and has no gradient'):
            fn(i0, i1, flows, slots, taus)                                  # without the keyword: as before
        with pytest.raises(RuntimeError, match='flows only'):
            fn(i0.clone().requires_grad_(True), i1, flows, slots, taus, flow_grad=True)
        with pytest.raises(RuntimeError, match='is an inference operator and has no gradient'):
            fn(i0.clone().requires_grad_(True), i1, fl, slots, taus)
    with pytest.raises(ValueError, match='u8'):
        flowsynth.gather(i0, i1, flows, slots, taus, flow_grad=True, u8=True)
    with pytest.raises(ValueError, match='out='):
        flowsynth.gather(i0, i1, flows, slots, taus, flow_grad=True, out=torch.empty(2, 3, 3, 13, 37))
    # flows that need no gradient, or grad mode off: the plain result
    plain = flowsynth.gather_composed(i0, i1, fl, slots, taus, flow_grad=True)
    assert not plain.requires_grad
    with torch.no_grad():
        assert not flowsynth.gather_composed(i0, i1, flows, slots, taus, flow_grad=True).requires_grad
    assert torch.equal(plain, flowsynth.gather_composed(i0, i1, fl, slots, taus))


_trainer_args = G.trainer_args


def test_trainer_surface():
    from sin_inn_amd import flowtrainer
    off = flowtrainer.FlowTrainer(_trainer_args())
    assert not hasattr(off.args, 'loss_between')                            # like --holdout: the attribute exists only with the flag
    zero = flowtrainer.FlowTrainer(_trainer_args(argv=['--loss-between', '0']))
    assert zero.between_weight == 0 and zero.between_rng is None
    assert off.between_weight == 0 and off.between_rng is None              # the parent's trainer: no generator, no draw
    on = flowtrainer.FlowTrainer(_trainer_args(argv=['--loss-between', '1', '--between-taus', '2'], between_dt=2 / 3))
    assert on.between_weight == 1.0 and on.between_rng is not None
    state = on.between_rng.getstate()
    taus = [0.25, 0.75]
    times = [-1.0, -1 / 3, 1 / 3]
    stamps, table, blend = on.between_table(times, taus)
    want_stamps, want = flowsynth.gather_slots(times, taus, 2 / 3, 'network')
    assert stamps == want_stamps and tuple(table.shape) == (3, 4, 6) and table.dtype == torch.int32
    assert torch.equal(table[:, :2], want) and torch.equal(table[:, 2:], want) and blend == [0.0, 0.0, 1.0, 1.0]
    assert bool((want[0, :, 0] == want[0, :, 1]).all()) and bool((want[1:, :, 2] == 2).all())      # the first pair: reverse rows
    assert on.between_rng.getstate() == state                               # building the table draws nothing
    with pytest.raises(ValueError, match='between_dt'):
        flowtrainer.FlowTrainer(_trainer_args(argv=['--loss-between', '1']))
    # a network on (y, x) has no time axis
    args = _trainer_args(argv=['--loss-between', '1'], between_dt=2 / 3)

    class Flat(torch.nn.Module):
        domain_dim = 2
    args.net = Flat()
    with pytest.raises(ValueError, match='domain_dim 2'):
        flowtrainer.FlowTrainer(args)


def test_namespace_without_the_switches_builds_the_parent_trainer():
    from sin_inn_amd import flowtrainer
    ns = argparse.Namespace(**vars(_trainer_args()))
    assert not any(hasattr(ns, name) for name in ('loss_between', 'between_taus', 'between_back'))
    model = flowtrainer.FlowTrainer(ns)
    assert model.between_weight == 0 and model.between_rng is None
