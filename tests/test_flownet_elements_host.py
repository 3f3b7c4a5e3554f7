"""CPU: what tests/test_gpu_flownet_elements.py rests on, established from the float64 reference alone (tests/flownet_element_refs.py, no
kernel runs), for every case of that file; its largest forward grid (3 x 151 x 290) is replaced by `past_caps` (3 x 113 x 200).  DESIGN 14.13

  1. the launch plan rebuilt from the sources' constants walks unequal numbers of tiles at `past_caps` (chain blocks 2 or 3, hidden
     chunks 8 or 9, layer-1 chunks 16 or 17, narrow chunks 4 or 5) and five forward blocks take a second tile at 3 x 151 x 290;
  2. the exactness precondition of the integer backward pass: sum |terms| of every output element and of every intermediate dh element
     is below 2^23, so every partial sum in any order is an integer below 2^24; an fp32 torch evaluation (another order) EQUALS float64;
  3. the fp32 torch restatement (another summation order, torch's own sin and exp) is within every per-element budget: gW1 of the integer
     regime and the four forward stages.  A ratio above 1 here would mean a wrong budget, not a wrong kernel;
  4. seeded defects, built from the float64 pieces, fall outside the budget or break the equality:
     (a) one tile's contribution removed from one element of gW2; (b) one chunk's partial added twice to one gb2; (e) the pad rows' 3
     leaking into gW4 (the pad rows taking the clamped point's dout); (c) one column of gW1 below 1e-3 of the tensor's maximum scaled by
     1.1; (d) one row of saved[1] replaced by the neighbouring point's row.
     For (c) and (d) the yardstick of the other flownet tests, max |a - ref| / max |ref| <= min(4 units, 1e-4), does NOT see the defect.

On (c): in the integer regime the fp32-torch unit of gW1 is 1e-7 .. 3e-7 for the RBF / PE kinds, so the old budget is 4e-7 .. 1.2e-6 of the
maximum there and a column has to be below 1e-5 of it to hide a 10 % error; such columns belong to RBF centres whose feature is below
1e-5, where MULT delta = 8 u = 4.8e-7 per unit of |dh1| is itself 10 % of the feature: neither yardstick resolves them (0 of 512 columns
at any shape).  The column that shows the gap is where the old budget stands at its ceiling: a Fourier network, whose fp32-torch unit is
the phase error of torch's fp32 matmul (1e-5 .. 2.5e-5), at a point where a well-conditioned (slow) feature crosses zero.  The case is
the first point of the `few` pose list that has such a column.
On (d): the other tests assert of `saved` only that it is finite and non-negative, and compare flows, which a wrong row of `saved` does
not change; both are asserted blind.  Through gW3 = dh3^T saved[1] the old yardstick would see one wrong row of 1443 (change 4e-5 .. 1e-3
of the maximum against a budget of 1e-6) and only just misses the best-hidden row of 67 800 (1.2e-6 .. 1.5e-6 against 2e-6): printed.

Measured (python -m pytest -s), worst error / budget of the fp32 torch restatement:
  gW1     one 1.4e-7 (PE) .. 0.25 (FFN, RBFG: delta is the restatement's own error)   few 0.037 .. 0.048   past_caps 2.5e-4 .. 8.8e-4
  forward saved0 0.004 .. 0.13 (PE, PPE: 24 terms)   saved1 0.013 .. 0.022   saved2 0.012 .. 0.020   flows 0.005 .. 0.010
  worst sum |terms|: one 142, few 2574, past_caps 808 576 (gb1) against 2^23 = 8 388 608
"""
import os
import sys

import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import flownet_element_refs as R  # noqa: E402
from flownet_refs import PROGRESSIVE, net_tensors  # noqa: E402

F64 = torch.float64
B_HOST = {'one': R.B_SHAPES['one'], 'ragged': R.B_SHAPES['ragged'], 'past_caps': R.A_SHAPES['past_caps']}
B_CASES = [(name, shape) for name in R.NETS for shape in B_HOST if shape != 'past_caps' or name in R.B_PAST_CAP_NETS]
_integer, _nets = {}, {}


def integer_case(shape):
    """(points, inputs, float64 gradients, [dh1, dh2, dh3], dout, worst sum |terms|) of a part A shape, computed once and left unchanged"""
    if shape not in _integer:
        pts = R.Points(R.A_SHAPES[shape])
        inp = R.integer_inputs(pts.n, R.Plan(pts.n).npad)
        _integer[shape] = (pts, inp, *R.backward_ref(inp, pts.n))
    return _integer[shape]


def network(name):
    """(buffers, weights, host mask, k_active)"""
    if name not in _nets:
        _nets[name] = (*net_tensors(R.build(name)), *R.ramp(name))
    return _nets[name]


def test_plans_walk_unequal_numbers_of_tiles():
    c = R.kernel_constants()
    assert (c['P'], c['FWD_CAP'], c['CHAIN_CAP'], c['CHUNK_ELEMS']) == (64, 2048, 512, 1 << 15)
    wide, narrow = R.Plan(R.Points(R.A_SHAPES['past_caps']).n, 'RBF'), R.Plan(R.Points(R.A_SHAPES['past_caps']).n, 'PE')
    assert (wide.n, wide.ntiles, wide.npad - wide.n) == (67800, 1060, 40) and 113 * 200 % 64 != 0
    assert (wide.chain_blocks, wide.hidden_chunks, wide.l1_chunks, narrow.l1_chunks) == (512, 128, 64, 256)
    assert (wide.chain_walk, wide.hidden_walk, wide.l1_walk, narrow.l1_walk) == ((2, 3), (8, 9), (16, 17), (4, 5))
    few = R.Plan(171, 'RBF')
    assert (few.ntiles, few.npad - few.n, few.chain_walk, few.hidden_walk, few.l1_walk) == (3, 21, (1, 1), (1, 1), (1, 1))
    one = R.Plan(1, 'PE')
    assert (one.ntiles, one.npad, one.l1_chunks) == (1, 64, 1)
    cap = R.Plan(R.Points(R.B_SHAPES['past_cap']).n)
    assert (cap.n, cap.ntiles, cap.fwd_blocks, cap.fwd_walk) == (131370, 2053, 2048, (1, 2)) and cap.ntiles - cap.fwd_blocks == 5
    ragged = R.Plan(R.Points(R.B_SHAPES['ragged']).n)
    assert (ragged.n, ragged.ntiles, ragged.n % 64, 13 * 37 % 64) == (1443, 23, 35, 33)


@pytest.mark.parametrize('shape', list(R.A_SHAPES))
def test_integer_backward_is_exact_in_any_order(shape):
    pts, inp, grads, dh, dout, worst = integer_case(shape)
    print(f'worst sum|terms| ({shape}, N = {pts.n}): ' + '  '.join(f'{k} {v:.0f}' for k, v in worst.items()) + f'   limit {R.EXACT_LIMIT:.0f}')
    assert set(worst) == {'dh1', 'dh2', 'dh3'} | set(R.EXACT_NAMES)
    assert max(worst.values()) < R.EXACT_LIMIT
    s = inp['saved']
    assert set(s[:, :pts.n].unique().tolist()) <= {0.0, 1.0, 2.0} and bool((s[:, pts.n:] == 3).all())
    assert 0.4 < float((s[:, :pts.n] == 0).float().mean()) < 0.6 or pts.n == 1
    for k in ('W2', 'W3', 'W4', 'dflows'):
        assert set(inp[k].unique().tolist()) <= {-1.0, 0.0, 1.0}
    # another order, in fp32: torch's own matmul and sums
    n, f32 = pts.n, torch.float32
    sv = s[:, :n]
    d32 = inp['dflows'].t() * R.SCALE_A
    h3 = (d32 @ inp['W4']) * (sv[2] > 0)
    h2 = (h3 @ inp['W3']) * (sv[1] > 0)
    h1 = (h2 @ inp['W2']) * (sv[0] > 0)
    got = {'gW4': d32.t() @ sv[2], 'gb4': d32.sum(0), 'gW3': h3.t() @ sv[1], 'gb3': h3.sum(0), 'gW2': h2.t() @ sv[0], 'gb2': h2.sum(0),
           'gb1': h1.sum(0)}
    for nm in R.EXACT_NAMES:
        assert got[nm].dtype == f32 and torch.equal(got[nm].to(F64), grads[nm]), nm
    assert torch.equal(h1.to(F64), dh[0])


@pytest.mark.parametrize('shape', list(R.A_SHAPES))
@pytest.mark.parametrize('name', R.NETS)
def test_gw1_budget_holds_for_the_fp32_restatement(name, shape):
    pts, inp, grads, dh, dout, worst = integer_case(shape)
    bufs, weights, mask, k_active = network(name)
    plan = R.Plan(pts.n, name)
    ref, budget, _ = R.gw1_ref(name, bufs, pts, mask, dh[0], plan)
    got = dh[0].float().t() @ R.layer1_in(name, bufs, pts, mask, torch.float32)
    ratio = R.element_ratio(got, ref, budget)
    print(f'ratio({name} {shape} gW1, fp32 torch) = {ratio:.3g}   [chain {plan.p * plan.l1_walk[1]}, partials {plan.l1_chunks}]')
    assert ratio <= 1
    assert tuple(ref.shape) == (256, {'PE': 24, 'PPE': 27, 'PRBF': 515}.get(name, 512))
    if name in PROGRESSIVE:
        closed = R.closed_columns(mask, k_active)
        # the sign of the zero is the kernel's property (its reduce kernel writes +0), not the restatement's (-d x 0 = -0)
        assert bool(closed.any()) and float(got[:, closed].abs().max()) == 0.0 and float(ref[:, closed].abs().max()) == 0.0


@pytest.mark.parametrize('name,shape', B_CASES)
def test_forward_budgets_hold_for_the_fp32_restatement(name, shape):
    pts = R.Points(B_HOST[shape])
    bufs, weights, mask, _ = network(name)
    saved, flows = R.fp32_forward(name, bufs, weights, pts, mask)
    stages = R.forward_stages(name, bufs, weights, pts, mask, saved, flows)
    assert list(stages) == ['saved0', 'saved1', 'saved2', 'flows']
    for stage, (got, ref, budget) in stages.items():
        ratio = R.element_ratio(got, ref, budget)
        print(f'ratio({name} {shape} {stage}, fp32 torch) = {ratio:.3g}')
        assert ratio <= 1, stage


# ---- seeded defects ----
@pytest.mark.parametrize('shape', ['few', 'past_caps'])
def test_defects_break_the_equalities(shape):
    pts, inp, grads, dh, dout, worst = integer_case(shape)
    plan = R.Plan(pts.n, 'RBF')
    s = inp['saved'].to(F64)
    # (a) one tile's contribution removed from one element of gW2: the last, ragged tile and the element it contributes most to
    rows = slice((plan.ntiles - 1) * plan.p, pts.n)
    tile = dh[1][rows].t() @ s[0, rows]
    j, k = divmod(int(tile.abs().argmax()), 256)
    assert tile[j, k] != 0
    wrong = grads['gW2'].clone()
    wrong[j, k] -= tile[j, k]
    assert not torch.equal(wrong, grads['gW2'])
    # (b) one chunk's partial added twice to one gb2: the last chunk of the plan
    part = dh[1][plan.chunk_rows(plan.hidden_chunks - 1, plan.hidden_chunks)].sum(0)
    j = int(part.abs().argmax())
    assert part[j] != 0
    wrong = grads['gb2'].clone()
    wrong[j] += part[j]
    assert not torch.equal(wrong, grads['gb2'])
    # (e) the pad rows' 3 leaking into gW4: every pad row takes the dout of the clamped point N - 1
    assert plan.npad > pts.n and bool((dout[-1] != 0).all())
    leak = (plan.npad - pts.n) * dout[-1][:, None] * s[2, pts.n:pts.n + 1]
    assert bool((leak != 0).all()) and not torch.equal(grads['gW4'] + leak, grads['gW4'])


def hidden_column_case():
    """(points, dh1, the column): the first single point of the `few` list at which an FFN column of gW1 is below 1e-3 of the maximum,
    hidden from the old yardstick when scaled by 1.1 and outside its own budget"""
    bufs, weights, _, _ = network('FFN')
    _, inp, _, dh, _, _ = integer_case('few')
    for first in range(171):
        pts = R.Points(('list', 1, first))
        dh1 = dh[0][first:first + 1]
        if float(dh1.abs().max()) == 0:
            continue
        ref, budget, _ = R.gw1_ref('FFN', bufs, pts, None, dh1, R.Plan(1, 'FFN'))
        got32 = dh1.float().t() @ R.layer1_in('FFN', bufs, pts, None, torch.float32)
        old = R.relmax_budget(got32, ref)
        colmax = ref.abs().amax(0)
        ok = (colmax < 1e-3 * ref.abs().max()) & (0.1 * colmax <= old * ref.abs().max()) & ((0.1 * ref.abs()) > budget).any(0)
        if bool(ok.any()):
            return pts, dh1, ref, budget, got32, int(torch.nonzero(ok)[0])
    raise AssertionError('no point of the list has such a column')


def test_defect_in_a_small_column_of_gw1_is_outside_the_budget_and_hidden_from_the_old_yardstick():
    pts, dh1, ref, budget, got32, k = hidden_column_case()
    wrong = ref.clone()
    wrong[:, k] *= 1.1
    old = R.relmax_budget(got32, ref)
    seen_old, seen_new = R.relmax(wrong, ref), R.element_ratio(wrong, ref, budget)
    print(f'(c) FFN, one point {pts.list.tolist()}, column {k}: |column| / max = {float(ref[:, k].abs().max() / ref.abs().max()):.3g}; '
          f'old yardstick error {seen_old:.3g} against its budget {old:.3g}; per element error / budget = {seen_new:.3g}')
    assert float(ref[:, k].abs().max()) < 1e-3 * float(ref.abs().max())
    assert seen_old <= old, 'the old yardstick sees it'
    assert seen_new > 1, 'the per-element budget does not'
    assert R.element_ratio(got32, ref, budget) <= 1
    # the integer regime of the RBF kinds: what each yardstick resolves (see the module's docstring); figures only
    for shape in ('few', 'past_caps'):
        p, _, _, dh, _, _ = integer_case(shape)
        bufs, _, _, _ = network('RBF')
        r, b, _ = R.gw1_ref('RBF', bufs, p, None, dh[0], R.Plan(p.n, 'RBF'))
        g32 = dh[0].float().t() @ R.layer1_in('RBF', bufs, p, None, torch.float32)
        colmax, top = r.abs().amax(0), float(r.abs().max())
        small = colmax < 1e-3 * top
        caught, hidden = ((0.1 * r.abs()) > b).any(0), 0.1 * colmax <= R.relmax_budget(g32, r) * top
        print(f'    RBF {shape}: {int(small.sum())} columns below 1e-3 of the maximum; a 10 % error is outside the per-element budget in '
              f'{int((small & caught).sum())}, hidden from the old yardstick in {int((small & hidden).sum())}, both in {int((small & caught & hidden).sum())}')


@pytest.mark.parametrize('name,shape', [('RBF', 'ragged'), ('PRBF', 'ragged'), ('PE', 'ragged'), ('RBF', 'past_caps')])
def test_defect_in_one_row_of_saved_is_outside_the_budget_and_hidden_from_the_old_checks(name, shape):
    pts = R.Points(B_HOST[shape])
    bufs, weights, mask, _ = network(name)
    saved, flows = R.fp32_forward(name, bufs, weights, pts, mask)
    n = pts.n
    # the row: the last point of the first frame, whose neighbour in memory is the first point of the next frame (a tile straddles both)
    p = n // 3 - 1
    wrong = saved.clone()
    wrong[1, p] = saved[1, p + 1]
    assert not torch.equal(wrong[1, p], saved[1, p])
    stages = R.forward_stages(name, bufs, weights, pts, mask, wrong, flows)
    ratios = {k: R.element_ratio(*v) for k, v in stages.items()}
    print(f'(d) {name} {shape}, row {p} of saved[1]: error / budget per stage ' + '  '.join(f'{k} {v:.3g}' for k, v in ratios.items()))
    assert ratios['saved1'] > 1 and ratios['saved2'] > 1, 'the row is wrong against its input and as the input of the next layer'
    assert ratios['saved0'] <= 1 and ratios['flows'] <= 1
    # what the other tests check of a forward call: `saved` finite and non-negative, flows against float64 in the max norm
    assert bool(torch.isfinite(wrong).all()) and float(wrong.min()) >= 0.0
    w64 = [q.to(F64) for q in weights]
    x = R.layer1_in(name, bufs, pts, mask, F64)
    for l in range(3):
        x = torch.relu(x @ w64[2 * l].t() + w64[2 * l + 1])
    ref64 = ((x @ w64[6].t() + w64[7]) * R.SCALE_B).t()
    assert R.relmax(flows, ref64) <= R.CEIL                             # the restatement is its own unit: the ceiling is what is left
    # through gW3 = dh3^T saved[1], with an upstream gradient as the other tests draw it: printed, see the module's docstring
    up = torch.randn(4, n, generator=torch.Generator().manual_seed(11)).to(F64)
    s = saved.to(F64)
    dh3 = ((up.t() * R.SCALE_B) @ w64[6]) * (s[2] > 0)
    gw3 = dh3.t() @ s[1]
    change = dh3[:-1].abs().amax(1) * (s[1][1:] - s[1][:-1]).abs().amax(1) / gw3.abs().max()
    old = R.relmax_budget(dh3.float().t() @ saved[1], gw3)
    print(f'    through gW3 the old yardstick (budget {old:.3g}) would meet a change of {float(change[p]):.3g} for this row, '
          f'{float(change.min()):.3g} for the best hidden row, median {float(change.median()):.3g}')
