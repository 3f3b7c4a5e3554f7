"""CPU: what tests/test_gpu_siren_elements.py rests on, established from torch alone (tests/siren_element_refs.py, no kernel runs).
DESIGN 14.14

  1. the launch plan and the layout of `saved` and the workspace, rebuilt from the sources' constants: the counts the cases rely on, and
     `views` round-trips;
  2. the exactness precondition of the integer backward pass (phases 0, omega 1): sum |terms| of every output element and of every
     intermediate dz element is below 2^23 (gW1: in units of 1/4), so every partial sum in any order is exact in fp32; an fp32 torch
     evaluation (another order) EQUALS float64;
  3. the fp32 torch restatement (another summation order, torch's own sin / cos) is within every per-element budget of parts A2 and B, in
     both phase regimes.  A ratio above 1 here would mean a wrong budget, not a wrong kernel.  gb5 is restated as the kernels sum it, in
     double and rounded once: its budget 2 u |sum| + u^2 N sum |dout| has no room for an fp32 sum;
  4. what uniform sine error the forward budgets resolve (the forward's sinf is visible only through 256-term sums);
  5. seeded defects, built from the float64 pieces, each outside a budget, with the yardstick of the other SIREN tests,
     max |a - ref| / max |ref| <= min(4 units, 1e-4), printed beside it.

Measured (python -m pytest -s):
  worst sum |terms| against 2^23 = 8 388 608 (W2 .. W4 density 1/32; gW1 in units of 1/4):
      one 5351 (g_poses)   few 22 549 (gW1)   ragged 200 081 (gW1)   past_cap 4 849 619 (gW1)   past_cap_list 4 828 965 (gW1)
      gb1 at 38 586 points: 2 165 728; |dz_1| <= 253, |dz_2| <= 104, |dz_3| <= 30, |dz_4| <= 4
  fp32 torch restatement, worst error / budget over the shapes, regime (a) | (b); d_sin = d_cos = 2 u (the floor) in both:
      hin 0.075 | 0.075   dz4 0.31 | 0.30   dz3, dz2 0.027 | 0.028   gW2 .. gW4 0.071 | 0.080   gb2 .. gb4 0.010 | 0.015
      gW5 0.034 | 0.028   gb5 0.35 | 0.35   gW1 0.0066 | 0.0052   gb1 0.0066 | 0.0052   g_poses 0.0016 | 0.0019
      forward: u1 0.52   u2 .. u4 0.019   flows 0.010; W1, b1 x 8 (|u_1| <= 310): u1 0.49, the rest as before
  the forward budgets resolve a uniform sine error of 8.9e-6 (149 u) or more, against the 4.8e-7 (8 u) the backward's `hin` stage resolves
  defects (ragged | past_cap): a tile removed from gb2 3650 | 34 budgets, a chain block's partial twice in gW1 265 | 8.5, pad rows in gb1
      569 | 4.7; W2^T / W3^T exchanged 4.5e4 budgets at dz2; u_2 gating dz_3 2.1e6 at dz3; a row of hin[1] from its neighbour 1460 budgets at
      gW3 (best hidden row: 64); a sine reduced with one fp32 2 pi 56 budgets of hin, first outside at |phase| = 22 rad (2.8 budgets at
      |phase| <= 40).  With these inputs the max norm would see each of the sum and chain defects too (0.05 .. 1.3 of the maximum against
      budgets of 4e-7 .. 2e-6); it does not look at dz, hin or the transposed weights at all, and no other test feeds phases beyond 40 rad
"""
import math
import os
import sys

import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import siren_element_refs as R  # noqa: E402
from siren_refs import OMEGA, siren_tensors  # noqa: E402

F64 = torch.float64
HOST_SHAPES = ('one', 'few', 'ragged', 'past_cap')
_integer, _stage, _weights = {}, {}, []


def weights():
    if not _weights:
        _weights.extend(siren_tensors(R.build()))
    return _weights


def integer_case(shape):
    """(points, inputs, float64 gradients, [dz_1 .. dz_4], g_poses, worst sum |terms|) of a shape, computed once and left unchanged"""
    if shape not in _integer:
        pts = R.quarter_points(R.SHAPES[shape])
        inp = R.integer_inputs(pts.n)
        _integer[shape] = (pts, inp, *R.integer_ref(inp, pts.poses(F64)))
    return _integer[shape]


def stage_case(shape, regime):
    """one backward call restated in fp32 torch: (points, plan, dflows, saved (4, N, 256), dz, hin, grads, g_poses), once"""
    if (shape, regime) not in _stage:
        pts = R.Points(R.SHAPES[shape])
        plan = R.Plan(pts.n)
        saved = R.fp32_forward(weights(), pts, OMEGA, R.SCALE)[0] if regime == 'a' else R.synthetic_phases(plan.npad)[:, :pts.n]
        dflows = R.upstream(pts.n)
        _stage[(shape, regime)] = (pts, plan, dflows, saved, *R.fp32_backward(weights(), pts, OMEGA, R.SCALE, dflows, saved))
    return _stage[(shape, regime)]


def test_plan_and_layout():
    c = R.kernel_constants()
    assert (c['P'], c['CHAIN_CAP'], c['SINES'], c['IN'], c['HID'], c['OUT']) == (64, 512, 4, 3, 256, 4)
    assert (c['PART_GB1'], c['PART_GW5'], c['PART_GB5'], c['PART']) == (768, 1024, 2048, 2056)
    one, few, ragged, cap = (R.Plan(R.Points(R.SHAPES[s]).n) for s in HOST_SHAPES)
    assert (one.n, one.ntiles, one.npad, one.chain_blocks, one.hidden_chunks) == (1, 1, 64, 1, 1)
    assert (few.n, few.ntiles, few.npad - few.n, few.chain_walk, few.hidden_walk) == (171, 3, 21, (1, 1), (1, 1)) and 64 - 21 == 43
    assert (ragged.n, ragged.ntiles, ragged.n % 64, 13 * 37 % 64, ragged.chain_walk, ragged.hidden_walk) == (1443, 23, 35, 33, (1, 1), (1, 1))
    assert (cap.n, cap.ntiles, cap.n - 602 * 64, 109 * 118 % 64) == (38586, 603, 58, 62)
    assert (cap.chain_blocks, cap.chain_walk, cap.hidden_chunks, cap.hidden_walk) == (512, (1, 2), 128, (4, 5))
    assert (cap.chain_terms, cap.hidden_terms, ragged.chain_terms, ragged.hidden_terms) == (642, 450, 89, 89)
    assert R.Points(R.SHAPES['past_cap_list']).n == cap.n
    # the layout helper round-trips: each region of a numbered workspace is where siren_backward_launch carves it
    for plan in (one, few):
        ls = plan.lstride
        ws, saved = torch.arange(plan.ws_floats + 7, dtype=F64), torch.arange(4 * ls, dtype=F64)
        dz, hin, wt, sv = R.views(ws, saved, plan.ntiles)
        assert tuple(dz.shape) == tuple(hin.shape) == (3, plan.npad, 256) and tuple(wt.shape) == (3, 256, 256) and tuple(sv.shape) == (4, plan.npad, 256)
        assert (float(dz[0, 0, 0]), float(hin[0, 0, 0]), float(wt[0, 0, 0]), float(wt[2, 255, 255])) == (0, 3 * ls, 6 * ls, plan.ws_floats - 1)
        assert float(dz[2, 5, 7]) == 2 * ls + 5 * 256 + 7 and float(hin[1, plan.npad - 1, 255]) == 5 * ls - 1 and float(sv[3, 1, 2]) == 3 * ls + 258
        dz[1, 3, 4] = -1.0
        assert float(ws[ls + 3 * 256 + 4]) == -1.0                      # views, not copies


@pytest.mark.parametrize('shape', list(R.SHAPES))
def test_integer_backward_is_exact_in_any_order(shape):
    pts, inp, grads, dz, g_poses, worst = integer_case(shape)
    top = max(worst, key=worst.get)
    print(f'worst sum|terms| ({shape}, N = {pts.n}): ' + '  '.join(f'{k} {v:.0f}' for k, v in worst.items()) + f'   worst {top}, limit {R.EXACT_LIMIT:.0f}')
    assert set(worst) == {'dz1', 'dz2', 'dz3', 'dz4', 'gb1', 'gb2', 'gb3', 'gb4', 'gb5', 'gW1', 'g_poses'}
    assert max(worst.values()) < R.EXACT_LIMIT
    for k in ('W1', 'W2', 'W3', 'W4', 'W5', 'dflows'):
        assert set(inp[k].unique().tolist()) <= {-1.0, 0.0, 1.0}
    assert inp['dflows'][:, -1].tolist() == [1.0, -1.0, 1.0, -1.0]
    c = pts.poses(torch.float32)
    assert bool((c * 4 == (c * 4).round()).all()) and float(c.abs().max()) <= 1
    # another order, in fp32: torch's own matmul and sums
    d = inp['dflows'].t() * R.SCALE_A1
    z4 = d @ inp['W5']
    z3 = z4 @ inp['W4']
    z2 = z3 @ inp['W3']
    z1 = z2 @ inp['W2']
    got = {'gb1': z1.sum(0), 'gb2': z2.sum(0), 'gb3': z3.sum(0), 'gb4': z4.sum(0), 'gb5': d.sum(0), 'gW1': z1.t() @ c}
    for nm, g in got.items():
        assert g.dtype == torch.float32 and torch.equal(g.to(F64), grads[nm]), nm
    for a, b in zip((z1, z2, z3, z4), dz):
        assert torch.equal(a.to(F64), b)
    assert torch.equal((z1 @ inp['W1']).to(F64), g_poses)
    # at phase 0 the sine is 0 and the cosine 1, exactly, in torch as in any correct sincosf
    zero = torch.zeros(3)
    assert torch.equal(torch.sin(zero), zero) and torch.equal(torch.cos(zero), torch.ones(3))


@pytest.mark.parametrize('regime', ['a', 'b'])
@pytest.mark.parametrize('shape', HOST_SHAPES)
def test_backward_budgets_hold_for_the_fp32_restatement(shape, regime):
    pts, plan, dflows, saved, dz, hin, grads, g_poses = stage_case(shape, regime)
    stages = R.backward_stages(weights(), pts, OMEGA, R.SCALE, dflows, saved, dz, hin, grads, plan, g_poses)
    assert list(stages) == ['hin0', 'hin1', 'hin2', 'dz4', 'dz3', 'dz2', 'gW2', 'gb2', 'gW3', 'gb3', 'gW4', 'gb4', 'gW5', 'gb5', 'gW1', 'gb1', 'g_poses']
    ratios = {k: R.element_ratio(*v) for k, v in stages.items()}
    print(f'ratio({shape} regime {regime}, fp32 torch): ' + '  '.join(f'{k} {v:.3g}' for k, v in ratios.items())
          + f'   [max |phase| {float(saved.abs().max()):.4g}, d_sin {R.trig_delta(saved)[0] / R.U:.3g} u, d_cos {R.trig_delta(saved)[1] / R.U:.3g} u]')
    assert all(v <= 1 for v in ratios.values()), ratios


@pytest.mark.parametrize('shape', HOST_SHAPES + ('ragged x8',))
def test_forward_budgets_hold_for_the_fp32_restatement(shape):
    w = weights() if shape in R.SHAPES else R.scaled_first_layer(weights())
    pts = R.Points(R.SHAPES[shape.split()[0]])
    saved, flows = R.fp32_forward(w, pts, OMEGA, R.SCALE)
    stages = R.forward_stages(w, pts, OMEGA, R.SCALE, saved, flows)
    assert list(stages) == ['u1', 'u2', 'u3', 'u4', 'flows']
    ratios = {k: R.element_ratio(*v) for k, v in stages.items()}
    eps = R.resolved_sine_error(w, OMEGA, R.SCALE, saved, pts.n)
    print(f'ratio({shape}, fp32 torch): ' + '  '.join(f'{k} {v:.3g}' for k, v in ratios.items())
          + f'   [max |u_1| {float(saved[0].abs().max()):.4g}; resolves a uniform sine error of {eps:.3g} = {eps / R.U:.3g} u]')
    assert all(v <= 1 for v in ratios.values()), ratios
    assert eps > R.MULT * 2 * R.U                                        # what part B does not claim: a sine error below this passes it
    if shape == 'ragged x8':
        assert 200 < float(saved[0].abs().max()) < 1000


# ---- seeded defects ----
def old_yardstick(wrong, got32, ref):
    """(the defect's error, the budget) in the max norm of the other SIREN tests"""
    return R.relmax(wrong, ref), R.relmax_budget(got32, ref)


@pytest.mark.parametrize('shape', ['ragged', 'past_cap'])
def test_defects_in_the_sums(shape):
    pts, plan, dflows, saved, dz, hin, grads, g_poses = stage_case(shape, 'a')
    n, w = pts.n, [p.to(F64) for p in weights()]
    stages = R.backward_stages(weights(), pts, OMEGA, R.SCALE, dflows, saved, dz, hin, grads, plan, g_poses)
    dz1, _ = R.dz_stage(dz[0].to(F64), w[2], saved[0].to(F64), OMEGA, 2 * R.U)
    c = pts.poses(F64)

    def report(tag, stage, delta):
        """`delta`: per element, the change the defect makes if it strikes that element"""
        got32, ref, budget = stages[stage]
        caught = delta.abs() > budget
        _, old = old_yardstick(ref, got32, ref)
        hidden = delta.abs() <= old * ref.abs().max()
        k = int((delta.abs() / budget).argmax())
        wrong = ref.clone()
        wrong.view(-1)[k] += delta.reshape(-1)[k]
        seen_old, seen_new = R.relmax(wrong, ref), R.element_ratio(wrong, ref, budget)
        print(f'{tag} ({shape}, {stage}): outside the per-element budget in {int(caught.sum())} of {delta.numel()} elements, hidden from the max '
              f'norm (budget {old:.3g}) in {int(hidden.sum())}, both in {int((caught & hidden).sum())}; the most visible element: {seen_new:.3g} '
              f'budgets, {seen_old:.3g} in the max norm')
        assert seen_new > 1
        assert R.element_ratio(got32, ref, budget) <= 1
        return int((caught & hidden).sum())

    # one tile's contribution removed from an element of gb2: the last, ragged tile
    rows = slice((plan.ntiles - 1) * plan.p, n)
    report('a tile removed', 'gb2', -dz[0][rows].to(F64).sum(0))
    # one chain block's partial added twice to a gW1 element: the last block of the plan
    r = plan.chunk_rows(plan.chain_blocks - 1, plan.chain_blocks)
    report('a partial twice', 'gW1', dz1[r].t() @ c[r])
    # the pad rows entering gb1 with the clamped point's dout (and its phases: the forward clamps the point)
    assert plan.npad > n
    report('pad rows leak', 'gb1', (plan.npad - n) * dz1[n - 1])


def test_defects_in_the_chain():
    pts, plan, dflows, saved, dz, hin, grads, g_poses = stage_case('ragged', 'a')
    n, w = pts.n, [p.to(F64) for p in weights()]
    stages = R.backward_stages(weights(), pts, OMEGA, R.SCALE, dflows, saved, dz, hin, grads, plan, g_poses)
    u = saved.to(F64)
    # W2^T and W3^T exchanged in the chain: dz_2 from W2
    wrong, _ = R.dz_stage(dz[1].to(F64), w[2], u[1], OMEGA, 2 * R.U)
    got32, ref, budget = stages['dz2']
    ratio = R.element_ratio(wrong, ref, budget)
    seen, old = old_yardstick(wrong.sum(0), grads[3], stages['gb2'][1])
    print(f'W2^T / W3^T exchanged: dz2 {ratio:.3g} budgets; through gb2 the max norm sees {seen:.3g} against {old:.3g}')
    assert ratio > 1
    # the phase of the wrong layer gating dz_3: u_2 instead of u_3
    wrong, _ = R.dz_stage(dz[2].to(F64), w[6], u[1], OMEGA, 2 * R.U)
    got32, ref, budget = stages['dz3']
    ratio = R.element_ratio(wrong, ref, budget)
    seen, old = old_yardstick(wrong.sum(0), grads[5], stages['gb3'][1])
    print(f'u_2 gating dz_3: dz3 {ratio:.3g} budgets; through gb3 the max norm sees {seen:.3g} against {old:.3g}')
    assert ratio > 1
    # one row of hin[1] replaced by its neighbour in memory, read by the weight gradient: per element at gW3
    got32, ref, budget = stages['gW3']
    d3, h2 = dz[1].to(F64), hin[1].to(F64)
    change = d3[:-1].abs().amax(1) * (h2[1:] - h2[:-1]).abs().amax(1) / ref.abs().max()
    _, old = old_yardstick(ref, got32, ref)
    worst = {}
    for tag, p in (('the last point of the first frame', n // 3 - 1), ('the best hidden row', int(change.argmin()))):
        wrong = ref + d3[p][:, None] * (h2[p + 1] - h2[p])[None, :]
        worst[tag] = R.element_ratio(wrong, ref, budget)
        print(f'row {p} of hin[1] ({tag}) replaced by row {p + 1}: gW3 {worst[tag]:.3g} budgets per element; the max norm sees '
              f'{R.relmax(wrong, ref):.3g} against {old:.3g}')
        bad = hin[1].clone()
        bad[p] = hin[1][p + 1]
        assert R.element_ratio(bad, *stages['hin1'][1:]) > 1             # and if the stored row itself were wrong: the hin stage
    assert all(v > 1 for v in worst.values()), worst


def test_a_sine_reduced_with_one_fp32_two_pi_is_outside_the_hin_budget():
    plan = R.Plan(171)
    u = R.synthetic_phases(plan.npad)[0, :171]
    two_pi = torch.tensor(2 * math.pi, dtype=torch.float32)
    reduced = u - torch.round(u / two_pi) * two_pi                         # fp32 throughout, one constant
    bad = torch.sin(reduced.to(F64))
    ref = torch.sin(u.to(F64))
    d_sin, _ = R.trig_delta(u)
    budget = R.MULT * d_sin
    ratio = R.element_ratio(bad.float(), ref, budget)
    err = (bad - ref).abs()
    first = float(u.abs()[err > budget].min())
    print(f'a sine with a single fp32 2 pi: {ratio:.3g} budgets of hin at |phase| <= {R.PHASE_RANGE:.0f} (d_sin = {d_sin / R.U:.3g} u); first outside '
          f'the budget at |phase| = {first:.4g} rad; at |phase| <= 40 rad: {float(err[u.abs() <= 40].max()) / budget:.3g} budgets')
    assert float(u.abs().max()) > 500 and ratio > 1
    assert R.element_ratio(torch.sin(u), ref, budget) <= 1
