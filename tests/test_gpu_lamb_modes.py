"""GPU: FusedLAMB (csrc/lamb.hip) away from its default path -- every switch of sininn_lamb_args, bias correction far from step 1,
the clip boundary, more chunks than blocks, param groups with their own hyper-parameters and a hostile chunk table.

The method is that of tests/test_gpu_lamb.py and its helpers are imported from there: the reference is `lamb_step_ref` in float64 on
the optimiser's own fp32 state copied before each step, the unit of error the same restatement in fp32, the budget
max(MULT * unit, FLOOR), and every comparison prints its `ratio(...)` line.  No other tolerance is introduced.

A mode is only tested where it shows: `flag_margin` evaluates the float64 reference once more with the flipped switches back at their
defaults, on the same state, and the test asserts that its p differs from the true reference's p by at least MARGIN = 10 budgets of
that step's p comparison.  That is a condition on the inputs (it never looks at the kernel's output).  Two things follow from the
formulas and shape the inputs: m and v start from a seeded state, because from m = v = 0 the first update is sign(g) up to eps whatever
the clip factor is; and the gradient scale changes from step to step, because a clip that divides every step by the same G cancels in
m / sqrt(v).

Measured on an MI355X (run with -s; worst ratio(...) = error / budget per quantity over the steps of a test, against float64):
  test                     p      m      v      trust ratios
  modes l2                 0.25   0.25   0.25   0.449
  modes no_grad_averaging  0.25   0.25   0.25   0.25
  modes no_bias_correction 0.25   0.25   0.25   0.25
  modes nvlamb_nowd        0.25   0.25   0.25   0.263
  modes no_clip            0.25   0.25   0.25   0.25
  modes all                0.25   0.25   0.25   0.25
  step 5000                0.25   0.25   0.25   0.203
  clip boundary            0.25   0.25   0.25   0.25
  more chunks than blocks  0.25   0.25   0.437  0.068
  own hyper-parameters     0.25   0.25   0.25   0.783
  hostile chunk table      0.25   0.25   0.25   0.004
A ratio of 0.25 is the kernel's error equal to the unit: it evaluates the update with the restatement's own fp32 operations.  The
"flag matters" margins (reference difference / budget of that step's p comparison, required >= 10), steps 1, 2, 3: l2 39200, 10100,
4380; no_grad_averaging 21900, 9950, 10900; no_bias_correction 3870, 3710, 4790; nvlamb_nowd 14700, 11200, 18200; no_clip 30400,
14500, 2150; all 24800, 13600, 16600; step 5000, on the trust ratios: 10700.  11 tests in 3 s, of which more chunks than blocks
(8.4 M elements, two steps with both references) takes 0.14 s.
The tests bite: with the `!h.adam_w_mode` branch of lamb_stage1_kernel dropped, modes l2 and modes all fail at step 1 (p off by
7.7e-3 and 3.4e-3 of max |p| against budgets of 2e-7); with `up2 = 0.0; uu2 = 0.0;` moved out of the chunk loop, more chunks than blocks
fails at step 1 (p off by 1.7e-4 against 1.7e-7).  tests/test_gpu_lamb.py passes on both of these builds.
"""
import os
import sys

import pytest
import torch

pytestmark = pytest.mark.gpu
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from lamb_refs import lamb_step_ref  # noqa: E402
from test_gpu_lamb import (FLOOR, MULT, F64, bits, check, dev, hyper_of, make_params, offsets_of, padding_mask,  # noqa: E402,F401
                           relmax, set_grads, step_and_compare)

MARGIN = 10.0
SWITCH_DEFAULTS = dict(adam_w_mode=True, grad_averaging=True, bias_correction=True, use_nvlamb=False, max_grad_norm=1.0)


def fill_state(opt, gi, seed, m_scale=5e-3, v_scale=5e-5):
    """seeded m (normal * m_scale) and v (uniform * v_scale, so v >= 0) inside the tensors of group gi; the padding stays +0"""
    fl = opt._flat[gi]
    gen = torch.Generator().manual_seed(seed)
    m, v = torch.zeros(fl['m'].numel()), torch.zeros(fl['v'].numel())
    for o, k in offsets_of(opt, gi):
        m[o:o + k] = torch.randn(k, generator=gen) * m_scale
        v[o:o + k] = torch.rand(k, generator=gen) * v_scale
    fl['m'].copy_(m)
    fl['v'].copy_(v)


def flag_margin(opt, before, r64, r32, step, back_to_default):
    """(p of the float64 reference with `back_to_default` applied - p of the true float64 reference) / budget of the p comparison"""
    budget = max(MULT * relmax(r32['p'], r64['p']), FLOOR)
    base = lamb_step_ref(*(before[k] for k in 'pgmv'), offsets_of(opt), dict(hyper_of(opt), **back_to_default), step, 1.0, F64)
    return relmax(base['p'], r64['p']) / budget


# per case: the constructor's arguments and the gradient scale of steps 1, 2, 3 (normal gradients over 16 722 elements: G is about
# 129 times the scale, so every step clips at max_grad_norm = 1 where the clip is enabled)
MODES = {'l2': (dict(adam_w_mode=False, weight_decay=0.1), (0.03, 0.06, 0.02)),
         'no_grad_averaging': (dict(grad_averaging=False), (0.05, 0.1, 0.03)),
         'no_bias_correction': (dict(bias_correction=False), (0.05, 0.1, 0.03)),
         'nvlamb_nowd': (dict(use_nvlamb=True, weight_decay=0.0), (0.05, 0.1, 0.03)),
         'no_clip': (dict(max_grad_norm=0.0), (0.05, 0.2, 0.04)),
         'all': (dict(adam_w_mode=False, grad_averaging=False, bias_correction=False, use_nvlamb=True), (0.05, 0.1, 0.03))}


@pytest.mark.parametrize('case', list(MODES))
def test_modes(dev, case):
    from sin_inn_amd import FusedLAMB
    from sin_inn_amd.optim import LAMB_CHUNK as C
    kw, scales = MODES[case]
    sizes = [1, 5, 257, C - 1, C + 1, 2 * C + 7, 64]
    zero_p = len(sizes) - 1
    lr = 1e-3
    opt = FusedLAMB(make_params(sizes, dev, 11, zero=(zero_p,)), lr=lr, **kw)
    twin = FusedLAMB(make_params(sizes, dev, 11, zero=(zero_p,)), lr=lr, max_grad_norm=1e30) if case == 'no_clip' else None
    opts = [opt] + ([twin] if twin is not None else [])
    fl = opt._flat[0]
    fl['step'] = 0                                               # the compared steps are 1, 2, 3: bc1 = 0.1 at the first
    for o in opts:
        fill_state(o, 0, 12)
    back = {k: SWITCH_DEFAULTS[k] for k in kw if k != 'weight_decay'}
    lr32 = torch.tensor(lr, dtype=torch.float32, device=dev)
    zo, zk = offsets_of(opt)[zero_p]
    for step, scale in enumerate(scales, 1):
        for o in opts:
            set_grads(o, 0, 800 + step, scale)
            o._flat[0]['p'][zo:zo + zk].zero_()                  # the all-zero tensor is an input of every step
        (r64, r32, ratios, before), = step_and_compare(f'{case} step {step}', opt)
        assert fl['step'] == step
        margin = flag_margin(opt, before, r64, r32, step, back)
        print(f'margin({case} step {step}) = {margin:.3g} budgets between the reference and the reference with {sorted(back)} at default')
        assert margin >= MARGIN, (case, step, margin)
        if case == 'nvlamb_nowd':
            assert torch.equal(ratios[zero_p], lr32), 'zero parameters: the ratio is lr itself'
            assert bool((ratios[:zero_p] != lr32).all()), 'use_nvlamb: every tensor with parameters adapts its ratio without wd'
        if case == 'no_clip':
            assert float(r64['G']) >= 4.0
            twin.step()                                          # G < 1e30: no clip either
            assert torch.equal(bits(fl['m']), bits(twin._flat[0]['m'])), 'max_grad_norm = 0 and 1e30 both take clip = 1'


def test_bias_correction_at_step_5000(dev):
    """bc1 = 1 to fp32, bc2 = 1 - 0.999^5000 = 0.99328: the kernel sees step 5000 after one launch"""
    from sin_inn_amd import FusedLAMB
    from sin_inn_amd.optim import LAMB_CHUNK as C
    opt = FusedLAMB(make_params([5, 257, C + 1], dev, 21), lr=1e-3)
    fl = opt._flat[0]
    fill_state(opt, 0, 22)
    fl['step'] = 4999
    set_grads(opt, 0, 23, 0.05)
    (r64, r32, _, before), = step_and_compare('step-5000', opt)
    assert fl['step'] == 5000
    # the inputs show bc2: the float64 ratios without bias correction lie more than MARGIN budgets away
    budget = max(MULT * relmax(r32['ratios'], r64['ratios']), FLOOR)
    flat = lamb_step_ref(*(before[k] for k in 'pgmv'), offsets_of(opt), dict(hyper_of(opt), bias_correction=False), 5000, 1.0, F64)
    margin = relmax(flat['ratios'], r64['ratios']) / budget
    print(f'margin(step-5000 ratios) = {margin:.3g} budgets between bc2 = 0.99328 and bc2 = 1')
    assert margin >= MARGIN


def test_clip_boundary(dev):
    """G == max_grad_norm exactly does not clip (the comparison is strict); one ulp more on one element and a second element do"""
    from sin_inn_amd import FusedLAMB
    sizes = [4, 8]
    opt, twin = (FusedLAMB(make_params(sizes, dev, 31), lr=1e-3, max_grad_norm=mgn) for mgn in (1.0, 0.0))
    fl, tw = opt._flat[0], twin._flat[0]
    (o0, _), (o1, _) = offsets_of(opt)
    g = torch.zeros(fl['g'].numel())
    g[o1 + 5] = 1.0
    for f in (fl, tw):
        f['g'].copy_(g)
    (r64, _, _, _), = step_and_compare('clip-boundary G=1', opt)
    assert float(r64['G']) == 1.0
    twin.step()
    for k in 'pmv':
        assert torch.equal(bits(fl[k]), bits(tw[k])), f'G == max_grad_norm must not clip: {k} differs from the unclipped twin'
    g[o1 + 5] = torch.nextafter(torch.tensor(1.0), torch.tensor(2.0))
    g[o0 + 3] = 1.0
    fl['g'].copy_(g)
    (r64, _, _, _), = step_and_compare('clip-boundary G=sqrt2', opt)
    assert float(r64['G']) > 1.0 and abs(float(r64['G']) - 2.0 ** 0.5) < 1e-6


def test_more_chunks_than_blocks(dev):
    """2055 chunks against the 2048-block cap of csrc/lamb.hip: blocks 0..6 take a second chunk, and those seven span the end of
    tensor 0, all of tensor 1 and tensor 2, so a block's second trip reuses its shared memory, starts its partial sums again and
    applies another tensor's ratio.  8.4 M elements: the smallest size that reaches the loop through FusedLAMB's own layout."""
    from sin_inn_amd import FusedLAMB
    from sin_inn_amd.optim import LAMB_CHUNK as C
    opt = FusedLAMB(make_params([2050 * C + 3, 2 * C + 1, 5], dev, 41), lr=1e-3)
    fl = opt._flat[0]
    assert fl['chunks'].shape[0] == 2055
    fl['ws'].fill_(float('nan'))
    fl['u'].fill_(float('nan'))
    for step in range(1, 3):
        set_grads(opt, 0, 900 + step, 0.01)
        (r64, _, ratios, _), = step_and_compare(f'chunk-loop step {step}', opt)
        assert float(r64['G']) > 1.0
        assert bool((ratios != torch.tensor(1e-3, dtype=torch.float32, device=dev)).all())      # weight_decay 0.01: the ratios are live


def test_param_groups_with_their_own_hyper_parameters(dev):
    from sin_inn_amd import FusedLAMB
    from sin_inn_amd.optim import LAMB_CHUNK as C
    a, b = make_params([C + 5, 7], dev, 51), make_params([300, 33], dev, 52)
    opt = FusedLAMB([dict(params=a),
                     dict(params=b, lr=3e-3, betas=(0.8, 0.99), eps=1e-5, bias_correction=False, grad_averaging=False, max_grad_norm=8.0)],
                    lr=1e-3)
    for gi in (0, 1):
        fill_state(opt, gi, 53 + gi)
    for step in range(1, 3):
        set_grads(opt, 0, 1000 + step, 0.03)
        set_grads(opt, 1, 1100 + step, 0.1)
        (r0, _, _, _), (r1, _, _, _) = step_and_compare(f'own-hypers step {step}', opt)
        G = float(r0['G'])
        assert float(r1['G']) == G
        assert 1.0 < G < 8.0, G                                  # group 0 clips at the shared norm, group 1 does not


def test_hostile_chunk_table_stays_inside_the_buffers(dev):
    """The valid layout with bad entries inserted (the table stays sorted by tensor): every kernel skips them, so the step is the
    clean layout's step.  A processed bad chunk would apply the update twice or to the wrong tensor.  Every bad entry lies inside
    the allocated flat buffers (asserted before the launch), so even a broken chunk_ok writes only into this test's own memory."""
    from sin_inn_amd import FusedLAMB, ops
    from sin_inn_amd.optim import LAMB_CHUNK as C
    sizes = [C + 5, 300, 7]
    opt = FusedLAMB(make_params(sizes, dev, 61), lr=1e-3)
    fl = opt._flat[0]
    fill_state(opt, 0, 62)
    set_grads(opt, 0, 63, 0.05)
    nt, npad, k0 = len(sizes), fl['p'].numel(), sizes[0]
    off0 = fl['offsets'][0]
    good = [tuple(c) for c in fl['chunks'].cpu().tolist()]
    bad = {-1: [(-1, 0, 4)],
           0: [(0, off0, k0 + 8),                                # runs past its tensor
               (0, off0 + 2, 4),                                 # begin not a multiple of 4
               (0, off0, 0)],                                    # empty
           1: [(1, off0, 4)],                                    # begin below its tensor
           nt: [(nt, 0, 4)]}
    table = list(bad[-1])
    for t in range(nt):
        mine = [c for c in good if c[0] == t]
        table += mine[:1] + bad.get(t, []) + mine[1:]
    table += bad[nt]
    assert [c[0] for c in table] == sorted(c[0] for c in table) and len(table) == len(good) + 6
    assert [c for c in table if c in good] == good
    for t, b, n in table:
        assert 0 <= b and b + n <= npad, 'every entry, bad ones included, lies inside the flat buffers'
    hostile = torch.tensor(table, dtype=torch.int64).to(dev)
    nbytes = ops.lamb_workspace_bytes(len(table), nt)
    ws = torch.full((nbytes // 4,), float('nan'), device=dev, dtype=torch.float32)
    fl['u'].fill_(float('nan'))
    fl['chunks'], fl['ws'] = hostile, ws                         # kept alive by the optimiser's own table
    a = fl['args']
    a.chunks, a.n_chunks, a.workspace, a.workspace_bytes = hostile.data_ptr(), len(table), ws.data_ptr(), nbytes
    # step() raises unless sininn_lamb_grad_norm and sininn_lamb_step both return 0; step_and_compare checks p, m, v and the ratios
    # against the clean layout's references, the padding +0 bitwise and g unchanged bitwise
    step_and_compare('hostile-table', opt)
