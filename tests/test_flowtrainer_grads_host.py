"""CPU: the conditions tests/test_gpu_flowtrainer_grads.py rests on, established from the reference alone (tests/flowtrainer_refs.py,
no kernel runs), for every case that file uses:

  a. the float32 and the float64 evaluation of `step_masks_ref` threshold the same pixels: no input sits on a threshold;
  b. the fp32-torch unit of every (term, flow), max |g32 - g64| / max |g64| on the float64 masks, is finite, above 0 and at most 1e-3:
     the GPU budget of MULT = 4 units is then a statement about the gradient, not about noise;
  c. power: cutting `metric -> splat` or the splatted normaliser out of the float64 graph, or exchanging dflow12 and dflow21, moves the
     gradient of the summed loss by more than 4 units in the same norm, for each flow.  margin = change / (4 units), asserted > 1;
  d. the 'band' case: at least 5 % of softmax1 is exactly 0 in float64, and the gradient of the three photometric terms is exactly 0
     at source pixels whose four splat taps fall outside the frame.

The flows of the training_step and pair-fit cases come from the networks themselves, evaluated here with torch's own ops on the CPU
(tools/fit_flow.composed_flow_fields): the kernels' flows to fp32 rounding.

Measured (python -m pytest -s): units per case, smallest .. largest over the two flows, and the smallest power margin
  case            l1                 census             ssim               smooth             loss               margin (cut)
  wang 24x40      4.8e-06 .. 1.2e-05 9.3e-05 .. 1.3e-04 1.7e-05 .. 2.5e-05 9.4e-08 .. 1.4e-07 1.4e-05 .. 3.2e-05 2.1e+03 (metric)
  wang 13x37      7.9e-06 .. 3.2e-05 3.4e-05 .. 9.5e-05 7.5e-05 .. 3.6e-04 5.5e-08 .. 1.6e-07 1.2e-05 .. 3.0e-05 1.3e+03 (metric)
  brox 24x40      1.4e-05 .. 2.0e-05 3.6e-05 .. 9.3e-05 2.6e-05 .. 3.6e-05 9.4e-08 .. 1.4e-07 1.8e-05 .. 3.3e-05 5.2e+03 (metric)
  none 24x40      1.2e-05 .. 1.4e-05 9.3e-05 .. 1.3e-04 2.6e-05 .. 4.2e-05 9.4e-08 .. 1.4e-07 1.4e-05 .. 3.2e-05 2.8e+03 (metric)
  nossim 24x40    4.8e-06 .. 1.2e-05 9.3e-05 .. 1.3e-04 -                  9.4e-08 .. 1.4e-07 1.5e-05 .. 3.3e-05 2.1e+03 (metric)
  wang 1x37x70    2.0e-05 .. 1.8e-04 6.6e-05 .. 1.8e-04 3.0e-05 .. 3.9e-05 1.4e-07 .. 1.5e-07 3.1e-05 .. 1.9e-04 3.6e+02 (metric)
  band 24x40      1.2e-05 .. 1.5e-04 4.8e-05 .. 9.3e-05 2.5e-05 .. 7.4e-05 9.4e-08 .. 1.4e-07 1.4e-05 .. 1.4e-04 5.1e+02 (metric)
  step RBF        1.4e-05 .. 3.9e-05 8.1e-05 .. 9.5e-05 4.2e-05 .. 8.6e-05 1.3e-07 .. 1.5e-07 6.7e-05 .. 6.9e-05 1.4e+03 (metric)
  step PRBF       1.3e-05 .. 2.1e-05 9.6e-05 .. 1.5e-04 2.8e-05 .. 2.8e-04 6.1e-08 .. 1.9e-07 7.9e-05 .. 8.4e-05 1.1e+03 (metric)
  step siren      2.9e-06 .. 1.8e-05 6.8e-05 .. 6.8e-05 2.0e-05 .. 5.0e-05 9.4e-08 .. 1.1e-07 9.4e-06 .. 2.0e-05 5.4e+03 (metric)
  step MPFF       5.8e-06 .. 6.7e-05 6.5e-05 .. 1.6e-04 2.8e-05 .. 7.7e-05 1.6e-07 .. 2.1e-07 2.6e-05 .. 1.3e-04 5.0e+02 (metric)
  pair PRBF       8.8e-06 .. 1.2e-04 7.5e-05 .. 2.2e-04 -                  2.3e-07 .. 2.7e-07 7.5e-05 .. 1.5e-04 9.4e+02 (metric)
The weakest of the three mistakes is always the cut metric; the cut normaliser is at 1.2e+04 .. 8.6e+05, the exchange at 1.2e+03 .. 1.4e+05.
The masks are open on 44 % (brox), 70 % (band, mask1) and 88 .. 100 % of the values; 27 % of the band case's softmax1 is exactly 0.
"""
import os
import sys

import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import flowtrainer_refs as R  # noqa: E402

F64 = torch.float64
UNIT_CAP, POWER = 1e-3, 4.0
CASES = list(R.GRAD_CASES) + [f'step {name}' for name in R.STEP_NETS] + [f'pair {R.PAIR_NET}']
_inputs = {}


def inputs(case):
    """(frame1, frame2, flow12, flow21, args) of a case, made once"""
    if case not in _inputs:
        if case in R.GRAD_CASES:
            _inputs[case] = R.grad_case(case)
        elif case.startswith('step '):
            frame1, frame2, times, scale, _ = R.step_batch()
            flows = R.composed_flows(R.step_net(case[5:]), times, 24, 40, float(scale[0]))
            _inputs[case] = (frame1, frame2, *flows, R.grad_args())
        else:
            pair_flow = R.pair_flow_module()
            frame1, frame2, scale = R.pair_inputs()
            flows = R.composed_flows(pair_flow.build_net(case[5:], 1000, 'cpu'), None, 24, 40, scale)
            _inputs[case] = (frame1, frame2, *flows, R.grad_args(loss_ssim=0, occl_thresh=pair_flow.OCCL_THRESH))
    return _inputs[case]


_refs = {}


def refs(case):
    """(float64 masks, float32 masks, softmax1 in float64, float64 gradients, float32 gradients on the float64 masks), computed once and
    left unchanged"""
    if case not in _refs:
        frame1, frame2, flow12, flow21, args = inputs(case)
        wide = [t.to(F64) for t in (frame1, frame2, flow12, flow21)]
        m64 = R.step_masks_ref(*wide, args.occl, args.occl_thresh)
        m32 = R.step_masks_ref(frame1, frame2, flow12, flow21, args.occl, args.occl_thresh)
        g64 = R.step_grads_ref(frame1, frame2, flow12, flow21, args, m64[:2], F64)
        g32 = R.step_grads_ref(frame1, frame2, flow12, flow21, args, m64[:2], torch.float32)
        _refs[case] = (m64[:2], m32[:2], m64[2], g64, g32)
    return _refs[case]


@pytest.mark.parametrize('case', CASES)
def test_masks_agree_between_the_dtypes(case):
    m64, m32, _, _, _ = refs(case)
    for i, (a, b) in enumerate(zip(m64, m32)):
        print(f'{case} mask{i + 1}: open {float(a.to(F64).mean()):.3f}')
        assert a.shape == b.shape and torch.equal(a.to(F64), b.to(F64)), f'{case}: an input of mask{i + 1} sits on a threshold: change the seed'
        assert 0.3 < float(a.to(F64).mean()), 'a mask that is nearly shut tests nothing'


@pytest.mark.parametrize('case', CASES)
def test_units_are_small(case):
    *_, args = inputs(case)
    _, _, _, g64, g32 = refs(case)
    assert set(g64) == {t for t in R.GRAD_TERMS if t != 'ssim' or args.loss_ssim != 0}
    units = R.grad_units(g32, g64)
    for (term, flow), unit in units.items():
        i = ('flow12', 'flow21').index(flow)
        print(f'unit({case} {term} d{flow}) = {unit:.3g}   [max |g64| {float(g64[term][i].abs().max()):.3g}]')
    for key, unit in units.items():
        assert 0 < unit <= UNIT_CAP, (case, key, unit)                 # NaN and inf fail both comparisons


@pytest.mark.parametrize('case', CASES)
def test_power_of_the_budget(case):
    """the three mistakes the issue names, made in the float64 reference: each moves d loss / d flow by more than POWER units"""
    frame1, frame2, flow12, flow21, args = inputs(case)
    m64, _, _, g64, g32 = refs(case)
    units = R.grad_units(g32, g64)
    true = g64['loss']
    wrong = {cut: R.step_grads_ref(frame1, frame2, flow12, flow21, args, m64, F64, detach=(cut,))['loss'] for cut in ('metric', 'normaliser')}
    wrong['exchanged'] = (true[1], true[0])
    failures = []
    for what, grads in wrong.items():
        for i, flow in enumerate(('flow12', 'flow21')):
            change = R.relmax(grads[i], true[i])
            margin = change / (POWER * units[('loss', flow)])
            print(f'margin({case} {what} d{flow}) = {margin:.3g}   [change {change:.3g}, unit {units[("loss", flow)]:.3g}]')
            if not margin > 1:
                failures.append((what, flow, margin))
    assert not failures, failures


def test_band_case_leaves_pixels_nothing_lands_on():
    frame1, frame2, flow12, flow21, args = inputs('band 24x40')
    m64, _, softmax1, g64, g32 = refs('band 24x40')
    empty = float((softmax1 == 0).to(F64).mean())
    outside = R.all_taps_outside(flow21)
    print(f'band: softmax1 exactly 0 on {empty:.3%} of values; {int(outside.sum())} of {outside.numel()} source pixels splat nowhere')
    assert empty >= 0.05
    assert int(outside.sum()) >= 0.05 * outside.numel()
    for i, flow in enumerate((flow12, flow21)):                        # flow12 carries a few edge pixels out of the frame as well
        where = R.all_taps_outside(flow)[:, None].expand_as(flow)
        assert bool(where.any())
        for grads in (g64, g32):
            for term in ('l1', 'census', 'ssim'):
                assert float(grads[term][i][where].abs().max()) == 0.0, term
                assert float(grads[term][i][~where].abs().max()) > 0.0, term
            assert float(grads['smooth'][i][where].abs().max()) > 0.0  # the smoothness term reads the flow itself


def test_detach_defaults_to_the_plain_reference():
    """`detach=()` is the function the other tests of the trainer use; a cut leaves the values and changes only the gradient"""
    frame1, frame2, flow12, flow21, args = inputs('wang 13x37')
    wide = [t.to(F64) for t in (frame1, frame2, flow12, flow21)]
    plain, _ = R.step_losses_ref(*wide, args)
    for cut in ('metric', 'normaliser'):
        other, _ = R.step_losses_ref(*wide, args, detach=(cut,))
        for term in R.GRAD_TERMS:
            assert abs(float(plain[term]) - float(other[term])) <= 1e-15 * abs(float(plain[term])), (cut, term)
