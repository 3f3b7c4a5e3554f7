"""CPU: the stage checks of the frame synthesis (tests/flowsynth_stage_refs.py) held against a numpy fp32 model of the
kernels.  Shown here, with no device: the derived budgets are wide enough for a correct kernel under every order of summation and
with the contractible steps fused or not (the worst ratio per stage is printed); each seeded defect leaves the budget of a named
stage on a named case; the cases have the properties they were built for.
"""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import flowsynth_stage_refs as S  # noqa: E402

_WORST = {}


@pytest.mark.parametrize('name', list(S.CASES))
def test_model_passes_every_stage(name):
    case = S.case(name)
    zero = S.case(name, zero_frames=True) if name in S.EXACT_FLOWS else None
    for contract in (False, True):
        for order in S.ORDERS:
            acc, out, u8 = S.model(case, contract, order)
            assert np.isfinite(acc).all() and np.isfinite(out).all()
            r1, wrong = S.stage1(case, acc)
            r2 = S.stage2(case, acc)
            bits, bytes_ = S.stage3(case, acc, out, u8)
            print(f'model {name} contract={contract} {order}: stage 1 {r1:.3f}  stage 2 {r2:.3f}  stage 3 {bits} bits {bytes_} bytes')
            assert r1 <= 1 and wrong == 0 and r2 <= 1 and bits == 0 and bytes_ == 0, (name, contract, order, r1, wrong, r2, bits, bytes_)
            _WORST[1], _WORST[2] = max(_WORST.get(1, 0), r1), max(_WORST.get(2, 0), r2)
            if zero is not None:
                assert S.exact_check(zero, S.model(zero, contract, order)[0]) == 0, (name, contract, order)
    print(f'worst so far: stage 1 {_WORST[1]:.3f}  stage 2 {_WORST[2]:.3f}')


def _negative_zero_accumulator(case, acc):
    """the accumulator of a call with the empty N elements of side 0 turned into -0.0: the kernel cannot produce one (every term is
    w * tap >= 0 and a zero term is not added), so the blend's rule for it is only reachable from a made-up accumulator"""
    acc = acc.copy()
    c = case[0].shape[1]
    n0 = acc[:, :, 0, c]
    assert (n0 == 0).any()
    n0[n0 == 0] = np.float32(-0.0)
    return acc


# defect -> (stage that catches it, case); every entry of S.DEFECTS is here or in NOT_SEPARABLE
CAUGHT_BY = {
    'south hand-over dropped': ('stage 2', 'shift'),
    'east give across lanes 31-32': ('exact', 'random'),
    'give_h without nwy': ('stage 2', 'shear'),
    'merged value one element off': ('stage 2', 'shift'),
    'dead neighbour takes': ('stage 2', 'non-finite'),
    'side 1 uses tau': ('stage 2', '9x33'),
    't * F fused into the add': ('stage 2', '9x33'),
    'tiles past the cap skipped': ('stage 1', 'past cap'),
    'plane stride C': ('stage 1', '9x33'),
    'metric summed over channels': ('stage 1', '9x33'),
    'negative zero not a hole': ('stage 3', 'fold'),            # on a made-up accumulator only (see above)
    'fallback tau for both': ('stage 3', 'fold'),
}
# The tests on (lane & 31) of give_h / take_h guard nothing the coordinate comparisons do not: with both removed a value handed from
# lane 31 to lane 32 still lands on the address it was computed for.  The variant with only the giver's test removed loses the value
# and is in CAUGHT_BY.
NOT_SEPARABLE = ('east hand-over across lanes 31-32',)


def _failures(case, acc, out, u8):
    r1, wrong = S.stage1(case, acc)
    bits, bytes_ = S.stage3(case, acc, out, u8)
    return {'stage 1': r1 > 1 or wrong > 0, 'stage 2': S.stage2(case, acc) > 1, 'stage 3': bits > 0 or bytes_ > 0}


@pytest.mark.parametrize('defect', S.DEFECTS)
def test_seeded_defect_is_caught(defect):
    assert (defect in CAUGHT_BY) != (defect in NOT_SEPARABLE)
    if defect in NOT_SEPARABLE:
        stats = {}
        S.model(S.case('random'), False, 'merged', stats=stats)
        assert stats['seam_31_32'] > 0                          # the hand-over it would allow does occur
        for name in S.CASES:
            if name == 'past cap':
                continue
            case = S.case(name)
            assert not any(_failures(case, *S.model(case, False, 'merged', defect=defect)).values()), name
            if name in S.EXACT_FLOWS:
                zero = S.case(name, zero_frames=True)
                assert S.exact_check(zero, S.model(zero, False, 'merged', defect=defect)[0]) == 0, name
        return
    stage, name = CAUGHT_BY[defect]
    case = S.case(name)
    if stage == 'exact':
        zero = S.case(name, zero_frames=True)
        assert S.exact_check(zero, S.model(zero, False, 'merged')[0]) == 0
        differing = S.exact_check(zero, S.model(zero, False, 'merged', defect=defect)[0])
        print(f'{defect}: {differing} elements differ in the exact case on {name}')
        assert differing > 0
        return
    if defect == 'negative zero not a hole':
        acc = _negative_zero_accumulator(case, S.model(case, False, 'merged')[0])
        good, bad = S.blend32(case, acc), S.blend32(case, acc, defect)
        assert S.stage3(case, acc, *good) == (0, 0)
        bits, _ = S.stage3(case, acc, *bad)
        print(f'{defect}: {bits} outputs differ on the made-up accumulator of {name}')
        assert bits > 0
        assert not any(_failures(case, *S.model(case, False, 'merged', defect=defect)).values())     # unreachable from a call
        return
    for contract in (False, True):                  # in the kernel's own order: the hand-overs exist in no other
        assert not any(_failures(case, *S.model(case, contract, 'merged')).values())
        failed = _failures(case, *S.model(case, contract, 'merged', defect=defect))
        print(f'{defect} on {name}, contract={contract}: fails {[s for s, f in failed.items() if f]}')
        assert failed[stage], (defect, stage, name, contract)


def test_case_table():
    cap, tx, ty = S.R.scatter_block_cap()
    assert (tx, ty) == (32, 8)
    for name, (seed, b, c, h, w, taus, flows) in S.CASES.items():
        t = S.tau32(taus)
        assert 0.0 in t and 1.0 in t and len(t) <= 64 and bool(((t >= 0) & (t <= 1)).all()), name
        i0, i1, f01, f10, _ = S.case(name)
        assert i0.shape == i1.shape == (b, c, h, w) and f01.shape == f10.shape == (b, 2, h, w)
        assert float(min(i0.min(), i1.min())) >= 0.05 and float(max(i0.max(), i1.max())) <= 0.95
    assert S.tile_counts(2, 9, 33)[:3] == (2, 2, 16)                      # two ragged tiles each way
    assert S.tile_counts(1, 1, 40)[:3] == (2, 1, 4) and S.tile_counts(1, 12, 1)[:3] == (1, 2, 4) and S.tile_counts(1, 1, 1)[2] == 2
    _, b, _, h, w, taus, _ = S.CASES['past cap']
    assert S.tile_counts(b, h, w)[2] == 2056 > cap == 2048 and S.tile_counts(b - 1, h, w)[2] <= cap
    assert len(S.CASES['K=64'][5]) == 64 == S.tau32(S.CASES['K=64'][5]).size
    # times whose 1 - tau rounds in fp32: some of those below 1/2 (from 1/2 on the difference is exact, 0.7 included)
    assert 0.7 in S.CASES['9x33'][5]
    for tau in (0.1,):
        assert tau in S.CASES['9x33'][5]
        t = np.float32(tau)
        assert float(np.float32(1) - t) != 1.0 - float(t)
    assert sum(float(np.float32(1) - t) != 1.0 - float(t) for t in S.tau32(S.CASES['K=64'][5])) > 20
    props = {}
    for name in S.CASES:
        if name == 'past cap':
            continue
        case = S.case(name)
        stats = {}
        acc = S.model(case, False, 'merged', stats=stats)[0]
        c = case[0].shape[1]
        _, _, n = S.stage2_reference(case, S.own_w(case, acc))
        inner = [k for k, t in enumerate(S.tau32(case[4])) if 0 < t < 1 and t != 0.5]
        empty = n[:, inner][:, :, :, c] == 0
        stats['holes'] = int(empty.sum())
        stats['both empty'] = int((empty[:, :, 0] & empty[:, :, 1]).sum())
        stats['most sources'] = int(n[:, :, :, c].max())
        props[name] = stats
        print(name, stats)
    assert props['9x33']['give_h'] > 0 and props['9x33']['give_v'] > 0 and props['9x33']['refused_h_by_row'] > 0
    assert props['9x33']['holes'] > 0 and props['9x33']['most sources'] > 3
    assert props['1x40']['give_h'] > 0 and props['12x1']['give_v'] > 0
    hw_k = 9 * 33 * len(S.QUARTER_TAUS) * 2
    assert props['shift']['give_h'] > 0.9 * hw_k * 31 / 33 and props['shift']['refused_h_by_row'] == 0       # every lane merges
    assert 0 < props['random']['give_h'] < 0.3 * hw_k and props['random']['refused_h_by_row'] > 0 and props['random']['seam_31_32'] > 0
    assert props['fold']['most sources'] >= 33 and props['fold']['both empty'] > 0
    assert props['shear']['refused_h_by_row'] > 0 and props['shear']['give_h'] > 0
    assert props['out of frame']['split_validity'] > 0 and props['out of frame']['holes'] > 0
    assert props['non-finite']['give_h'] > 0 and props['non-finite']['holes'] > 0
    # each of the four sides loses sources in the out-of-frame case, with taps of one source on both sides of the border
    i0, i1, f01, f10, taus = S.case('out of frame')
    for sample, (axis, border) in enumerate(((1, -1), (1, 8), (0, -1), (0, 32))):            # nwy or nwx of a straddling source
        straddles = 0
        for t in (0.25, 0.5, 0.75):
            ox, oy = S.landing32(np.float32(t), f01[sample, 0], f01[sample, 1])
            ok, nwx, nwy, wts, val = S.taps32(ox, oy, 9, 33)
            straddles += int((((nwx, nwy)[axis] == border) & (val[0] != val[3])).sum())
        assert straddles > 0, sample
        ox, oy = S.landing32(np.float32(1), f01[sample, 0], f01[sample, 1])
        assert bool((~np.any(S.taps32(ox, oy, 9, 33)[4], axis=0)).any()), sample         # a source with no valid tap at all
    # the non-finite case: every kind, and the two sources set up beside a lane without taps
    _, _, f01, f10, _ = S.case('non-finite')
    both = np.concatenate([f01.ravel(), f10.ravel()])
    assert np.isnan(both).any() and (both == np.inf).any() and (both == -np.inf).any() and (both == 3e9).any() and (both == -3e9).any()
    ox, oy = S.landing32(np.float32(0.5), f01[0, 0], f01[0, 1])
    ok, nwx, nwy, _, _ = S.taps32(ox, oy, 9, 33)
    assert ok[3, 10] and not ok[3, 11] and (nwx[3, 10], nwy[3, 10]) == (-1, 0)
    assert ok[4, 20] and not ok[5, 20] and (nwx[4, 20], nwy[4, 20]) == (0, -1)


def test_exact_case_sums_are_exact_in_fp32():
    """zero frames, w = 1: every N sum of the exact case is a multiple of 1/256 below 2^16, whatever the order -- all three orders
    of the model give the float64 sums bit for bit"""
    for name in S.EXACT_FLOWS:
        zero = S.case(name, zero_frames=True)
        assert all(float(t) * 4 == int(float(t) * 4) for t in zero[4])
        for f in zero[2:4]:
            fin = f[np.isfinite(f) & (np.abs(f) < 1e9)]
            assert bool((fin * 4 == np.rint(fin * 4)).all())
        for order in S.ORDERS:
            assert S.exact_check(zero, S.model(zero, True, order)[0]) == 0, (name, order)
