"""CPU: the stage checks of the error stash (tests/flowstash_stage_refs.py) held against a numpy fp32 model of the three
kernels.  Shown here, with no device: a correct kernel passes every stage on every case, in the documented order of summation and with
every lane's and wave's order reversed (stages 1 and 2 whatever the order, stages 0 and 3 against the restatement in the same order);
each seeded defect fails a named stage on a named case, or is accounted for; the cases have the properties they are named for.
"""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import flowstash_stage_refs as T  # noqa: E402

_WORST = {}


@pytest.mark.parametrize('name', list(T.CASES))
def test_model_passes_every_stage(name):
    case = T.case(name)
    for order in T.ORDERS:
        e, ws, buf, cnt, acc, prod = T.model(case, order)
        r = T.stages(case, e, ws, buf, cnt, order)
        print(f'model {name} {order}: {T.describe(r)}')
        assert not any(T.failures(r).values()), (name, order, T.failures(r))
        for key in ('stage1', 'R2', 'Cy', 'Cx'):
            _WORST[key] = max(_WORST.get(key, 0), r[key][0])
        if 'fractional' not in case['flags']:
            T.end_to_end(case, acc, prod, what=f'model {name} {order}')
    print(f'worst so far: {_WORST}')


def test_the_orders_differ():
    """the reversed model is another order of summation: its R1 differs in bits from the documented one where a slot has many terms"""
    case = T.case('x_const')
    a, b = (T.split(case, T.model(case, order)[1])[0] for order in T.ORDERS)
    assert (a != b).any()
    case = T.case('h70_yshuffled_b5')
    a, b = (T.model(case, order) for order in T.ORDERS)
    assert (T.split(case, a[1])[1] != T.split(case, b[1])[1]).any() and (a[2] != b[2]).any()
    assert T.stages(case, *b[:4], 'documented')['stage3'] != (0, 0)          # stage 3 does tell the order of b apart


# defect -> (the stage that catches it, the case, whether the end-to-end (n_terms + 12) U bound of flowstash_refs alone catches it there)
CAUGHT_BY = {
    'chunk skip tests ix <= clo': ('stage 1', 'w63_res3', True),
    'upper half compared through c & 0xffff': ('stage 1', 'w63_res3', True),
    'tile sum starts at tile 1': ('stage 2', 'w1025_res65_c1', True),
    'tile sum stops one short': ('stage 2', 'w1025_res65_c1', True),
    'second base iteration skipped': ('stage 2', 'w1025_res65_c1', True),
    'ix < res guard dropped on the R2 store': ('stage 2', 'w63_res3', True),
    '<1> divides by 3': ('stage 0', 'w64_res4_c1', True),
    'mask1 read at channel c': ('stage 0', 'w65_res5_b5', True),
    'a_y lower and upper swapped': ('stage 2', 'y_past', True),
    'Cx summed over H entries': ('stage 2', 'w63_res3', True),
    'cell decode ix fastest': ('stage 3', 'w63_res3', True),
    'clamped pixel counted once': ('stage 1', 'x_past', True),
    'log_counter is ct (cy cx)': ('stage 3', 'h70_yshuffled_b5', False),
}
NOT_SEPARABLE = ('padding taken as a cell',)


def _old_bound_catches(case, acc, prod):
    try:
        T.end_to_end(case, acc, prod)
    except AssertionError:
        return True
    return False


@pytest.mark.parametrize('defect', T.DEFECTS)
def test_seeded_defect_is_caught(defect):
    assert (defect in CAUGHT_BY) != (defect in NOT_SEPARABLE)
    if defect in NOT_SEPARABLE:
        # The padding of a ragged tile is staged with e0 = e1 = 0, so a wave that takes it for pixels of cell 0 adds exact zeros: the
        # bits of every buffer are those of the correct kernel.  What the -1 and the empty range (ES_MAX_RES, -1) buy is the skip of
        # the chunks behind the end of the row, which the defect loses -- a cost, not an error, and no check of values can see it.
        changed = 0
        for name in T.CASES:
            case = T.case(name)
            good_stats, bad_stats = {}, {}
            good, bad = T.model(case, stats=good_stats), T.model(case, defect=defect, stats=bad_stats)
            assert all(np.array_equal(g, b, equal_nan=True) for g, b in zip(good, bad)), name
            assert bad_stats['chunks_visited'] >= good_stats['chunks_visited']
            changed += bad_stats['chunks_visited'] > good_stats['chunks_visited']
        assert changed > 0                              # the seeded defect did take effect: chunks of padding were visited
        return
    stage, name, old = CAUGHT_BY[defect]
    case = T.case(name)
    good = T.model(case)
    assert not any(T.failures(T.stages(case, *good[:4])).values())
    bad = T.model(case, defect=defect)
    r = T.stages(case, *bad[:4])
    failed = T.failures(r)
    caught_old = _old_bound_catches(case, bad[4], bad[5])
    print(f'{defect} on {name}: fails {[s for s, f in failed.items() if f]}; the end-to-end bound alone: {caught_old};  {T.describe(r)}')
    assert failed[stage], (defect, stage, name)
    assert caught_old == old


def test_case_table():
    """each case has the property it is named for"""
    cases = {name: T.case(name) for name in T.CASES}
    plain = {name: c for name, c in cases.items() if not c['flags']}
    # row tiles: one ragged, one full, one pixel into the second; two full, one pixel into the third
    widths = {c['W'] for c in cases.values()}
    assert {63, 64, 65, 1023, 1024, 1025, 2048, 2049} <= widths
    assert [T.tiles(w) for w in (63, 64, 65, 1023, 1024, 1025, 2048, 2049)] == [1, 1, 1, 1, 1, 2, 2, 3]
    assert all(w - (T.tiles(w) - 1) * T.ES_TX == 1 for w in (1025, 2049)) and all(w % T.ES_TX == 0 for w in (1024, 2048))
    # the base loop of error_columns, and four waves of error_rows over fewer than, exactly and more than four x cells
    assert {3, 4, 5, 50, 64, 65, 130} <= {c['res'] for c in cases.values()}
    assert [T.base_trips(r) for r in (3, 4, 5, 50, 64, 65, 130)] == [1, 1, 1, 1, 1, 2, 3]
    assert {(c['C'], c['cm']) for c in plain.values()} == {(1, 1), (3, 1), (3, 3)}
    assert {(c['C'], c['cm']) for c in cases.values() if 'fractional' in c['flags']} == {(1, 1), (3, 1), (3, 3)}
    assert {1, 3, 4, 5, 70} <= {c['H'] for c in cases.values()} and {c['B'] for c in cases.values()} == {1, 5}
    assert all(c['H'] <= 6 for name, c in cases.items() if not name.startswith('h70'))
    for c in cases.values():
        assert T.workspace_floats(c['B'], c['H'], c['W'], c['res']) == sum(a.size for a in T.split(c, T.workspace(c))[:4])
        assert T.split(c, T.workspace(c))[4].size == T.SURPLUS
        assert all(bool((o != 0).all()) for o in c['old'])
        for m in (c['six'][2], c['six'][5]):
            assert m.shape[1] == c['cm']
            between = int(((m > 0) & (m < 1)).sum())
            assert between > 0 if 'fractional' in c['flags'] else between == 0
            assert int((m == 0).sum()) > 0
        if c['H'] > 2:
            assert bool((T.e32(c)[:, 1, 1] == 0).all())                      # the pixel masked in every channel and direction
        for d in range(3):                                                   # the model's cells are those of `axis_cells`, bit for bit
            (i0, i1), (a0, a1), _ = T.axis32(c['axes'][d], d, c['res'], c['cs'])
            (j0, j1), (b0, b1) = T.cells_of(c, d)
            assert np.array_equal(i0, j0) and np.array_equal(i1, j1) and np.array_equal(a0, b0) and np.array_equal(a1, b1)
    # unsorted times, one of them twice: two frames in the same two time cells
    t = np.array(T.SHUFFLED_TIMES, np.float32)
    assert (np.diff(t) < 0).any() and (np.diff(t) > 0).any() and t[0] == t[2]
    (i0, i1), _ = T.cells_of(cases['w65_res5_b5'], 0)
    assert (i0[0], i1[0]) == (i0[2], i1[2]) and i0[0] != i1[0]
    # every kind of axis on every axis
    for d in range(3):
        kinds = {c['kinds'][d] for c in plain.values() if c['axes'][d].size > 1}
        assert kinds == {'asc', 'desc', 'shuffled', 'const', 'past', 'edge'}, (d, kinds)
    for name, c in plain.items():
        for d, kind in enumerate(c['kinds']):
            v, res = c['axes'][d], c['res']
            (i0, i1), (a0, a1), u = T.axis32(v, d, res, c['cs'])
            if v.size == 1:
                continue
            if kind == 'asc':
                assert bool((np.diff(v) > 0).all())
            if kind == 'desc':
                assert bool((np.diff(v) < 0).all())
            if kind == 'shuffled':
                assert (np.diff(v) < 0).any() and (np.diff(v) > 0).any()
            if kind == 'const':
                assert len(set(v.tolist())) == 1 and len(set(i0.tolist())) == 1 and i0[0] != i1[0]
            if kind == 'past':                                               # both halves clamped to the same cell, at both ends
                assert ((i0 == i1) & (i0 == 0) & (u < 0)).any() and ((i0 == i1) & (i0 == res - 1) & (u > res - 1)).any(), name
                assert (i0 != i1).any()
            if kind == 'edge':                                               # u within 1e-6 below a boundary: the weights add up to 2
                near = (a0 + a1 > 1.5)
                assert int(near.sum()) == res - 2, name
                assert bool((np.ceil(u[near]) - u[near] <= 1e-6).all()) and bool((i1[near] - i0[near] == 2).all())
            else:
                assert not (a0 + a1 > 1.5).any() or kind == 'past'
    # the chunk skip: a shuffled row leaves no chunk to skip (every chunk's cells span the grid), a sorted one nearly all
    c = cases['w2048_xshuffled']
    (i0, i1), _, _ = T.axis32(c['axes'][2], 2, c['res'], c['cs'])
    assert bool((np.minimum(i0, i1).reshape(-1, 64).min(1) == 0).all()) and bool((np.maximum(i0, i1).reshape(-1, 64).max(1) == c['res'] - 1).all())
    stats = {}
    T.model(c, stats=stats)
    assert stats['chunks_skipped'] == 0 and stats['chunks_visited'] == c['B'] * c['H'] * 2 * c['res'] * 16
    for name in ('w1023_res50', 'w2049_res130', 'w1024_res64_ydesc'):
        T.model(cases[name], stats=stats)
        assert stats['chunks_skipped'] > 4 * stats['chunks_visited'], name
    # centre and scale as set_scale makes them
    c = cases['scaled']
    assert c['cs'] != T.IDENTITY and all(abs(x) > 0 for x in c['cs'][3:]) and c['cs'][0] != 0
    for d in range(3):
        _, _, u = T.axis32(c['axes'][d], d, c['res'], c['cs'])
        assert abs(float(u.min()) - 0.5) < 1e-5 and abs(float(u.max()) - (c['res'] - 1.5)) < 1e-5
