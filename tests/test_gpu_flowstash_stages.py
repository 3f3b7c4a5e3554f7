"""GPU: the error stash (`flowtrainer.error_stash`, csrc/flowtrain.hip) stage by stage from the buffers the call leaves in the caller's
workspace.

Every call gets a NaN-filled workspace a few floats larger than needed, a NaN-filled `error_out` and logs that are not zero.
    stage 0   E bit for bit the numpy fp32 restatement, fractional masks included
    stage 1   every R1[b][y][tile][ix] against the exact sum of fl32(a_x E), E the call's own: budget n 2^-24 A, n <= 1 exact
    stage 2   every R2[b][iy][ix] against the exact sum of fl32(a_y row), row the fp32 tile sum of the call's own R1; Cy, Cx likewise
    stage 3   the logs bit for bit old + what one thread makes of the call's own R2, Cy, Cx
    fill      no slot of the workspace left unwritten, the surplus untouched
then, from zeroed logs, `check_logs` of tests/flowstash_refs.py against float64, two calls bitwise equal, with and without `error_out`.
References, budgets and cases: tests/flowstash_stage_refs.py; tests/test_flowstash_stages_host.py holds them against a model of the
kernels and against seeded defects.  Nothing is excluded and no budget is measured.
"""
import os
import sys

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import flowstash_stage_refs as T  # noqa: E402
from sin_inn_amd import _lib, flowtrainer  # noqa: E402


@pytest.fixture(scope='module')
def dev():
    assert torch.cuda.is_available(), 'GPU tests need a GPU'
    return torch.device('cuda', 0)


def _call(dev, case, old=None, error_out=True, poisoned=True):
    """(E, workspace, log_buffer, log_counter) of one call as numpy arrays; E and the workspace None where the call got none"""
    b, h, w, res = case['B'], case['H'], case['W'], case['res']
    six = [torch.from_numpy(a).to(dev) for a in case['six']]
    axes = [torch.from_numpy(a).to(dev) for a in case['axes']]
    buf, cnt = (torch.zeros(res ** 3, device=dev) for _ in range(2)) if old is None else (torch.from_numpy(o).to(dev) for o in old)
    e = torch.full((b, h, w), float('nan'), device=dev) if error_out else None
    ws = torch.from_numpy(T.workspace(case)).to(dev) if poisoned else None
    if poisoned:
        assert _lib.lib().sininn_flow_error_stash_workspace_floats(b, h, w, res) == ws.numel() - T.SURPLUS
        assert bool(torch.isnan(ws).all()) and bool(torch.isnan(e).all() if error_out else True)
    flowtrainer.error_stash(*six, *axes, res, case['cs'], buf, cnt, error_out=e, workspace=ws)
    return (e.cpu().numpy() if error_out else None, ws.cpu().numpy() if poisoned else None, buf.cpu().numpy(), cnt.cpu().numpy())


@pytest.mark.parametrize('name', list(T.CASES))
def test_stages(dev, name):
    case = T.case(name)
    e, ws, buf, cnt = _call(dev, case, old=case['old'])
    r = T.stages(case, e, ws, buf, cnt)
    print(f'flowstash stages {name}: {T.describe(r)}')
    failed = T.failures(r)
    assert not failed['fill'], (name, r['unwritten'], r['surplus_touched'])
    assert bool(np.isfinite(e).all())
    assert not failed['stage 0'], (name, r['stage0'])
    assert not failed['stage 1'], (name, r['stage1'])
    assert not failed['stage 2'], (name, r['R2'], r['Cy'], r['Cx'])
    assert not failed['stage 3'], (name, r['stage3'])


@pytest.mark.parametrize('name', list(T.CASES))
def test_end_to_end(dev, name):
    case = T.case(name)
    e, ws, buf, cnt = _call(dev, case)
    if 'fractional' not in case['flags']:              # the (n_terms + 12) U of flowstash_refs counts the roundings of E under 0 / 1 masks
        T.end_to_end(case, buf, cnt, what=f'flowstash end to end {name}')
    again = _call(dev, case)
    assert all(np.array_equal(a, b) for a, b in zip((e, buf, cnt), (again[0], again[2], again[3])))          # equal inputs, equal bits
    assert np.array_equal(ws, again[1], equal_nan=True)
    bare = _call(dev, case, error_out=False, poisoned=False)                                                 # the wrapper's own workspace
    assert np.array_equal(buf, bare[2]) and np.array_equal(cnt, bare[3])
