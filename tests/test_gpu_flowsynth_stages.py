"""GPU: the frame synthesis (csrc/flowsynth.hip) stage by stage from the accumulator the call leaves in its workspace.

Each call gets a NaN-poisoned workspace and times that include 0 and 1, so that the kernel's own w = exp(Z) can be read back.
    stage 1   w of every source pixel against float64 under a per-pixel budget derived from the kernel's roundings; I * w == fl32(I * w)
    stage 2   every accumulator element against the exact sum of fl32(I * w) * tap, budget (n + 1) 2^-24 sum |term|; holes exact zeros
    stage 3   out bit for bit the blend restated in numpy fp32 on that accumulator; the bytes by the host rule
    exact     zero frames, quarter-pixel flows and times: the N planes equal float64 exactly, whatever the atomics' order
The references, budgets and cases are in tests/flowsynth_stage_refs.py; tests/test_flowsynth_stages_host.py holds them against a model
of the kernel and against seeded defects.  Nothing is excluded and no unit is taken from another fp32 path.
"""
import os
import sys

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import flowsynth_stage_refs as S  # noqa: E402
from sin_inn_amd import flowsynth  # noqa: E402


@pytest.fixture(scope='module')
def dev():
    assert torch.cuda.is_available(), 'GPU tests need a GPU'
    return torch.device('cuda', 0)


def _call(dev, case):
    """(acc, out, u8) of one `synthesize` call as numpy arrays; the workspace is poisoned, the call zeroes it"""
    i0, i1, f01, f10, taus = case
    b, c, h, w = i0.shape
    need = flowsynth.workspace_floats(b, len(taus), c, h, w)
    assert need == b * len(taus) * 2 * (c + 1) * h * w
    ws = torch.full((need,), float('nan'), device=dev)
    out, u8 = flowsynth.synthesize(*[torch.from_numpy(a).to(dev) for a in (i0, i1, f01, f10)], list(taus), u8=True, workspace=ws)
    acc = ws.cpu().numpy().reshape(b, len(taus), 2, c + 1, h, w)
    return acc, out.cpu().numpy(), u8.cpu().numpy()


@pytest.mark.parametrize('name', list(S.CASES))
def test_stages(dev, name):
    case = S.case(name)
    b, _, h, w = case[0].shape
    if name == 'past cap':
        tiles_x, tiles_y, tiles, cap = S.tile_counts(b, h, w)
        assert tiles > cap
    acc, out, u8 = _call(dev, case)
    finite = bool(np.isfinite(acc).all()) and bool(np.isfinite(out).all())
    r1, wrong = S.stage1(case, acc)
    r2 = S.stage2(case, acc)
    bits, bytes_ = S.stage3(case, acc, out, u8)
    print(f'flowsynth stages {name}: stage 1 error / budget {r1:.3f}, {wrong} products differ;  stage 2 error / budget {r2:.3f};  '
          f'stage 3 {bits} outputs and {bytes_} bytes differ;  finite {finite}')
    assert finite
    assert r1 <= 1 and wrong == 0, (name, r1, wrong)
    assert r2 <= 1, (name, r2)
    assert bits == 0 and bytes_ == 0, (name, bits, bytes_)


@pytest.mark.parametrize('name', S.EXACT_FLOWS)
def test_exact_merges(dev, name):
    case = S.case(name, zero_frames=True)
    acc, out, _ = _call(dev, case)
    differing = S.exact_check(case, acc)
    print(f'flowsynth exact {name}: {differing} accumulator elements differ from float64')
    assert differing == 0
    assert bool((out == 0).all())                    # both frames are zero: every blend and every fallback is 0
