"""CPU: the gather synthesis (sin_inn_amd.flowsynth.gather_composed / gather_slots) against the float64 reference and its
derived per-element budget (tests/flowgather_refs.py), seeded defects, exact integer-shift checks, the slot logic and the refusals of
the C entry point (which come before any launch and need no device)."""
import ctypes as C
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import flowgather_refs as R  # noqa: E402
from sin_inn_amd import _lib, flowsynth  # noqa: E402

F64 = torch.float64
U = R.U


@pytest.fixture(scope='module')
def refs():
    """name -> (inputs, float64 result, budget), computed once"""
    out = {}
    for name in R.CASES:
        inputs = R.case(name)
        out[name] = (inputs, *R.gather64(*inputs))
    return out


def _ratio(got, x64, budget):
    """the worst |got - x64| / budget over every element; inf where got is not finite"""
    err = (got.to(F64) - x64).abs()
    err = torch.where(torch.isfinite(err), err, torch.full_like(err, float('inf')))
    return float((err / budget).max())


# ---- the composed form against the reference ----

@pytest.mark.parametrize('name', list(R.CASES))
def test_composed_fp32_within_budget_everywhere(refs, name):
    (i0, i1, fl, slots, taus), x64, budget = refs[name]
    assert fl.shape[0] > i0.shape[0] * len(taus)                       # T' > B K
    got = flowsynth.gather_composed(i0, i1, fl, slots, taus)
    assert got.dtype == torch.float32 and got.shape == x64.shape
    ratio = _ratio(got, x64, budget)
    print(f'gather_composed fp32 {name}: worst err / budget {ratio:.3f}, median budget {float(budget.median()) / U:.1f} u, '
          f'largest budget {float(budget.max()) / U:.0f} u')
    assert ratio <= 1.0
    # in float64 the composed form is the reference itself, to float64 rounding
    got64 = flowsynth.gather_composed(i0.to(F64), i1.to(F64), fl.to(F64), slots, taus)
    assert float((got64 - x64).abs().max()) < 1e-12


def test_budget_is_tight_in_the_interior(refs):
    """a few tens of u where both samples are inside; loose only where the denominator is e itself"""
    (i0, i1, fl, slots, taus), x64, budget = refs['13x37']
    assert float(budget.median()) < 64 * U
    assert float(budget.max()) < 2.0 ** 11 * 16 * U


def test_non_finite_flow_gives_the_linear_blend(refs):
    """a NaN and an inf flow value: that pixel has no tap inside and is L; its neighbours are not affected"""
    (i0, i1, fl, slots, taus), x64, _ = refs['13x37']
    bad = fl.clone()
    bad[:, 0, 6, 20] = float('nan')
    bad[:, 2, 6, 20] = float('nan')
    bad[:, 1, 3, 9] = float('inf')
    bad[:, 3, 3, 9] = float('-inf')
    y64, budget = R.gather64(i0, i1, bad, slots, taus)
    got = flowsynth.gather_composed(i0, i1, bad, slots, taus)
    assert _ratio(got, y64, budget) <= 1.0
    tau = torch.tensor(taus, dtype=torch.float32).to(F64).view(1, -1, 1)
    for y, x in ((6, 20), (3, 9)):
        lin = (1 - tau) * i0[:, None, :, y, x].to(F64) + tau * i1[:, None, :, y, x].to(F64)
        assert float((y64[..., y, x] - lin).abs().max()) < 1e-12
    keep = torch.ones_like(x64, dtype=torch.bool)
    keep[..., 6, 20] = False
    keep[..., 3, 9] = False
    assert torch.equal(y64[keep], x64[keep])


# ---- seeded defects ----

def _quirk(img, qx, qy):
    """Resample2d's geometry: the coordinate divided by (W - 1, H - 1) and read with align_corners = False"""
    h, w = img.shape[-2:]
    return flowsynth.bilinear_gather(img, qx * w / (w - 1) - 0.5, qy * h / (h - 1) - 0.5)


def _uncounted(img, qx, qy):
    total, n = flowsynth.bilinear_gather(img, qx, qy)
    return total, torch.ones_like(n)


def _defects(i0, i1, fl, slots, taus):
    values = [float(t) for t in taus]
    no_ch2 = slots.clone()
    no_ch2[..., 2] = 0
    flipped = slots.clone()
    reverse = flipped[..., 2] == 0
    flipped[..., 4] = torch.where(reverse, flipped[..., 4] ^ torch.tensor(-2 ** 31, dtype=torch.int32), flipped[..., 4])
    assert bool(reverse.any()) and bool((~reverse).any())
    g = flowsynth.gather_from
    return {
        'quirk geometry': lambda: g(i0, i1, fl, slots, values, sample=_quirk),
        'tau and 1 - tau swapped': lambda: g(i0, i1, fl, slots, [1 - v for v in values]),
        'x and y swapped': lambda: g(i0, i1, fl[:, [1, 0, 3, 2]], slots, values),
        'ch0 read as 0': lambda: g(i0, i1, fl, no_ch2, values),
        'sign of the reverse rule': lambda: g(i0, i1, fl, flipped, values),
        'e dropped': lambda: g(i0, i1, fl, slots, values, eps=0.0),
        'n not counted': lambda: g(i0, i1, fl, slots, values, sample=_uncounted),
    }


@pytest.mark.parametrize('defect', ['none', 'quirk geometry', 'tau and 1 - tau swapped', 'x and y swapped', 'ch0 read as 0',
                                    'sign of the reverse rule', 'e dropped', 'n not counted'])
def test_seeded_defects_fall_outside_the_budget(refs, defect):
    (i0, i1, fl, slots, taus), x64, budget = refs['13x37']
    if defect == 'none':
        assert _ratio(flowsynth.gather_from(i0, i1, fl, slots, [float(t) for t in taus]), x64, budget) <= 1.0
        return
    ratio = _ratio(_defects(i0, i1, fl, slots, taus)[defect](), x64, budget)
    print(f'defect {defect}: worst err / budget {ratio:.3g}')
    assert ratio > 1.0


# ---- exact checks with integer shifts ----

def _shift_case(d, h=6, w=24, c=3):
    g = torch.Generator().manual_seed(5)
    i0 = torch.rand(1, c, h, w, generator=g)
    i1 = torch.zeros_like(i0)
    i1[..., d:] = i0[..., :w - d]                                     # I1(x) = I0(x - d)
    fl = torch.tensor([float(d), 0.0, float(-d), 0.0]).view(1, 4, 1, 1).expand(1, 4, h, w).contiguous()
    half = int(np.float32(0.5).view(np.int32))
    slots = torch.tensor([[[0, 0, 2, 0, half, half]]], dtype=torch.int32)          # G0 = bw, c0 = tau;  G1 = fw, c1 = 1 - tau
    return i0, i1, fl, slots


@pytest.mark.parametrize('d', [2, 4])
def test_integer_shift_pins_the_roles(d):
    """I1(x) = I0(x - d), G1 = (d, 0), G0 = (-d, 0), tau = 1/2: both samples read I0(x - d / 2) =: v on the grid with n = 1, so the
    float64 result is (v + e L) / (1 + e) exactly -- v itself up to the guard's share e (L - v) / (1 + e), at most 2^-10 -- and
    the fp32 composed form is within 4 u of it.  Exchanging the two channel pairs moves both samples the other way and breaks it."""
    i0, i1, fl, slots = _shift_case(d)
    h, w = i0.shape[-2:]
    inner = slice(d, w - d)
    v = i0[..., d - d // 2:w - d - d // 2].to(F64)
    lin = 0.5 * i0[..., inner].to(F64) + 0.5 * i1[..., inner].to(F64)
    want = (v + R.EPS * lin) / (1 + R.EPS)
    x64, budget = R.gather64(i0, i1, fl, slots, [0.5])
    assert float((x64[0, 0][..., inner] - want).abs().max()) < 1e-15
    assert float((x64[0, 0][..., inner] - v).abs().max()) <= R.EPS
    got = flowsynth.gather_composed(i0, i1, fl, slots, [0.5])
    assert float((got[0, 0][..., inner].to(F64) - want).abs().max()) <= 4 * U
    assert _ratio(got, x64, budget) <= 1.0
    swapped = slots.clone()
    swapped[..., 2], swapped[..., 3] = 0, 2
    other = flowsynth.gather_composed(i0, i1, fl, swapped, [0.5])
    assert float((other[0, 0][..., inner].to(F64) - want).abs().max()) > 1e-2


def test_tau_0_and_1_on_the_grid_give_the_source_frames():
    i0, i1, fl, _ = _shift_case(2)
    stamps, slots = flowsynth.gather_slots([0.0], [0.0, 1.0], 0.5)
    flows = fl.expand(len(stamps), -1, -1, -1).contiguous()
    got = flowsynth.gather_composed(i0, i1, flows, slots, [0.0, 1.0])
    assert float((got[:, 0] - i0).abs().max()) <= 4 * U              # tau = 0: c0 = 0, the sample is I0(p)
    assert float((got[:, 1] - i1).abs().max()) <= 4 * U              # tau = 1: c1 = 0, the sample is I1(p)


# ---- gather_slots ----

def _coef(slots):
    return flowsynth.slot_coefficients(slots).tolist()


def test_slots_of_a_middle_pair():
    dt = 0.25
    stamps, slots = flowsynth.gather_slots(torch.tensor([-0.5, 0.25]), [0.25, 0.5], dt)
    assert stamps == [-0.4375, -0.375, 0.3125, 0.375, -0.6875, -0.625, 0.0625, 0.125]
    assert slots.dtype == torch.int32 and tuple(slots.shape) == (2, 2, 6) and not slots.is_cuda
    assert slots[..., :4].tolist() == [[[4, 0, 2, 0], [5, 1, 2, 0]], [[6, 2, 2, 0], [7, 3, 2, 0]]]
    assert _coef(slots) == [[[0.25, 0.75], [0.5, 0.5]], [[0.25, 0.75], [0.5, 0.5]]]


def test_slots_of_the_first_pair_fall_back_where_the_time_is_before_the_clip():
    dt = 0.5
    taus = [0.0, 0.25, 0.5, 0.75, 1.0]
    stamps, slots = flowsynth.gather_slots([-1.0, -0.5], taus, dt)
    k = len(taus)
    before = [[t0 + tau * dt - dt < -1.0 for tau in taus] for t0 in (-1.0, -0.5)]
    assert before == [[True, True, True, True, False], [False] * 5]
    reverse = (slots[..., 2] == 0).tolist()
    assert reverse == before                                            # exactly those (b, k) with s - dt < -1
    assert stamps[:2 * k] == [-1.0, -0.875, -0.75, -0.625, -0.5, -0.5, -0.375, -0.25, -0.125, 0.0]
    assert stamps[2 * k:] == [-1.0] + [-1.0, -0.875, -0.75, -0.625, -0.5]
    for b in range(2):
        for j, tau in enumerate(taus):
            idx0, idx1, ch0, ch1 = slots[b, j, :4].tolist()
            c0, c1 = _coef(slots)[b][j]
            assert (idx1, ch1, c1) == (b * k + j, 0, 1 - tau)
            if before[b][j]:
                assert (idx0, ch0, c0) == (idx1, 0, -tau)
            else:
                assert ch0 == 2 and c0 == tau and stamps[idx0] == stamps[idx1] - dt


def test_slots_reverse_never_evaluates_a_second_stamp():
    stamps, slots = flowsynth.gather_slots([-1.0, 0.0, 0.5], [0.25, 0.75], 0.5, back='reverse')
    assert stamps == [-0.875, -0.625, 0.125, 0.375, 0.625, 0.875]
    assert slots[..., 0].tolist() == slots[..., 1].tolist() == [[0, 1], [2, 3], [4, 5]]
    assert bool((slots[..., 2:4] == 0).all())
    assert _coef(slots) == [[[-0.25, 0.75], [-0.75, 0.25]]] * 3


def test_slots_times_of_a_float32_clip():
    """the data set's times are fp32 linspace values: pair 1 at tau = 0 asks for bw at the first frame's time, not for the fallback"""
    times = torch.linspace(-1, 1, 8)
    dt = 2 / 7
    stamps, slots = flowsynth.gather_slots(times[:3], [0.0, 1.0], dt)
    assert (slots[..., 2] == 0).tolist() == [[True, False], [False, False], [False, False]]
    assert all(np.float32(s) == s for s in stamps)


def test_slots_refusals():
    with pytest.raises(ValueError, match=r'range \[0, 1\]'):
        flowsynth.gather_slots([0.0], [1.5], 0.5)
    with pytest.raises(ValueError, match=r'range \[0, 1\]'):
        flowsynth.gather_slots([0.0], [-0.1], 0.5)
    with pytest.raises(ValueError, match='at most 64'):
        flowsynth.gather_slots([0.0], [i / 65 for i in range(65)], 0.5)
    with pytest.raises(ValueError, match='back'):
        flowsynth.gather_slots([0.0], [0.5], 0.5, back='mirror')
    with pytest.raises(ValueError, match='dt > 0'):
        flowsynth.gather_slots([0.0], [0.5], 0.0)


def test_table_is_validated_on_the_host():
    i0, i1, fl, slots = _shift_case(2)
    for column, value, message in ((0, -1, 'negative'), (1, 1, 'time slice 1'), (2, 1, 'channel'), (3, 3, 'channel'),
                                   (4, int(np.float32('nan').view(np.int32)), 'finite')):
        bad = slots.clone()
        bad[0, 0, column] = value
        with pytest.raises(ValueError, match=message):
            flowsynth.gather_composed(i0, i1, fl, bad, [0.5])
    with pytest.raises(ValueError, match='int32'):
        flowsynth.gather_composed(i0, i1, fl, slots.long(), [0.5])
    with pytest.raises(ValueError, match='1 or 3 channels'):
        flowsynth.gather_composed(i0[:, :2], i1[:, :2], fl, slots, [0.5])
    with pytest.raises(RuntimeError, match='no gradient'):
        flowsynth.gather_composed(i0, i1, fl.clone().requires_grad_(True), slots, [0.5])


# ---- the C entry point refuses before any launch ----

def test_entry_point_refusals():
    lib = _lib.lib()
    fake = C.c_void_p(4096)

    def call(**kw):
        a = dict(i0=fake, i1=fake, flows=fake, stride=4 * 6, slots=fake, tau=fake, b=1, k=1, c=3, h=2, w=3, out=fake)
        a.update(kw)
        rc = lib.sininn_flow_gather(a['i0'], a['i1'], a['flows'], a['stride'], a['slots'], a['tau'], a['b'], a['k'], a['c'], a['h'],
                                    a['w'], 0, a['out'], None, None)
        assert rc != 0
        return lib.sininn_last_error().decode()

    for name in ('i0', 'i1', 'flows', 'slots', 'tau', 'out'):
        assert call(**{name: None}) == 'flow_gather: null pointer'
    assert call(c=2) == 'flow_gather: frames have 1 or 3 channels (got 2)'
    assert call(k=0) == 'flow_gather: K = 0 times in one call, 1 to 64 are supported'
    assert call(k=65) == 'flow_gather: K = 65 times in one call, 1 to 64 are supported'
    assert call(stride=23) == 'flow_gather: sample stride 23 is smaller than four channel planes (24)'
    assert call(h=65536, w=65536, stride=2 ** 40) == 'flow_gather: H * W = 4294967296 is past an int index'
    assert 'needs more blocks than one launch has' in call(b=2 ** 20, k=64, h=30000, w=30000, stride=2 ** 40)
    assert call(b=0) == 'flow_gather: bad shape (every size must be positive)'
