"""CPU: the host side of FusedLAMB -- the flat layout and chunk table, the plain-torch restatement against an element-by-element
numpy loop, the descriptor guards of the C ABI (refused before any launch, so no GPU is needed) and the constructor's refusals."""
import ctypes as C
import math
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from lamb_refs import lamb_step_ref  # noqa: E402


def test_lamb_layout_tiles_every_tensor_once_and_never_touches_padding():
    import sin_inn_amd  # noqa: F401
    from sin_inn_amd.optim import LAMB_CHUNK, lamb_layout
    for c in (LAMB_CHUNK, 8):
        sizes = [1, 3, 4, 5, 255, 256, 257, c - 1, c, c + 1, 3 * c + 7]
        offs, npad, chunks = lamb_layout(sizes, chunk=c)
        assert len(offs) == len(sizes) and npad % 4 == 0
        assert all(o % 4 == 0 for o in offs)
        for t in range(len(sizes)):                               # tensors in order, not overlapping, inside the buffer
            end = offs[t] + sizes[t]
            assert end <= (offs[t + 1] if t + 1 < len(sizes) else npad)
            assert (offs[t + 1] if t + 1 < len(sizes) else npad) - end < 4
        covered = np.zeros(npad, dtype=np.int64)
        owner = np.full(npad, -1, dtype=np.int64)
        for t, (o, k) in enumerate(zip(offs, sizes)):
            owner[o:o + k] = t
        prev = (-1, -1)
        for t, b, n in chunks:
            assert 0 < n <= c and b % 4 == 0
            assert (t, b) > prev, 'chunks are listed in order'
            prev = (t, b)
            assert offs[t] <= b and b + n <= offs[t] + sizes[t], 'a chunk crosses its tensor or touches padding'
            assert (owner[b:b + n] == t).all()
            covered[b:b + n] += 1
        assert (covered[owner >= 0] == 1).all(), 'every element of every tensor belongs to exactly one chunk'
        assert (covered[owner < 0] == 0).all(), 'padding belongs to no chunk'
        per_tensor = [sum(1 for t, _, _ in chunks if t == k) for k in range(len(sizes))]
        assert per_tensor == [-(-k // c) for k in sizes]


def _numpy_lamb(p, g, m, v, offsets, lr, b1, b2, eps, wd, mgn, step, gs, bias_correction=True, adam_w_mode=True,
                grad_averaging=True, use_nvlamb=False):
    """the formula block of include/sininn.h, one element at a time, in Python floats (float64)"""
    p, m, v = p.copy(), m.copy(), v.copy()
    G = math.sqrt(sum((gs * g[i]) ** 2 for b, k in offsets for i in range(b, b + k)))
    clip = G / mgn if (mgn > 0 and G > mgn) else 1.0
    bc1, bc2 = (1 - b1 ** step, 1 - b2 ** step) if bias_correction else (1.0, 1.0)
    beta3 = 1 - b1 if grad_averaging else 1.0
    ratios = []
    for b, k in offsets:
        u = np.zeros(k)
        for j, i in enumerate(range(b, b + k)):
            sg = gs * g[i] / clip
            if not adam_w_mode:
                sg += wd * p[i]
            m[i] = b1 * m[i] + beta3 * sg
            v[i] = b2 * v[i] + (1 - b2) * sg * sg
            u[j] = (m[i] / bc1) / (math.sqrt(v[i] / bc2) + eps)
            if adam_w_mode:
                u[j] += wd * p[i]
        pn = math.sqrt(sum(p[i] ** 2 for i in range(b, b + k)))
        un = math.sqrt(sum(x * x for x in u))
        ratio = lr * pn / un if ((use_nvlamb or wd != 0) and pn != 0 and un != 0) else lr
        for j, i in enumerate(range(b, b + k)):
            p[i] -= ratio * u[j]
        ratios.append(ratio)
    return p, m, v, np.array(ratios), G


@pytest.mark.parametrize('gmul, clipped', [(4.0, True), (0.05, False)])
def test_restatement_matches_an_element_by_element_loop(gmul, clipped):
    rng = np.random.default_rng(5)
    offsets = [(0, 5), (8, 3)]                                   # 5 and 3 elements, the second on the next 4-element boundary
    p, g, m, v = (np.zeros(12) for _ in range(4))
    for b, k in offsets:
        p[b:b + k] = rng.standard_normal(k)
        g[b:b + k] = rng.standard_normal(k) * gmul
        m[b:b + k] = rng.standard_normal(k) * 0.1
        v[b:b + k] = rng.random(k) * 0.01
    hyper = dict(lr=2e-3, betas=(0.9, 0.999), eps=1e-6, weight_decay=0.01, max_grad_norm=1.0)
    for step, gs in ((1, 1.0), (3, 0.5)):
        want = _numpy_lamb(p, g, m, v, offsets, 2e-3, 0.9, 0.999, 1e-6, 0.01, 1.0, step, gs)
        assert (want[4] > 1.0) == clipped
        got = lamb_step_ref(*(torch.from_numpy(a) for a in (p, g, m, v)), offsets, hyper, step, gs, torch.float64)
        for name, w in zip(('p', 'm', 'v', 'ratios'), want):
            np.testing.assert_allclose(got[name].numpy(), w, rtol=1e-13, atol=0, err_msg=name)
        assert abs(float(got['G']) - want[4]) <= 1e-13 * want[4]
        for a in (got['p'], got['m'], got['v']):                  # padding stays what it was
            assert float(a[5:8].abs().max()) == 0 and float(a[11]) == 0


# every switch of the formula block away from its default: alone, max_grad_norm = 0, and all four together.  use_nvlamb only shows
# where wd = 0 (with wd != 0 the ratio is adapted anyway), so its own case runs without weight decay.
MODE_CASES = {'l2': dict(adam_w_mode=False),
              'no_grad_averaging': dict(grad_averaging=False),
              'no_bias_correction': dict(bias_correction=False),
              'nvlamb_nowd': dict(use_nvlamb=True, weight_decay=0.0),
              'no_clip': dict(max_grad_norm=0.0),
              'all': dict(adam_w_mode=False, grad_averaging=False, bias_correction=False, use_nvlamb=True)}
MODE_DEFAULTS = dict(adam_w_mode=True, grad_averaging=True, bias_correction=True, use_nvlamb=False, max_grad_norm=1.0)


@pytest.mark.parametrize('case', list(MODE_CASES))
def test_restatement_modes_match_an_element_by_element_loop(case):
    """the restatement's branches against the loop's, and each flipped switch visible in p: the float64 p moves by more than 1e-6 of
    max |p| (four orders above the rtol) when the switch goes back to its default, so no mode is compared on inputs that hide it"""
    rng = np.random.default_rng(7)
    offsets = [(0, 5), (8, 3)]
    p, g, m, v = (np.zeros(12) for _ in range(4))
    for b, k in offsets:
        p[b:b + k] = rng.standard_normal(k)
        g[b:b + k] = rng.standard_normal(k) * 4.0                # G > max_grad_norm = 1: the clip is live wherever it is enabled
        m[b:b + k] = rng.standard_normal(k) * 0.1
        v[b:b + k] = rng.random(k) * 0.01
    flipped = MODE_CASES[case]
    hyper = dict(lr=2e-3, betas=(0.9, 0.999), eps=1e-6, weight_decay=0.01, **MODE_DEFAULTS)
    hyper.update(flipped)
    tensors = [torch.from_numpy(a) for a in (p, g, m, v)]
    for step, gs in ((1, 1.0), (3, 0.5)):
        flags = {k: hyper[k] for k in ('bias_correction', 'adam_w_mode', 'grad_averaging', 'use_nvlamb')}
        want = _numpy_lamb(p, g, m, v, offsets, 2e-3, 0.9, 0.999, 1e-6, hyper['weight_decay'], hyper['max_grad_norm'], step, gs,
                           **flags)
        assert want[4] > 1.0
        got = lamb_step_ref(*tensors, offsets, hyper, step, gs, torch.float64)
        for name, w in zip(('p', 'm', 'v', 'ratios'), want):
            np.testing.assert_allclose(got[name].numpy(), w, rtol=1e-13, atol=0, err_msg=name)
        assert abs(float(got['G']) - want[4]) <= 1e-13 * want[4]
        for a in (got['p'], got['m'], got['v']):
            assert float(a[5:8].abs().max()) == 0 and float(a[11]) == 0
        # the flipped switches back at their defaults, all at once and one at a time.  Two of 'all' cannot show alone, by the
        # formulas: with wd != 0 the ratio is adapted whatever use_nvlamb says, and without the decoupled wd * p term the adapted
        # ratio divides out the scale sqrt(bc2) / bc1 that bias_correction puts on u (up to eps)
        switches = [k for k in flipped if k != 'weight_decay']
        alone = [[k] for k in switches if len(switches) > 1 and k in ('adam_w_mode', 'grad_averaging')]
        for keys in [switches] + alone:
            back = lamb_step_ref(*tensors, offsets, dict(hyper, **{k: MODE_DEFAULTS[k] for k in keys}), step, gs, torch.float64)
            moved = float((back['p'] - got['p']).abs().max() / got['p'].abs().max())
            print(f'{case} step {step}: {", ".join(keys)} back at the default moves p by {moved:.3g} of max |p|')
            assert moved > 1e-6, (case, keys, moved)


def test_lamb_descriptor_guards_refuse_before_any_launch():
    """as test_descriptor_guards_refuse_before_any_launch of test_host_cpu.py: the pointers are never dereferenced"""
    import sin_inn_amd  # noqa: F401
    from sin_inn_amd import _lib
    lib = _lib.lib()
    assert lib.sininn_sizeof(8) == C.sizeof(_lib.LambArgs)
    fake = 0x7f0000000000                         # 16-byte aligned, never dereferenced on the host
    n_chunks, n_tensors = 7, 3
    need = lib.sininn_lamb_workspace_bytes(n_chunks, n_tensors)
    assert need >= 4 * (n_tensors + 3 * n_chunks)
    assert lib.sininn_lamb_workspace_bytes(0, 3) == 0 and lib.sininn_lamb_workspace_bytes(7, 0) == 0

    def args(**over):
        a = _lib.LambArgs(n=4096 * 4, n_chunks=n_chunks, n_tensors=n_tensors, lr=1e-3, beta1=0.9, beta2=0.999, eps=1e-6,
                          weight_decay=0.01, max_grad_norm=1.0, grad_scale=1.0, step=1, bias_correction=1, adam_w_mode=1,
                          grad_averaging=1, use_nvlamb=0, group=0, n_groups=1, workspace_bytes=need)
        a.p = a.g = a.m = a.v = a.u = a.chunks = a.tensor_offsets = a.norm_slots = a.workspace = fake
        for k, val in over.items():
            setattr(a, k, val)
        return a
    cases = ((dict(struct_bytes=C.sizeof(_lib.LambArgs) - 8), b'struct_bytes'),
             (dict(struct_bytes=0), b'struct_bytes'),
             (dict(m=None), b'null pointer'),
             (dict(chunks=None), b'null pointer'),
             (dict(norm_slots=None), b'null pointer'),
             (dict(v=fake + 4), b'16-byte aligned'),
             (dict(u=fake + 8), b'16-byte aligned'),
             (dict(step=0), b'step must be >= 1'),
             (dict(n_tensors=0), b'must be positive'),
             (dict(n_chunks=0), b'must be positive'),
             (dict(workspace_bytes=need - 4), b'workspace holds'),
             (dict(group=1), b'group index'),
             (dict(group=-1), b'group index'),
             (dict(n_groups=0), b'group index'))
    for fn in (lib.sininn_lamb_grad_norm, lib.sininn_lamb_step):
        for over, word in cases:
            rc = fn(C.byref(args(**over)), None)
            assert rc != 0 and word in lib.sininn_last_error(), (over, lib.sininn_last_error())
        assert fn(None, None) != 0


def test_fused_lamb_refuses_cpu_parameters_and_amsgrad():
    import sin_inn_amd
    lin = torch.nn.Linear(3, 2)
    with pytest.raises(NotImplementedError):
        sin_inn_amd.FusedLAMB(lin.parameters(), lr=1e-3)
    with pytest.raises(RuntimeError, match='does not support the AMSGrad variant'):
        sin_inn_amd.FusedLAMB(lin.parameters(), amsgrad=True)
