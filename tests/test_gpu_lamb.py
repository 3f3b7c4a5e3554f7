"""GPU: FusedLAMB (csrc/lamb.hip) against the float64 restatement of tests/lamb_refs.py.

Method, the same for every comparison:
  * before each step the optimiser's own fp32 p, m, v, g are copied into the float64 reference and into the fp32 restatement, so an
    error is one step's and does not compound;
  * per quantity the budget is MULT = 4 times the max-norm deviation of the fp32 restatement from float64 measured in that test,
    relative to max |ref| (the rule and the margin of DESIGN 14), and never less than one fp32 rounding of max |ref| (2^-24
    relative), because the unit is itself a measurement and can come out as zero;
  * every comparison prints `ratio(name) = error / budget`.

Measured on an MI355X (`worst ratios` line of a run with -s): p 0.25, m 0.266, v 0.25, trust ratios 0.25, module parameters 0.25.  The
kernel evaluates the update with the restatement's own fp32 operations, so its error equals the unit wherever the two share the clip
factor (e.g. many-chunks step 2: p 2.78e-08 / 2.78e-08, m 9.24e-08 / 9.24e-08); a ratio over many chunks is closer to float64 than the
unit (7.5e-08 against 2.4e-07).  Integration: first loss 0.1354332, last 0.0556429 fused / 0.0556431 restated.  10 tests, 5 s.
"""
import os
import sys

import pytest
import torch

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from lamb_refs import lamb_grad_sq, lamb_step_ref  # noqa: E402

F64 = torch.float64
MULT, FLOOR = 4.0, 2.0 ** -24
FIT_LR, FIT_STEPS = 3e-3, 60        # at lr 1e-3 sixty steps bring the loss to 0.92 of its first value, at 3e-3 to 0.41


@pytest.fixture(scope='module')
def dev():
    import sin_inn_amd  # noqa: F401
    assert torch.cuda.is_available(), 'GPU tests need a GPU'
    return torch.device('cuda', 0)


def relmax(a, ref):
    a, ref = a.detach().to(F64), ref.detach().to(F64)
    err = (a - ref).abs()
    err = torch.where(torch.isfinite(a), err, torch.full_like(err, float('inf')))
    scale = float(ref.abs().max())
    if scale == 0.0:
        return 0.0 if float(err.max()) == 0.0 else float('inf')
    return float(err.max()) / scale


WORST = {}


def check(name, got, ref64, ref32):
    unit = relmax(ref32, ref64)
    budget = max(MULT * unit, FLOOR)
    err = relmax(got, ref64)
    key = name.split()[-1]
    WORST[key] = max(WORST.get(key, 0.0), err / budget)
    print(f'ratio({name}) = {err / budget:.3g}   [err {err:.3g}, fp32-torch unit {unit:.3g}, budget {budget:.3g}]')
    assert err <= budget, (name, err, budget)


def bits(t):
    return t.view(torch.int32)


def make_params(sizes, dev, seed, zero=()):
    gen = torch.Generator().manual_seed(seed)
    ps = []
    for i, k in enumerate(sizes):
        t = torch.randn(k, generator=gen) * (0.02 + 0.3 * (i % 3))
        if i in zero:
            t.zero_()
        ps.append(torch.nn.Parameter(t.to(dev)))
    return ps


def offsets_of(opt, gi=0):
    fl = opt._flat[gi]
    return [(o, p.numel()) for o, p in zip(fl['offsets'], fl['params'])]


def hyper_of(opt, gi=0):
    h = {k: v for k, v in opt.param_groups[gi].items() if k != 'params'}
    h.update(adam_w_mode=bool(opt.adam_w_mode), use_nvlamb=bool(opt.use_nvlamb))
    return h


def set_grads(opt, gi, seed, scale, zero_tensors=()):
    """seeded normal gradients times `scale` written into the flat buffer of group gi; padding and `zero_tensors` stay zero"""
    fl = opt._flat[gi]
    gen = torch.Generator().manual_seed(seed)
    host = torch.zeros(fl['g'].numel())
    for i, (o, k) in enumerate(offsets_of(opt, gi)):
        if i not in zero_tensors:
            host[o:o + k] = torch.randn(k, generator=gen) * scale
    fl['g'].copy_(host)


def padding_mask(opt, gi=0):
    fl = opt._flat[gi]
    mask = torch.ones(fl['p'].numel(), dtype=torch.bool)
    for o, k in offsets_of(opt, gi):
        mask[o:o + k] = False
    return mask.to(fl['p'].device)


def step_and_compare(tag, opt, grad_scale=1.0):
    """one step of every group of `opt` next to the references; returns per group (ref64, ref32, the ratios applied, the state before)"""
    n_groups = len(opt._flat)
    before = [{k: fl[k].clone() for k in 'pgmv'} for fl in opt._flat]
    sq = {dt: sum(lamb_grad_sq(before[gi]['g'], offsets_of(opt, gi), grad_scale, dt) for gi in range(n_groups))
          for dt in (F64, torch.float32)}
    refs = [{dt: lamb_step_ref(*(before[gi][k] for k in 'pgmv'), offsets_of(opt, gi), hyper_of(opt, gi), opt._flat[gi]['step'] + 1,
                               grad_scale, dt, global_sq=sq[dt]) for dt in (F64, torch.float32)} for gi in range(n_groups)]
    opt.step(grad_scale=grad_scale)
    out = []
    for gi, fl in enumerate(opt._flat):
        r64, r32 = refs[gi][F64], refs[gi][torch.float32]
        ratios = opt.last_trust_ratios()[gi]
        for k in 'pmv':
            check(f'{tag} g{gi} {k}', fl[k], r64[k], r32[k])
        check(f'{tag} g{gi} ratio', ratios, r64['ratios'], r32['ratios'])
        assert torch.equal(bits(fl['g']), bits(before[gi]['g'])), 'step() changed the gradient buffer'
        pad = padding_mask(opt, gi)
        for k in 'pmv':
            assert not bool(bits(fl[k])[pad].any()), f'padding of {k} is not +0'
        out.append((r64, r32, ratios.clone(), before[gi]))
    return out


CASES = {'wd_clip': dict(wd=0.01, g_norm=4.0, gs=1.0, clipped=True),
         'wd_noclip': dict(wd=0.01, g_norm=0.4, gs=1.0, clipped=False),
         'nowd_clip': dict(wd=0.0, g_norm=4.0, gs=1.0, clipped=True),
         'wd_gradscale': dict(wd=0.01, g_norm=4.0 * 8, gs=0.125, clipped=True)}


@pytest.mark.parametrize('case', list(CASES))
def test_ragged_tensors(dev, case):
    from sin_inn_amd import FusedLAMB
    from sin_inn_amd.optim import LAMB_CHUNK as C
    cfg = CASES[case]
    sizes = [1, 3, 4, 5, 255, 256, 257, C - 1, C, C + 1, 3 * C + 7, 4, 64]
    zero_p, zero_g = len(sizes) - 2, len(sizes) - 1
    lr, mgn = 1e-3, 1.0
    opt = FusedLAMB(make_params(sizes, dev, 1, zero=(zero_p,)), lr=lr, weight_decay=cfg['wd'], max_grad_norm=mgn)
    fl = opt._flat[0]
    n_live = sum(sizes) - sizes[zero_g]
    lr32 = torch.tensor(lr, dtype=torch.float32, device=dev)
    for step in range(1, 6):
        # normal gradients of expected norm g_norm: the G conditions below are asserted on the reference, not assumed
        set_grads(opt, 0, 100 + step, cfg['g_norm'] / n_live ** 0.5, zero_tensors=(zero_g,))
        o, k = offsets_of(opt)[zero_p]
        fl['p'][o:o + k].zero_()                                  # the all-zero tensor is an input of every step
        (r64, _, ratios, before), = step_and_compare(f'{case} step {step}', opt, cfg['gs'])
        G = float(r64['G'])
        assert (G >= 2 * mgn) if cfg['clipped'] else (G <= 0.5 * mgn), (case, G)
        assert torch.equal(ratios[zero_p], lr32), 'zero parameters: the ratio is lr itself'
        if cfg['wd'] == 0.0:
            assert bool((ratios == lr32).all()), 'wd = 0: every ratio is lr itself'
            o, k = offsets_of(opt)[zero_g]
            assert torch.equal(bits(fl['p'][o:o + k]), bits(before['p'][o:o + k])), 'zero gradient, wd = 0: p must not move'
            assert not bool(bits(fl['m'][o:o + k]).any()) and not bool(bits(fl['v'][o:o + k]).any())
    print('worst ratios so far:', {k: round(v, 3) for k, v in WORST.items()})


def test_many_chunks(dev):
    from sin_inn_amd import FusedLAMB
    from sin_inn_amd.optim import LAMB_CHUNK as C
    sizes = [300 * C + 3, 4]
    opt = FusedLAMB(make_params(sizes, dev, 2), lr=1e-3)
    assert opt._flat[0]['chunks'].shape[0] == 302
    for step in range(1, 3):
        set_grads(opt, 0, 200 + step, 0.01)
        (r64, _, _, _), = step_and_compare(f'many-chunks step {step}', opt)
        assert float(r64['G']) > 1.0                              # 1.2 M gradients of 0.01: the clip is active


@pytest.mark.parametrize('name', ['RBF', 'RFF'])
def test_real_parameter_sets(dev, name):
    from sin_inn_amd import FusedLAMB, flownet
    torch.manual_seed(3)
    net = {**flownet.model_dict, **flownet.learnable_model_dict}[name](flownet.ModelParams()).to(dev)
    opt = FusedLAMB(net.parameters(), lr=1e-4)
    params = [p for p in net.parameters() if p.requires_grad]
    assert len(params) == (9 if name == 'RFF' else 8)
    if name == 'RFF':
        assert any(tuple(p.shape) == (3, 256) for p in params)
    lo, hi = opt._flat[0]['p'].data_ptr(), opt._flat[0]['p'].data_ptr() + opt._flat[0]['p'].numel() * 4
    assert all(lo <= p.data_ptr() < hi for p in params)
    for step in range(1, 6):
        set_grads(opt, 0, 300 + step, 1e-3)
        (r64, r32, _, _), = step_and_compare(f'{name} step {step}', opt)
        # the module's parameters are views of the flat buffer: what the network computes with is what the reference holds
        got = torch.cat([p.detach().reshape(-1) for p in params])
        want64, want32 = (torch.cat([r['p'][o:o + k] for o, k in offsets_of(opt)]) for r in (r64, r32))
        check(f'{name} step {step} module-parameters', got, want64, want32)


def test_two_param_groups_share_one_gradient_norm(dev):
    from sin_inn_amd import FusedLAMB
    from sin_inn_amd.optim import LAMB_CHUNK as C
    a, b = make_params([C + 5, 7], dev, 4), make_params([300], dev, 5)
    opt = FusedLAMB([dict(params=a), dict(params=b, weight_decay=0.0)], lr=1e-3)
    for step in range(1, 3):
        set_grads(opt, 0, 400 + step, 0.01)
        set_grads(opt, 1, 500 + step, 0.1)                        # ten times the other group's
        before = [fl['g'].clone() for fl in opt._flat]
        (r0, _, _, _), (r1, _, _, _) = step_and_compare(f'two-groups step {step}', opt)
        own = [float(lamb_grad_sq(before[gi], offsets_of(opt, gi), 1.0, F64).sqrt()) for gi in (0, 1)]
        G = float(r0['G'])
        assert float(r1['G']) == G and abs(G - (own[0] ** 2 + own[1] ** 2) ** 0.5) <= 1e-12 * G
        assert own[0] < 1.0 < own[1] < G, (own, G)              # group 0 alone would not clip: its step shows the shared norm


def test_repeatable_bitwise_and_state_dict_round_trip(dev):
    from sin_inn_amd import FusedLAMB
    from sin_inn_amd.optim import LAMB_CHUNK as C
    sizes = [5, 3 * C + 7, 257, C]
    opts = [FusedLAMB(make_params(sizes, dev, 6), lr=1e-3) for _ in range(2)]
    for opt in opts:
        opt._flat[0]['ws'].fill_(float('nan'))
        opt._flat[0]['u'].fill_(float('nan'))
    ratios = []
    for step in range(1, 4):
        for opt in opts:
            set_grads(opt, 0, 600 + step, 0.05)
            opt.step()
        ratios.append([opt.last_trust_ratios()[0].clone() for opt in opts])
    x, y = (opt._flat[0] for opt in opts)
    for k in 'pmv':
        assert bool(torch.isfinite(x[k]).all()) and torch.equal(bits(x[k]), bits(y[k])), k
    for rx, ry in ratios:
        assert bool(torch.isfinite(rx).all()) and torch.equal(bits(rx), bits(ry))
    third = FusedLAMB([torch.nn.Parameter(p.detach().clone()) for p in x['params']], lr=7.0)
    third.load_state_dict(opts[0].state_dict())
    assert third.param_groups[0]['lr'] == 1e-3 and third._flat[0]['step'] == 3
    for opt in (opts[0], third):
        set_grads(opt, 0, 700, 0.05)
        opt.step()
    z = third._flat[0]
    for k in 'pmv':
        assert torch.equal(bits(x[k]), bits(z[k])), k
    assert torch.equal(bits(opts[0].last_trust_ratios()[0]), bits(third.last_trust_ratios()[0]))


def test_fit_flow_with_lamb(dev, monkeypatch):
    """tools/fit_flow.py at 32 x 48 with optimizer='lamb', next to the same loop stepped by the fp32 restatement (the flat buffers of
    FusedLAMB, none of its kernels): both bring the loss below 0.9 of its first value, all losses finite.  Wiring, not accuracy."""
    import math
    import sin_inn_amd
    sys.path.insert(0, os.path.join(ROOT, 'tools'))
    import fit_flow
    from sin_inn_amd.modules import bump_weights_epoch

    class RestatedLAMB(sin_inn_amd.FusedLAMB):
        @torch.no_grad()
        def step(self, closure=None, grad_scale=1.0):
            fl = self._flat[0]
            fl['step'] += 1
            new = lamb_step_ref(fl['p'], fl['g'], fl['m'], fl['v'], offsets_of(self), hyper_of(self), fl['step'], grad_scale,
                                torch.float32)
            for k in 'pmv':
                fl[k].copy_(new[k])
            bump_weights_epoch()

    fused = fit_flow.fit('RBF', 32, 48, FIT_STEPS, lr=FIT_LR, optimizer='lamb')
    monkeypatch.setattr(sin_inn_amd, 'FusedLAMB', RestatedLAMB)
    restated = fit_flow.fit('RBF', 32, 48, FIT_STEPS, lr=FIT_LR, optimizer='lamb')
    for s in range(0, FIT_STEPS, 6):
        print(f'step {s:2d}: fused {fused[s]:.7f} restated {restated[s]:.7f}')
    print(f'final  : fused {fused[-1]:.7f} restated {restated[-1]:.7f}')
    assert all(math.isfinite(x) for x in fused + restated)
    assert restated[-1] < 0.9 * restated[0], 'the step count / lr of this test must let the restatement loop converge'
    assert fused[-1] < 0.9 * fused[0], (fused[0], fused[-1])
