"""CPU: the progressive flow-field networks (sin_inn_amd/flownet.py) and their controllers (sin_inn_amd/progressive.py) against
fixtures written by the reference's own model.py and progressive_controller.py (tests/golden/make_golden_flownet_progressive.py), and
the float64 restatement with concatenation and mask that tests/test_gpu_flownet_progressive.py measures the kernels with.
"""
import ctypes as C
import os
import sys

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from flownet_refs import net_tensors, own_gates, restate  # noqa: E402

NETS = ('PRBF', 'PFF', 'PUFF')
SEED = {'PRBF': 404, 'PFF': 505, 'PUFF': 606}
TIMES, GH, GW, SCALE, STRIDE = (0.0, 0.5), 20, 28, 3.0, 97
MAX_ITERATION, EPSILON, N_RAMP, N_MID = 1000, 1e-3, 98, 100
ITERS = (1, 2, 3, 4, 7, 8, 9, 12, 16, 97, 98, 100, 299, 300, 301, 302, 500, 671, 672, 673, 1000)
KEYS = [f'model.model.{i}.{s}' for i in (0, 2, 4, 6) for s in ('weight', 'bias')]


@pytest.fixture(scope='module')
def gold():
    return np.load(os.path.join(ROOT, 'tests', 'golden', 'golden_flownet_progressive.npz'))


def build(name):
    from sin_inn_amd import flownet
    torch.manual_seed(SEED[name])
    return flownet.progressive_model_dict[name](flownet.ModelParams())


def controller(kind, net):
    from sin_inn_amd import progressive
    if kind == 'lin':
        return progressive.LinearController(net, MAX_ITERATION)
    return progressive.LinearControllerEarly(net, MAX_ITERATION, epsilon=EPSILON)


def scripted_loss(i):
    return torch.tensor(0.5 if i < 300 else 5e-4)


@pytest.mark.parametrize('name', NETS)
def test_port_holds_the_reference_numbers(gold, name):
    net = build(name)
    sd = net.state_dict()
    assert list(sd.keys()) == [str(k) for k in gold[f'{name}_keys']]
    params = dict(net.named_parameters())
    assert sorted(params) == sorted(KEYS)
    for key, v in sd.items():
        if key in params:
            flat = v.detach().reshape(-1)
            assert np.array_equal(flat[:32].numpy(), gold[f'{name}_head_{key}']), key
            assert np.array_equal(flat[-32:].numpy(), gold[f'{name}_tail_{key}']), key
            assert flat.double().sum().item() == float(gold[f'{name}_sum_{key}']), key
        else:
            assert np.array_equal(v.numpy(), gold[f'{name}_buf_{key}']), key
    assert net.is_progressive and net.encoding_dim == 515 and net.domain_dim == 3
    assert tuple(sd['model.model.0.weight'].shape) == (256, 515) and tuple(sd['model.model.6.weight'].shape) == (4, 256)
    with pytest.raises(NotImplementedError):
        net(torch.zeros(4, 3))
    with pytest.raises(NotImplementedError):
        controller('early', net)(torch.zeros(4, 3))


@pytest.mark.parametrize('kind', ['lin', 'early'])
def test_controller_trajectory(gold, kind):
    ctl = controller(kind, build('PRBF'))
    assert ctl.is_progressive and ctl.encoding_dim == 515 and ctl.domain_dim == 3
    assert ctl.name == {'lin': 'linear', 'early': 'linear_early'}[kind]
    assert [ctl.block_size, ctl.block_iterations, ctl.progress_iterations] == gold['traj_meta'].tolist() == [6, 8, 672]
    assert np.array_equal(ctl.mask.numpy(), gold['mask_init']) and np.array_equal(ctl.init_mask().numpy(), np.ones(515, np.float32))
    ctl.eval()
    at = 0
    for i in range(MAX_ITERATION):
        ctl.stash_iteration(scripted_loss(i))
        if i + 1 in ITERS:
            state = ctl.state_dict()
            assert np.array_equal(ctl.mask.numpy(), gold[f'traj_{kind}_mask'][at]), i + 1
            assert ctl.cur_block == int(gold[f'traj_{kind}_cur'][at]) and ctl.next_block == int(gold[f'traj_{kind}_next'][at]), i + 1
            assert np.array_equal(state['mask_stashed'].numpy(), gold[f'traj_{kind}_stashed'][at]), i + 1
            at += 1
        if i + 1 == N_MID:
            assert np.array_equal(ctl.mask.numpy(), gold['mask_mid'])
        if i + 1 == N_RAMP:
            assert np.array_equal(ctl.mask.numpy(), gold['mask_ramp'])
    assert at == len(ITERS) and ctl.iteration == MAX_ITERATION
    assert ctl.training                       # `not self.train()` of update_mask switched the module back to training mode
    if kind == 'early':
        assert ctl.trigger and ctl.cur_block == 228 and float(ctl.mask.sum()) == 234.0
    else:
        assert ctl.cur_block == 515 and float(ctl.mask.sum()) == 515.0


@pytest.mark.parametrize('kind', ['lin', 'early'])
def test_state_dict_keys_and_round_trips(gold, kind):
    ctl = controller(kind, build('PRBF'))
    keys = list(ctl.state_dict().keys())
    assert keys == ['mask_stashed', 'model.encode.centres', 'model.encode.sigma'] + ['model.' + k for k in KEYS]
    for i in range(MAX_ITERATION):
        ctl.stash_iteration(scripted_loss(i))
        if i + 1 in (N_RAMP, MAX_ITERATION):
            tag = 'ramp' if i + 1 == N_RAMP else 'final'
            other = controller(kind, build('PRBF'))
            with torch.no_grad():
                for p in other.parameters():
                    p.zero_()
            other.load_state_dict({k: v.clone() for k, v in ctl.state_dict().items()})
            assert np.array_equal(ctl.mask.numpy(), gold[f'rt_{kind}_{tag}_saved'])
            assert np.array_equal(other.mask.numpy(), gold[f'rt_{kind}_{tag}_loaded'])
            assert other.mask.shape == (515,)
            for a, b in zip(ctl.parameters(), other.parameters()):
                assert torch.equal(a, b)
            if tag == 'ramp':       # six entries at 0.5 are stored as their sum and come back as three ones
                assert ctl.mask[78:84].tolist() == [0.5] * 6 and other.mask[78:84].tolist() == [1.0, 1.0, 1.0, 0.0, 0.0, 0.0]
            else:
                assert torch.equal(ctl.mask, other.mask)


@pytest.mark.parametrize('name', NETS)
def test_restatement_reproduces_the_reference_in_float64(gold, name):
    net = build(name)
    bufs, weights = net_tensors(net)
    times, ys, xs = torch.tensor(TIMES), torch.linspace(-1, 1, GH), torch.linspace(-1, 1, GW)
    w64 = [p.double().requires_grad_(True) for p in weights]
    masks = {k: torch.from_numpy(gold[f'mask_{k}']) for k in ('mid', 'ramp')}
    masks['ones'] = torch.ones(515)
    for k, mask in masks.items():
        flows = restate(name, bufs, w64, times, ys, xs, SCALE, torch.float64, mask)
        ref = torch.from_numpy(gold[f'{name}_out64_{k}'])
        assert float((flows.detach() - ref).abs().max() / ref.abs().max()) < 1e-12, k
        if k != 'ramp':
            with torch.no_grad():
                f32 = restate(name, bufs, weights, times, ys, xs, SCALE, torch.float32, mask)
            ref32 = torch.from_numpy(gold[f'{name}_out32_{k}'])
            assert float((f32 - ref32).abs().max() / ref32.abs().max()) < 1e-4, k   # two fp32 evaluations (thread count, BLAS blocking)
    # gradients under the ramping mask, with forced gates equal to the ReLU's own decision
    mask = masks['ramp']
    forced = restate(name, bufs, w64, times, ys, xs, SCALE, torch.float64, mask, own_gates(name, bufs, w64, times, ys, xs, mask))
    ref = torch.from_numpy(gold[f'{name}_out64_ramp'])
    assert float((forced.detach() - ref).abs().max() / ref.abs().max()) < 1e-12
    up = torch.from_numpy(gold['up']).double()
    grads = torch.autograd.grad((forced * up).sum(), w64)
    for key, g in zip(KEYS, grads):
        full = g
        g = g.reshape(-1)
        sub = g if g.numel() <= 1024 else g[::STRIDE]
        want = torch.from_numpy(gold[f'{name}_gsub_{key}'])
        scale = float(want.abs().max())
        assert float((sub - want).abs().max()) <= 1e-12 * scale, key
        gabs = float(gold[f'{name}_gabs_{key}'])
        assert abs(g.sum().item() - float(gold[f'{name}_gsum_{key}'])) <= 1e-12 * gabs, key
        assert abs(g.abs().sum().item() - gabs) <= 1e-12 * gabs, key
        if key == 'model.model.0.weight':
            want = torch.from_numpy(gold[f'{name}_gcoord'])
            assert float((full[:, :3] - want).abs().max()) <= 1e-12 * float(want.abs().max())
            assert float(want.abs().max()) > 0 and bool((full[:, mask == 0] == 0).all())


def test_abi_and_refusals():
    import sin_inn_amd  # noqa: F401
    from sin_inn_amd import _lib, flownet
    lib = _lib.lib()
    assert lib.sininn_version() == 4
    sym = 'sininn_flownet_forward_workspace_bytes'
    assert hasattr(lib, sym) and sym in _lib.EXPORTED and sym in open(os.path.join(ROOT, 'include', 'sininn.h')).read()
    assert lib.sininn_sizeof(7) == C.sizeof(_lib.FlowNetArgs)
    assert [f[0] for f in _lib.FlowNetArgs._fields_][-3:] == ['progressive', 'k_active', 'mask']
    for encoding in (0, 1):
        a = _lib.FlowNetArgs()
        a.encoding, a.enc_dim, a.hidden, a.layers, a.out_dim = encoding, 515, 256, 3, 4
        assert lib.sininn_flownet_supported(C.byref(a)) == 0          # 515 inputs without the flag
        assert lib.sininn_flownet_forward_workspace_bytes(C.byref(a)) == 0
        a.progressive = 1
        assert lib.sininn_flownet_supported(C.byref(a)) == 1
        assert lib.sininn_flownet_forward_workspace_bytes(C.byref(a)) == 256 * (512 + 4) * 4
        a.enc_dim = 512
        assert lib.sininn_flownet_supported(C.byref(a)) == 0          # the flag without the coordinates
        a.enc_dim, a.progressive = 515, 2
        assert lib.sininn_flownet_supported(C.byref(a)) == 0
    a = _lib.FlowNetArgs()
    a.encoding, a.enc_dim, a.hidden, a.layers, a.out_dim, a.progressive, a.k_active = 0, 515, 256, 3, 4, 1, 515
    a.T, a.H, a.W = 2, 8, 8
    assert lib.sininn_flownet_forward(C.byref(a), None, None) != 0              # null mask: refused before any launch
    assert b'mask' in lib.sininn_last_error()
    assert lib.sininn_flownet_backward(C.byref(a), None, None) != 0
    assert b'mask' in lib.sininn_last_error()
    n = 3 * 109 * 253
    npad = (n + 63) // 64 * 64
    assert lib.sininn_flownet_saved_bytes(n) == 3 * npad * 256 * 4
    assert lib.sininn_flownet_workspace_bytes(n) > lib.sininn_flownet_saved_bytes(n)
    assert sorted(flownet.model_dict) == ['FFN', 'RBF', 'UFF']
    assert sorted(flownet.progressive_model_dict) == ['PFF', 'PRBF', 'PUFF']
    net = build('PRBF')
    with pytest.raises(NotImplementedError):
        flownet.flow_fields(net, torch.tensor([0.0, 0.5]), 8, 8, 1.0)
    fake = torch.zeros(2)
    with pytest.raises(ValueError):
        flownet._args(net, fake, fake, fake, 1.0)                         # a progressive network without a mask
    with pytest.raises(ValueError):
        flownet._args(flownet.RbfModel(flownet.ModelParams()), fake, fake, fake, 1.0, mask=torch.ones(515))
    assert flownet.last_open(torch.from_numpy(np.zeros(515, np.float32))) == 0
    assert flownet.last_open(torch.tensor([1.0, 1.0, 0.5, 0.0, 0.0])) == 3
